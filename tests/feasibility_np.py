"""NumPy restatement of the feasibility projection (TEST INFRASTRUCTURE ONLY; csrc/fcr_feasibility.h is the kernel).

The reference's feasibility recovery (UL/Main.py:584-657, solved per step by FeasibilityRecovery.feasibility_recover)
is ``min (u_NN - u)^2`` over one scalar ``u`` under four hard pressure bounds on the model's state after one and two
RK4 steps with ``u`` held; its slacks are in the cost only and vanish at the optimum. That is a projection of one
number onto a feasible set on the line, restated here as the deterministic search DESIGN.md §7 specifies, on
``oracle.plant_np.rk4_step`` (the non-smooth ``forging_model``), vectorised over states.
"""
from __future__ import annotations

import numpy as np

from oracle.closed_loop_np import closed_loop
from oracle.plant_np import rk4_step

P_SCALE = 1 / 32e6                      # scaling_factors['p1'] = scaling_factors['p2'], UL/Main.py:607-608
DEFAULTS = dict(p1=(0.0, 32e6), p2=(0.0, 32e6), u_bounds=(-0.2, 0.2), ts=1e-3, substeps=4, expand=10, bisect=30)


def violation(x, u, p1=DEFAULTS["p1"], p2=DEFAULTS["p2"], ts=1e-3, substeps=4):
    """v(x, u): the largest scaled bound excess of p1, p2 after one and two steps; u is feasible iff v <= 0.
    NaN propagates (np.maximum), and a NaN v counts as infeasible."""
    x = np.asarray(x, np.float64)
    u = np.asarray(u, np.float64)
    v = np.full(u.shape, -np.inf)
    with np.errstate(all="ignore"):
        for _ in range(2):
            x = rk4_step(x, u, ts, substeps, smooth=False)
            for p, (lo, hi) in ((x[..., 2], p1), (x[..., 3], p2)):
                s = p * P_SCALE
                v = np.maximum(v, np.maximum(lo * P_SCALE - s, s - hi * P_SCALE))
    return v


def _feasible(v):
    with np.errstate(invalid="ignore"):
        return v <= 0          # False for NaN


def project(x, u_nn, p1=DEFAULTS["p1"], p2=DEFAULTS["p2"], u_bounds=DEFAULTS["u_bounds"], ts=1e-3, substeps=4,
            expand=10, bisect=30):
    """(u, flag, v(u)) of the search: flag 0 = u_nn feasible (returned as is), 1 = corrected to the feasible end of
    the bisected bracket, 2 = no probe feasible (clip(u_nn), the reference's ``except`` branch)."""
    x = np.asarray(x, np.float64)
    u_nn = np.asarray(u_nn, np.float64)
    u_lo, u_hi = float(u_bounds[0]), float(u_bounds[1])
    kw = dict(p1=p1, p2=p2, ts=ts, substeps=substeps)
    clip = lambda c: np.clip(c, u_lo, u_hi)
    v0 = violation(x, u_nn, **kw)
    u = u_nn.copy()
    flag = np.zeros(u_nn.shape, np.int32)
    v = v0.copy()
    bad = np.flatnonzero(~_feasible(v0))
    if bad.size == 0:
        return u, flag, v
    xb, ub = x[bad], u_nn[bad]
    n = bad.size
    delta = (u_hi - u_lo) / 2.0 ** expand
    step = delta * 2.0 ** np.arange(expand + 1)                       # (K,)
    cm, cp = clip(ub[:, None] - step), clip(ub[:, None] + step)       # (n, K) probes, all k at once
    xk = np.broadcast_to(xb[:, None, :], (n, expand + 1, 5))
    vm, vp = violation(xk, cm, **kw), violation(xk, cp, **kw)
    fm, fp = _feasible(vm), _feasible(vp)
    any_k = fm | fp
    found = any_k.any(axis=1)
    k = np.argmax(any_k, axis=1)                                      # the first k with a feasible probe
    r = np.arange(n)
    fm_k, fp_k = fm[r, k], fp[r, k]
    take_m = fm_k & (~fp_k | (np.abs(ub - cm[r, k]) <= np.abs(cp[r, k] - ub)))   # both feasible: nearer, ties to c-
    g = np.where(take_m, cm[r, k], cp[r, k])
    vg = np.where(take_m, vm[r, k], vp[r, k])
    kp = np.maximum(k - 1, 0)
    a = np.where(k == 0, ub, np.where(take_m, cm[r, kp], cp[r, kp]))  # the previous probe on that side: infeasible
    # no probe feasible: clip(u_nn) and the violation there (u_nn itself inside the range, else the last probe)
    last = expand
    ub_clip = clip(ub)
    v_clip = np.where(ub > u_hi, vp[:, last], np.where(ub < u_lo, vm[:, last], v0[bad]))
    act = np.flatnonzero(found)
    xa, aa, ga, vga = xb[act], a[act], g[act], vg[act]
    for _ in range(bisect):
        m = 0.5 * (aa + ga)
        vmid = violation(xa, m, **kw)
        ok = _feasible(vmid)
        ga, vga = np.where(ok, m, ga), np.where(ok, vmid, vga)
        aa = np.where(ok, aa, m)
    ub_out, vb, fb = ub_clip.copy(), v_clip.copy(), np.full(n, 2, np.int32)
    ub_out[act], vb[act], fb[act] = ga, vga, 1
    u[bad], v[bad], flag[bad] = ub_out, vb, fb
    return u, flag, v


def closed_loop_recover(x0, ref, W_inp, b_inp, W_out, in_scale, ref_scale, out_scale, ts=1e-3, substeps=4, smooth=True,
                        process_noise=None, meas_noise=None, feas=None, project_reads_record=True):
    """The batched loop with recovery: per step the controller on the record, the projection on the record, the
    plant step with the projected command (process noise held over the step's stages, measurement noise on the
    record only). ``project_reads_record=False`` is the WRONG loop a test sets beside the right one: its projection
    sees the noisy y_dot and z the controller reads but the press's own y, p1, p2. Returns x (B,T+1,5), u (B,T),
    u_nn (B,T), flag (B,T)."""
    feas = dict(feas or {})
    seen = (lambda m, x: m) if project_reads_record else (lambda m, x: np.stack([x[:, 0], m[:, 1], x[:, 2], x[:, 3], m[:, 4]], 1))
    return closed_loop(x0, ref, W_inp, b_inp, W_out, in_scale, ref_scale, out_scale, ts, substeps, smooth, process_noise,
                       meas_noise, project=lambda m, x, u_nn: project(seen(m, x), u_nn, **feas)[:2])
