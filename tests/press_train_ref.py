"""fp64 torch restatement of training a bank on the press (TEST INFRASTRUCTURE ONLY), on top of
tests/press_torch.py, which is imported and not edited.

* :func:`cost` is the MPC loss on a given record, per trajectory; ``mutant`` names one deliberate mistake.
* :func:`closed_loop` is press_torch.closed_loop with ``x = x.detach()`` at the truncation steps ``t = K, 2K, ... < T``.
* :func:`seeds` are the loss's cotangents on a record, by autograd of :func:`cost` (scaled by 1/B: the loss of a model).
* :func:`bank_stepwise` is the bank's stepwise adjoint: ``press_torch.stepwise_adjoint`` per model with those seeds. The
  truncation is taken by segments: the recursion is run on every stretch ``[jK, (j+1)K]`` of the record on its own with
  the seeds on the stretch's states but its first, so lambda starts from zero at every truncation step; ``dv`` is the
  stretches' side by side, the parameter gradients are their sum and ``g_x0`` is the first stretch's.
* :func:`case` builds the inputs the CPU and the GPU tests share, the loss's bounds chosen from the restatement's own
  pressures so that every ReLU is active on a share of the steps and none sits at a bound.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import press_torch as pt

F64 = torch.float64
S_V, S_U = float(pt.SCALERS["y_dot"]), float(pt.SCALERS["output"])
P_SCALE = (32e6 / 2.122366, 32e6 / 1.036233)   # 32 MPa over the default scaled bounds (P1_MAX, P2_MAX)
MUTANTS = ("no_1_over_T", "du_to_u_t_only", "upper_relu_lower_sign", "lambda_not_cleared", "direct_term_cleared",
           "model_0_row")


def cost(x, u, ref, row, p_scale=P_SCALE, u_prev=None, mutant=None):
    """cost (B,) of one model on the record x (B,T+1,5), u (B,T), ref (B,T) under row = (alpha, lo1, hi1, lo2, hi2, w)."""
    alpha, lo1, hi1, lo2, hi2, w = (float(v) for v in row)
    T = u.shape[1]
    if T == 0:
        return torch.zeros(u.shape[0], dtype=F64)
    e = (x[:, 1:, 1] - ref) / S_V
    first = u[:, :1] - u_prev[:, None] if u_prev is not None else torch.zeros_like(u[:, :1])
    before = u[:, :-1].detach() if mutant == "du_to_u_t_only" else u[:, :-1]
    d = torch.cat([first, u[:, 1:] - before], 1) / S_U
    P1, P2 = x[:, 1:, 2] / p_scale[0], x[:, 1:, 3] / p_scale[1]
    r = torch.relu
    up = -1.0 if mutant == "upper_relu_lower_sign" else 1.0     # its value's gradient with the lower bound's sign
    c = w * (r(lo1 - P1) + up * r(P1 - hi1) + r(lo2 - P2) + up * r(P2 - hi2))
    total = (e * e + alpha * d * d + c).sum(1)
    return total if mutant == "no_1_over_T" else total / T


def closed_loop(x0, ref, Wi, bi, Wo, smooth, K=0, cdt=torch.float32, substeps=4, table=None):
    """x (B,T+1,5), u (B,T) of press_torch's loop with the states at t = K, 2K, ... < T detached (K = 0: none)."""
    x, xs, us = x0, [x0], []
    for t in range(ref.shape[1]):
        if K > 0 and t > 0 and t % K == 0:
            x = x.detach()
        u = pt.controller(x, ref[:, t], Wi, bi, Wo, cdt)[0]
        x = pt.step(x, u, smooth, 1e-3, substeps, table)
        xs.append(x)
        us.append(u)
    return torch.stack(xs, 1), (torch.stack(us, 1) if us else torch.zeros(x0.shape[0], 0, dtype=F64))


def seeds(x, u, ref, row, u_prev=None, mutant=None):
    """(g_x (B,T+1,5), g_u (B,T), cost (B,)) of loss = mean_b cost on the record (numpy in and out)."""
    xs = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    us = torch.tensor(np.asarray(u, np.float64), requires_grad=True)
    c = cost(xs, us, torch.tensor(np.asarray(ref, np.float64)), row,
             u_prev=None if u_prev is None else torch.tensor(np.asarray(u_prev, np.float64)), mutant=mutant)
    if u.shape[1] == 0:
        return np.zeros_like(x), np.zeros_like(u), c.detach().numpy()
    g_x, g_u = torch.autograd.grad(c.sum() / x.shape[0], (xs, us))
    return g_x.numpy(), g_u.numpy(), c.detach().numpy()


def model_stepwise(x, u, ref, w, row, smooth, K=0, u_prev=None, substeps=4, table=None, mutant=None, f64=False):
    """One model: {g_x0, dv, g_w_inp, g_b_inp, g_w_out, cost} by the stepwise adjoint on its record, truncated at K."""
    B, T = u.shape
    g_x, g_u, c = seeds(x, u, ref, row, u_prev, mutant)
    if mutant == "lambda_not_cleared":
        K = 0
    cuts = [0] + (list(range(K, T, K)) if K > 0 else []) + [T]
    out = None
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        gx = g_x[:, t0:t1 + 1].copy()
        if t0 > 0:
            gx[:, 0] = 0.0                                       # x_{t0}'s direct term belongs to the stretch before
        if mutant == "direct_term_cleared" and t1 < T:
            gx[:, -1] = 0.0
        part = pt.stepwise_adjoint(x[:, t0:t1 + 1], u[:, t0:t1], gx, smooth, g_u[:, t0:t1], w, ref[:, t0:t1],
                                   substeps=substeps, table=table, f64=f64)
        if out is None:
            out = part
        else:
            out = {"g_x0": out["g_x0"], "dv": np.concatenate([out["dv"], part["dv"]], 1),
                   **{k: out[k] + part[k] for k in ("g_w_inp", "g_b_inp", "g_w_out")}}
    out["cost"] = c
    return out


def bank_stepwise(xs, us, refs, ws, rows, smooth, K=0, u_prevs=None, substeps=4, tables=None, mutant=None, f64=False):
    """The bank: per-model lists in, a dict of arrays stacked over the models out (``loss`` (M,) = the costs' means)."""
    M = len(xs)
    outs = []
    for m in range(M):
        row = rows[0] if mutant == "model_0_row" else rows[m]
        outs.append(model_stepwise(xs[m], us[m], refs[m], ws[m], row, smooth, K, None if u_prevs is None else u_prevs[m],
                                   substeps, None if tables is None else tables[m], mutant, f64))
    got = {k: np.stack([o[k] for o in outs]) for k in outs[0]}
    got["loss"] = got["cost"].mean(1)
    return got


# ------------------------------------------------------------------------------------------------ the comparison

GRAD_KEYS = ("g_x0", "dv", "g_w_inp", "g_b_inp", "g_w_out")


def bank_figures(got: dict, want: dict, keys=GRAD_KEYS) -> dict:
    """press_torch.figures per model (``g_x0`` per state column), the worst model of each tensor."""
    out = {}
    for m in range(len(want[keys[0]])):
        f = pt.figures({k: np.asarray(got[k][m]) for k in keys}, {k: np.asarray(want[k][m]) for k in keys})
        for k, v in f.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def bank_refused(got: dict, want: dict, bar=pt.BAR, keys=GRAD_KEYS) -> bool:
    """Whether the comparison of the GPU tests turns ``got`` down."""
    return any(not v <= bar for v in bank_figures(got, want, keys).values())


# ------------------------------------------------------------------------------------------------ inputs

def _between(values, q, side):
    """A bound at the q-quantile of ``values``, half way between two neighbours (never at a value); one value alone:
    5 % (side 0, a lower bound: active) or 10 % (side 1, an upper bound: inactive) above it."""
    s = np.sort(np.asarray(values).ravel())
    if len(s) < 2 or s[0] == s[-1]:
        return float(s[0] * (1.05 if side == 0 else 1.10))
    i = min(max(int(q * len(s)), 1), len(s) - 1)
    while i < len(s) - 1 and s[i] == s[i - 1]:
        i += 1
    return float(0.5 * (s[i - 1] + s[i]))


def rows_from(xs, M):
    """Model m's row from ITS restated pressures: lower bounds at the 0.20 + 0.05 m quantile, upper at 0.80 - 0.05 m,
    alpha = 10 (m + 1) (so that the command term weighs in beside the tracking error), weight = 1 + 0.5 m."""
    rows = []
    for m in range(M):
        P1, P2 = xs[m][:, 1:, 2] / P_SCALE[0], xs[m][:, 1:, 3] / P_SCALE[1]
        lo_q, hi_q = 0.20 + 0.05 * m, 0.80 - 0.05 * m
        lo1, hi1, lo2, hi2 = _between(P1, lo_q, 0), _between(P1, hi_q, 1), _between(P2, lo_q, 0), _between(P2, hi_q, 1)
        rows.append((10.0 * (m + 1), lo1, max(hi1, lo1), lo2, max(hi2, lo2), 1.0 + 0.5 * m))
    return rows


def model_weights(M, hidden):
    """M controllers of width ``hidden``: press_torch.ctrl_weights at gains 2, 1, 1.5, ... (the first saturates)."""
    return [pt.ctrl_weights(hidden, (2.0, 1.0, 1.5)[m % 3]) for m in range(M)]


def table_of(kind, M, B):
    """The press of a case: None, "row" (28,), "traj" (B,28), "model" (M,B,28) — three distinct rows (by b % 3; by
    (b + m) % 3 per model). Returns (what the library takes, the per-model (B,28) tables of the restatement or None)."""
    if kind is None:
        return None, None
    base = pt.three_rows_table(B + M)
    if kind == "row":
        return base[1].copy(), [np.tile(base[1], (B, 1))] * M
    if kind == "traj":
        return base[:B].copy(), [base[:B]] * M
    tab = np.stack([base[m:m + B] for m in range(M)])
    return tab, [tab[m] for m in range(M)]


@functools.lru_cache(maxsize=None)
def case(M, B, T, hidden=50, smooth=True, substeps=4, press=None, stacked=False, with_u_prev=False):
    """The inputs of one case, shared by the CPU and the GPU tests: ``x0``, ``ref`` ((B,..) shared, or (M,B,..) stacked:
    model m reads the batch rolled by m trajectories), the models' weights ``ws``, the press in the library's form and
    per model, ``u_prev`` (M,B) or None, and the ``rows`` chosen from the restatement's own closed loop (float32
    controller chain, as the kernel's) — its records ``xs`` ride along. Treat everything as read-only."""
    x0, ref = pt.loop_batch(B, max(T, 1))
    ref = ref[:, :T]
    ws = model_weights(M, hidden)
    lib_table, tables = table_of(press, M, B)
    if stacked:
        x0s, refs = np.stack([np.roll(x0, m, 0) for m in range(M)]), np.stack([np.roll(ref, m, 0) for m in range(M)])
    else:
        x0s, refs = [x0] * M, [ref] * M
    u_prev = 0.02 * np.cos(np.arange(M * B)).reshape(M, B) if with_u_prev else None
    xs = []
    with torch.no_grad():
        for m in range(M):
            x, _ = closed_loop(torch.tensor(x0s[m]), torch.tensor(refs[m]), *(torch.tensor(k.astype(np.float64)) for k in ws[m]),
                               smooth, substeps=substeps, table=None if tables is None else tables[m])
            xs.append(x.numpy())
    return dict(M=M, B=B, T=T, hidden=hidden, smooth=smooth, substeps=substeps, ws=ws, x0=x0s if stacked else x0,
                ref=refs if stacked else ref, x0s=x0s, refs=refs, table=lib_table, tables=tables, u_prev=u_prev,
                rows=rows_from(xs, M) if T > 0 else [(0.1, 0.0, 1.0, 0.0, 1.0, 1.0)] * M, xs=xs)


def shares(xs, rows):
    """Per model and ReLU: the share of (b,t) on which it is active, and the least scaled distance of a pressure from a
    bound."""
    out, gap = [], np.inf
    for x, (_, lo1, hi1, lo2, hi2, _) in zip(xs, rows):
        P1, P2 = x[:, 1:, 2] / P_SCALE[0], x[:, 1:, 3] / P_SCALE[1]
        out.append({"lo1": (P1 < lo1).mean(), "hi1": (P1 > hi1).mean(), "lo2": (P2 < lo2).mean(), "hi2": (P2 > hi2).mean()})
        gap = min(gap, np.abs(P1 - lo1).min(), np.abs(P1 - hi1).min(), np.abs(P2 - lo2).min(), np.abs(P2 - hi2).min())
    return out, gap
