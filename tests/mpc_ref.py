"""fp64 torch restatement of the shooting MPC on the press (TEST INFRASTRUCTURE ONLY).

Built on ``tests/press_torch.py`` (imported, not edited): :func:`residuals` / :func:`cost` restate the objective,
:func:`jacobian` its Jacobian — step Jacobians by AUTOGRAD on ``press_torch.step`` at the rolled-out states, chained by
forward sensitivities ``S_{k+1} = A_k S_k + b_k e_k^T`` (not the kernel's reverse sweeps) — :func:`one_iteration` one
Levenberg-Marquardt iteration from ``(U, lambda)``, :func:`solve` K of them, :func:`closed_loop` the T-step loop.
:func:`compare_iteration` is THE comparison of the GPU tests (teacher-forced: each kernel iteration is checked against
``one_iteration`` from the kernel's own previous state); ``mutant`` names one deliberate mistake it must refuse.
"""
from __future__ import annotations

import numpy as np
import torch

import press_torch as PT

F64 = torch.float64
INF = float("inf")
TOL = 1e-9
MUTANTS = ("no_terminal", "no_u_prev", "no_active_set", "identity_damping", "hinge_sign", "no_preview")


def config(N=10, r_u=0.02, p1=(-INF, INF), p2=(-INF, INF), w=0.0, s_p=32e6, u_bounds=(-INF, INF), ts=1e-3, substeps=4,
           smooth=True):
    return dict(N=N, r_u=r_u, p1=p1, p2=p2, w=w, s_p=s_p, u_lo=u_bounds[0], u_hi=u_bounds[1], ts=ts, substeps=substeps,
                smooth=smooth)


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _step(x, u, cfg, table):
    return PT.step(x, u, cfg["smooth"], cfg["ts"], cfg["substeps"], table)


def rollout(x0, U, cfg, table=None):
    """x_0..x_N (B,N+1,5)."""
    return PT.trajectory(x0, U, cfg["smooth"], cfg["ts"], cfg["substeps"], table)


def residuals_of(xs, U, u_prev, ref, cfg, mutant=None):
    """(B, 6N): e_1..e_N, d_0..d_{N-1}, then per k = 1..N the four hinges (p1 hi, p1 lo, p2 hi, p2 lo); an inactive or
    switched-off hinge is a zero (torch.relu: slope 0 at 0)."""
    N = cfg["N"]
    e = xs[:, 1:, 1] - ref
    if mutant == "no_terminal":
        e = torch.cat([e[:, :-1], torch.zeros_like(e[:, -1:])], 1)
    first = torch.zeros_like(u_prev) if mutant == "no_u_prev" else u_prev
    d = np.sqrt(cfg["r_u"]) * (U - torch.cat([first[:, None], U[:, :-1]], 1))
    sw = np.sqrt(cfg["w"])
    hs = []
    for col, (lo, hi) in ((2, cfg["p1"]), (3, cfg["p2"])):
        p = xs[:, 1:, col]
        up = sw * torch.relu((p - hi) / cfg["s_p"]) if cfg["w"] > 0 and np.isfinite(hi) else torch.zeros_like(p)
        if mutant == "hinge_sign" and cfg["w"] > 0 and np.isfinite(hi):
            up = sw * torch.relu((hi - p) / cfg["s_p"])
        dn = sw * torch.relu((lo - p) / cfg["s_p"]) if cfg["w"] > 0 and np.isfinite(lo) else torch.zeros_like(p)
        hs += [up, dn]
    return torch.cat([e, d, torch.stack(hs, -1).reshape(U.shape[0], 4 * N)], 1)


def residuals(x0, U, u_prev, ref, cfg, table=None, mutant=None):
    return residuals_of(rollout(x0, U, cfg, table), U, u_prev, ref, cfg, mutant)


def cost(x0, U, u_prev, ref, cfg, table=None, mutant=None):
    return (residuals(x0, U, u_prev, ref, cfg, table, mutant) ** 2).sum(1)


def step_jacobians(xs, U, cfg, table=None):
    """A (B,N,5,5) = dx_{k+1}/dx_k, b (B,N,5) = dx_{k+1}/du_k at the rolled-out states, by autograd on press_torch.step
    (all steps of all lanes as one batch of B*N independent steps)."""
    B, N = U.shape
    X = xs[:, :N].reshape(B * N, 5).detach().clone().requires_grad_(True)
    Uf = U.reshape(B * N).detach().clone().requires_grad_(True)
    tab = None if table is None else np.repeat(np.asarray(table, np.float64), N, axis=0)
    xn = _step(X, Uf, cfg, tab)
    A, b = torch.empty(B * N, 5, 5, dtype=F64), torch.empty(B * N, 5, dtype=F64)
    for c in range(5):
        gx, gu = torch.autograd.grad(xn[:, c].sum(), (X, Uf), retain_graph=c < 4)
        A[:, c], b[:, c] = gx, gu
    return A.reshape(B, N, 5, 5), b.reshape(B, N, 5)


def jacobian(x0, U, u_prev, ref, cfg, table=None, mutant=None):
    """(r (B,6N), J (B,6N,N), xs) at U: J's state rows from the sensitivities S_k = dx_k/dU."""
    B, N = U.shape
    with torch.no_grad():
        xs = rollout(x0, U, cfg, table)
        r = residuals_of(xs, U, u_prev, ref, cfg, mutant)
    A, b = step_jacobians(xs, U, cfg, table)
    S = torch.zeros(B, 5, N, dtype=F64)
    Ss = []
    for k in range(N):
        S = A[:, k] @ S
        S[:, :, k] += b[:, k]
        Ss.append(S)
    Ss = torch.stack(Ss, 1)                                   # (B,N,5,N): dx_{k+1}/dU
    Je = Ss[:, :, 1, :].clone()
    if mutant == "no_terminal":
        Je[:, -1] = 0
    Jd = np.sqrt(cfg["r_u"]) * (torch.eye(N, dtype=F64) - torch.diag(torch.ones(N - 1, dtype=F64), -1)).expand(B, N, N)
    sw, sp = np.sqrt(cfg["w"]), cfg["s_p"]
    Jh = []
    for col, (lo, hi) in ((2, cfg["p1"]), (3, cfg["p2"])):
        p = xs[:, 1:, col]
        on = cfg["w"] > 0
        up = ((p > hi) & on).to(F64) * (sw / sp)
        if mutant == "hinge_sign" and on and np.isfinite(hi):
            up = -(p < hi).to(F64) * (sw / sp)
        dn = -((p < lo) & on).to(F64) * (sw / sp)
        Jh += [up[:, :, None] * Ss[:, :, col, :], dn[:, :, None] * Ss[:, :, col, :]]
    Jh = torch.stack(Jh, 2).reshape(B, 4 * N, N)
    return r, torch.cat([Je, Jd, Jh], 1), xs


def clip(U, cfg):
    return torch.clamp(U, cfg["u_lo"], cfg["u_hi"])


def one_iteration(x0, U, lam, u_prev, ref, cfg, table=None, mutant=None, plain_clip=False):
    """One iteration from (U (B,N), lam (B,)): (c, c', U', accept, pivot_fail) per lane; c' = inf and U' = U at a pivot
    failure. ``info``: the sixth entry, {"g", "active", "grad_inf"}. plain_clip: the step without the active set (the
    variant the active-set rule is measured against)."""
    B, N = U.shape
    r, J, _ = jacobian(x0, U, u_prev, ref, cfg, table, mutant)
    with torch.no_grad():
        c = (r * r).sum(1)
        H = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])[:, :, 0]
        dH = torch.diagonal(H, dim1=1, dim2=2).clone()
        act = ((U <= cfg["u_lo"]) & (g > 0)) | ((U >= cfg["u_hi"]) & (g < 0))
        if mutant == "no_active_set" or plain_clip:
            act = torch.zeros_like(act)
        keep = (~act).to(F64)
        Hm = H * keep[:, :, None] * keep[:, None, :] + torch.diag_embed(act.to(F64))
        gm = g * keep
        damp = torch.ones_like(dH) if mutant == "identity_damping" else dH
        M = Hm + torch.diag_embed(lam[:, None] * damp)
        L, info = torch.linalg.cholesky_ex(M)
        fail = (info != 0) | ~torch.isfinite(L).all(-1).all(-1) | ~torch.isfinite(M).all(-1).all(-1)
        Ls = torch.where(fail[:, None, None], torch.eye(N, dtype=F64).expand(B, N, N), L)
        delta = torch.cholesky_solve(-gm[:, :, None], Ls)[:, :, 0]
        Un = torch.where(fail[:, None], U, clip(U + delta, cfg))
        cn = cost(x0, Un, u_prev, ref, cfg, table, mutant)
        cn = torch.where(fail, torch.full_like(cn, INF), cn)
        accept = (cn < c) & ~fail
        ginf = torch.where(act, torch.zeros_like(g), g.abs()).amax(1)
    return c, cn, Un, accept, fail, {"g": g, "active": act, "grad_inf": ginf}


def next_lambda(lam, accept):
    return torch.where(accept, torch.clamp(lam * 0.3, min=1e-12), torch.clamp(lam * 10.0, max=1e12))


def solve(x0, U0, u_prev, ref, cfg, K, lam0=1e-3, table=None, mutant=None, plain_clip=False):
    """K iterations: {"U", "cost", "accepted", "lam", "history": per iteration (c, c', U after, accept, fail)}."""
    U, lam = U0.clone(), torch.full((U0.shape[0],), lam0, dtype=F64)
    acc, hist, c = torch.zeros(U0.shape[0], dtype=torch.int64), [], None
    for _ in range(K):
        c0, cn, Un, accept, fail, _ = one_iteration(x0, U, lam, u_prev, ref, cfg, table, mutant, plain_clip)
        U = torch.where(accept[:, None], Un, U)
        c = torch.where(accept, cn, c0)
        lam = next_lambda(lam, accept)
        acc += accept
        hist.append((c0, cn, U.clone(), accept, fail))
    return {"U": U, "cost": c, "accepted": acc, "lam": lam, "history": hist}


def horizon_refs(ref, t, N, preview=True, mutant=None):
    """r_1..r_N (B,N) of step t from ref (B,T): ref[min(t+k-1, T-1)] with preview, else ref[t]."""
    T = ref.shape[1]
    if not preview or mutant == "no_preview":
        return ref[:, t:t + 1].expand(-1, N).clone()
    return ref[:, [min(t + k, T - 1) for k in range(N)]]


def shift_plan(U):
    return torch.cat([U[:, 1:], U[:, -1:]], 1)


def plant_step(x, u, cfg, table=None, w=None):
    """The true press's step; w (B,5): process noise in the units of x_dot, added to every stage."""
    if w is None:
        return _step(x, u, cfg, table)
    dt = cfg["ts"] / cfg["substeps"]
    f = lambda xs: PT.rhs(xs, u, cfg["smooth"], table) + w
    for _ in range(cfg["substeps"]):
        k1 = f(x)
        k2 = f(x + dt / 2 * k1)
        k3 = f(x + dt / 2 * k2)
        k4 = f(x + dt * k3)
        x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def closed_loop(x0, ref, cfg, K, lam0=1e-3, model=None, plant=None, preview=True, u_init=0.0, wn=None, vn=None):
    """{"x" (B,T+1,5) the record, "u" (B,T), "plans" (B,T,N), "cost", "accepted" (B,T)}."""
    B, T = ref.shape
    N = cfg["N"]
    x = m = x0
    up = torch.full((B,), float(u_init), dtype=F64)
    U = clip(up[:, None].expand(B, N).clone(), cfg)          # the starting plan is projected into the box, u_prev is not
    xs, us, plans, costs, accs = [x0], [], [], [], []
    for t in range(T):
        if t > 0:
            U = shift_plan(U)
        s = solve(m, U, up, horizon_refs(ref, t, N, preview), cfg, K, lam0, model)
        U = s["U"]
        up = U[:, 0].clone()
        with torch.no_grad():
            x = plant_step(x, up, cfg, plant, None if wn is None else wn[:, t])
        m = x if vn is None else x + vn[:, t]
        xs.append(m)
        us.append(up)
        plans.append(U)
        costs.append(s["cost"])
        accs.append(s["accepted"])
    st = lambda l, d: torch.stack(l, 1) if l else torch.zeros(B, 0, *d, dtype=F64)
    return {"x": torch.stack(xs, 1), "u": st(us, ()), "plans": st(plans, (N,)), "cost": st(costs, ()), "accepted": st(accs, ())}


# ------------------------------------------------------------------------------------------------ the comparison

def compare_iteration(got: dict, want, tol=TOL):
    """One iteration of every lane. ``got``: the kernel's {"c", "cn", "accept", "fail" (B,), "U_before", "U_after" (B,N),
    "lam_before", "lam_after" (B,)}; ``want``: :func:`one_iteration`'s result from (U_before, lam_before). Returns
    (figures, reasons): figures = the largest relative errors of c, c' and of the accepted trial points (over max|U'|);
    reasons = why the comparison refuses (empty: it passes). The accept flag must be the restatement's unless
    |c' - c| <= tol c (a tie: either is right); (U_after, lam_after) must be exactly what the kernel's own flag implies."""
    c, cn, Un, accept, fail = (np.asarray(v) for v in want[:5])
    g = {k: np.asarray(v) for k, v in got.items()}
    reasons = []
    ga, gf = g["accept"].astype(bool), g["fail"].astype(bool)
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    fig = {"c": float(rel(g["c"], c).max()), "cn": 0.0, "U": 0.0}
    if not fig["c"] <= tol:
        reasons.append(f"c off by {fig['c']:.3e}")
    if not np.array_equal(gf, fail):
        reasons.append(f"pivot flags differ in {int((gf != fail).sum())} lanes")
    ok = ~gf & ~fail
    if ok.any():
        fig["cn"] = float(rel(g["cn"][ok], cn[ok]).max())
        if not fig["cn"] <= tol:
            reasons.append(f"c' off by {fig['cn']:.3e}")
    tie = np.abs(cn - c) <= tol * np.abs(c)
    bad = (ga != accept) & ~tie & ok
    if bad.any():
        reasons.append(f"accept flags differ off a tie in {int(bad.sum())} lanes")
    if (ga & gf).any():
        reasons.append("accepted at a pivot failure")
    took = ga & ok
    if took.any():
        fig["U"] = float((np.abs(g["U_after"][took] - Un[took]).max(1) / np.abs(Un[took]).max(1).clip(1e-300)).max())
        if not fig["U"] <= tol:
            reasons.append(f"U' off by {fig['U']:.3e}")
    if not np.array_equal(g["U_after"][~ga], g["U_before"][~ga]):
        reasons.append("a rejected iteration moved U")
    lam_want = np.where(ga, np.maximum(g["lam_before"] * 0.3, 1e-12), np.minimum(g["lam_before"] * 10.0, 1e12))
    if not np.array_equal(g["lam_after"], lam_want):
        reasons.append("lambda is not what the flag implies")
    return fig, reasons


def as_got(c, cn, Un, accept, fail, U, lam):
    """A restatement's iteration dressed as a kernel's record (the host tests' stand-in for the GPU)."""
    accept = np.asarray(accept)
    lam = np.asarray(lam)
    return {"c": np.asarray(c), "cn": np.asarray(cn), "accept": accept, "fail": np.asarray(fail), "U_before": np.asarray(U),
            "U_after": np.where(accept[:, None], np.asarray(Un), np.asarray(U)), "lam_before": lam,
            "lam_after": np.where(accept, np.maximum(lam * 0.3, 1e-12), np.minimum(lam * 10.0, 1e12))}


# ------------------------------------------------------------------------------------------------ inputs

def trace_mpc():
    return np.load(PT.GOLDEN + "/plant_trace.npz")["mpc"]     # columns time, ref, y, y_dot, p1, p2, z, u


def warm_problems(n=85):
    """Logged state, logged reference held over the horizon, U0 = u_prev = the previous logged command: (x0, ref, u_prev)."""
    d = trace_mpc()
    idx = np.linspace(1, len(d) - 1, n).astype(int)
    return d[idx, 2:7].copy(), d[idx, 1].copy(), d[idx - 1, 7].copy()


def near_kink(xs, cfg, tol=1e-6):
    """Lanes with a rolled-out state within tol of a kink: z = 0, |y_dot| = 0.5, a finite pressure bound (in units of s_p)."""
    xs = np.asarray(xs)
    bad = (np.abs(xs[..., 4]) < tol) | (np.abs(np.abs(xs[..., 1]) - 0.5) < tol)
    for col, bounds in ((2, cfg["p1"]), (3, cfg["p2"])):
        for v in bounds:
            if np.isfinite(v) and cfg["w"] > 0:
                bad |= np.abs(xs[..., col] - v) / cfg["s_p"] < tol
    return bad.reshape(bad.shape[0], -1).any(1)


def draw(B, N, seed, jump=True):
    """Cold problems around the reference's trace: states jittered by 5 %, u_prev the logged command, a reference in +-0.9
    per lane that jumps once inside the horizon (jump), U0 = u_prev plus noise of 0.04 per entry."""
    rng = np.random.default_rng(seed)
    d = trace_mpc()
    rows = d[rng.integers(0, len(d), B)]
    x0 = rows[:, 2:7] * (1 + 0.05 * rng.standard_normal((B, 5)))
    u_prev = rows[:, 7].copy()
    ref = np.repeat(rng.uniform(-0.9, 0.9, (B, 1)), N, 1)
    if jump and N > 1:
        at = rng.integers(1, N, B)
        other = rng.uniform(-0.9, 0.9, B)
        ref = np.where(np.arange(N)[None, :] >= at[:, None], other[:, None], ref)
    U0 = u_prev[:, None] + 0.04 * rng.standard_normal((B, N))
    return x0, ref, u_prev, U0


def problems(B, N, cfg, seed=5, table=None):
    """:func:`draw` with the lanes whose initial rollout comes within 1e-6 of a kink replaced from a second draw; returns
    (x0, ref, u_prev, U0, replaced)."""
    a = draw(B, N, seed)
    xs = rollout(t64(a[0]), t64(a[3]), cfg, table)
    bad = near_kink(xs, cfg)
    if bad.any():
        b = draw(B, N, seed + 1000)
        a = tuple(np.where(bad.reshape((-1,) + (1,) * (u.ndim - 1)), v, u) for u, v in zip(a, b))
    return (*a, int(bad.sum()))


def clear_quantile(v, q, gap):
    """A value near the q-quantile of v that no entry of v is within ``gap`` of: the middle of the first space wider than
    2 gap between neighbouring sorted entries, from the quantile's position upwards (np.quantile itself interpolates
    between — or lands on — data points, which puts a bound chosen with it next to a state by construction)."""
    s = np.sort(np.asarray(v, np.float64).reshape(-1))
    for j in range(int(q * (len(s) - 1)), len(s) - 1):
        if s[j + 1] - s[j] > 2 * gap:
            return float(0.5 * (s[j] + s[j + 1]))
    return float(s[-1] + 2 * gap)


def bounds_at_quantiles(x0, ref, u_prev, U0, cfg, table=None):
    """Bounds that bind where the tests evaluate: the command box at the 25 % / 75 % quantiles of the initial guess, the
    pressure bounds near those of the restatement's own rollout from the clipped guess (:func:`clear_quantile`: no
    rolled-out pressure within 2e-6 s_p of a bound), so each side of the box and each hinge is active on 5-95 % of the
    entries. Returns (u_bounds, p1, p2)."""
    ub = (float(np.quantile(U0, 0.25)), float(np.quantile(U0, 0.75)))
    xs = rollout(t64(x0), torch.clamp(t64(U0), *ub), cfg, table).numpy()
    q = lambda v: (clear_quantile(v, 0.25, 2e-6 * cfg["s_p"]), clear_quantile(v, 0.75, 2e-6 * cfg["s_p"]))
    return ub, q(xs[:, 1:, 2]), q(xs[:, 1:, 3])
