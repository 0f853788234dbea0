"""The press of tests/press_torch.py with its 28 parameters as a torch tensor that may require grad, and the stepwise
adjoint oracle with parameter gradients (TEST INFRASTRUCTURE ONLY).

* :func:`rhs` / :func:`step` / :func:`trajectory` / :func:`closed_loop` restate ``press_torch``'s with ``row`` a
  ``(B,28)`` (or ``(28,)``) fp64 tensor read column by column, so autograd carries gradients to it (``press_torch._press``
  goes through numpy and cannot). The values are ``press_torch``'s to 1e-15 (tests/test_press_param_grad_host.py); the
  ``torch.where`` masks are the same, so autograd yields the conventions of §7.15: the deformation fields receive
  gradient only where ``y > 0 and yd > 0``, the valve's 0 at a zero pressure difference with ``PS`` / ``PT`` by the branch
  ``z >= 0``, ``FT`` ``yd / 0.5`` inside the knee and 1 outside.
* :func:`stepwise_param_adjoint` is ``press_torch.stepwise_adjoint``'s recursion on a STORED ``(x, u)`` with each step's
  vector-Jacobian product taken with respect to ``(x_t, u_t, row)``; it returns ``g_press (B,28)`` beside the others.
* :func:`figures` / :func:`refused` are ``press_torch``'s, with ``g_press`` compared per parameter column, each over its
  own maximum over the batch (the columns differ by 20 orders of magnitude); a column that is all zero in the oracle
  must be all zero in the result.
* ``mutant`` names one deliberate mistake in how the parameters receive their gradient (:data:`MUTANTS`); the values and
  the state gradients of a mutant are the right ones.
"""
from __future__ import annotations

import numpy as np
import torch

import oracle.plant_np as P
import press_torch as pt

NAMES, F64, BAR = pt.NAMES, pt.F64, pt.BAR
IX = {n: i for i, n in enumerate(NAMES)}
DEFORMATION = ("MU", "K", "W0", "H0", "B0", "T_DEF", "M0", "M1", "M2", "M3", "M4")
MUTANTS = ("d1_reaches_a1_only", "t_def_gets_m1s_gradient", "spread_exponent_constant", "inv_m_chain_without_square",
           "params_last_substep_only", "params_weighted_by_lambda_only", "ps_working_sign_on_return")


def _grad_as(v, slope):
    """``v``'s value with ``slope`` as its derivative with respect to itself (a wrong chain-rule factor)."""
    return v.detach() + (v - v.detach()) * slope.detach()


def rhs(x, u, smooth, row, mutant=None):
    c = {n: row[..., i] for i, n in enumerate(NAMES)}
    y, yd, p1, p2, z = (x[..., k] for k in range(5))
    if smooth:
        p1 = 0.5 * (p1 + torch.sqrt(p1 * p1 + P.SMOOTH_EPS))
        p2 = 0.5 * (p2 + torch.sqrt(p2 * p2 + P.SMOOTH_EPS))
    ratio = c["B0"] / c["W0"]
    if mutant == "spread_exponent_constant":
        ratio = ratio.detach()
    a_spread = 0.14 + 0.36 * ratio - 0.054 * ratio ** 2
    a1, a2 = np.pi * c["D1"] ** 2 / 4, np.pi * c["D2"] ** 2 / 4
    d1_press = c["D1"].detach() if mutant == "d1_reaches_a1_only" else c["D1"]
    on = (y > 0) & (yd > 0)
    ys = torch.where(on, y, torch.full_like(y, 0.1))
    yds = torch.where(on, yd, torch.full_like(yd, 0.1))
    h1 = c["H0"] - ys
    w1 = c["W0"] * (c["H0"] / h1) ** a_spread
    b1 = c["B0"] * (1 + 0.67 * (c["H0"] / h1 * c["W0"] / w1 - 1))
    kd = c["K"] * (1 + c["MU"] * b1 / (2 * ys) + ys / (4 * b1))
    e = torch.log(c["H0"] / h1)
    t_def = c["T_DEF"]
    if mutant == "t_def_gets_m1s_gradient":         # d(M1 T_DEF)/dT_DEF taken as T_DEF, M1's factor
        t_def = _grad_as(t_def, t_def / c["M1"])
    fd = kd * (w1 * b1) * c["M0"] * torch.exp(c["M1"] * t_def) * e ** c["M2"] * (yds / h1) ** c["M3"] * torch.exp(c["M4"] / e)
    fd = torch.where(on, fd, torch.zeros_like(fd))

    def q(a):
        nz = a != 0
        a_s = torch.where(nz, a, torch.ones_like(a))
        r = np.pi * c["D"] * z * c["CD"] * torch.sqrt(2 / c["RHO"] * a_s.abs()) * torch.sign(a_s)
        return torch.where(nz, r, torch.zeros_like(r))

    ps_ret = c["PS"]
    if mutant == "ps_working_sign_on_return":       # the return stroke's PS (in p2's flow) with the working stroke's sign
        ps_ret = _grad_as(ps_ret, -torch.ones_like(ps_ret))
    qpb = torch.where(z >= 0, q(c["PS"] - p1), q(p1 - c["PT"]))
    qat = torch.where(z >= 0, q(p2 - c["PT"]), q(ps_ret - p2))
    v1 = c["V1_0"] / 2 + a1 * y
    v2 = c["V2_0"] / 2 - a2 * y
    ft = torch.where(yd.abs() <= 0.5, c["FT"] * yd / 0.5, c["FT"] + torch.zeros_like(yd))
    m_mass = c["M_MASS"]
    if mutant == "inv_m_chain_without_square":      # d(1/m)/dm taken as -1/m
        m_mass = _grad_as(m_mass, m_mass)
    return torch.stack([
        yd,
        (3 * np.pi * d1_press ** 2 * p1 / 4 - np.pi * c["D2"] ** 2 * p2 / 2 - c["B_DAMP"] * yd - ft - fd) / m_mass + c["G"],
        c["KB"] / v1 * (qpb / 3 - a1 * yd - c["KL_1"] * p1),
        c["KB"] / v2 * (-qat / 2 + a2 * yd - c["KL_2"] * p2),
        -z / c["T1"] + u / c["T1"]], -1)


def step(x, u, smooth, row, ts=1e-3, substeps=4, mutant=None):
    dt = ts / substeps
    const = row.detach()
    for m in range(substeps):
        r = const if mutant == "params_last_substep_only" and m < substeps - 1 else row
        if mutant == "params_weighted_by_lambda_only":
            # the state path with the parameters held, plus a zero-valued term whose gradient is dt/6 lambda^T df/dc at
            # each of the four stage points (the mu terms of the stage weights dropped)
            f = lambda xs: rhs(xs, u, smooth, const, mutant)
            k1 = f(x)
            x2 = x + dt / 2 * k1
            k2 = f(x2)
            x3 = x + dt / 2 * k2
            k3 = f(x3)
            x4 = x + dt * k3
            k4 = f(x4)
            extra = dt / 6 * sum(rhs(s.detach(), u.detach(), smooth, row, mutant) for s in (x, x2, x3, x4))
            x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4) + (extra - extra.detach())
            continue
        f = lambda xs: rhs(xs, u, smooth, r, mutant)
        k1 = f(x)
        k2 = f(x + dt / 2 * k1)
        k3 = f(x + dt / 2 * k2)
        k4 = f(x + dt * k3)
        x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def trajectory(x0, U, smooth, row, ts=1e-3, substeps=4):
    xs, x = [x0], x0
    for t in range(U.shape[1]):
        x = step(x, U[:, t], smooth, row, ts, substeps)
        xs.append(x)
    return torch.stack(xs, 1)


def closed_loop(x0, ref, Wi, bi, Wo, smooth, row, cdt=torch.float64, ts=1e-3, substeps=4):
    """x (B,T+1,5), u (B,T): ``press_torch.closed_loop`` with the press read from ``row``."""
    x, xs, us = x0, [x0], []
    for t in range(ref.shape[1]):
        u = pt.controller(x, ref[:, t], Wi, bi, Wo, cdt)[0]
        x = step(x, u, smooth, row, ts, substeps)
        xs.append(x)
        us.append(u)
    return torch.stack(xs, 1), torch.stack(us, 1)


def step_vjp(xt, ut, lam, smooth, table, ts=1e-3, substeps=4, mutant=None):
    """(J_x^T lam, f_u^T lam, (dF/drow)^T lam per trajectory) of one sampling step at the stored (xt, ut); numpy."""
    x = torch.tensor(xt, dtype=F64, requires_grad=True)
    u = torch.tensor(ut, dtype=F64, requires_grad=True)
    row = torch.tensor(table, dtype=F64, requires_grad=True)
    xn = step(x, u, smooth, row, ts, substeps, mutant)
    gx, gu, gp = torch.autograd.grad((xn * torch.tensor(lam)).sum(), (x, u, row))
    return gx.numpy(), gu.numpy(), gp.numpy()


def stepwise_param_adjoint(x, u, g_x, smooth, table, g_u=None, ctrl=None, ref=None, ts=1e-3, substeps=4, mutant=None,
                           f64=False):
    """``press_torch.stepwise_adjoint`` on the stored x (B,S+1,5), u (B,S) with ``table`` (B,28) a leaf of every step:
    its outputs and ``g_press (B,28)``, each trajectory's own (a shared press: the caller sums over B)."""
    B, S = u.shape
    table = np.broadcast_to(np.asarray(table, np.float64), (B, 28)).copy()
    lam = np.zeros((B, 5))
    out_u = np.zeros((B, S))
    g_press = np.zeros((B, 28))
    if ctrl is not None:
        W_inp, b_inp, W_out = (np.asarray(w, np.float64) for w in ctrl)
        W_out = W_out.reshape(-1)
        g_wi, g_bi, g_wo = np.zeros_like(W_inp), np.zeros_like(b_inp), np.zeros_like(W_out)
        os_ = float(pt.SCALERS["output"]) if f64 else float(np.float32(pt.SCALERS["output"]))
        r32 = (lambda w: w) if f64 else (lambda w: w.astype(np.float32).astype(np.float64))
    for t in reversed(range(S)):
        lam = lam + g_x[:, t + 1]
        lam, gup, gp = step_vjp(x[:, t], u[:, t], lam, smooth, table, ts, substeps, mutant)
        lam = lam.copy()
        g_press += gp
        if ctrl is None:
            out_u[:, t] = gup
            continue
        s, z, v = pt.controller_chain(x[:, t], ref[:, t], W_inp, b_inp, W_out, f64)
        mask = ((v > -1) & (v < 1)).astype(np.float64)
        dv = (g_u[:, t] + gup) * os_ * mask
        dz = dv[:, None] * r32(W_out)[None, :] * (z > 0)
        wi32 = r32(W_inp)
        lam[:, 1] += dz @ wi32[:, 0] / pt.SCALERS["input"][0]
        lam[:, 4] += dz @ wi32[:, 1] / pt.SCALERS["input"][1]
        out_u[:, t] = dv
        g_wo += (dv[:, None] * np.maximum(z, 0).astype(np.float64)).sum(0)
        g_wi += dz.T @ s.astype(np.float64)
        g_bi += dz.sum(0)
    g_x0 = lam + g_x[:, 0]
    if ctrl is None:
        return {"g_x0": g_x0, "g_u": out_u, "g_press": g_press}
    return {"g_x0": g_x0, "dv": out_u, "g_w_inp": g_wi, "g_b_inp": g_bi, "g_w_out": g_wo, "g_press": g_press}


def summed(d: dict) -> dict:
    """``d`` with ``g_press (B,28)`` summed over the trajectories: a shared row's gradient."""
    return {k: (np.asarray(v).sum(0) if k == "g_press" else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ the comparison

def column_figures(got, want) -> np.ndarray:
    """(28,): per parameter column max|got - want| / max|want| over the batch ((28,) inputs: one number a column); a
    column all zero in ``want`` gives 0 if it is all zero in ``got``, else inf; a non-finite ``got`` gives inf."""
    g = np.asarray(got, np.float64).reshape(-1, 28)
    w = np.asarray(want, np.float64).reshape(-1, 28)
    assert g.shape == w.shape, (g.shape, w.shape)
    out = np.zeros(28)
    for i in range(28):
        den, err = np.abs(w[:, i]).max(), np.abs(g[:, i] - w[:, i]).max()
        out[i] = np.inf if not np.all(np.isfinite(g[:, i])) else err / den if den > 0 else (0.0 if err == 0 else np.inf)
    return out


def figures(got: dict, want: dict) -> dict:
    """``press_torch.figures`` for every tensor of ``want``; ``g_press``: the worst of :func:`column_figures`."""
    rest = {k: v for k, v in want.items() if k != "g_press"}
    out = pt.figures(got, rest)
    if "g_press" in want:
        out["g_press"] = float(column_figures(got["g_press"], want["g_press"]).max())
    return out


def refused(got: dict, want: dict, bar=BAR) -> bool:
    """Whether the comparison of the GPU tests turns ``got`` down."""
    return any(not v <= bar for v in figures(got, want).values())


# ------------------------------------------------------------------------------------------------ the fit's yardstick

FIT_FIELDS = ("CD", "M0", "KB")
FIT_TRUE = (0.85, 0.9, 1.1)
FIT_GOLDEN = "press_fit_cpu.json"


def fit_inputs(B=16, S=12, smooth=True):
    """The trace the fit's tests recover a press from: ``open_batch(B, S)`` run, on this restatement, under the oracle's
    press with CD x 0.85, M0 x 0.9, KB x 1.1 -> (x_obs (B,S+1,5), U (B,S)) numpy."""
    x0, U = pt.open_batch(B, S)
    row = pt.oracle_row()
    for f, m in zip(FIT_FIELDS, FIT_TRUE):
        row[IX[f]] *= m
    with torch.no_grad():
        x_obs = trajectory(torch.tensor(x0), torch.tensor(U), smooth, torch.tensor(row)).numpy()
    return x_obs, U


def fit_cpu(x_obs, U, fields=FIT_FIELDS, smooth=True, max_iter=60):
    """``plant.fit_press`` on this restatement: the same unknowns, loss and L-BFGS settings, from the oracle's press ->
    {"multipliers": [...], "loss0", "loss", "evals"}."""
    xo, Ut = torch.tensor(x_obs), torch.tensor(U)
    scale = xo.abs().amax((0, 1))
    base = torch.tensor(pt.oracle_row())
    index = torch.tensor([IX[f] for f in fields])
    q = torch.zeros(len(fields), dtype=F64, requires_grad=True)

    def loss_of(q):
        row = base.index_put((index,), base[index] * torch.exp(q))
        return (((trajectory(xo[:, 0], Ut, smooth, row) - xo) / scale) ** 2).mean()

    opt = torch.optim.LBFGS([q], lr=1, max_iter=max_iter, history_size=10, line_search_fn="strong_wolfe",
                            tolerance_grad=1e-14, tolerance_change=1e-16)
    evals = [0]

    def closure():
        evals[0] += 1
        opt.zero_grad()
        loss = loss_of(q)
        loss.backward()
        return loss

    with torch.no_grad():
        loss0 = float(loss_of(q))
    opt.step(closure)
    with torch.no_grad():
        return {"multipliers": torch.exp(q).tolist(), "loss0": loss0, "loss": float(loss_of(q)), "evals": evals[0]}


def fit_errors(multipliers) -> list:
    """|multiplier / true - 1| per field of :data:`FIT_FIELDS`."""
    return [abs(m / t - 1.0) for m, t in zip(multipliers, FIT_TRUE)]
