"""The MPC loss with its terms as data, restated (a helper, not a test; torch on the CPU in fp64, autograd).

``oracle/`` states the reference's loss with its literals; this module states the semantics of
``MPCLoss(terms=...)`` / ``forward(..., ref_horizon=...)`` in the reference's op order
(oracle/rollout_torch.mpc_loss, Functions.py:1386-1472): for horizon step j and x̂_j = (ẏ, p1, p2, z)

    err_j = (x̂_j[0] − r_j)²
    con_j = w · (relu(p1_lo − p1) + relu(p2_lo − p2) + relu(p1 − p1_hi) + relu(p2 − p2_hi))
    tot  += (err_j + alpha·Δu²) + con_j ;   u_{j+1} = controller(x̂_j[0], x̂_j[3], r_{j+1})

with ``r_j = ref_h[b, j]`` (no gradient), or ``X[b, 2]`` at every j without a preview. tests/test_loss_terms_host.py
holds it to the oracle where the two overlap (default terms; upper bounds through the oracle's ``P1_MAX`` / ``P2_MAX``).

The cases (:func:`build`), shared by the CPU and the GPU test, come from seeds on the synthetic inputs of
tests/axis_cases.py:

* A: bounds at the quartiles of the restatement's own x̂ pressures (each in the middle of a gap between two samples),
  weight 3.5, alpha 3.5 — every one of the four branches active in >= 10 % of the (trajectory, step) pairs;
* B: ``ref_h`` changes sign at j = N / 2 (N = 12 at H = 50: windows before and past the lookback);
* C: A and B together, with noise;
* D: ``p1_hi = +inf``, ``p2_lo = -inf``.

A trajectory within ``BAND`` of any kink (the controller's ReLUs and Hardtanh at the r_{j+1} the call sees, the four
bounds) is replaced from a second draw, as axis_cases.select does; at most ``MAX_REPLACED`` per batch.
:data:`MUTANTS` are the restatement with one term dropped; :func:`failures` is the comparison the GPU test applies.
"""
import functools
import math

import numpy as np
import torch

import axis_cases as A
from kink_cases import controller_u0
from oracle import rollout_torch as T
from tests.golden.make_golden import synth_inputs

P1_MAX, P2_MAX = 2.122366, 1.036233
BAND = A.BAND
MAX_REPLACED = 1
FEATS, GRADS = A.FEATS, A.GRADS
MUTANTS = ("no_lower", "no_weight", "default_upper", "const_ref", "ref_lag")


def default_row(alpha):
    return (float(alpha), 0.0, P1_MAX, 0.0, P2_MAX, 1.0)


def _ref_of(X, ref_h, j, mutant=None, call=False):
    """r_j for the error (call False) or for the controller call that produces u_j (call True)."""
    if ref_h is None:
        return X[:, -1]
    if mutant == "const_ref":
        return ref_h[:, 0]
    if mutant == "ref_lag" and call:
        return ref_h[:, j - 1]          # r_j where r_{j+1} belongs: the call producing u_j sees the step before
    return ref_h[:, j]


def mpc_loss_terms(sim, ctrl, X, u0, states, N, row, ref_h=None, noise=None, mutant=None):
    """oracle.rollout_torch.mpc_loss with the terms ``row`` = (alpha, p1_lo, p1_hi, p2_lo, p2_hi, w) and ``ref_h``."""
    alpha, p1_lo, p1_hi, p2_lo, p2_hi, w = row
    if mutant == "no_lower":
        p1_lo = p2_lo = -math.inf
    if mutant == "no_weight":
        w = 1.0
    if mutant == "default_upper":
        p1_hi, p2_hi = P1_MAX, P2_MAX
    relu = torch.relu

    def con(xh):   # today's summation order
        return w * (relu(p1_lo - xh[:, 1]) + relu(p2_lo - xh[:, 2]) + relu(xh[:, 1] - p1_hi) + relu(xh[:, 2] - p2_hi))

    B = X.shape[0]
    if ref_h is not None:
        ref_h = ref_h.detach()
    window = states.clone()
    window[:, -1, -1] = u0.reshape(B)
    xh = sim(window)
    if noise is not None:
        xh = xh + noise[:, 0]
    err_terms = [torch.square(xh[:, 0] - _ref_of(X, ref_h, 0, mutant))]
    cmd_terms = [alpha * torch.square(window[:, -2, -1] - window[:, -1, -1])]
    tot_terms = [err_terms[0] + cmd_terms[0] + con(xh)]
    u_prev = u0.reshape(B, 1)
    preds, xhs = [u_prev], [xh]
    for j in range(1, N):
        u_next = ctrl(torch.stack((xh[:, 0], xh[:, 3], _ref_of(X, ref_h, j, mutant, call=True)), dim=1))
        window = torch.cat((window[:, 1:10, :], torch.cat((xh, u_next), dim=1).unsqueeze(1)), dim=1)
        xh = sim(window)
        if noise is not None:
            xh = xh + noise[:, j]
        err_terms.append(torch.square(xh[:, 0] - _ref_of(X, ref_h, j, mutant)))
        cmd_terms.append(alpha * torch.square(u_prev.reshape(B) - u_next.reshape(B)))
        tot_terms.append(err_terms[-1] + cmd_terms[-1] + con(xh))
        u_prev = u_next
        preds.append(u_next)
        xhs.append(xh)
    cost = torch.stack(tot_terms).sum(0) / N
    feats = {"loss": cost, "command": torch.stack(cmd_terms).sum(0) / N, "error": torch.stack(err_terms).sum(0) / N,
             "prediction": torch.cat(preds, dim=1).flatten(), "xhat": torch.stack(xhs, dim=1)}
    return cost.mean(), feats


def loss_and_grads(params, X, u0, states, N, row, ref_h=None, noise=None, dtype=torch.float64, mutant=None):
    """oracle.rollout_torch.loss_and_grads for :func:`mpc_loss_terms`: the same names, numpy arrays."""
    sim, ctrl = T.build_modules(params, dtype, lstm_requires_grad=False)
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype)
    u0_t = t(u0).reshape(-1, 1).clone().requires_grad_(True)
    loss, feats = mpc_loss_terms(sim, ctrl, t(X), u0_t, t(states), N, row, t(ref_h), t(noise), mutant)
    loss.backward()
    out = {k: v.detach().numpy() for k, v in feats.items()}
    out["loss_scalar"] = float(loss.detach())
    out["g_u0"] = u0_t.grad.reshape(-1).numpy()
    g = lambda p: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy()
    out["g_W_inp"], out["g_b_inp"], out["g_W_out"] = g(ctrl.fc_inp.weight), g(ctrl.fc_inp.bias), g(ctrl.fc_out.weight)
    return out


def kink_margin(params, X, xhat, row, ref_h=None):
    """oracle.rollout_torch.kink_margin with the terms' bounds as the constraint's kinks (an infinite bound has none)
    and r_{j+1} in the controller call fed by step j. (B,) fp64."""
    X, xhat = np.asarray(X, np.float64), np.asarray(xhat, np.float64)
    B, N = xhat.shape[0], xhat.shape[1]
    m = np.full(B, np.inf)
    for col, bounds in ((1, row[1:3]), (2, row[3:5])):
        for b in bounds:
            if math.isfinite(b):
                m = np.minimum(m, np.abs(xhat[:, :, col] - b).min(axis=1))
    if N < 2:
        return m
    r = np.repeat(X[:, 2:3], N, axis=1) if ref_h is None else np.asarray(ref_h, np.float64)
    cin = np.stack((xhat[:, :-1, 0], xhat[:, :-1, 3], r[:, 1:]), axis=-1)
    z = cin @ params["W_inp"].T + params["b_inp"]
    v = np.maximum(z, 0.0) @ params["W_out"][0]
    return np.minimum(m, np.minimum(np.abs(z).min(axis=(1, 2)), np.abs(1.0 - np.abs(v)).min(axis=1)))


def quartile_bounds(p):
    """(lo, hi) for the samples p: lo at the midpoint between the two neighbouring order statistics nearest the 25th
    percentile, hi likewise at the 75th; where a gap is below 1e-4, the next gap towards the median (so a branch's
    share only grows)."""
    s = np.sort(np.asarray(p, np.float64).ravel())

    def mid(frac, step):
        k = min(int(round(frac * (len(s) - 1))), len(s) - 2)
        while 0 < k + step < len(s) - 1 and s[k + 1] - s[k] < 1e-4:
            k += step
        assert s[k + 1] - s[k] >= 1e-4, "no gap of 1e-4 among the samples"
        return float(np.float32(0.5 * (s[k] + s[k + 1])))   # through float32: the kernels' number

    lo, hi = mid(0.25, 1), mid(0.75, -1)
    assert lo < hi, (lo, hi)
    return lo, hi


def flip_ref(X, N):
    """ref_h (B,N): X[:, 2] before j = N / 2, its negative from there on (closed_loop.reference_speeds' sign flip)."""
    r = np.repeat(np.asarray(X, np.float32)[:, 2:3], N, axis=1)
    r[:, N // 2:] *= -1.0
    return r


# name: kind (A..D), H, B, N, input seed, the kernel families its shape reaches (tests/test_gpu_axes.py's names).
# noise: pre-drawn noise in a case other than C. The synthetic surrogates (H = 24, 64) answer synth_inputs (stretched or
# not) with pressures inside a range of 0.004, 132 samples a few 1e-5 apart: no gap of 1e-4 near a quartile, and any
# bound among them within the kink band of several. The noise (std 0.01 on the predictions) spreads them.
_W4 = ("pipe", "onewg", "fused", A.F16)
CASES = {
    "A_h50_b20_n3": dict(kind="A", H=50, B=20, N=3, seed=4101, families=_W4),
    "B_h50_b20_n12": dict(kind="B", H=50, B=20, N=12, seed=4102, families=_W4),
    "C_h50_b20_n12": dict(kind="C", H=50, B=20, N=12, seed=4103, families=_W4),
    "D_h50_b20_n3": dict(kind="D", H=50, B=20, N=3, seed=4104, families=_W4),
    "A_h24_b33_n4": dict(kind="A", H=24, B=33, N=4, seed=4105, noise=True, families=("pipe", "onewg", "fused")),
    "C_h24_b33_n4": dict(kind="C", H=24, B=33, N=4, seed=4106, families=("pipe", "onewg", "fused")),
    "A_h64_b24_n3": dict(kind="A", H=64, B=24, N=3, seed=4107, noise=True, families=("wide",)),
    "C_h64_b24_n3": dict(kind="C", H=64, B=24, N=3, seed=4108, families=("wide",)),
    "D_h64_b24_n3": dict(kind="D", H=64, B=24, N=3, seed=4109, families=("wide",)),
}
ALPHA = A.ALPHA           # the loss's own alpha where the terms leave it alone (B, D)
W = 50                    # controller width: the reference's


def _terms_of(kind, xhat):
    """(row, LossTerms keywords) of a case from the x̂ of its own draw."""
    if kind in ("A", "C"):
        (l1, h1), (l2, h2) = quartile_bounds(xhat[:, :, 1]), quartile_bounds(xhat[:, :, 2])
        return (3.5, l1, h1, l2, h2, 3.5), dict(p1=(l1, h1), p2=(l2, h2), weight=3.5, alpha=3.5)
    if kind == "D":
        return (ALPHA, 0.0, math.inf, -math.inf, P2_MAX, 1.0), dict(p1=(0.0, math.inf), p2=(-math.inf, P2_MAX))
    return default_row(ALPHA), {}


def _make(name, params, X, S, nz, Xr, Sr, nzr, kind, N, row_kw=None):
    """One case on the draw (X, S, nz) with replacements from (Xr, Sr, nzr)."""
    X, S = X.copy(), S.copy()
    nz = None if nz is None else nz.copy()
    ref_of = (lambda x: flip_ref(x, N)) if kind in ("B", "C") else (lambda x: None)
    run = lambda x, s, z, row: loss_and_grads(params, x, controller_u0(params, x), s, N, row, ref_of(x), z)
    row, kw = row_kw or _terms_of(kind, run(X, S, nz, default_row(ALPHA))["xhat"])   # x̂ does not depend on the bounds
    m = kink_margin(params, X, run(X, S, nz, row)["xhat"], row, ref_of(X))
    inside = np.flatnonzero(m <= BAND)
    if len(inside):
        ok = np.flatnonzero(kink_margin(params, Xr, run(Xr, Sr, nzr, row)["xhat"], row, ref_of(Xr)) > BAND)
        assert len(ok) >= len(inside), (name, len(ok), len(inside))
        for i, r in zip(inside, ok):
            X[i], S[i] = Xr[r], Sr[r]
            if nz is not None:
                nz[i] = nzr[r]
    u0 = controller_u0(params, X)
    ref_h = ref_of(X)
    ref = loss_and_grads(params, X, u0, S, N, row, ref_h, nz)
    p1, p2 = ref["xhat"][:, :, 1], ref["xhat"][:, :, 2]
    active = {"p1_lo": float((p1 < row[1]).mean()), "p1_hi": float((p1 > row[2]).mean()),
              "p2_lo": float((p2 < row[3]).mean()), "p2_hi": float((p2 > row[4]).mean())}
    return {"name": name, "kind": kind, "N": N, "params": params, "X": X, "u0": u0, "states": S, "noise": nz,
            "ref_h": ref_h, "row": row, "terms_kw": kw, "alpha": ALPHA, "ref": ref, "replaced": len(inside),
            "active": active,
            "margin": float(kink_margin(params, X, ref["xhat"], row, ref_h).min())}


@functools.lru_cache(maxsize=None)
def build(name):
    """Case ``name`` of CASES: params, X, u0, states, noise, ref_h (or None), row (the six scalars the restatement ran),
    terms_kw (the keywords of the LossTerms that give that row under alpha = ALPHA), ref (the restatement's fp64
    outputs under test_gpu_parity.run's names), replaced, active (the share of (trajectory, step) pairs in each of the
    four branches), margin. Shared between the tests: do not write to the arrays."""
    s = CASES[name]
    params = {**A.lstm_params(s["H"]), **A.ctrl_params(W)}
    noise = s["kind"] == "C" or s.get("noise", False)
    X, S, nz = synth_inputs(s["B"], s["N"], s["seed"], noise=noise)
    Xr, Sr, nzr = synth_inputs(A.spare(s["B"]), s["N"], s["seed"] + A.REPLACEMENT_SEED, noise=noise)
    c = _make(name, params, X, S, nz, Xr, Sr, nzr, s["kind"], s["N"])
    c["families"], c["H"] = s["families"], s["H"]
    return c


BANK = dict(H=50, M=3, B=17, N=3, seed=4120)


@functools.lru_cache(maxsize=None)
def build_bank():
    """ControllerBank(3, W) on the reference's surrogate, B = 17, N = 3, a sign-flipping ``ref_h (M,B,N)`` and three
    different rows: model 0 case A's kind (quartile bounds, weight and alpha 3.5), model 1 the defaults at alpha 0.5,
    model 2 case D's bounds at weight 2. ``models``: model m as a case of its own."""
    M, B, N = BANK["M"], BANK["B"], BANK["N"]
    lstm = A.lstm_params(BANK["H"])
    X, S, _ = synth_inputs(M * B, N, BANK["seed"])
    Xr, Sr, _ = synth_inputs(M * A.spare(B), N, BANK["seed"] + A.REPLACEMENT_SEED)
    X, S, Xr, Sr = X.reshape(M, B, 3), S.reshape(M, B, 10, 5), Xr.reshape(M, -1, 3), Sr.reshape(M, -1, 10, 5)
    fixed = {1: ((0.5, 0.0, P1_MAX, 0.0, P2_MAX, 1.0), dict(alpha=0.5)),
             2: ((ALPHA, 0.0, math.inf, -math.inf, P2_MAX, 2.0), dict(p1=(0.0, math.inf), p2=(-math.inf, P2_MAX), weight=2.0))}
    models = [_make(f"bank[{m}]", {**lstm, **A.ctrl_params(W, m)}, X[m], S[m], None, Xr[m], Sr[m], None, "C" if m == 0 else "B",
                    N, fixed.get(m)) for m in range(M)]
    stack = lambda k: np.stack([c[k] for c in models])
    return {"lstm": lstm, "ctrls": [A.ctrl_params(W, m) for m in range(M)], "N": N, "X": stack("X"),
            "states": stack("states"), "u0": stack("u0").reshape(M, B, 1), "ref_h": stack("ref_h"), "models": models}


def errors(c, o):
    """Tensor-wide relerr (conftest.relerr) of outputs ``o`` against the restatement's, per output."""
    ref = c["ref"]
    e = {"loss_scalar": abs(float(o["loss_scalar"]) - ref["loss_scalar"]) / abs(ref["loss_scalar"])}
    e.update({k: A.relerr(np.asarray(o[k]).reshape(-1), np.asarray(ref[k]).reshape(-1)) for k in FEATS + GRADS})
    return e


def failures(c, o, tol, f16_tols=None):
    """{output: (error, bound)} of what misses: every tensor-wide relerr <= tol (fp32), or f16_tols = (loss, features,
    gradients), test_gpu_precision's bounds. Empty when the outputs pass."""
    bad = {}
    for k, v in errors(c, o).items():
        bound = tol if f16_tols is None else f16_tols[0 if k == "loss_scalar" else 1 if k in FEATS else 2]
        if not v <= bound:
            bad[k] = (v, bound)
    return bad


def report(c, label, o):
    e = errors(c, o)
    return f"loss_terms {c['name']} {label}: max {max(e.values()):.3g} " + " ".join(f"{k}={v:.3g}" for k, v in e.items())


def mutant_outputs(c, mutant):
    return loss_and_grads(c["params"], c["X"], c["u0"], c["states"], c["N"], c["row"], c["ref_h"], c["noise"], mutant=mutant)
