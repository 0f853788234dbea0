"""Stress cases that drive every kink of the MPC loss (a helper, not a test; NumPy and the oracles only).

The rollout loss is piecewise linear in the pressure constraint (four ReLUs, Functions.py:1411, :1449) and in the
in-loss controller's Hardtanh (:287). On the inputs of the golden fixtures and of ``synth_inputs`` the p1 > P1_MAX
branch and the in-loss Hardtanh clamp never fire, and on the synthetic H > 52 weights every constraint mask is constant
over the batch. :func:`calibrate` moves the readout rows of the pressures and the controller's output layer so that the
quartiles of the fp64 oracle's p1, p2 and pre-Hardtanh ``v`` sit on the kinks; :func:`build` makes one case of
:data:`CASES` from its seeds and checks, on the fp64 oracle alone, the conditions a case must meet:

* coverage floor: each of the nine states of :func:`shares` holds at least ``FLOOR`` of the (trajectory, step) pairs of
  the batch that is run (with the noise on where the case has noise);
* the only exclusion: candidates whose ``oracle.rollout_torch.kink_margin`` is <= ``BAND`` are removed before
  anything runs — an fp32 evaluation within its own rounding of a kink may take the other slope, whatever its
  accuracy — and at most ``MAX_REMOVED`` of the candidates may go; the parameters are not recalibrated afterwards.

tests/test_kink_cases.py holds every case to these and to the mutants' sensitivity; tests/test_gpu_kinks.py runs the
cases through each kernel family.
"""
import functools
import os

import numpy as np
import torch

from oracle import rollout_np as R
from oracle.rollout_torch import kink_margin
from tests.golden.make_golden import synth_inputs, synth_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHA = 20.0          # UL/Main.py:192
ROUNDS = 4
FLOOR = 0.05          # smallest share of each of the nine states
BAND = 1e-5           # kink_margin at or below which a candidate is removed
MAX_REMOVED = 0.05    # largest share of the candidates that may be removed
STATES = ("p1<0", "p1 in", "p1>max", "p2<0", "p2 in", "p2>max", "v<=-1", "v in", "v>=1")

# name: (H, B, N, weights, noise, seed of synth_inputs, families the GPU test forces). "small" is the small-batch
# family in both of its geometries (layer-pipelined and one workgroup per group); "pipe" and "onewg" name one of them.
CASES = {
    "h50_b48_n6": (50, 48, 6, "ref", False, 2003, ("pipe", "onewg", "fused")),
    "h50_b48_n6_noise": (50, 48, 6, "ref", True, 2003, ("pipe", "onewg", "fused")),
    "h50_b33_n11": (50, 33, 11, "ref", False, 2001, ("pipe", "fused")),
    "h50_b20_n12": (50, 20, 12, "ref", False, 2000, ("fused",)),
    "h50_b300_n3": (50, 300, 3, "ref", False, 2005, ("onewg", "fused")),
    "h16_b48_n4": (16, 48, 4, "synth", False, 2002, ("fused",)),
    "h32_b48_n4": (32, 48, 4, "synth", False, 2000, ("small", "fused")),
    "h40_b48_n4": (40, 48, 4, "synth", False, 2001, ("small", "fused")),
    "h52_b20_n3": (52, 20, 3, "synth", False, 2000, ("small", "fused")),
    "h64_b48_n4": (64, 48, 4, "synth", False, 2000, ("wide",)),
    "h128_b140_n3": (128, 140, 3, "synth", False, 2005, ("wide",)),
    "h264_b130_n2": (264, 130, 2, "synth", False, 2000, ("wide",)),
}


def ref_params():
    """The reference's trained weights (tests/golden/weights_ref.npz), as the oracle's fp64 parameter dict."""
    w = np.load(os.path.join(GOLDEN, "weights_ref.npz"))
    f64 = lambda a: np.asarray(a, np.float64)
    return {"Wih": [f64(w[f"Wih{k}"]) for k in range(3)], "Whh": [f64(w[f"Whh{k}"]) for k in range(3)],
            **{k: f64(w[k]) for k in ("fcW", "fcb", "W_inp", "b_inp", "W_out")}}


def copy_params(params):
    return {k: [np.array(a, np.float64) for a in v] if isinstance(v, list) else np.array(v, np.float64)
            for k, v in params.items()}


def controller_u0(params, X):
    """u0 = controller(X), the caller's command that enters the loss as data, as float32."""
    u, _ = R.fnn_forward(np.asarray(X, np.float64), params["W_inp"], params["b_inp"], params["W_out"])
    return u.astype(np.float32)


def in_loss_v(tape):
    """The pre-Hardtanh outputs of the controller evaluations inside the loss, (B, N - 1): u0 is not among them."""
    B = tape["B"]
    return np.stack([fc[3] for fc in tape["fcaches"]], axis=1) if tape["fcaches"] else np.zeros((B, 0))


def calibrate(params, X, S, N_cal):
    """A copy of ``params`` whose data put the quartiles of p1, p2 and of the in-loss ``v`` on the kinks.

    Controller hidden unit 0 becomes the constant 1 (W_inp[0] = 0, b_inp[0] = 1), so W_out[0, 0] is an output bias.
    Each of ROUNDS rounds runs the fp64 oracle over ``N_cal`` steps of the same inputs, then maps the quartiles of
    x̂[..., r] (r = 1, 2, over all trajectories and steps) to 0 and P1_MAX / P2_MAX through readout row r, and those of
    the in-loss v to -1 and +1 through W_out and its bias. The two interact (the pressures feed back through the
    window, v through the command), hence the rounds. At the end every array is rounded through float32, so a float32
    kernel and the oracle see the same numbers."""
    p = copy_params(params)
    p["W_inp"][0] = 0.0
    p["b_inp"][0] = 1.0
    p["W_out"][0, 0] = 0.0
    for _ in range(ROUNDS):
        _, feats, tape = R.rollout_forward(p, X, controller_u0(p, X), S, N_cal, ALPHA)
        for r, pmax in ((1, R.P1_MAX), (2, R.P2_MAX)):
            lo, hi = np.quantile(feats["xhat"][..., r], (0.25, 0.75))
            a = pmax / (hi - lo)
            p["fcW"][r] *= a
            p["fcb"][r] = a * (p["fcb"][r] - lo)
        lo, hi = np.quantile(in_loss_v(tape), (0.25, 0.75))
        s = 2.0 / (hi - lo)
        bias = p["W_out"][0, 0]
        p["W_out"] *= s
        p["W_out"][0, 0] = s * (bias - lo) - 1.0
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return {k: [f32(a) for a in v] if isinstance(v, list) else f32(v) for k, v in p.items()}


def shares(params, X, u0, S, N, noise=None):
    """The share of (trajectory, step) pairs in each of the nine STATES on the fp64 oracle: p1 and p2 below 0, inside,
    above their bound over the N predictions; the in-loss v at or below -1, inside, at or above +1 over the N - 1
    controller evaluations inside the loss."""
    _, feats, tape = R.rollout_forward(params, X, u0, S, N, ALPHA, noise)
    out = {}
    for name, r, pmax in (("p1", 1, R.P1_MAX), ("p2", 2, R.P2_MAX)):
        x = feats["xhat"][..., r]
        out[f"{name}<0"], out[f"{name}>max"] = float((x < 0).mean()), float((x > pmax).mean())
        out[f"{name} in"] = 1.0 - out[f"{name}<0"] - out[f"{name}>max"]
    v = in_loss_v(tape)
    out["v<=-1"], out["v>=1"] = float((v <= -1).mean()), float((v >= 1).mean())
    out["v in"] = 1.0 - out["v<=-1"] - out["v>=1"]
    return out


def in_loss_saturated(params, X, u0, S, N, noise=None):
    """How many controller evaluations inside the loss saturate, counted from v (``prediction`` also holds u0)."""
    _, _, tape = R.rollout_forward(params, X, u0, S, N, ALPHA, noise)
    v = in_loss_v(tape)
    return int((v <= -1).sum()), int((v >= 1).sum())


@functools.lru_cache(maxsize=None)
def build(name, seed=None):
    """The case ``name`` of CASES (or the same case from another ``seed``), with the oracle's results on it:
    params, X, u0, states, N, alpha, noise (or None) of the batch that is run; candidates, removed; shares; loss,
    feats and grads of the fp64 oracle. The arrays are shared between the tests: do not write to them."""
    H, B, N, weights, noisy, seed0, families = CASES[name]
    seed = seed0 if seed is None else seed
    base = ref_params() if weights == "ref" else synth_params(H, 1000 + H)
    assert base["Whh"][0].shape[1] == H
    X, S, nz = synth_inputs(B, N, seed, noise=noisy)
    params = calibrate(base, X, S, min(N, 4))
    u0 = controller_u0(params, X)
    nz64 = None if nz is None else nz.astype(np.float64)
    _, feats, _ = R.rollout_forward(params, X, u0, S, N, ALPHA, nz64)
    margin = kink_margin(params, torch.as_tensor(X), feats["xhat"]).numpy()
    keep = margin > BAND
    X, S, u0 = X[keep], S[keep], u0[keep]
    nz, nz64 = (None, None) if nz is None else (nz[keep], nz64[keep])
    loss, feats, tape = R.rollout_forward(params, X, u0, S, N, ALPHA, nz64)
    return {"name": name, "H": H, "N": N, "alpha": ALPHA, "families": families, "params": params, "X": X, "u0": u0,
            "states": S, "noise": nz, "candidates": B, "removed": int(B - keep.sum()),
            "shares": shares(params, X, u0, S, N, nz64), "max_abs_xhat": float(np.abs(feats["xhat"]).max()),
            "loss": loss, "feats": feats, "grads": R.rollout_backward(params, tape)}


def check(case):
    """The conditions of the module docstring on a built case; raises AssertionError with the figures."""
    assert case["removed"] <= MAX_REMOVED * case["candidates"], (case["name"], case["removed"], case["candidates"])
    low = {k: v for k, v in case["shares"].items() if v < FLOOR}
    assert set(case["shares"]) == set(STATES) and not low, (case["name"], low)
