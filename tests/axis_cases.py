"""Cases that vary what the rollout's C ABI accepts and no other test varies (a helper, not a test; NumPy, torch on the
CPU and the oracles only): the controller's hidden width, ``alpha``, and pre-drawn noise in the H > 52 family.

Every golden fixture, ``kink_cases.CASES`` and the full-size tests run a 50-unit controller at alpha = 20, and noise
only at H = 50. A kernel that compiled one of the three in as a constant would pass them all. :func:`build` makes one
case of :data:`CASES` (or one bank of :data:`BANKS`) from its seeds:

* LSTM weights: the reference's (tests/golden/weights_ref.npz) at H = 50, ``synth_params(H, 1000 + H)`` otherwise;
* controller: the controller part of ``synth_params(16, 500 + w, ctrl_hidden=w)`` (model m of a bank: seed
  ``500 + w + 100 m``);
* inputs: ``synth_inputs(B, N, 3000 + w, noise=...)`` (a bank: ``synth_inputs(M B, ...)``, a slice per model). A
  trajectory whose ``oracle.rollout_torch.kink_margin`` on the fp64 oracle is <= ``BAND`` is replaced by one of
  ``synth_inputs(spare, N, 13000 + w, ...)`` outside the band — the exclusion kink_cases.py makes: an fp32 evaluation
  within its own rounding of a ReLU's kink may take the other slope, whatever its accuracy, and with 52 units a batch
  of 20 already comes that close. Nothing else about the draw changes;
* u0: the fp64 controller on X, rounded to float32;
* every array has been through float32, so a float32 kernel and the fp64 oracle see the same numbers.

tests/test_axis_cases.py holds each case to the conditions a defect on these axes needs to show (activity of the
units, the mutants' sensitivity, both fp64 restatements); tests/test_gpu_axes.py runs the cases through each kernel
family and judges the outputs with :func:`failures` — the comparison lives here so that the CPU test can feed it the
mutants' outputs where the GPU's would go.
"""
import functools

import numpy as np
import torch

from kink_cases import controller_u0, ref_params
from oracle import rollout_np as R
from oracle import rollout_torch as T
from oracle.rollout_torch import kink_margin
from tests.golden.make_golden import synth_inputs, synth_params

ALPHA = 20.0             # UL/Main.py:192, what every other rollout test runs
ALPHA_DEFAULT = 0.1      # MPCLoss() without alpha, the reference's default (Functions.py:1343)
DEAD_BIAS = -10.0        # b_inp of the unit that is dead by construction
BAND = 1e-5              # kink_cases.BAND: an fp32 evaluation this close to a kink may take the other slope
CTRL = ("W_inp", "b_inp", "W_out")
UNIT_GRADS = ("g_W_inp", "g_b_inp", "g_W_out")
FEATS = ("loss", "command", "error", "prediction", "xhat")
GRADS = ("g_u0",) + UNIT_GRADS
F16 = "fused-f16"

_W4 = ("pipe", "onewg", "fused", F16)


def _case(H, w, B, N, families, alpha=ALPHA, noise=False, kind="width", dead=None):
    """alpha None: the GPU call gives MPCLoss no alpha and the oracle runs ALPHA_DEFAULT. kind: which mutants of
    tests/test_axis_cases.py apply ("width": last unit; "alpha": alpha; "noise": noise; "crossed": all three; "n1":
    none, there is no in-loss controller call). dead: the unit whose b_inp becomes DEAD_BIAS."""
    return dict(H=H, w=w, B=B, N=N, families=families, alpha=alpha, noise=noise, kind=kind, dead=dead)


# "small" is the small-batch family in both of its geometries (layer-pipelined and one workgroup per group), "pipe" and
# "onewg" one of them, F16 the fused family in the reduced-precision mode (test_gpu_kinks.run_family's names otherwise).
CASES = {
    # controller width, at alpha = 20 without noise: a failure names its axis
    **{f"h50_w{w}_b20_n3": _case(50, w, 20, 3, _W4) for w in (1, 3, 4, 5, 49, 51, 52)},
    "h50_w52_b20_n12": _case(50, 52, 20, 12, ("pipe", "fused")),            # the window fully self-predicted
    "h32_w7_b20_n3": _case(32, 7, 20, 3, ("small", "fused")),
    "h16_w52_b20_n3": _case(16, 52, 20, 3, ("fused",)),
    **{f"h64_w{w}_b24_n3": _case(64, w, 24, 3, ("wide",)) for w in (1, 7, 52)},
    "h128_w52_b140_n2": _case(128, 52, 140, 2, ("wide",)),                  # ragged second block of 128
    # alpha, at width 50
    "h50_alpha0": _case(50, 50, 20, 3, _W4, alpha=0.0, kind="alpha"),
    "h50_alpha3.5": _case(50, 50, 20, 3, _W4, alpha=3.5, kind="alpha"),
    "h50_alpha_default": _case(50, 50, 20, 3, _W4, alpha=None, kind="alpha"),
    "h64_alpha0": _case(64, 50, 24, 3, ("wide",), alpha=0.0, kind="alpha"),
    "h64_alpha3.5": _case(64, 50, 24, 3, ("wide",), alpha=3.5, kind="alpha"),
    "h64_alpha_default": _case(64, 50, 24, 3, ("wide",), alpha=None, kind="alpha"),
    # pre-drawn noise in the H > 52 family
    "h64_b24_n3_noise": _case(64, 50, 24, 3, ("wide",), noise=True, kind="noise"),
    "h128_b140_n2_noise": _case(128, 50, 140, 2, ("wide",), noise=True, kind="noise"),
    # every axis off its usual value at once: alpha 0.1 with noise
    "h64_w7_crossed": _case(64, 7, 24, 3, ("wide",), alpha=ALPHA_DEFAULT, noise=True, kind="crossed"),
    "h16_w3_crossed": _case(16, 3, 20, 3, ("fused",), alpha=ALPHA_DEFAULT, noise=True, kind="crossed"),
    "h50_w51_crossed_dead": _case(50, 51, 20, 3, ("pipe", "onewg", "fused"), alpha=ALPHA_DEFAULT, noise=True,
                                  kind="crossed", dead=50),
    # N = 1: no controller call inside the loss, the controller gradients are zero
    "h50_w7_b20_n1": _case(50, 7, 20, 1, ("pipe", "onewg", "fused"), kind="n1"),
}

# ControllerBank(M, w) on the reference's surrogate, B = 17 (one full and one ragged group per model), N = 3
BANKS = {f"h50_bank3_w{w}": dict(H=50, w=w, M=3, B=17, N=3) for w in (1, 7, 52)}


def lstm_params(H):
    p = ref_params() if H == 50 else synth_params(H, 1000 + H)
    assert p["Whh"][0].shape[1] == H
    return {k: v for k, v in p.items() if k not in CTRL}


def ctrl_params(w, m=0):
    p = synth_params(16, 500 + w + 100 * m, ctrl_hidden=w)
    return {k: np.array(p[k], np.float64) for k in CTRL}


REPLACEMENT_SEED = 10000   # added to a case's input seed for the draw its replacements come from


def spare(B):
    return max(4, B // 16)


def margins(params, X, S, nz, N, alpha):
    """(u0, kink_margin per trajectory on the fp64 oracle). A trajectory's margin depends on that trajectory alone."""
    u0 = controller_u0(params, X)
    _, feats, _ = R.rollout_forward(params, X, u0, S, N, alpha, None if nz is None else nz.astype(np.float64))
    return u0, kink_margin(params, torch.as_tensor(X), feats["xhat"]).numpy()


def select(params, inputs, replacements, N, alpha):
    """``inputs`` = (X, S, noise) with every trajectory whose kink_margin is <= BAND replaced, in order, by the next of
    ``replacements`` whose margin exceeds it: (X, u0, S, noise, number replaced). A batch with no trajectory in the
    band is returned as it was drawn."""
    X, S, nz = (None if a is None else a.copy() for a in inputs)
    _, m = margins(params, X, S, nz, N, alpha)
    inside = np.flatnonzero(m <= BAND)
    if len(inside):
        Xr, Sr, nzr = replacements
        ok = np.flatnonzero(margins(params, Xr, Sr, nzr, N, alpha)[1] > BAND)
        assert len(ok) >= len(inside), (len(ok), len(inside))
        for i, r in zip(inside, ok):
            X[i], S[i] = Xr[r], Sr[r]
            if nz is not None:
                nz[i] = nzr[r]
    return X, controller_u0(params, X), S, nz, len(inside)


def oracle(params, X, u0, S, N, alpha, noise=None):
    """The fp64 NumPy oracle's results under the names test_gpu_parity.run gives the GPU's, and the tape."""
    nz = None if noise is None else np.asarray(noise, np.float64)
    loss, feats, tape = R.rollout_forward(params, X, u0, S, N, alpha, nz)
    return {"loss_scalar": float(loss), **feats, **R.rollout_backward(params, tape)}, tape


def _finish(name, spec, params, inputs, replacements, alpha):
    N = spec["N"]
    X, u0, S, nz, passed_over = select(params, inputs, replacements, N, alpha)
    ref, tape = oracle(params, X, u0, S, N, alpha, nz)
    t32 = T.loss_and_grads(params, X, u0, S, N, alpha, nz, dtype=torch.float32)
    margin = float(kink_margin(params, torch.as_tensor(X), ref["xhat"]).min())
    z = np.stack([fc[1] for fc in tape["fcaches"]], axis=0) if tape["fcaches"] else np.zeros((0, len(X), spec["w"]))
    unit32 = {k: per_unit(t32[k], ref[k]) for k in UNIT_GRADS}
    return {"name": name, **{k: spec[k] for k in ("H", "w", "N")}, "kind": spec.get("kind", "width"),
            "families": spec.get("families", ("many",)), "dead": spec.get("dead"), "alpha": alpha,
            "alpha_given": spec.get("alpha", ALPHA) is not None, "params": params, "X": X, "u0": u0, "states": S,
            "noise": nz, "passed_over": passed_over, "ref": ref, "z": z, "margin": margin, "unit32": unit32,
            "unit_bound": max(1e-5, 4.0 * max(unit32.values()))}


@functools.lru_cache(maxsize=None)
def build(name):
    """Case ``name`` of CASES with the oracles' results on it: params, X, u0, states, noise (or None), passed_over (the
    trajectories that were replaced), N, alpha (the number the oracle ran; alpha_given False: the GPU call leaves it to MPCLoss), ref (the fp64 oracle's outputs by
    test_gpu_parity.run's names), z (the in-loss controller's fp64 pre-activations, (N - 1, B, w)), margin (the least
    kink_margin of the batch), unit32 (per_unit of the fp32 torch restatement against fp64, per tensor) and unit_bound
    (what :func:`failures` holds the per-unit metric to). Shared between the tests: do not write to the arrays."""
    spec = CASES[name]
    w, B, N = spec["w"], spec["B"], spec["N"]
    params = {**lstm_params(spec["H"]), **ctrl_params(w)}
    if spec["dead"] is not None:
        params["b_inp"][spec["dead"]] = DEAD_BIAS          # before u0 is formed
    inputs = synth_inputs(B, N, 3000 + w, noise=spec["noise"])
    replacements = synth_inputs(spare(B), N, 3000 + w + REPLACEMENT_SEED, noise=spec["noise"])
    return _finish(name, spec, params, inputs, replacements, ALPHA_DEFAULT if spec["alpha"] is None else spec["alpha"])


@functools.lru_cache(maxsize=None)
def build_bank(name):
    """Bank ``name`` of BANKS: the stacked inputs (X (M,B,3), u0 (M,B,1), states (M,B,10,5)), lstm, ctrls, N, and
    ``models``: model m as a case of its own (what :func:`build` returns), on its slice of the inputs."""
    spec = BANKS[name]
    w, M, B, N = spec["w"], spec["M"], spec["B"], spec["N"]
    lstm = lstm_params(spec["H"])
    ctrls = [ctrl_params(w, m) for m in range(M)]
    X, S, _ = synth_inputs(M * B, N, 3000 + w)
    X, S = X.reshape(M, B, 3), S.reshape(M, B, 10, 5)
    Xr, Sr, _ = synth_inputs(M * spare(B), N, 3000 + w + REPLACEMENT_SEED)
    Xr, Sr = Xr.reshape(M, -1, 3), Sr.reshape(M, -1, 10, 5)
    models = [_finish(f"{name}[{m}]", spec, {**lstm, **ctrls[m]}, (X[m], S[m], None), (Xr[m], Sr[m], None), ALPHA)
              for m in range(M)]
    stack = lambda k: np.stack([c[k] for c in models])
    return {"name": name, "w": w, "N": N, "lstm": lstm, "ctrls": ctrls, "X": stack("X"), "states": stack("states"),
            "u0": stack("u0").reshape(M, B, 1), "models": models}


# ---------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------
def relerr(a, b):
    """conftest.relerr: max|a - b| / max|b| per tensor (the absolute error where b is all zero)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a - b).max() if a.size else 0.0)


def per_unit(got, ref):
    """The worst hidden unit of a controller gradient: each unit's row (of g_W_inp (w,3); its entry of g_b_inp (w,) and
    of g_W_out (1,w)) normalised by that row's own fp64 maximum. The tensor-wide metric hides a unit whose gradient is
    small beside the largest unit's. A unit whose fp64 row is all zero must be all zero: anything else counts as inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.ndim == 2 and ref.shape[0] == 1:
        got, ref = got.reshape(-1), ref.reshape(-1)
    if got.shape != ref.shape:
        return float("inf")
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    err, den = np.abs(got - ref).max(1), np.abs(ref).max(1)
    rel = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(rel.max())


def errors(c, o):
    """(tensor-wide relerr per output, per-unit error per controller gradient) of outputs ``o`` against case ``c``."""
    ref = c["ref"]
    wide = {"loss_scalar": abs(float(o["loss_scalar"]) - ref["loss_scalar"]) / abs(ref["loss_scalar"])}
    wide.update({k: relerr(o[k], ref[k]) for k in FEATS + GRADS})
    return wide, {k: per_unit(o[k], ref[k]) for k in UNIT_GRADS}


def failures(c, o, tol, f16_tols=None):
    """What is wrong with outputs ``o`` of case ``c``, as {check: figures}; empty when the outputs pass.

    fp32 (f16_tols None): every tensor-wide relerr <= tol, and every per-unit error <= c["unit_bound"]. f16: f16_tols =
    (loss, features, gradients), the tensor-wide bounds of test_gpu_precision.py; no per-unit bound. Both: the
    gradients have the caller's shapes; at alpha = 0 ``command`` is exactly zero; the dead unit's rows are exactly
    zero."""
    w = c["w"]
    bad = {}
    for k, shape in (("g_W_inp", (w, 3)), ("g_b_inp", (w,)), ("g_W_out", (1, w)), ("g_u0", (len(c["X"]),))):
        if tuple(np.shape(o[k])) != shape:
            bad[f"shape {k}"] = (tuple(np.shape(o[k])), shape)
    if bad:
        return bad
    wide, unit = errors(c, o)
    for k, v in wide.items():
        bound = tol if f16_tols is None else f16_tols[0 if k == "loss_scalar" else 1 if k in FEATS else 2]
        if not v <= bound:
            bad[k] = (v, bound)
    if f16_tols is None:
        bad.update({f"per-unit {k}": (v, c["unit_bound"]) for k, v in unit.items() if not v <= c["unit_bound"]})
    if c["alpha"] == 0.0 and np.any(np.asarray(o["command"]) != 0.0):
        bad["command at alpha 0"] = float(np.abs(o["command"]).max())
    if c["dead"] is not None:
        j = c["dead"]
        rows = {"g_W_inp": np.asarray(o["g_W_inp"])[j], "g_b_inp": np.asarray(o["g_b_inp"])[j],
                "g_W_out": np.asarray(o["g_W_out"])[0, j]}
        bad.update({f"dead unit {k}": float(np.abs(v).max()) for k, v in rows.items() if np.any(v != 0.0)})
    return bad


def report(c, label, o):
    """One line of figures: the worst tensor-wide error, the worst per-unit error with its unit and that unit's size
    beside the tensor's largest, the fp32 restatement's per-unit error and the bound, then every tensor."""
    wide, unit = errors(c, o)
    k = max(unit, key=unit.get)
    rows = lambda a: np.asarray(a, np.float64).reshape(-1, 3 if k == "g_W_inp" else 1)
    ref, got = rows(c["ref"][k]), rows(o[k])
    den = np.abs(ref).max(1)
    j = int(np.argmax(np.abs(got - ref).max(1) / np.where(den > 0, den, 1.0)))
    return (f"axes {c['name']} {label}: max {max(wide.values()):.3g} per-unit {unit[k]:.3g} in {k}[{j}], "
            f"a row {den[j] / den.max() if den.max() > 0 else 0.0:.2g} of the tensor's largest "
            f"(fp32 restatement {max(c['unit32'].values()):.3g}, bound {c['unit_bound']:.3g}) "
            + " ".join(f"{n}={v:.3g}" for n, v in wide.items()))
