"""CPU: the kink stress cases (tests/kink_cases.py) reach every branch of the loss, and a broken branch shows.

Per-branch coverage of the pressure constraint's four ReLUs and of the in-loss controller's Hardtanh: every case keeps
each of the nine states above the floor with at most 5 % of its candidates removed, and seven mutants of the fp64
oracle — one branch broken each — move the loss or a gradient by at least 1e-3, a hundred times the 1e-5 the kernels are
held to on the same cases (tests/test_gpu_kinks.py). A kernel that carries one of these defects cannot pass there.
"""
import numpy as np
import pytest

import kink_cases as K
from conftest import load_case, relerr
from oracle import rollout_np as R

MOVED = 1e-3
GRADS = ("g_u0", "g_W_inp", "g_b_inp", "g_W_out")


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_meets_floor_and_removal_cap(name):
    c = K.build(name)
    print(name, "removed", c["removed"], "of", c["candidates"], "max|xhat|", c["max_abs_xhat"], c["shares"])
    K.check(c)
    assert len(c["X"]) == c["candidates"] - c["removed"]
    assert c["max_abs_xhat"] < 100.0                       # far inside the f16 split's range: no range guard here
    # the in-loss saturation is counted from v, not from `prediction` (whose first entry per trajectory is u0)
    lo, hi = K.in_loss_saturated(c["params"], c["X"], c["u0"], c["states"], c["N"],
                                 None if c["noise"] is None else c["noise"].astype(np.float64))
    pairs = len(c["X"]) * (c["N"] - 1)
    assert lo >= K.FLOOR * pairs and hi >= K.FLOOR * pairs, (name, lo, hi, pairs)


# ---------------------------------------------------------------------------------------------
# mutants: the fp64 oracle with one branch broken
# ---------------------------------------------------------------------------------------------
def _drop_low(col):
    """_constraint and _constraint_grad without the ReLU(-p) term of column ``col``."""
    other = 3 - col

    def con(xh):
        p1, p2, q = xh[:, 1], xh[:, 2], xh[:, other]
        return np.maximum(-q, 0.0) + np.maximum(p1 - R.P1_MAX, 0.0) + np.maximum(p2 - R.P2_MAX, 0.0)

    def grad(xh):
        p1, p2 = xh[:, 1], xh[:, 2]
        g = np.zeros_like(xh)
        g[:, 1] = 1.0 * (p1 - R.P1_MAX > 0)
        g[:, 2] = 1.0 * (p2 - R.P2_MAX > 0)
        g[:, other] += -1.0 * (-xh[:, other] > 0)
        return g

    return con, grad


def _fnn_forward_clamped(lo, hi):
    def fnn_forward(x, W_inp, b_inp, W_out):
        z = x @ W_inp.T + b_inp
        a = np.maximum(z, 0.0)
        v = a @ W_out[0]
        return np.clip(v, lo, hi), (x, z, a, v)
    return fnn_forward


def _fnn_backward_unmasked(du, cache, W_inp, W_out):
    x, z, a, v = cache
    dz = (du[:, None] * W_out[0][None, :]) * (z > 0.0)
    return dz @ W_inp, dz.T @ x, dz.sum(0), (du[:, None] * a).sum(0)[None, :]


def _swap_p1(mp):
    mp.setattr(R, "P1_MAX", R.P2_MAX)


def _swap_p2(mp):
    mp.setattr(R, "P2_MAX", R.P1_MAX)


def _no_p1_low(mp):
    con, grad = _drop_low(1)
    mp.setattr(R, "_constraint", con)
    mp.setattr(R, "_constraint_grad", grad)


def _no_p2_low(mp):
    con, grad = _drop_low(2)
    mp.setattr(R, "_constraint", con)
    mp.setattr(R, "_constraint_grad", grad)


MUTANTS = {
    "P1_MAX:=P2_MAX": _swap_p1,
    "P2_MAX:=P1_MAX": _swap_p2,
    "no p1<0 term": _no_p1_low,
    "no p2<0 term": _no_p2_low,
    "no Hardtanh mask": lambda mp: mp.setattr(R, "fnn_backward", _fnn_backward_unmasked),
    "no clamp at -1": lambda mp: mp.setattr(R, "fnn_forward", _fnn_forward_clamped(-np.inf, 1.0)),
    "no clamp at +1": lambda mp: mp.setattr(R, "fnn_forward", _fnn_forward_clamped(-1.0, np.inf)),
}


def moved_by(c, mutate):
    """The largest relerr of the mutant's loss and gradients against the oracle's, on the batch the case runs. u0 is
    data here (the caller's controller computed it outside the loss), so a broken controller acts inside the loss only."""
    with pytest.MonkeyPatch.context() as mp:
        mutate(mp)
        nz = None if c["noise"] is None else c["noise"].astype(np.float64)
        loss, _, tape = R.rollout_forward(c["params"], c["X"], c["u0"], c["states"], c["N"], c["alpha"], nz)
        g = R.rollout_backward(c["params"], tape)
    return max([relerr(loss, c["loss"])] + [relerr(g[k], c["grads"][k]) for k in GRADS])


@pytest.mark.parametrize("mutant", list(MUTANTS))
@pytest.mark.parametrize("name", list(K.CASES))
def test_every_mutant_moves_the_loss_or_a_gradient(name, mutant):
    c = K.build(name)
    moved = moved_by(c, MUTANTS[mutant])
    print(name, mutant, f"{moved:.3g}")
    assert moved >= MOVED, (name, mutant, moved)
    # and the patch is gone: the oracle reproduces itself
    nz = None if c["noise"] is None else c["noise"].astype(np.float64)
    assert R.rollout_forward(c["params"], c["X"], c["u0"], c["states"], c["N"], c["alpha"], nz)[0] == c["loss"]


def test_golden_stress_fixture_never_saturates_inside_the_loss():
    """Why this file exists: on ref_wide_b64_n10, the fixture whose ``u_saturated`` test_oracle.py asserts > 0, every
    saturated command is u0 — the caller's controller, outside the loss. The in-loss v never reaches +-1 there, and
    p1 never exceeds P1_MAX."""
    c, params = load_case("ref_wide_b64_n10")
    _, feats, tape = R.rollout_forward(params, c["X"], c["u0"], c["states"], c["N"], c["alpha"])
    v = K.in_loss_v(tape)
    assert v.shape == (c["B"], c["N"] - 1) and np.abs(v).max() < 1.0
    pred = feats["prediction"].reshape(c["B"], c["N"])
    assert c["u_saturated"] == int((np.abs(pred[:, 0]) >= 1.0).sum()) > 0
    assert (feats["xhat"][..., 1] > R.P1_MAX).sum() == 0
