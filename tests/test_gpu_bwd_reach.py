"""The fused H <= 52 backward (csrc/fcr_bwd.h) runs only the cells a gradient can reach: every layer phase of window j
stops after t_lo(j) = max(0, 9 - j) (tests/test_bwd_reach_rule.py pins the rule). Every case forces the fused family
(small_batch_limit=0: the default routes B <= 8192 to the small-batch kernels, which run every cell and serve here as
the independent comparator), at every truncation depth, in every tier and mode, and with a forward of the other family
whose records the backward now reads a subset of.
"""
import numpy as np
import pytest

from conftest import load_case, relerr
from oracle import rollout_np as R
from test_gpu_parity import FEATS, GRADS, TOL, _synth, _u0, run
from test_gpu_precision import TOL_FEATS, TOL_GRADS, TOL_LOSS
from test_gpu_small import BIG, _run_mixed

pytestmark = pytest.mark.gpu
FUSED = ("fused", "fused")


@pytest.fixture(scope="module")
def ref_params():
    return load_case("ref_b15_n10")[1]


def _oracle(params, X, u0, S, N):
    loss, f, tape = R.rollout_forward(params, X, u0, S, N, 20.0)
    return float(loss), f, R.rollout_backward(params, tape)


@pytest.mark.parametrize("N", [1, 2, 3, 5, 9, 10, 11, 12])
def test_fp32_every_truncation_depth(ref_params, N):
    """H = 50, B = 33 (three waves, the last one padded): N = 1 is the one-cell window alone, N <= 9 ends at t_lo =
    10 - N, N = 10 .. 12 adds one to three full windows."""
    B = 33
    X, S, _ = _synth(B, N, 700 + N)
    u0 = _u0(ref_params, X)
    o = run(ref_params, X, u0, S, N, 20.0, small_batch_limit=0)
    assert o["families"] == FUSED
    _, _, g = _oracle(ref_params, X, u0, S, N)
    for k, _n in GRADS:
        assert relerr(o[k], g[k]) <= TOL, (N, k, relerr(o[k], g[k]))
    s = run(ref_params, X, u0, S, N, 20.0, small_batch_limit=BIG)
    assert s["families"] == ("small", "small")
    for k, _n in GRADS:
        assert relerr(o[k], s[k]) <= 2e-6, (N, k, relerr(o[k], s[k]))


@pytest.mark.parametrize("name", ["h16_b33_n4", "h32_b16_n6"])
def test_other_tiers(name):
    """HS = 4 (H = 16) and HS = 8 (H = 32) against the golden cases' fp64 values."""
    c, params = load_case(name)
    o = run(params, c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"], small_batch_limit=0)
    assert o["families"] == FUSED
    for k, _n in GRADS:
        assert relerr(o[k], c[f"{k}_64"]) <= TOL, (name, k, relerr(o[k], c[f"{k}_64"]))


@pytest.mark.parametrize("N", [1, 3, 10, 11])
def test_f16_mode(ref_params, N):
    B = 33
    X, S, _ = _synth(B, N, 800 + N)
    u0 = _u0(ref_params, X)
    o = run(ref_params, X, u0, S, N, 20.0, small_batch_limit=0, precision="f16")
    assert o["families"] == FUSED
    loss64, f, g = _oracle(ref_params, X, u0, S, N)
    assert abs(o["loss_scalar"] - loss64) <= TOL_LOSS * abs(loss64)
    for k in FEATS + ("xhat",):
        assert relerr(o[k], f[k]) <= TOL_FEATS, (N, k, relerr(o[k], f[k]))
    for k, _n in GRADS:
        assert relerr(o[k], g[k]) <= TOL_GRADS, (N, k, relerr(o[k], g[k]))


def test_noise_case():
    c, params = load_case("refnoise_b15_n10")
    o = run(params, c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"], small_batch_limit=0)
    assert o["families"] == FUSED
    for k, _n in GRADS:
        assert relerr(o[k], c[f"{k}_64"]) <= TOL, (k, relerr(o[k], c[f"{k}_64"]))


@pytest.mark.parametrize("N", [3, 10])
def test_small_forward_fused_backward(ref_params, N):
    """The fused backward reads a subset of the records the small-batch forward wrote."""
    B = 24
    X, S, _ = _synth(B, N, 850 + N)
    u0 = _u0(ref_params, X)
    o = _run_mixed(ref_params, X, u0, S, N, BIG, 0)
    assert o["families"] == ("small", "fused")
    _, _, g = _oracle(ref_params, X, u0, S, N)
    for k, _n in GRADS:
        assert relerr(o[k], g[k]) <= TOL, (N, k, relerr(o[k], g[k]))


def test_fused_deterministic_and_dloss_linear(ref_params):
    B, N = 4096, 10
    X, S, _ = _synth(B, N, 13)
    u0 = _u0(ref_params, X)
    a = run(ref_params, X, u0, S, N, 20.0, small_batch_limit=0)
    b = run(ref_params, X, u0, S, N, 20.0, small_batch_limit=0)
    c2 = run(ref_params, X, u0, S, N, 20.0, dloss=2.0, small_batch_limit=0)
    assert a["families"] == FUSED and c2["families"] == FUSED
    for k, _n in GRADS:
        assert np.array_equal(a[k], b[k]), k              # fixed-order reductions: bit-reproducible
        assert np.array_equal(2.0 * a[k], c2[k]), k       # exact linearity in the incoming gradient
