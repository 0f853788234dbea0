"""GPU: every kink of the MPC loss in every rollout kernel family, against the fp64 oracle.

The pressure constraint's four ReLUs and the in-loss controller's Hardtanh (clamp and backward mask) are written out
once per kernel family: fcr_fwd.h / fcr_bwd.h (fused), fcr_small.h (one workgroup per group), fcr_pipe.h (layer
pipelined) and fcr_wide.h (H > 52). The stress cases of tests/kink_cases.py put at least 5 % of the (trajectory, step)
pairs on each side of each kink (tests/test_kink_cases.py: the floors, and that a broken branch moves the loss or a
gradient by >= 1e-3); here each case runs in each family its shape can reach and must meet the project's 1e-5 bar over
the whole batch that is run, with no mask.
"""
import numpy as np
import pytest

import forging_control_amd as fca
import kink_cases as K
from conftest import relerr
from test_gpu_parity import FEATS, GRADS, TOL, run
from test_gpu_precision import TOL_FEATS, TOL_LOSS

pytestmark = pytest.mark.gpu
native = fca._native
BIG = 1 << 30

PAIRS = [(name, fam) for name, case in K.CASES.items() for fam in case[-1]]


def _with_pipe_limit(lim, fn):
    prev = native.set_small_pipe_limit(lim)
    try:
        return fn()
    finally:
        native.set_small_pipe_limit(prev)


def _run(c, **kw):
    return run(c["params"], c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"], **kw)


def run_family(c, fam):
    """[(label, output, the (forward, backward) family the call must report)] of case ``c`` forced into ``fam``."""
    B = len(c["X"])
    if fam == "fused":
        return [("fused", _run(c, small_batch_limit=0), ("fused", "fused"))]
    if fam == "wide":
        return [("wide", _run(c), ("wide", "wide"))]
    outs = []
    if fam in ("pipe", "small"):     # the default: B under the small-batch limit and under the pipe limit
        assert native.small_batch_limit() >= B and native.small_pipe_limit() >= B
        outs.append(("pipe", _run(c), ("small", "small")))
    if fam in ("onewg", "small"):
        outs.append(("onewg", _with_pipe_limit(0, lambda: _run(c, small_batch_limit=BIG)), ("small", "small")))
    return outs


@pytest.mark.parametrize("name,fam", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_kink_case_meets_oracle(name, fam):
    c = K.build(name)
    K.check(c)
    outs = run_family(c, fam)
    assert outs
    for label, o, families in outs:
        assert o["families"] == families, (name, label, o["families"])
        errs = {"loss_scalar": abs(o["loss_scalar"] - c["loss"]) / abs(c["loss"])}
        errs.update({k: relerr(o[k], c["feats"][k]) for k in FEATS + ("xhat",)})
        errs.update({k: relerr(o[k], c["grads"][k]) for k, _ in GRADS})
        print(f"kinks {name} {label}: B={len(c['X'])} max {max(errs.values()):.3g} "
              + " ".join(f"{k}={v:.3g}" for k, v in errs.items()))
        bad = {k: v for k, v in errs.items() if not v <= TOL}
        assert not bad, (name, label, bad)


def test_kink_case_f16_forward():
    """The reduced-precision mode on the first stress case, fused family: the forward outputs only (loss, features,
    x̂) at test_gpu_precision's bounds. The gradients are left out on purpose: the mode's forward error (up to 6e-3)
    puts a large share of a stressed batch within reach of a kink, and a flipped mask changes a slope by O(1) — no
    bound on them would say anything about the kernel. The backward's mask code is the fp32 instance's template,
    which the fp32 cases above cover."""
    c = K.build(next(iter(K.CASES)))
    o = _run(c, small_batch_limit=0, precision="f16")
    assert o["families"] == ("fused", "fused")
    errs = {k: relerr(o[k], c["feats"][k]) for k in FEATS + ("xhat",)}
    eloss = abs(o["loss_scalar"] - c["loss"]) / abs(c["loss"])
    print(f"kinks f16 forward: loss {eloss:.3g} " + " ".join(f"{k}={v:.3g}" for k, v in errs.items()))
    assert eloss <= TOL_LOSS, eloss
    bad = {k: v for k, v in errs.items() if not v <= TOL_FEATS}
    assert not bad, bad
    assert np.isfinite(o["g_u0"]).all()
