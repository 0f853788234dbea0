"""GPU: every axis the rollout's C ABI accepts, in every kernel family, against the fp64 oracle.

The controller's width decides how many of the 13 x 4 controller slots are padding, the strides of the partial-gradient
slabs and the grid of their reduction; ``alpha`` is written out in the command cost and its two gradient terms by each
family itself; the H > 52 family adds the noise in its readout and feeds it to the range guard. Every other rollout test
runs width 50 at alpha = 20, and noise only at H = 50. The cases of tests/axis_cases.py vary each of the three
(tests/test_axis_cases.py: a kernel that compiled one in moves the loss or a gradient by >= 1e-3 on them); here each
case runs in each family its shape reaches, forced there the way tests/test_gpu_kinks.py does, and is judged by
axis_cases.failures: the project's 1e-5 on every output (test_gpu_precision's bounds in the f16 mode), a per-unit bound
on the controller gradients, and the exact properties (shapes, ``command`` at alpha = 0, a dead unit's rows).
"""
import numpy as np
import pytest
import torch

import axis_cases as A
import forging_control_amd as fca
import test_gpu_parity as P
from oracle import rollout_np as R
from test_gpu_kinks import BIG, _with_pipe_limit
from test_gpu_many import forced_onewg, run_many
from test_gpu_parity import DEV, TOL, modules, run
from test_gpu_precision import TOL_FEATS, TOL_GRADS, TOL_LOSS

pytestmark = pytest.mark.gpu
native = fca._native
F16_TOLS = (TOL_LOSS, TOL_FEATS, TOL_GRADS)
OUT = A.FEATS + A.GRADS

PAIRS = [(name, fam) for name, spec in A.CASES.items() for fam in spec["families"]]


class _DefaultAlpha:
    """test_gpu_parity.run always hands MPCLoss an alpha. For the case that is about MPCLoss's own default, ``run`` sees
    this in place of the package: its MPCLoss drops the alpha ``run`` passes, so the constructor's default is what
    reaches the kernels."""

    def __getattr__(self, name):
        return getattr(fca, name)

    @staticmethod
    def MPCLoss(*args, alpha=None, **kw):
        fn = fca.MPCLoss(*args, **kw)
        assert fn.alpha == A.ALPHA_DEFAULT
        return fn


def _run(c, **kw):
    args = (c["params"], c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"])
    if c["alpha_given"]:
        return run(*args, **kw)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(P, "fca", _DefaultAlpha())
        return run(*args, **kw)


def run_family(c, fam):
    """[(label, output, the (forward, backward) family the call must report)] of case ``c`` forced into ``fam``
    (test_gpu_kinks.run_family, plus the f16 mode and, on the H > 52 noise cases, both ends of the keep budget)."""
    B = len(c["X"])
    if fam == "fused":
        return [("fused", _run(c, small_batch_limit=0), ("fused", "fused"))]
    if fam == A.F16:
        return [(A.F16, _run(c, small_batch_limit=0, precision="f16"), ("fused", "fused"))]
    if fam == "wide":
        if c["noise"] is None:
            return [("wide", _run(c), ("wide", "wide"))]
        return [(f"wide keep {b}", _run(c, wide_keep_budget=b), ("wide", "wide")) for b in (0, 1 << 40)]
    outs = []
    if fam in ("pipe", "small"):     # the default: B under the small-batch limit and under the pipe limit
        assert native.small_batch_limit() >= B and native.small_pipe_limit() >= B
        outs.append(("pipe", _run(c), ("small", "small")))
    if fam in ("onewg", "small"):
        outs.append(("onewg", _with_pipe_limit(0, lambda: _run(c, small_batch_limit=BIG)), ("small", "small")))
    return outs


@pytest.mark.parametrize("name,fam", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_axis_case_meets_oracle(name, fam):
    c = A.build(name)
    outs = run_family(c, fam)
    assert outs
    for label, o, families in outs:
        assert o["families"] == families, (name, label, o["families"])
        print(A.report(c, f"{label} -> {'/'.join(o['families'])}", o))
        bad = A.failures(c, o, TOL, F16_TOLS if fam == A.F16 else None)
        assert not bad, (name, label, bad)
        assert o["lstm_grad_untouched"]
    if fam == "wide" and c["noise"] is not None:
        (_, none, _), (_, every, _) = outs
        assert (none["kept_windows"], every["kept_windows"]) == (0, c["N"])
        for k in OUT:
            assert np.array_equal(none[k], every[k]), (name, k)       # kept windows are the recompute's, bit for bit


def _model_outputs(o, m, w):
    """Model m of test_gpu_many.run_many's output under test_gpu_parity.run's names and shapes."""
    return {"loss_scalar": o["loss"][m], "loss": o["cost"][m], **{k: o[k][m] for k in ("command", "error", "xhat", "g_u0")},
            "prediction": o["prediction"][m], "g_W_inp": o["g_W_inp"][m], "g_b_inp": o["g_b_inp"][m],
            "g_W_out": o["g_W_out"][m].reshape(1, w)}


@pytest.mark.parametrize("name", list(A.BANKS), ids=[f"{n}-many" for n in A.BANKS])
def test_bank_case_meets_oracle_and_its_single_model_calls(name):
    """ControllerBank(3, w) in one launch per pass: every model against the fp64 oracle, and bit-equal to its own
    single-model call forced into the one-workgroup family (test_gpu_many has this at width 50, within 1e-6; the bits
    are what DESIGN.md §7.9 records there). Every model is checked before anything is asserted about the oracle."""
    b = A.build_bank(name)
    w = b["w"]
    o = run_many(b["lstm"], b["ctrls"], b["X"], b["u0"], b["states"], b["N"])
    assert o["info"].route == "many" and (o["info"].forward, o["info"].backward) == ("small", "small")
    assert o["g_W_inp"].shape == (3, w, 3) and o["g_b_inp"].shape == (3, w) and o["g_W_out"].shape == (3, w)
    bad = {}
    for m, c in enumerate(b["models"]):
        om = _model_outputs(o, m, w)
        print(A.report(c, "many -> " + "/".join((o["info"].forward, o["info"].backward)), om))
        s = forced_onewg(lambda: _run(c, small_batch_limit=BIG))
        assert s["families"] == ("small", "small")
        assert np.float32(s["loss_scalar"]) == om["loss_scalar"], (name, m)
        for k in OUT:
            assert np.array_equal(np.asarray(om[k]).reshape(-1), np.asarray(s[k]).reshape(-1)), (name, m, k)
        bad.update({(m, k): v for k, v in A.failures(c, om, TOL).items()})
    assert not bad, (name, bad)


def test_enable_noise_draws_reference_stream_in_the_wide_family():
    """test_gpu_parity.test_enable_noise_draws_reference_stream at H = 64: enable_noise with no ``noise`` draws
    randn(B, 4) * 0.01 once per horizon step in order (Functions.py:1401, 1439), so under one seed it equals the call
    given the same draws — which must also be the fp64 oracle's rollout under them."""
    c = A.build("h64_b24_n3_noise")
    B, N = len(c["X"]), c["N"]
    sim, ctrl = modules(c["params"])
    d = lambda a: torch.as_tensor(a, device=DEV)
    fn = fca.MPCLoss(N, c["alpha"])
    torch.manual_seed(123)
    l1, f1 = fn(sim, ctrl, d(c["X"]), d(c["u0"]).reshape(-1, 1), d(c["states"]), DEV, enable_noise=True)
    x1, fam1 = fn.last_trajectory, (fn.last_call.forward, fn.last_call.backward)
    torch.manual_seed(123)
    nz = torch.stack([torch.randn(B, 4, device=DEV) * 0.01 for _ in range(N)], dim=1)
    l2, f2 = fn(sim, ctrl, d(c["X"]), d(c["u0"]).reshape(-1, 1), d(c["states"]), DEV, noise=nz, enable_noise=True)
    assert fam1[0] == "wide" and fn.last_call.forward == "wide"
    assert torch.equal(l1, l2) and torch.equal(x1, fn.last_trajectory)
    for k in ("loss", "command", "error", "prediction"):
        assert torch.equal(f1[k], f2[k]), k
    _, feats, _ = R.rollout_forward(c["params"], c["X"], c["u0"], c["states"], N, c["alpha"],
                                    nz.cpu().numpy().astype(np.float64))
    errs = {k: A.relerr(f1[k].cpu().numpy(), feats[k]) for k in ("loss", "command", "error", "prediction")}
    errs["xhat"] = A.relerr(x1.cpu().numpy(), feats["xhat"])
    print("axes enable_noise h64:", " ".join(f"{k}={v:.3g}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    assert A.relerr(x1.cpu().numpy(), c["ref"]["xhat"]) > 1e-3          # and they are other draws than the case's
