"""GPU: the loss's terms as data (MPCLoss(terms=...), forward(..., ref_horizon=...)) in every kernel family.

The cases of tests/loss_terms_ref.py — bounds at the quartiles of the predictions with weight and alpha 3.5 (A), a
reference that changes sign in mid-horizon (B), both with noise (C), infinite bounds (D) — run in each family their
shape reaches, forced there the way tests/test_gpu_axes.py does, against the fp64 restatement at the project's 1e-5
(test_gpu_precision's bounds in the f16 mode); tests/test_loss_terms_host.py shows that comparison refusing every
mutant. Then the bit-equalities: default terms are no terms, a materialised constant preview is no preview, a bank model
is its single-model one-workgroup call under its own row, a shared row is the row repeated, a model's row is its own
business, both routes of forward_many agree; and training: per-model alpha in train_models against separate runs, a
replayed CapturedStep with terms against eager.
"""
import copy

import numpy as np
import pytest
import torch

import axis_cases as A
import forging_control_amd as fca
import loss_terms_ref as L
from forging_control_amd.loss_terms import LossTerms
from test_gpu_kinks import BIG, _with_pipe_limit
from test_gpu_many import forced_onewg, make_bank, simulator
from test_gpu_parity import DEV, GRADS, TOL, modules
from test_gpu_precision import TOL_FEATS, TOL_GRADS, TOL_LOSS

pytestmark = pytest.mark.gpu
native = fca._native
F16_TOLS = (TOL_LOSS, TOL_FEATS, TOL_GRADS)
OUT = L.FEATS + L.GRADS
PAIRS = [(name, fam) for name, spec in L.CASES.items() for fam in spec["families"]]
d = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)


def run(c, terms="case", preview="case", **loss_kw):
    """test_gpu_parity.run on case ``c`` with its LossTerms ("case"; None: no terms; or a LossTerms) and its ref_h
    ("case"; None: no preview; or a tensor)."""
    sim, ctrl = modules(c["params"])
    u0_t = d(c["u0"]).reshape(-1, 1).requires_grad_(True)
    if terms == "case":
        terms = LossTerms(**c["terms_kw"])
    if terms is not None:
        loss_kw["terms"] = terms
    fn = fca.MPCLoss(prediction_horizon=c["N"], alpha=c["alpha"], **loss_kw)
    kw = {}
    if isinstance(preview, str):
        preview = None if c["ref_h"] is None else d(c["ref_h"])
    if preview is not None:
        kw["ref_horizon"] = preview
    loss, feats = fn(sim, ctrl, d(c["X"]), u0_t, d(c["states"]), DEV, enable_noise=c["noise"] is not None,
                     noise=None if c["noise"] is None else d(c["noise"]), **kw)
    loss.backward()
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy() for k, v in feats.items()}
    out["loss_scalar"] = loss.item()
    out["xhat"] = fn.last_trajectory.cpu().numpy()
    out["g_u0"] = u0_t.grad.reshape(-1).cpu().numpy()
    for k, name in GRADS[1:]:
        mod, attr = name.split(".")
        out[k] = getattr(getattr(ctrl, mod), attr).grad.cpu().numpy()
    out["families"] = (fn.last_call.forward, fn.last_call.backward)
    assert all(p.grad is None for p in sim.parameters())
    return out


def run_family(c, fam, **kw):
    """[(label, output, the families the call must report)] of ``c`` forced into ``fam`` (test_gpu_axes.run_family)."""
    B = len(c["X"])
    if fam == "fused":
        return [("fused", run(c, small_batch_limit=0, **kw), ("fused", "fused"))]
    if fam == A.F16:
        return [(A.F16, run(c, small_batch_limit=0, precision="f16", **kw), ("fused", "fused"))]
    if fam == "wide":
        return [("wide", run(c, **kw), ("wide", "wide"))]
    if fam == "pipe":
        assert native.small_batch_limit() >= B and native.small_pipe_limit() >= B
        return [("pipe", run(c, **kw), ("small", "small"))]
    assert fam == "onewg"
    return [("onewg", _with_pipe_limit(0, lambda: run(c, small_batch_limit=BIG, **kw)), ("small", "small"))]


@pytest.mark.parametrize("name,fam", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_case_meets_the_restatement(name, fam):
    c = L.build(name)
    for label, o, families in run_family(c, fam):
        assert o["families"] == families, (name, label, o["families"])
        print(L.report(c, f"{label} -> {'/'.join(o['families'])}", o))
        bad = L.failures(c, o, TOL, F16_TOLS if fam == A.F16 else None)
        assert not bad, (name, label, bad)


def _same_bits(a, b, what):
    assert np.float32(a["loss_scalar"]) == np.float32(b["loss_scalar"]), what
    for k in OUT:
        assert np.array_equal(a[k], b[k]), (what, k)


DEFAULTS = [("B_h50_b20_n12", f) for f in ("pipe", "onewg", "fused", A.F16)] + [("A_h24_b33_n4", "pipe"), ("A_h24_b33_n4", "fused"),
                                                                               ("D_h64_b24_n3", "wide")]


@pytest.mark.parametrize("name,fam", DEFAULTS, ids=[f"{n}-{f}" for n, f in DEFAULTS])
def test_default_terms_and_a_constant_preview_leave_the_bits(name, fam):
    """MPCLoss(terms=LossTerms()) is MPCLoss(), and ref_horizon = X[:, 2] materialised over the horizon is no preview:
    the same bits, in every family (the calls with terms run fcr_forward_terms / fcr_backward_terms)."""
    c = L.build(name)
    (_, base, fams), = run_family(c, fam, terms=None, preview=None)
    (_, dflt, _), = run_family(c, fam, terms=LossTerms(), preview=None)
    X = d(c["X"])
    (_, mat, _), = run_family(c, fam, terms=None, preview=X[:, 2:3].expand(len(c["X"]), c["N"]).contiguous())
    assert base["families"] == fams
    _same_bits(base, dflt, "default terms")
    _same_bits(base, mat, "materialised preview")
    (_, case, _), = run_family(c, fam)
    assert case["loss_scalar"] != base["loss_scalar"]     # and the case's own terms / preview are something else


# ---------------------------------------------------------------------------------------------------------------------
# the bank
# ---------------------------------------------------------------------------------------------------------------------
def run_bank(b, terms, preview=True, **loss_kw):
    sim, bank = simulator(b["lstm"]), make_bank(b["ctrls"])
    M = len(b["ctrls"])
    u0_t = d(b["u0"]).reshape(M, -1, 1).requires_grad_(True)
    loss_kw.setdefault("many_min_models", 1)
    fn = fca.MPCLoss(prediction_horizon=b["N"], alpha=L.ALPHA, terms=terms, **loss_kw)
    losses, f = fn.forward_many(sim, bank, d(b["X"]), u0_t, d(b["states"]), DEV,
                                ref_horizon=d(b["ref_h"]) if preview else None)
    losses.sum().backward()
    torch.cuda.synchronize()
    n = lambda t: t.detach().cpu().numpy()
    w = bank.hidden
    out = [{"loss_scalar": n(losses)[m], "loss": n(f["loss"])[m], "command": n(f["command"])[m], "error": n(f["error"])[m],
            "prediction": n(f["prediction"])[m], "xhat": n(fn.last_trajectory)[m], "g_u0": n(u0_t.grad)[m].reshape(-1),
            "g_W_inp": n(bank.w_inp.grad)[m], "g_b_inp": n(bank.b_inp.grad)[m], "g_W_out": n(bank.w_out.grad)[m].reshape(1, w)}
           for m in range(M)]
    return out, fn.last_call


def test_bank_models_run_under_their_own_rows_in_one_launch():
    b = L.build_bank()
    terms = [LossTerms(**c["terms_kw"]) for c in b["models"]]
    outs, info = run_bank(b, terms)
    assert info.route == "many" and (info.forward, info.backward) == ("small", "small")
    bad = {}
    for m, c in enumerate(b["models"]):
        print(L.report(c, "many", outs[m]))
        bad.update({(m, k): v for k, v in L.failures(c, outs[m], TOL).items()})
        # model m is its single-model one-workgroup call under its own row, bit for bit
        s = forced_onewg(lambda: run(c, small_batch_limit=BIG))
        assert s["families"] == ("small", "small")
        _same_bits(outs[m], s, f"model {m} against its single call")
    assert not bad, bad
    # both routes of forward_many agree (the loop through the one-workgroup family: the same program on the same rows)
    loop, linfo = forced_onewg(lambda: run_bank(b, terms, many_min_models=99, small_batch_limit=BIG))
    assert linfo.route == "loop" and len(linfo.calls) == 3
    for m in range(3):
        _same_bits(outs[m], loop[m], f"route loop, model {m}")
    # changing model 1's row leaves model 0's (and 2's) bits, and moves model 1
    moved, _ = run_bank(b, [terms[0], terms[1].replace(alpha=9.0, weight=0.25), terms[2]])
    _same_bits(outs[0], moved[0], "model 0 under another row of model 1")
    _same_bits(outs[2], moved[2], "model 2 under another row of model 1")
    assert moved[1]["loss_scalar"] != outs[1]["loss_scalar"]


def test_a_shared_row_is_the_row_repeated():
    b = L.build_bank()
    t = LossTerms(**b["models"][0]["terms_kw"])
    shared, info = run_bank(b, t)
    repeated, _ = run_bank(b, [t, t, t])
    assert info.route == "many"
    for m in range(3):
        _same_bits(shared[m], repeated[m], f"shared row, model {m}")
    none, _ = run_bank(b, None, preview=False)
    dflt, _ = run_bank(b, LossTerms(), preview=False)
    for m in range(3):
        _same_bits(none[m], dflt[m], f"default terms, model {m}")
    assert none[0]["loss_scalar"] != shared[0]["loss_scalar"]


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def test_train_models_with_per_model_alpha_matches_separate_runs():
    """test_gpu_many.test_train_models_matches_separate_runs with a row per model (alpha 0.1 / 3.5 / 20, and bounds and
    a weight off their defaults) and a preview: three AdamW steps, every parameter within 1e-6 of its tensor's max."""
    from test_gpu_many import _train_setup
    M, B, N = 3, 15, 10
    c, sim, batches = _train_setup(M, B, 3)
    batches = [(X, y, z, torch.cat((X[:, :, 2:3].expand(M, B, N // 2), -X[:, :, 2:3].expand(M, B, N - N // 2)), dim=2).contiguous())
               for X, y, z in batches]
    terms = [LossTerms(alpha=0.1), LossTerms(p1=(0.1, 0.4), p2=(0.05, 0.3), weight=3.5, alpha=3.5), LossTerms(alpha=20.0, weight=2.0)]
    bank = make_bank(c["ctrls"])
    fn = fca.MPCLoss(prediction_horizon=N, alpha=7.0, many_min_models=1, terms=terms)
    opt = torch.optim.AdamW(bank.parameters(), lr=1e-4)
    avg, feats = fca.NeuralNetwork.train_models(batches, sim, bank, fn, opt, DEV)
    assert fn.last_call.route == "many" and feats["loss"].shape == (M, 3 * B)
    for m in range(M):
        ctrl = modules({**c["lstm"], **c["ctrls"][m]})[1]
        o = torch.optim.AdamW(ctrl.parameters(), lr=1e-4)
        single = fca.MPCLoss(prediction_horizon=N, alpha=7.0, terms=terms[m])
        l, f = fca.NeuralNetwork.train_model([(X[m], y[m], z[m], r[m]) for X, y, z, r in batches], sim, ctrl, single, o, DEV)
        assert abs(avg[m] - l) <= 1e-5 * abs(l)
        for name, a, b in (("w_inp", bank.w_inp[m], ctrl.fc_inp.weight), ("b_inp", bank.b_inp[m], ctrl.fc_inp.bias),
                           ("w_out", bank.w_out[m], ctrl.fc_out.weight.reshape(-1))):
            err = float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
            print(f"train_models with terms, model {m} {name}: {err:.3g}")
            assert err <= 1e-6, (m, name, err)
    assert len({round(v, 6) for v in avg}) == 3


def test_captured_step_with_terms_replays_the_eager_bits():
    from test_graphed import _controller_batches, _controller_setup
    dev = torch.device("cuda", 0)
    sim, ctrl = _controller_setup(dev)
    ctrl_g = copy.deepcopy(ctrl)
    loss_fn = fca.MPCLoss(prediction_horizon=10, alpha=20.0, terms=LossTerms(p1=(0.1, 0.4), p2=(0.05, 0.3), weight=3.5, alpha=3.5))
    opt = torch.optim.AdamW(ctrl.parameters(), lr=1e-3, capturable=True)
    opt_g = torch.optim.AdamW(ctrl_g.parameters(), lr=1e-3, capturable=True)
    loader = _controller_batches(dev, [15] * 4)
    step = fca.NeuralNetwork.captured_step(sim, ctrl_g, loss_fn, opt_g, dev)
    l_e, f_e = fca.NeuralNetwork.train_model(loader, sim, ctrl, loss_fn, opt, dev)
    l_g, f_g = fca.NeuralNetwork.train_model(loader, sim, ctrl_g, loss_fn, opt_g, dev, step=step)
    assert step.replays >= 1
    assert abs(l_g - l_e) <= 1e-6 * abs(l_e)
    for k in ("loss", "command", "error", "prediction"):
        assert torch.equal(f_g[k], f_e[k]), k
    for a, b in zip(ctrl.parameters(), ctrl_g.parameters()):
        assert torch.equal(a, b)
    plain = fca.MPCLoss(prediction_horizon=10, alpha=20.0)
    X, _, z = loader[0]
    assert plain(sim, ctrl, X, ctrl(X), z, dev)[0].item() != loss_fn(sim, ctrl, X, ctrl(X), z, dev)[0].item()
    with pytest.raises(NotImplementedError, match="preview"):
        fca.NeuralNetwork.train_model([(X, None, z, X[:, 2:3].expand(-1, 10).contiguous())], sim, ctrl_g, loss_fn, opt_g, dev,
                                      step=step)


def test_gather_with_a_preview_on_the_device():
    from forging_control_amd.data import reference_preview
    g = np.random.default_rng(11)
    T_traj, n_traj, N = 25, 3, 12
    rows = T_traj * n_traj
    X, Y, Z = (g.normal(size=(rows, k)).astype(np.float32) for k in (3, 1, 5))
    w = fca.SequenceWindows(X, Y, Z, T_traj, device=DEV)
    idx = np.array([0, 5, T_traj - 1, T_traj, 2 * T_traj - 3, rows - 1])
    x, y, z, r = w.gather(idx, preview=N)
    x3, y3, z3 = w.gather(idx)
    assert torch.equal(x, x3) and torch.equal(y, y3) and torch.equal(z, z3) and r.shape == (len(idx), N)
    want = reference_preview(torch.as_tensor(X), idx, T_traj, N)
    assert torch.equal(r.cpu(), want) and torch.equal(r[:, 0], x[:, 2])
    batches = list(fca.DeviceLoader(w, 16, preview=N))
    assert all(len(b) == 4 and b[3].shape == (b[0].shape[0], N) for b in batches)
    assert all(len(b) == 3 for b in fca.DeviceLoader(w, 16))
