"""GPU: M controllers side by side (fcr_forward_many / fcr_backward_many, the MANY instantiations of csrc/fcr_small.h)
through MPCLoss.forward_many and NeuralNetwork.train_models — parity per model against the fp64 oracle at the
project's 1e-5, agreement with the single-model one-workgroup kernels at 1e-6 (test_gpu_pipe.py's bar between
families), independence of the models bit for bit, per-model backward weights, a kink case, determinism, training
against separate runs, and the fallback loop."""
import functools
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import kink_cases as K
from conftest import GOLDEN, load_case, relerr
from forging_control_amd.many import ControllerBank
from oracle import rollout_np as R
from oracle.rollout_torch import kink_margin
from test_gpu_parity import modules
from tests.golden.make_golden import synth_inputs, synth_params

pytestmark = pytest.mark.gpu
native = fca._native
DEV = "cuda:0"
TOL = 1e-5           # against the fp64 oracle (test_gpu_parity.TOL)
TOL_FAMILY = 1e-6    # against the single-model one-workgroup kernels (test_gpu_pipe.py)
BIG = 1 << 30
ALPHA = 20.0
OUT = ("loss", "cost", "command", "error", "prediction", "xhat", "g_u0", "g_W_inp", "g_b_inp", "g_W_out")
CTRL = ("W_inp", "b_inp", "W_out")


def seed_ctrls(M):
    """The first M of the reference's ten shipped seeds (tests/golden/ul_seed_controllers.npz), fp64 dicts."""
    w = np.load(os.path.join(GOLDEN, "ul_seed_controllers.npz"))
    return [{k: w[k][i].astype(np.float64) for k in CTRL} for i in range(M)]


def u0_of(ctrl, X):
    u, _ = R.fnn_forward(np.asarray(X, np.float64), ctrl["W_inp"], ctrl["b_inp"], ctrl["W_out"])
    return u.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(H, M, B, N, noise=False):
    """LSTM parameters, M controllers, stacked inputs and the fp64 oracle's per-model results (computed once, shared:
    do not write to the arrays). H = 50: the reference's surrogate and shipped seeds; (H, B, N) = (50, 15, 10) without
    noise: the golden B = 15 inputs for every model; otherwise synthetic inputs, a slice per model."""
    if H == 50:
        c, lstm = load_case("ref_b15_n10")
        ctrls = seed_ctrls(M)
    else:
        lstm = synth_params(H, 1000 + H)
        ctrls = [{k: synth_params(H, 3000 + m)[k] for k in CTRL} for m in range(M)]
    if (H, B, N, noise) == (50, 15, 10, False):
        X = np.stack([c["X"]] * M).astype(np.float32)
        S = np.stack([c["states"]] * M).astype(np.float32)
        nz = None
    else:
        X, S, nz = synth_inputs(M * B, N, 4000 + 7 * B + N, noise=noise)
        X, S = X.reshape(M, B, 3), S.reshape(M, B, 10, 5)
        nz = None if nz is None else nz.reshape(M, B, N, 4)
    u0 = np.stack([u0_of(ctrls[m], X[m]) for m in range(M)]).reshape(M, B, 1)
    ref = []
    for m in range(M):
        p = {**lstm, **ctrls[m]}
        loss, f, tape = R.rollout_forward(p, X[m], u0[m].reshape(B), S[m], N, ALPHA,
                                          None if nz is None else nz[m].astype(np.float64))
        g = R.rollout_backward(p, tape)
        ref.append({"loss": np.float64(loss), "cost": f["loss"], "command": f["command"], "error": f["error"],
                    "prediction": f["prediction"], "xhat": f["xhat"], **{k: g[k] for k in OUT[6:]}})
    return {"lstm": lstm, "ctrls": ctrls, "X": X, "S": S, "u0": u0, "noise": nz, "N": N, "ref": ref}


def make_bank(ctrls):
    bank = ControllerBank(len(ctrls), ctrls[0]["W_inp"].shape[0]).to(DEV)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)
    with torch.no_grad():
        for m, c in enumerate(ctrls):
            bank.w_inp[m].copy_(t(c["W_inp"]))
            bank.b_inp[m].copy_(t(c["b_inp"]))
            bank.w_out[m].copy_(t(c["W_out"]).reshape(-1))
    return bank


def simulator(lstm):
    return modules({**lstm, "W_inp": np.zeros((50, 3)), "b_inp": np.zeros(50), "W_out": np.zeros((1, 50))})[0]


def run_many(lstm, ctrls, X, u0, S, N, noise=None, w=None, **loss_kw):
    """One forward_many + backward on the GPU with u0 given as data (a leaf, as test_gpu_parity.run has it): per-model
    outputs stacked over the model, and the route the call took."""
    sim, bank = simulator(lstm), make_bank(ctrls)
    d = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)
    M = len(ctrls)
    u0_t = d(u0).reshape(M, -1, 1).requires_grad_(True)
    loss_kw.setdefault("many_min_models", 1)
    fn = fca.MPCLoss(prediction_horizon=N, alpha=ALPHA, **loss_kw)
    losses, f = fn.forward_many(sim, bank, d(X), u0_t, d(S), DEV, enable_noise=noise is not None,
                                noise=None if noise is None else d(noise))
    (losses if w is None else losses * d(w)).sum().backward()
    torch.cuda.synchronize()
    n = lambda t: t.detach().cpu().numpy()
    zero = lambda p: n(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)   # N = 1: no in-loss call
    out = {"loss": n(losses), "cost": n(f["loss"]), "command": n(f["command"]), "error": n(f["error"]),
           "prediction": n(f["prediction"]), "xhat": n(fn.last_trajectory), "g_u0": n(u0_t.grad).reshape(M, -1),
           "g_W_inp": zero(bank.w_inp), "g_b_inp": zero(bank.b_inp), "g_W_out": zero(bank.w_out)}
    out["info"] = fn.last_call
    assert all(p.grad is None for p in sim.parameters())
    return out


def run_case(c, **kw):
    return run_many(c["lstm"], c["ctrls"], c["X"], c["u0"], c["S"], c["N"], c["noise"], **kw)


def run_single(c, m, **loss_kw):
    """Model m of the case through MPCLoss.forward (test_gpu_parity.run's steps), with the case's outputs' names."""
    from test_gpu_parity import run
    o = run({**c["lstm"], **c["ctrls"][m]}, c["X"][m], c["u0"][m], c["S"][m], c["N"], ALPHA,
            None if c["noise"] is None else c["noise"][m], **loss_kw)
    o["cost"], o["loss"] = o["loss"], np.float32(o["loss_scalar"])
    o["g_W_out"] = o["g_W_out"].reshape(-1)
    return o


def forced_onewg(fn):
    """fn() with the single-model path forced to the one-workgroup family (pipelining off, restored afterwards)."""
    prev = native.set_small_pipe_limit(0)
    try:
        return fn()
    finally:
        native.set_small_pipe_limit(prev)


def errs_against(o, m, ref):
    return {k: relerr(np.asarray(o[k][m]).reshape(-1), np.asarray(ref[k]).reshape(-1)) for k in OUT}


PARITY = [(50, 3, 15, 10, False), (50, 10, 15, 10, False), (50, 2, 17, 3, False), (50, 5, 1, 1, False),
          (50, 2, 16, 12, False), (24, 3, 33, 4, False), (50, 3, 15, 10, True)]


@pytest.mark.parametrize("H,M,B,N,noise", PARITY, ids=[f"h{h}_m{m}_b{b}_n{n}" + ("_noise" if z else "")
                                                      for h, m, b, n, z in PARITY])
def test_parity_per_model_against_fp64(H, M, B, N, noise):
    c = case(H, M, B, N, noise)
    o = run_case(c)
    assert o["info"].route == "many" and (o["info"].forward, o["info"].backward) == ("small", "small")
    for m in range(M):
        errs = errs_against(o, m, c["ref"][m])
        print(f"many h{H} m{M} b{B} n{N} model {m}: max {max(errs.values()):.3g} "
              + " ".join(f"{k}={v:.3g}" for k, v in errs.items()))
        bad = {k: v for k, v in errs.items() if not v <= TOL}
        assert not bad, (m, bad)


@pytest.mark.parametrize("H,M,B,N", [(50, 3, 15, 10), (50, 2, 17, 3), (24, 3, 33, 4), (50, 1, 15, 10), (50, 1, 17, 3)])
def test_agrees_with_the_single_model_one_workgroup_kernels(H, M, B, N):
    """Every output of model m within 1e-6 relative of its own single call forced into the one-workgroup family; M = 1
    through the many-model kernels meets the same bar. Bit-equality is what the design predicts (the same program on
    the same rows): the print says whether it holds (DESIGN.md §7.9 records it)."""
    c = case(H, M, B, N)
    o = run_case(c)
    assert o["info"].route == "many"
    for m in range(M):
        s = forced_onewg(lambda: run_single(c, m, small_batch_limit=BIG))
        assert s["families"] == ("small", "small")
        errs = errs_against(o, m, s)
        same = {k: bool(np.array_equal(np.asarray(o[k][m]).reshape(-1), np.asarray(s[k]).reshape(-1))) for k in OUT}
        print(f"many vs one-workgroup h{H} m{M} b{B} n{N} model {m}: bit-equal {all(same.values())} "
              + " ".join(f"{k}={v:.3g}" for k, v in errs.items() if not same[k]))
        bad = {k: v for k, v in errs.items() if not v <= TOL_FAMILY}
        assert not bad, (m, bad)


def _bits_equal(a, b, rows_a, rows_b, what):
    for k in OUT:
        assert np.array_equal(a[k][rows_a], b[k][rows_b]), (what, k)


def test_models_are_independent_bit_for_bit():
    c = case(50, 3, 17, 3)
    base = run_case(c)
    # model 1's weights and inputs changed: model 0 (and 2) keep their bits
    ctrls = [dict(x) for x in c["ctrls"]]
    ctrls[1] = {k: v * 1.25 for k, v in ctrls[1].items()}
    X, S, u0 = c["X"].copy(), c["S"].copy(), c["u0"].copy()
    X[1], S[1], u0[1] = X[1] * 0.5, S[1] * 0.5, u0[1] * 0.5
    moved = run_many(c["lstm"], ctrls, X, u0, S, c["N"])
    _bits_equal(moved, base, [0, 2], [0, 2], "model 1 changed")
    assert not np.array_equal(moved["cost"][1], base["cost"][1])
    # the models permuted: the outputs permuted bit for bit
    perm = [2, 0, 1]
    p = run_many(c["lstm"], [c["ctrls"][i] for i in perm], c["X"][perm], c["u0"][perm], c["S"][perm], c["N"])
    _bits_equal(p, base, [0, 1, 2], perm, "permuted")
    # two models with equal weights and inputs: equal bits
    twice = [0, 1, 0]
    t = run_many(c["lstm"], [c["ctrls"][i] for i in twice], c["X"][twice], c["u0"][twice], c["S"][twice], c["N"])
    _bits_equal(t, t, [0], [2], "twins")
    _bits_equal(t, base, [0, 1], [0, 1], "twins vs base")


def test_backward_weights_scale_each_model():
    c = case(50, 3, 17, 3)
    base = run_case(c)
    w = np.array([0.5, -3.0, 7.0], np.float32)
    o = run_case(c, w=w)
    for m in range(3):
        for k in ("g_u0", "g_W_inp", "g_b_inp", "g_W_out"):
            assert relerr(o[k][m], w[m] * base[k][m].astype(np.float64)) <= 1e-6, (m, k)
        for k in OUT[:6]:
            assert np.array_equal(o[k][m], base[k][m]), (m, k)


def test_same_call_twice_is_bit_identical():
    c = case(50, 3, 15, 10)
    a, b = run_case(c), run_case(c)
    _bits_equal(a, b, slice(None), slice(None), "repeat")


def test_kink_case_both_models_meet_the_oracle():
    """h50_b48_n6 of tests/kink_cases.py (the small family reaches it): its calibrated controller is model 0, a copy
    with W_out halved is model 1, on the rows that lie outside test_gpu_kinks.py's 1e-5 kink band for both."""
    k = K.build("h50_b48_n6")
    K.check(k)
    p0 = k["params"]
    p1 = {**p0, "W_out": p0["W_out"] * 0.5}
    X, S, N = k["X"], k["states"], k["N"]
    u1 = u0_of(p1, X)
    _, f1, _ = R.rollout_forward(p1, X, u1, S, N, ALPHA)
    keep = kink_margin(p1, torch.as_tensor(X), f1["xhat"]).numpy() > K.BAND     # model 0's band is out already (K.build)
    assert keep.sum() >= 0.9 * len(X)
    X, S = X[keep], S[keep]
    ctrls = [{n: p[n] for n in CTRL} for p in (p0, p1)]
    u0 = np.stack([u0_of(c, X) for c in ctrls])
    o = run_many(p0, ctrls, np.stack([X, X]), u0, np.stack([S, S]), N)
    assert o["info"].route == "many"
    for m, p in enumerate((p0, p1)):
        loss, f, tape = R.rollout_forward(p, X, u0[m], S, N, ALPHA)
        g = R.rollout_backward(p, tape)
        ref = {"loss": loss, "cost": f["loss"], **{n: f[n] for n in ("command", "error", "prediction", "xhat")}, **g}
        errs = errs_against(o, m, ref)
        print(f"many kinks model {m}: B={len(X)} " + " ".join(f"{n}={v:.3g}" for n, v in errs.items()))
        bad = {n: v for n, v in errs.items() if not v <= TOL}
        assert not bad, (m, bad)


def _train_setup(M, B, steps, seed=1):
    c = case(50, M, B, 10)
    g = torch.Generator().manual_seed(seed)
    batches = [(torch.rand(M, B, 3, generator=g) * 2 - 1, torch.zeros(M, B, 1), torch.rand(M, B, 10, 5, generator=g) * 2 - 1)
               for _ in range(steps)]
    sim = simulator(c["lstm"])
    for p in sim.parameters():
        p.requires_grad_(False)
    return c, sim, [tuple(t.to(DEV) for t in b) for b in batches]


def test_train_models_matches_separate_runs():
    """Three AdamW steps (lr 1e-4, UL/Main.py:195) of train_models against three separate train_model runs on the
    existing path: every parameter within 1e-6 of its tensor's max-abs."""
    M, B = 3, 15
    c, sim, batches = _train_setup(M, B, 3)
    bank = make_bank(c["ctrls"])
    fn = fca.MPCLoss(prediction_horizon=10, alpha=ALPHA, many_min_models=1)
    opt = torch.optim.AdamW(bank.parameters(), lr=1e-4)
    avg, feats = fca.NeuralNetwork.train_models(batches, sim, bank, fn, opt, DEV)
    assert fn.last_call.route == "many" and feats["loss"].shape == (M, 3 * B)
    for m in range(M):
        ctrl = modules({**c["lstm"], **c["ctrls"][m]})[1]
        o = torch.optim.AdamW(ctrl.parameters(), lr=1e-4)
        single = fca.MPCLoss(prediction_horizon=10, alpha=ALPHA)
        l, f = fca.NeuralNetwork.train_model([(X[m], y[m], z[m]) for X, y, z in batches], sim, ctrl, single, o, DEV)
        assert abs(avg[m] - l) <= 1e-5 * abs(l)
        for name, a, b in (("w_inp", bank.w_inp[m], ctrl.fc_inp.weight), ("b_inp", bank.b_inp[m], ctrl.fc_inp.bias),
                           ("w_out", bank.w_out[m], ctrl.fc_out.weight.reshape(-1))):
            a, b = a.detach(), b.detach()
            err = float((a - b).abs().max() / b.abs().max())
            print(f"train_models model {m} {name}: {err:.3g}")
            assert err <= 1e-6, (m, name, err)
        start = torch.as_tensor(np.asarray(c["ctrls"][m]["W_inp"], np.float32), device=DEV)
        assert float((bank.w_inp[m].detach() - start).abs().max()) > 1e-4   # three steps of lr 1e-4 did move it


def test_train_models_captured_equals_eager_bits():
    """train_models through CapturedStep (two eager warm-up steps, then a captured and replayed one) leaves the bits of
    the eager train_models; both optimizers are capturable, as CapturedStep makes its own (graphed.py)."""
    M, B = 3, 15
    c, sim, batches = _train_setup(M, B, 4)
    out = []
    for graphed in (False, True):
        bank = make_bank(c["ctrls"])
        fn = fca.MPCLoss(prediction_horizon=10, alpha=ALPHA, many_min_models=1)
        opt = torch.optim.AdamW(bank.parameters(), lr=1e-4, capturable=True)
        step = fca.NeuralNetwork.captured_models_step(sim, bank, fn, opt, DEV) if graphed else None
        avg, feats = fca.NeuralNetwork.train_models(batches, sim, bank, fn, opt, DEV, step=step)
        torch.cuda.synchronize()
        if graphed:
            assert step.replays == 2 and step.eager_steps == 2
        out.append((avg, feats, [p.detach().clone() for p in bank.parameters()]))
    (avg_e, f_e, p_e), (avg_g, f_g, p_g) = out
    assert avg_e == avg_g
    for k in f_e:
        assert torch.equal(f_e[k], f_g[k]), k
    for a, b in zip(p_e, p_g):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H,precision", [(64, "fp32"), (50, "f16")])
def test_fallback_loops_over_the_single_model_path(H, precision):
    M, B, N = 2, 17, 3
    if H == 50:
        c = case(50, M, B, N)
    else:
        lstm = synth_params(H, 1000 + H)
        ctrls = [{k: synth_params(H, 3000 + m)[k] for k in CTRL} for m in range(M)]
        X, S, _ = synth_inputs(M * B, N, 77)
        X, S = X.reshape(M, B, 3), S.reshape(M, B, 10, 5)
        c = {"lstm": lstm, "ctrls": ctrls, "X": X, "S": S, "N": N, "noise": None,
             "u0": np.stack([u0_of(ctrls[m], X[m]) for m in range(M)]).reshape(M, B, 1)}
    o = run_case(c, precision=precision)
    assert o["info"].route == "loop" and len(o["info"].calls) == M and o["info"].why
    for m in range(M):
        s = run_single(c, m, precision=precision)
        for k in OUT:
            assert np.array_equal(np.asarray(o[k][m]).reshape(-1), np.asarray(s[k]).reshape(-1)), (m, k)


def test_bank_call_matches_the_models_and_their_gradients():
    """bank(X) (fcr_fnn_forward_many / _backward_many) against FNNModel per model: the same kernels' arithmetic, so the
    bits; B = 300 takes two blocks per model and the partial-sum reduction."""
    for B in (15, 300):
        c = case(50, 3, 15, 10)
        bank = make_bank(c["ctrls"])
        X = (torch.rand(3, B, 3, generator=torch.Generator().manual_seed(B)) * 2 - 1).to(DEV).requires_grad_(True)
        gu = torch.randn(3, B, 1, generator=torch.Generator().manual_seed(B + 1)).to(DEV)
        u = bank(X)
        u.backward(gu)
        for m in range(3):
            ctrl = modules({**c["lstm"], **c["ctrls"][m]})[1]
            Xm = X[m].detach().clone().requires_grad_(True)
            um = ctrl(Xm)
            um.backward(gu[m])
            assert torch.equal(u[m], um) and torch.equal(X.grad[m], Xm.grad)
            assert torch.equal(bank.w_inp.grad[m], ctrl.fc_inp.weight.grad)
            assert torch.equal(bank.b_inp.grad[m], ctrl.fc_inp.bias.grad)
            assert torch.equal(bank.w_out.grad[m], ctrl.fc_out.weight.grad.reshape(-1))
