"""GPU: training the surrogate on its free run — ``surrogate.free_run`` (fcr_lstm_rollout forward,
fcr_lstm_rollout_backward backward, csrc/fcr_lro_bwd.h) against end-to-end fp64 autograd (tests/free_run_ref.py).

Measured on an MI355X (per-tensor max|err| / max|ref|, the worst over the parity cases and both losses): see DESIGN.md
§7.19; the bar is the project's 1e-5 for fp32-accurate paths."""
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import free_run_ref as R
from test_gpu_loop import load_weights, lstm_model
from test_surrogate import params_for, model_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-5
GAIN = (1.1, 0.9, 1.05, 0.8)
#        weights B   T   gain  noise
CASES = [("ref", 1, 1, None, 0.0),        # one lane, no feedback
         ("ref", 17, 2, None, 0.0),       # a one-lane second wave; one fed-back row
         ("ref", 40, 10, None, 0.0),      # window exactly regenerated
         ("ref", 33, 12, GAIN, 0.01),     # ring wraps; gain and noise
         ("ref", 130, 3, None, 0.0),      # second workgroup
         ("h16", 17, 12, None, 0.0),      # HS = 4
         ("h32", 16, 11, None, 0.0)]      # HS = 8


@functools.lru_cache(maxsize=None)
def case_inputs(B, T, noise_std):
    d = R.inputs(B, T, B * T)
    d["noise"] = None if not noise_std else noise_std * np.random.default_rng(T).standard_normal((B, T, 4))
    return d


@functools.lru_cache(maxsize=None)
def reference(name, B, T, gain, noise_std, loss):
    d = case_inputs(B, T, noise_std)
    kw = {"G": d["G"]} if loss == "dot" else {"target": d["target"]}
    return R.autograd_free_run(R.params_of(load_weights(name)), d["window0"], d["cmd"], gain, d["noise"], **kw)


def dev(a, grad=False):
    return None if a is None else torch.tensor(a, dtype=torch.float32, device=DEV, requires_grad=grad)


def grads_of(m, w0, c):
    g = {"window0": w0.grad, "cmd": c.grad, "fcW": m.fc.weight.grad, "fcb": m.fc.bias.grad}
    for k in range(3):
        g[f"Wih{k}"], g[f"Whh{k}"] = getattr(m.lstm, f"weight_ih_l{k}").grad, getattr(m.lstm, f"weight_hh_l{k}").grad
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in g.items()}


def run(m, d, gain, loss, need=(True, True), G=None):
    """One forward + backward of free_run on the device: (x̂, gradients) as numpy."""
    m.zero_grad(set_to_none=True)
    w0, c = dev(d["window0"], need[0]), dev(d["cmd"], need[1])
    xhat = fca.free_run(m, w0, c, gain, dev(d["noise"]))
    if loss == "dot":
        (xhat * dev(d["G"] if G is None else G)).sum().backward()
    else:
        torch.nn.functional.mse_loss(xhat, dev(d["target"])).backward()
    return xhat.detach().cpu().numpy(), grads_of(m, w0, c)


@pytest.mark.parametrize("loss", ["mse", "dot"])
@pytest.mark.parametrize("name,B,T,gain,noise_std", CASES)
def test_free_run_gradients_match_fp64_autograd(name, B, T, gain, noise_std, loss):
    ref = reference(name, B, T, gain, noise_std, loss)
    m = lstm_model(load_weights(name))
    xhat, g = run(m, case_inputs(B, T, noise_std), gain, loss)
    assert fca.free_run.last_route == "fused"
    errs = {f"xhat[{c}]": R.rel(xhat[..., c], ref["xhat"][..., c]) for c in range(4)}
    errs.update({k: R.rel(g[k], ref[k]) for k in R.KEYS})
    print(f"{name} B={B} T={T} {loss}:", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    assert np.all(g["window0"][:, 9, 4] == 0.0)


def test_scaled_cotangent_rows():
    """G's rows scaled per trajectory by 0, 1e-30, 1 and 1e4: every trajectory's g_window0 holds the bar against its
    own maximum (the dgates are scaled per trajectory), and a zero row gives exact zeros."""
    B, T = 32, 6
    d = case_inputs(B, T, 0.0)
    scale = np.array([0.0, 1e-30, 1.0, 1e4])[np.arange(B) % 4]
    G = d["G"] * scale[:, None, None]
    p = R.params_of(load_weights("ref"))
    unit = R.autograd_free_run(p, d["window0"], d["cmd"], None, None, G=d["G"])   # trajectories are independent
    _, g = run(lstm_model(load_weights("ref")), d, None, "dot", G=G)
    worst = 0.0
    for b in range(B):
        if scale[b] == 0.0:
            assert np.all(g["window0"][b] == 0.0) and np.all(g["cmd"][b] == 0.0)
            continue
        want = unit["window0"][b] * scale[b]
        err = np.abs(g["window0"][b].astype(np.float64) - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= TOL, (b, scale[b], err)
    print("scaled rows: worst per-trajectory error", f"{worst:.1e}")


def test_exact_properties():
    name, B, T = "ref", 33, 12
    d = case_inputs(B, T, 0.01)
    m = lstm_model(load_weights(name))
    xhat, g = run(m, d, GAIN, "dot")
    assert np.all(g["window0"][:, 9, 4] == 0.0)
    with torch.no_grad():
        plain = fca.simulate_rollout(m, dev(d["window0"]), dev(d["cmd"]), GAIN, dev(d["noise"])).cpu().numpy()
    assert np.array_equal(xhat, plain)
    xhat2, g2 = run(m, d, GAIN, "dot")
    assert np.array_equal(xhat, xhat2) and all(np.array_equal(g[k], g2[k]) for k in R.KEYS)
    _, g3 = run(m, d, GAIN, "dot", need=(False, False))
    assert g3["window0"] is None and g3["cmd"] is None
    assert all(np.array_equal(g[k], g3[k]) for k in R.KEYS[:8])
    _, g4 = run(m, d, GAIN, "dot", need=(False, True))
    assert g4["window0"] is None and np.array_equal(g4["cmd"], g["cmd"])


def test_non_finite_cotangent_reaches_the_weight_gradients():
    B, T = 20, 4
    d = case_inputs(B, T, 0.0)
    G = d["G"].copy()
    G[7, 2, 1] = np.inf
    _, g = run(lstm_model(load_weights("ref")), d, None, "dot", G=G)
    for k in R.KEYS[:8]:
        assert not np.isfinite(g[k]).all(), k
    assert np.isfinite(g["window0"][np.arange(B) != 7]).all()


def test_wide_model_composes_the_steps():
    p = params_for(64, seed=64)
    B, T = 24, 3
    d = case_inputs(B, T, 0.0)
    ref = R.autograd_free_run(p, d["window0"], d["cmd"], GAIN, None, target=d["target"])
    m = model_for(p)
    xhat, g = run(m, d, GAIN, "mse")
    assert fca.free_run.last_route == "steps"
    errs = {"xhat": R.rel(xhat, ref["xhat"]), **{k: R.rel(g[k], ref[k]) for k in R.KEYS}}
    print("H=64:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v <= TOL for v in errs.values()), errs


def test_train_free_run_follows_the_fp64_restatement():
    """B = 64, T = 5, H = 50, AdamW lr 1e-3: the first five step losses against fp64, and a held-out batch's loss falls
    over 20 steps."""
    B, T, steps = 64, 5, 20
    w = load_weights("ref")
    data = [R.inputs(B, T, 1000 + s) for s in range(steps)]
    held = R.inputs(B, T, 999)
    m64 = R.S.build(R.params_of(w))
    opt64 = torch.optim.AdamW(m64.parameters(), lr=1e-3, weight_decay=0.0)
    ref_losses = []
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    for d in data[:5]:
        opt64.zero_grad()
        loss = torch.nn.functional.mse_loss(R.free_run(m64, t64(d["window0"]), t64(d["cmd"]), t64(GAIN), None), t64(d["target"]))
        loss.backward()
        opt64.step()
        ref_losses.append(float(loss.detach()))

    m = lstm_model(w)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    mse = torch.nn.MSELoss()
    losses = []

    def recording(out, target):
        loss = mse(out, target)
        losses.append(float(loss.detach()))
        return loss

    held_loss = lambda: float(mse(fca.free_run(m, dev(held["window0"]), dev(held["cmd"]), GAIN).detach(), dev(held["target"])))
    before = held_loss()
    batches = [(dev(d["window0"]), dev(d["cmd"]), dev(d["target"])) for d in data]
    avg = fca.train_free_run(batches, m, recording, opt, gain=GAIN)
    after = held_loss()
    print("losses", losses[:5], "fp64", ref_losses, "held-out", before, "->", after)
    assert avg == pytest.approx(sum(losses) / steps, rel=1e-6)
    for got, want in zip(losses[:5], ref_losses):
        assert abs(got - want) <= TOL * abs(want), (got, want)
    assert after < before
