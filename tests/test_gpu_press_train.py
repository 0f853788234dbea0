"""Training a bank of controllers on the press, on the GPU: the bank's adjoint under incoming gradients
(fcr_closed_loop_bank_vjp) against the single-model call, the fused loss (fcr_closed_loop_bank_loss_vjp) against the
general adjoint fed the loss's cotangents and both against the stepwise oracle of tests/press_train_ref.py on the GPU's
own record, truncated back-propagation, and the plumbing: ``ClosedLoopBank.run(differentiable=True)``, ``PressLoss``,
``train_on_press``.

The inputs are press_train_ref.case's, which tests/test_press_train_host.py shows to drive every ReLU of the loss on both
sides; the oracle comparison is press_train_ref.bank_figures / bank_refused at the project's bar, 1e-5 of each tensor's
maximum (per state column for g_x0), which that file shows to refuse six deliberate mistakes."""
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import press_torch as pt
import press_train_ref as tr
from forging_control_amd.closed_loop import bank_loss_vjp, bank_vjp, loop_vjp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (M, B, T, hidden, smooth, substeps, press, stacked, with_u_prev), K
CASES = {
    "main": ((3, 300, 12, 50, True, 4, None, False, False), 0),
    "stacked_table_k5": ((3, 300, 12, 65, False, 4, "model", True, True), 5),
    "one_unit_k1": ((1, 70, 12, 1, True, 3, "traj", False, False), 1),
    "one_step_row": ((3, 70, 1, 50, False, 4, "row", True, False), 0),
    "one_lane_k12": ((1, 1, 12, 50, True, 4, None, False, True), 12),
    "one_lane_one_step": ((3, 1, 1, 65, True, 3, "model", False, False), 0),
    "three_substeps_k5": ((3, 300, 12, 50, False, 3, "traj", False, False), 5),
}


def gpu(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bank_of(ws):
    bank = fca.ControllerBank(len(ws), ws[0][0].shape[0]).to(DEV)
    with torch.no_grad():
        for m, (W_inp, b_inp, W_out) in enumerate(ws):
            bank.w_inp[m].copy_(torch.tensor(W_inp))
            bank.b_inp[m].copy_(torch.tensor(b_inp))
            bank.w_out[m].copy_(torch.tensor(W_out).reshape(-1))
    return bank


def controller_of(w):
    W_inp, b_inp, W_out = w
    ctrl = fca.FNNModel(3, W_inp.shape[0], 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(W_inp))
        ctrl.fc_inp.bias.copy_(torch.tensor(b_inp))
        ctrl.fc_out.weight.copy_(torch.tensor(W_out))
    return ctrl


def loop_of(c):
    return fca.ClosedLoopBank(bank_of(c["ws"]), pt.SCALERS, substeps=c["substeps"], smooth=c["smooth"])


def inputs_of(c):
    return gpu(c["x0"]), gpu(c["ref"]), None if c["table"] is None else gpu(c["table"])


@functools.lru_cache(maxsize=None)
def forward(name):
    """The case, its loop, the GPU's record (one launch), and the loss's cotangents on that record by autograd of the
    restatement — computed once and shared; read-only."""
    c = tr.case(*CASES[name][0])
    loop = loop_of(c)
    x0, ref, tab = inputs_of(c)
    r = loop.run(x0, ref, plant_params=tab)
    x, u = host(r["x"]), host(r["u"])
    sd = [tr.seeds(x[m], u[m], c["refs"][m], c["rows"][m], None if c["u_prev"] is None else c["u_prev"][m])
          for m in range(c["M"])]
    g_x, g_u, cost = (np.stack([s[i] for s in sd]) for i in range(3))
    return c, loop, r, x, u, g_x, g_u, cost


@functools.lru_cache(maxsize=None)
def oracle(name):
    c, _, _, x, u, *_ = forward(name)
    return tr.bank_stepwise(list(x), list(u), c["refs"], c["ws"], c["rows"], c["smooth"], CASES[name][1], c["u_prev"],
                            c["substeps"], c["tables"])


def fused(name, **kw):
    c, loop, r, *_ = forward(name)
    _, ref, tab = inputs_of(c)
    return bank_loss_vjp(loop, r["x"], r["u"], ref, c["rows"], tr.P_SCALE, None if c["u_prev"] is None else gpu(c["u_prev"]),
                         plant_params=tab, truncate=CASES[name][1], **kw)


def general(name, g_x, g_u, K=None):
    c, loop, r, *_ = forward(name)
    _, ref, tab = inputs_of(c)
    return bank_vjp(loop, r["x"], r["u"], ref, gpu(g_x), gpu(g_u), plant_params=tab, truncate=CASES[name][1] if K is None else K)


def worst(got, want, keys=tr.GRAD_KEYS):
    """Per tensor max|got - want| / max|want| over the whole stacked tensor."""
    return {k: float(np.abs(host(got[k]) - np.asarray(want[k])).max() / max(np.abs(np.asarray(want[k])).max(), 1e-300))
            if np.asarray(want[k]).size else 0.0 for k in keys}


@pytest.mark.parametrize("name", list(CASES))
def test_general_adjoint_is_the_single_model_call(name):
    """Model m's g_x0, dv and three parameter gradients from fcr_closed_loop_bank_vjp against fcr_closed_loop_vjp on that
    model alone, under generic cotangents: within 1e-12 of each tensor's maximum (bit equality is the aim and is printed)."""
    c, loop, r, *_ = forward(name)
    M, B, T = c["M"], c["B"], c["T"]
    cot = [pt.cotangents(B, T, seed=11 + m) for m in range(M)]
    g_x, g_u = np.stack([k[0] for k in cot]), np.stack([k[1] for k in cot])
    got = general(name, g_x, g_u, K=0)
    for m in range(M):
        single = fca.ClosedLoop(controller_of(c["ws"][m]), pt.SCALERS, substeps=c["substeps"], smooth=c["smooth"])
        tab = None if c["tables"] is None else gpu(c["tables"][m])
        want = loop_vjp(single, r["x"][m], r["u"][m], gpu(c["refs"][m]), gpu(g_x[m]), gpu(g_u[m]), plant_params=tab)
        f = worst({k: got[k][m] for k in tr.GRAD_KEYS}, {k: host(want[k]) for k in tr.GRAD_KEYS})
        same = {k: bool(torch.equal(got[k][m], want[k])) for k in tr.GRAD_KEYS}
        print("model", m, "figures:", {k: f"{v:.2e}" for k, v in f.items()}, "bit-equal:", same)
        assert all(v <= 1e-12 for v in f.values()), (m, f)
        assert float(want["dv"].abs().max()) > 0


@pytest.mark.parametrize("name", list(CASES))
def test_fused_loss_against_the_general_adjoint_and_the_oracle(name):
    """LossSeed against TensorSeed fed the cotangents torch autograd gives for the loss restatement on the GPU's own
    record (cost and loss within 1e-12, gradients within 1e-10 of each tensor's maximum: only the order of the seed
    arithmetic differs), and both against the stepwise oracle — truncated where the case is — at 1e-5 of each tensor's
    maximum, per state column for g_x0, no trajectory left out."""
    c, _, _, _, _, g_x, g_u, cost = forward(name)
    a, b, want = fused(name), general(name, g_x, g_u), oracle(name)
    f_cost = worst(a, {"cost": cost, "loss": cost.mean(1)}, ("cost", "loss"))
    f_seed = worst(a, {k: host(b[k]) for k in tr.GRAD_KEYS})
    got_a, got_b = ({k: host(g[k]) for k in tr.GRAD_KEYS} for g in (a, b))
    f_a, f_b = tr.bank_figures(got_a, want), tr.bank_figures(got_b, want)
    print("cost/loss:", f_cost, "fused vs general:", {k: f"{v:.2e}" for k, v in f_seed.items()})
    print("fused vs oracle:", {k: f"{v:.2e}" for k, v in f_a.items()}, "general vs oracle:", {k: f"{v:.2e}" for k, v in f_b.items()})
    assert all(v <= 1e-12 for v in f_cost.values()), f_cost
    assert all(v <= 1e-10 for v in f_seed.values()), f_seed
    assert np.abs(want["dv"]).max() > 0
    assert not tr.bank_refused(got_a, want), f_a
    assert not tr.bank_refused(got_b, want), f_b
    value = fused(name, value_only=True)
    assert set(value) == {"cost", "loss"}
    assert all(v <= 1e-12 for v in worst(value, {"cost": cost, "loss": cost.mean(1)}, ("cost", "loss")).values())


def test_truncation_changes_the_gradient_and_not_the_loss():
    """K = 5 and K = 0 on the same record: the same cost, another gradient; K >= T is K = 0 bit for bit."""
    c, loop, r, *_ = forward("main")
    _, ref, tab = inputs_of(c)
    run = lambda K: bank_loss_vjp(loop, r["x"], r["u"], ref, c["rows"], tr.P_SCALE, plant_params=tab, truncate=K)
    full, cut, beyond = run(0), run(5), run(12)
    assert torch.equal(full["cost"], cut["cost"]) and torch.equal(full["loss"], cut["loss"])
    assert all(torch.equal(full[k], beyond[k]) for k in full)
    assert max(tr.bank_figures({k: host(cut[k]) for k in tr.GRAD_KEYS}, {k: host(full[k]) for k in tr.GRAD_KEYS}).values()) > 1e-3


def test_two_calls_give_the_same_bits_and_a_shared_x0_receives_the_model_sum():
    c, loop, r, *_ = forward("main")
    first, second = fused("main"), fused("main")
    assert all(torch.equal(first[k], second[k]) for k in first)
    x0, ref, _ = inputs_of(c)
    a = x0.clone().requires_grad_(True)
    pl = fca.PressLoss(loop, tr.P_SCALE, terms=[fca.LossTerms(r_[1:3], r_[3:5], r_[5], r_[0]) for r_ in c["rows"]])
    loss, feats = pl.forward(a, ref)
    assert torch.equal(loss.detach(), first["loss"]) and torch.equal(feats["cost"], first["cost"])
    loss.sum().backward()
    assert a.grad.shape == (c["B"], 5) and torch.equal(a.grad, first["g_x0"].sum(0))
    stacked = x0.expand(c["M"], -1, -1).clone().requires_grad_(True)
    pl.forward(stacked, ref)[0].sum().backward()
    assert torch.equal(stacked.grad, first["g_x0"])


def test_zero_steps_and_empty_banks():
    """T = 0: zero loss and gradients, and under incoming gradients g_x0 = g_x[:,:,0]; B = 0 and M = 0: no-ops that zero
    what they are given."""
    c = tr.case(3, 70, 0, 50, True, 4, None, False, False)
    loop = loop_of(c)
    x0, ref, _ = inputs_of(c)
    r = loop.run(x0, ref)
    g = bank_loss_vjp(loop, r["x"], r["u"], ref, c["rows"], tr.P_SCALE)
    assert all(float(v.abs().max()) == 0 for k, v in g.items() if v.numel()) and g["loss"].shape == (3,)
    g_x = gpu(np.random.default_rng(0).standard_normal((3, 70, 1, 5)))
    g = bank_vjp(loop, r["x"], r["u"], ref, g_x, gpu(np.zeros((3, 70, 0))))
    assert torch.equal(g["g_x0"], g_x[:, :, 0]) and float(g["g_w_inp"].abs().max()) == 0
    empty = bank_loss_vjp(loop, r["x"][:, :0], r["u"][:, :0], ref[:0], c["rows"], tr.P_SCALE)
    assert empty["cost"].shape == (3, 0) and float(empty["loss"].abs().max()) == 0 and float(empty["g_b_inp"].abs().max()) == 0
    no_models = tuple(p[:0] for p in (loop.bank.w_inp, loop.bank.b_inp, loop.bank.w_out))
    g = bank_loss_vjp(loop, r["x"][:0], r["u"][:0], ref, c["rows"][:1], tr.P_SCALE, weights=no_models)
    assert g["loss"].shape == (0,) and g["g_w_inp"].shape == (0, 50, 3)


# ------------------------------------------------------------------------------------------------ plumbing

def test_differentiable_bank_run_is_the_plain_run_with_the_bank_adjoint_behind_it():
    c, loop, r, *_ = forward("stacked_table_k5")
    M, B, T = c["M"], c["B"], c["T"]
    x0, ref, tab = inputs_of(c)
    cot = [pt.cotangents(B, T, seed=11 + m) for m in range(M)]
    g_x, g_u = gpu(np.stack([k[0] for k in cot])), gpu(np.stack([k[1] for k in cot]))
    bank = loop.bank
    bank.zero_grad(set_to_none=True)
    a = x0.clone().requires_grad_(True)
    out = loop.run(a, ref, plant_params=tab, differentiable=True)
    assert out["x"].requires_grad and out["u"].requires_grad and not out["x_final"].requires_grad
    assert torch.equal(out["x"], r["x"]) and torch.equal(out["u"], r["u"])
    assert all(torch.equal(out["metrics"][k], r["metrics"][k]) for k in r["metrics"])
    torch.autograd.backward([out["x"], out["u"]], [g_x, g_u])
    want = bank_vjp(loop, r["x"], r["u"], ref, g_x, g_u, plant_params=tab)
    for p, k in ((bank.w_inp, "g_w_inp"), (bank.b_inp, "g_b_inp"), (bank.w_out, "g_w_out")):
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32 and torch.equal(p.grad, want[k].to(torch.float32))
    assert torch.equal(a.grad, want["g_x0"])
    bank.zero_grad(set_to_none=True)
    with torch.no_grad():
        out = loop.run(a, ref, plant_params=tab, differentiable=True)
    assert not out["x"].requires_grad and torch.equal(out["x"], r["x"])


def test_press_loss_fills_the_banks_gradients_and_scales_them_by_the_loss_weights():
    c, loop, r, *_ = forward("stacked_table_k5")
    x0, ref, tab = inputs_of(c)
    u_prev = gpu(c["u_prev"])
    want = fused("stacked_table_k5")
    pl = fca.PressLoss(loop, tr.P_SCALE, terms=[fca.LossTerms(r_[1:3], r_[3:5], r_[5], r_[0]) for r_ in c["rows"]], truncate=5)
    bank = loop.bank
    params = ((bank.w_inp, "g_w_inp"), (bank.b_inp, "g_b_inp"), (bank.w_out, "g_w_out"))
    bank.zero_grad(set_to_none=True)
    loss, feats = pl.forward(x0, ref, plant_params=tab, u_prev=u_prev)
    assert loss.shape == (3,) and loss.requires_grad and torch.equal(loss.detach(), want["loss"])
    assert not feats["x"].requires_grad and torch.equal(feats["x"], r["x"]) and torch.equal(feats["u"], r["u"])
    assert torch.equal(feats["cost"], want["cost"]) and set(feats["metrics"]) == set(r["metrics"])
    loss.sum().backward()
    for p, k in params:
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype == torch.float32
        assert torch.equal(p.grad, want[k].to(torch.float32)) and float(p.grad.abs().max()) > 0
    weights = gpu([2.0, 0.0, -0.5])
    bank.zero_grad(set_to_none=True)
    (pl.forward(x0, ref, plant_params=tab, u_prev=u_prev)[0] * weights).sum().backward()
    for p, k in params:
        scaled = want[k] * weights.reshape(3, *([1] * (want[k].dim() - 1)))
        assert torch.equal(p.grad, scaled.to(torch.float32))
    bank.zero_grad(set_to_none=True)
    with torch.no_grad():
        loss, feats = pl.forward(x0, ref, plant_params=tab, u_prev=u_prev)
    assert not loss.requires_grad and bank.w_inp.grad is None
    assert float((loss - want["loss"]).abs().max()) <= 1e-12 * float(want["loss"].abs().max())


def test_a_single_loop_is_a_bank_of_one():
    c, loop, r, *_ = forward("one_unit_k1")
    x0, ref, tab = inputs_of(c)
    want = fused("one_unit_k1")
    ctrl = controller_of(c["ws"][0])
    single = fca.ClosedLoop(ctrl, pt.SCALERS, substeps=c["substeps"], smooth=c["smooth"], plant_params=tab)
    row = c["rows"][0]
    loss, feats = fca.PressLoss(single, tr.P_SCALE, fca.LossTerms(row[1:3], row[3:5], row[5], row[0]), truncate=1).forward(x0, ref)
    assert loss.shape == (1,) and torch.equal(loss.detach(), want["loss"]) and feats["x"].shape == (1, 70, 13, 5)
    loss.sum().backward()
    assert torch.equal(ctrl.fc_inp.weight.grad, want["g_w_inp"][0].to(torch.float32))
    assert torch.equal(ctrl.fc_inp.bias.grad, want["g_b_inp"][0].to(torch.float32))
    assert torch.equal(ctrl.fc_out.weight.grad, want["g_w_out"].to(torch.float32))


def test_training_on_the_press_lowers_every_loss_and_a_bank_member_trains_as_it_does_alone():
    """M = 3, B = 64, T = 12, 20 AdamW steps on a fixed batch under a three-row press table: every model's loss ends
    below where it started, and model m trained inside the bank equals the same model trained alone (a bank of one
    with its own optimizer) within 1e-12 of its parameters' maximum."""
    c = tr.case(3, 64, 12, 50, True, 4, "traj", False, True)
    x0, ref, tab = inputs_of(c)
    u_prev = gpu(c["u_prev"][0])
    terms = [fca.LossTerms(r_[1:3], r_[3:5], r_[5], r_[0]) for r_ in c["rows"]]

    def train(ws, terms):
        loop = loop_of(dict(c, ws=ws))
        pl = fca.PressLoss(loop, tr.P_SCALE, terms=terms)
        opt = torch.optim.AdamW(loop.bank.parameters(), lr=1e-3)
        calls = []
        sampler = lambda B: calls.append(B) or tab
        with torch.no_grad():
            before = pl.forward(x0, ref, plant_params=tab, u_prev=u_prev)[0]
        avg, feats = fca.train_on_press([(x0, ref, u_prev)] * 20, loop, pl, opt, plant_sampler=sampler)
        with torch.no_grad():
            after = pl.forward(x0, ref, plant_params=tab, u_prev=u_prev)[0]
        assert calls == [64] * 20 and len(avg) == len(ws) and feats["cost"].shape == (len(ws), 20 * 64)
        return loop.bank, before, after

    bank, before, after = train(c["ws"], terms)
    print("loss before:", before.tolist(), "after:", after.tolist())
    assert bool((after < before).all()), (before, after)
    for m in range(3):
        alone, _, _ = train(c["ws"][m:m + 1], terms[m:m + 1])
        for name in ("w_inp", "b_inp", "w_out"):
            p, q = getattr(bank, name)[m].detach(), getattr(alone, name)[0].detach()
            assert float((p - q).abs().max()) <= 1e-12 * float(q.abs().max()), (m, name)
