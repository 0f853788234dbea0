"""The differentiable press on the GPU: fcr_plant_rk4_vjp and fcr_closed_loop_vjp (csrc/fcr_press_grad.h) against the
stepwise adjoint oracle of tests/press_torch.py evaluated on the GPU's own stored (x, u), against end-to-end autograd of
the torch restatement, and the autograd plumbing of ``forging_rk4`` and ``ClosedLoop.run(differentiable=True)``.

The bar is the project's parity bar, 1e-5 of each tensor's maximum (per state column for g_x0): press_torch.figures /
refused, the comparison tests/test_press_grad_host.py shows to refuse six deliberate mistakes."""
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import press_torch as pt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def open_loop_gpu(x0, U, g_x, smooth, table=None):
    a, b = gpu(x0).requires_grad_(True), gpu(U).requires_grad_(True)
    X = fca.forging_rk4(a, b, 1e-3, 4, smooth, params=None if table is None else gpu(table))
    X.backward(gpu(g_x))
    return host(X), {"g_x0": host(a.grad), "g_u": host(b.grad)}


def assert_within_the_bar(got, want, bar=pt.BAR):
    f = pt.figures(got, want)
    print("figures:", {k: f"{v:.2e}" for k, v in f.items()})
    assert not pt.refused(got, want, bar), (f, bar)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 12), (300, 1), (300, 12)])
def test_open_loop_matches_the_stepwise_oracle(B, S, smooth, table):
    x0, U = pt.open_batch(B, S)
    g_x, _ = pt.cotangents(B, S)
    tab = pt.three_rows_table(B) if table else None
    X, got = open_loop_gpu(x0, U, g_x, smooth, tab)
    assert_within_the_bar(got, pt.stepwise_adjoint(X, U, g_x, smooth, table=tab))


@pytest.mark.parametrize("smooth", [False, True])
def test_open_loop_edge_rows(smooth):
    """Rest at y = 0; y > 0 with yd = 0; p1 = PS; p2 = 0 (the smooth floor); z = 0; |yd| = 0.5; yd just above 0.5; the
    return stroke: finite gradients, inside the bar."""
    x0, U = pt.edge_rows()
    g_x, _ = pt.cotangents(8, 1)
    X, got = open_loop_gpu(x0, U, g_x, smooth)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert_within_the_bar(got, pt.stepwise_adjoint(X, U, g_x, smooth))


@pytest.mark.parametrize("smooth", [False, True])
def test_open_loop_matches_end_to_end_autograd(smooth):
    B, S = 300, 12
    x0, U = pt.open_batch(B, S)
    g_x, _ = pt.cotangents(B, S)
    _, got = open_loop_gpu(x0, U, g_x, smooth)
    a = torch.tensor(x0, requires_grad=True)
    b = torch.tensor(U, requires_grad=True)
    (pt.trajectory(a, b, smooth) * torch.tensor(g_x)).sum().backward()
    assert_within_the_bar(got, {"g_x0": a.grad.numpy(), "g_u": b.grad.numpy()})


def test_open_loop_other_substep_counts_and_no_steps():
    """substeps != 4 takes the kernels that recompute every sub-step's entry state; S = 0 returns g_x[:, 0]."""
    B, S = 70, 3
    x0, U = pt.open_batch(B, S)
    g_x, _ = pt.cotangents(B, S)
    for substeps in (1, 3, 5):
        a, b = gpu(x0).requires_grad_(True), gpu(U).requires_grad_(True)
        X = fca.forging_rk4(a, b, 1e-3, substeps, True)
        X.backward(gpu(g_x))
        want = pt.stepwise_adjoint(host(X), U, g_x, True, substeps=substeps)
        assert_within_the_bar({"g_x0": host(a.grad), "g_u": host(b.grad)}, want)
    a = gpu(x0).requires_grad_(True)
    X = fca.forging_rk4(a, gpu(U[:, :0]), 1e-3, 4, True)
    X.backward(gpu(g_x[:, :1]))
    assert np.array_equal(host(a.grad), g_x[:, 0])


# ------------------------------------------------------------------------------------------------ closed loop

def controller_of(w):
    W_inp, b_inp, W_out = w
    ctrl = fca.FNNModel(3, W_inp.shape[0], 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(W_inp))
        ctrl.fc_inp.bias.copy_(torch.tensor(b_inp))
        ctrl.fc_out.weight.copy_(torch.tensor(W_out))
    return ctrl


@functools.lru_cache(maxsize=None)
def loop_inputs(B, T):
    x0, ref = pt.loop_batch(B, T)
    return x0, ref, pt.cotangents(B, T)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("gain", [1.0, 2.0])
@pytest.mark.parametrize("hidden", [1, 50, 65])
@pytest.mark.parametrize("T", [12, 40])
def test_closed_loop_matches_the_stepwise_oracle(T, hidden, gain, smooth, table):
    """The oracle runs on the GPU's own stored x, u, so the masks are the forward's own and no trajectory is left out."""
    B = 300
    x0, ref, (g_x, g_u) = loop_inputs(B, T)
    w = pt.ctrl_weights(hidden, gain)
    tab = pt.three_rows_table(B) if table else None
    loop = fca.ClosedLoop(controller_of(w), pt.SCALERS, smooth=smooth)
    x, u = loop.run(gpu(x0), gpu(ref), plant_params=None if tab is None else gpu(tab))
    got = fca.closed_loop.loop_vjp(loop, x, u, gpu(ref), gpu(g_x), gpu(g_u), plant_params=None if tab is None else gpu(tab))
    want = pt.stepwise_adjoint(host(x), host(u), g_x, smooth, g_u, w, ref, table=tab)
    assert np.abs(want["dv"]).max() > 0
    assert_within_the_bar({k: host(v) for k, v in got.items()}, want)


def restatement_grads(x0, ref, w, g_x, g_u, smooth, cdt):
    a = torch.tensor(x0, requires_grad=True)
    P_ = [torch.tensor(k.astype(np.float64), requires_grad=True) for k in w]
    X, U, margin = pt.closed_loop(a, torch.tensor(ref), *P_, smooth, cdt=cdt)
    ((X * torch.tensor(g_x)).sum() + (U * torch.tensor(g_u)).sum()).backward()
    return {"g_x0": a.grad.numpy(), "g_w_inp": P_[0].grad.numpy(), "g_b_inp": P_[1].grad.numpy(),
            "g_w_out": P_[2].grad.numpy().reshape(-1)}, margin.numpy()


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("gain", [1.0, 2.0])
def test_closed_loop_matches_end_to_end_autograd(gain, smooth):
    """T = 12, against full autograd of the restatement (float32 controller) on its own trajectory. Trajectories with a
    pre-activation or |v| - 1 inside 1e-6 are left out (their incoming gradients are zeroed on both sides), at most 5 %.
    Bound per tensor: max(1e-5, 4 x the same figure between the restatement with a float32 and a float64 controller)."""
    B, T = 300, 12
    x0, ref, (g_x, g_u) = loop_inputs(B, T)
    w = pt.ctrl_weights(50, gain)
    with torch.no_grad():
        margin = pt.closed_loop(torch.tensor(x0), torch.tensor(ref), *(torch.tensor(k.astype(np.float64)) for k in w),
                                smooth)[2].numpy()
    out = margin < 1e-6
    assert out.mean() <= 0.05, out.mean()
    g_x, g_u = g_x * ~out[:, None, None], g_u * ~out[:, None]
    r32, _ = restatement_grads(x0, ref, w, g_x, g_u, smooth, torch.float32)
    r64, _ = restatement_grads(x0, ref, w, g_x, g_u, smooth, torch.float64)
    own = pt.figures(r64, r32)
    bar = {k: max(pt.BAR, 4 * v) for k, v in own.items()}
    print("left out:", out.mean(), "float64-vs-float32 controller:", {k: f"{v:.2e}" for k, v in own.items()})
    ctrl = controller_of(w)
    a = gpu(x0).requires_grad_(True)
    x, u = fca.ClosedLoop(ctrl, pt.SCALERS, smooth=smooth).run(a, gpu(ref), differentiable=True)
    torch.autograd.backward([x, u], [gpu(g_x), gpu(g_u)])
    got = {"g_x0": host(a.grad), "g_w_inp": host(ctrl.fc_inp.weight.grad), "g_b_inp": host(ctrl.fc_inp.bias.grad),
           "g_w_out": host(ctrl.fc_out.weight.grad).reshape(-1)}
    assert_within_the_bar(got, r32, bar)


# ------------------------------------------------------------------------------------------------ plumbing

@pytest.mark.parametrize("table", [False, True])
def test_differentiable_run_is_the_plain_run_and_repeats_bit_for_bit(table):
    B, T = 300, 12
    x0, ref, (g_x, g_u) = loop_inputs(B, T)
    ctrl = controller_of(pt.ctrl_weights(50, 2.0))
    tab = gpu(pt.three_rows_table(B)) if table else None
    loop = fca.ClosedLoop(ctrl, pt.SCALERS)
    xp, up = loop.run(gpu(x0), gpu(ref), plant_params=tab)
    assert not xp.requires_grad and not up.requires_grad
    grads = []
    for _ in range(2):
        ctrl.zero_grad(set_to_none=True)
        a = gpu(x0).requires_grad_(True)
        x, u = loop.run(a, gpu(ref), plant_params=tab, differentiable=True)
        assert x.requires_grad and u.requires_grad
        assert torch.equal(x, xp) and torch.equal(u, up)
        torch.autograd.backward([x, u], [gpu(g_x), gpu(g_u)])
        params = (ctrl.fc_inp.weight, ctrl.fc_inp.bias, ctrl.fc_out.weight)
        for p in params:
            assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype == torch.float32
        assert a.grad.shape == (B, 5) and a.grad.dtype == torch.float64
        grads.append([a.grad.clone()] + [p.grad.clone() for p in params])
    assert all(torch.equal(g0, g1) for g0, g1 in zip(*grads))
    assert all(float(g.abs().max()) > 0 for g in grads[0])
    with torch.no_grad():
        x, u = loop.run(gpu(x0).requires_grad_(True), gpu(ref), plant_params=tab, differentiable=True)
    assert not x.requires_grad and not u.requires_grad and torch.equal(x, xp)


def test_forging_rk4_attaches_only_when_asked():
    B, S = 300, 12
    x0, U = pt.open_batch(B, S)
    plain = fca.forging_rk4(gpu(x0), gpu(U), smooth=True)
    assert not plain.requires_grad
    a = gpu(x0).requires_grad_(True)
    X = fca.forging_rk4(a, gpu(U), smooth=True)
    assert X.requires_grad and torch.equal(X, plain)
    g = gpu(pt.cotangents(B, S)[0])
    g1, = torch.autograd.grad(X, a, g, retain_graph=True)
    g2, = torch.autograd.grad(X, a, g)
    assert torch.equal(g1, g2) and g1.shape == (B, 5)
    with torch.no_grad():
        assert not fca.forging_rk4(a, gpu(U), smooth=True).requires_grad
    # a float32 command gets its gradient in float32, a 1-D command in its own shape
    u32 = gpu(U[:, 0]).to(torch.float32).requires_grad_(True)
    fca.forging_rk4(gpu(x0), u32, smooth=True).sum().backward()
    assert u32.grad.shape == (B,) and u32.grad.dtype == torch.float32
