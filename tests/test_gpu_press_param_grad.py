"""Gradients with respect to the 28 press parameters on the GPU: fcr_plant_rk4_vjp_press,
fcr_closed_loop_vjp_press and fcr_press_grad_sum (csrc/fcr_press_grad.h) against the stepwise oracle of
tests/press_param_torch.py evaluated on the GPU's own stored (x, u), the autograd plumbing of ``forging_rk4(params=)`` and
``ClosedLoop.run(differentiable=True, plant_params=)``, and ``fit_press``.

The bar is the project's parity bar, 1e-5: per parameter column of g_press (each over its own maximum over the batch; a
column that is all zero in the oracle must be all zero here), per state column of g_x0, per tensor for the rest —
press_param_torch.figures / refused, which tests/test_press_param_grad_host.py shows to refuse seven deliberate
mistakes. No trajectory is left out."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import press_param_torch as pp
import press_torch as pt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def assert_within_the_bar(got, want):
    f = pp.figures(got, want)
    print("figures:", {k: f"{v:.2e}" for k, v in f.items()})
    assert not pp.refused(got, want), f


def press_of(B, shared):
    """The (B,28) table of three presses, or the oracle's row for all: (what the oracle reads, the GPU's leaf)."""
    tab = pt.oracle_row() if shared else pt.three_rows_table(B)
    return tab, gpu(tab).requires_grad_(True)


def open_loop_gpu(x0, U, g_x, smooth, leaf, substeps=4):
    a, b = gpu(x0).requires_grad_(True), gpu(U).requires_grad_(True)
    X = fca.forging_rk4(a, b, 1e-3, substeps, smooth, params=leaf)
    X.backward(gpu(g_x))
    return host(X), {"g_x0": host(a.grad), "g_u": host(b.grad), "g_press": host(leaf.grad)}


@functools.lru_cache(maxsize=None)
def open_inputs(B, S):
    return pt.open_batch(B, S) + (pt.cotangents(B, S)[0],)


@pytest.mark.parametrize("shared", [False, True], ids=["table", "row"])
@pytest.mark.parametrize("substeps", [4, 3, 1])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 12), (300, 1), (300, 12)])
def test_open_loop_matches_the_stepwise_oracle(B, S, smooth, substeps, shared):
    """substeps 4: the kernels that keep the sub-steps' entry states; 3 and 1: the ones that recompute them. B = 300: one
    full block and 44 lanes, two partial records in the shared row's sum."""
    x0, U, g_x = open_inputs(B, S)
    tab, leaf = press_of(B, shared)
    X, got = open_loop_gpu(x0, U, g_x, smooth, leaf, substeps)
    assert leaf.grad.shape == leaf.shape
    want = pp.stepwise_param_adjoint(X, U, g_x, smooth, tab, substeps=substeps)
    assert_within_the_bar(got, pp.summed(want) if shared else want)


@pytest.mark.parametrize("smooth", [False, True])
def test_open_loop_edge_rows(smooth):
    """Rest at y = 0; y > 0 with yd = 0; p1 = PS; p2 = 0; z = 0; |yd| = 0.5; yd just above 0.5; the return stroke, S = 1:
    every gradient is finite and meets the oracle; the return stroke's eleven deformation columns are exactly 0."""
    x0, U = pt.edge_rows()
    g_x, _ = pt.cotangents(8, 1)
    tab = np.tile(pt.oracle_row(), (8, 1))
    leaf = gpu(tab).requires_grad_(True)
    X, got = open_loop_gpu(x0, U, g_x, smooth, leaf)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert_within_the_bar(got, pp.stepwise_param_adjoint(X, U, g_x, smooth, tab))
    cols = [pp.IX[n] for n in pp.DEFORMATION]
    assert len(cols) == 11 and np.all(got["g_press"][7, cols] == 0.0)
    assert np.abs(got["g_press"][5, cols]).min() > 0       # a row inside the branch has them all


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


@pytest.mark.parametrize("shared", [False, True], ids=["table", "row"])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("gain", [1.0, 2.0])
@pytest.mark.parametrize("hidden", [1, 50, 65])
def test_closed_loop_matches_the_stepwise_oracle(hidden, gain, smooth, shared):
    """B = 300, T = 12; W_out x 2 drives the Hardtanh into saturation. The oracle runs on the GPU's own stored x, u, so
    the masks are the forward's own. g_press, g_x0, dv and the controller's three gradients, all inside the bar."""
    B, T = 300, 12
    x0, ref, (g_x, g_u) = loop_inputs(B, T)
    w = pt.ctrl_weights(hidden, gain)
    tab, leaf = press_of(B, shared)
    loop = fca.ClosedLoop(controller_of(w), pt.SCALERS, smooth=smooth)
    x, u = loop.run(gpu(x0), gpu(ref), plant_params=leaf.detach())
    got = fca.closed_loop.loop_vjp(loop, x, u, gpu(ref), gpu(g_x), gpu(g_u), plant_params=leaf.detach(), press_grad=True)
    assert got["g_press"].shape == leaf.shape
    want = pp.stepwise_param_adjoint(host(x), host(u), g_x, smooth, tab, g_u, w, ref)
    assert np.abs(want["dv"]).max() > 0
    assert_within_the_bar({k: host(v) for k, v in got.items()}, pp.summed(want) if shared else want)


@pytest.mark.parametrize("substeps", [4, 3])
def test_closed_loop_autograd_reaches_the_press_and_leaves_the_rest_alone(substeps):
    """``run(differentiable=True, plant_params=leaf)``: leaf.grad is loop_vjp's g_press; x, u are the plain run's bits;
    g_x0 and the controller's gradients agree with the run whose press does not ask for a gradient to 1e-12 of each
    tensor's maximum (the same expressions in another instantiation)."""
    B, T = 300, 12
    x0, ref, (g_x, g_u) = loop_inputs(B, T)
    ctrl = controller_of(pt.ctrl_weights(50, 2.0))
    loop = fca.ClosedLoop(ctrl, pt.SCALERS, substeps=substeps)
    params = (ctrl.fc_inp.weight, ctrl.fc_inp.bias, ctrl.fc_out.weight)
    grads = {}
    for with_press in (False, True):
        ctrl.zero_grad(set_to_none=True)
        leaf = gpu(pt.three_rows_table(B)).requires_grad_(with_press)
        a = gpu(x0).requires_grad_(True)
        x, u = loop.run(a, gpu(ref), plant_params=leaf, differentiable=True)
        torch.autograd.backward([x, u], [gpu(g_x), gpu(g_u)])
        grads[with_press] = [x.detach(), u.detach(), a.grad] + [p.grad.clone() for p in params]
        if with_press:
            direct = fca.closed_loop.loop_vjp(loop, x.detach(), u.detach(), gpu(ref), gpu(g_x), gpu(g_u),
                                              plant_params=leaf.detach(), press_grad=True)
            assert leaf.grad.shape == (B, 28) and torch.equal(leaf.grad, direct["g_press"])
        else:
            assert leaf.grad is None
    xp, up = loop.run(gpu(x0), gpu(ref), plant_params=gpu(pt.three_rows_table(B)))
    assert torch.equal(grads[True][0], xp) and torch.equal(grads[True][1], up)
    same = [torch.equal(p, q) for p, q in zip(grads[False][2:], grads[True][2:])]
    print("state and controller gradients bit-equal with the parameter gradient on:", same)
    for p, q in zip(grads[False][2:], grads[True][2:]):
        assert float((p - q).abs().max()) <= 1e-12 * float(p.abs().max())


def test_closed_loop_still_refuses_noise_and_recovery():
    leaf = gpu(pt.oracle_row()).requires_grad_(True)
    loop = fca.ClosedLoop(controller_of(pt.ctrl_weights(50)), pt.SCALERS)
    x0, ref = gpu(np.zeros((2, 5))), gpu(np.zeros((2, 3)))
    for kw in (dict(process_noise=gpu(np.zeros((2, 3, 5)))), dict(feasibility=fca.FeasibilityRecovery())):
        with pytest.raises(ValueError, match="differentiable=True"):
            loop.run(x0, ref, differentiable=True, plant_params=leaf, **kw)


# ------------------------------------------------------------------------------------------------ plumbing

@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("substeps", [4, 3])
def test_open_loop_state_gradients_are_the_existing_paths(substeps, smooth):
    """g_x0 and g_u with the parameter gradient on against the call whose params do not require grad: 1e-12 of each
    tensor's maximum."""
    B, S = 300, 12
    x0, U, g_x = open_inputs(B, S)
    out = {}
    for with_press in (False, True):
        leaf = gpu(pt.three_rows_table(B)).requires_grad_(with_press)
        a, b = gpu(x0).requires_grad_(True), gpu(U).requires_grad_(True)
        fca.forging_rk4(a, b, 1e-3, substeps, smooth, params=leaf).backward(gpu(g_x))
        out[with_press] = (a.grad, b.grad)
    print("bit-equal:", [torch.equal(p, q) for p, q in zip(out[False], out[True])])
    for p, q in zip(out[False], out[True]):
        assert float((p - q).abs().max()) <= 1e-12 * float(p.abs().max())


def test_a_shared_rows_gradient_repeats_bit_for_bit():
    B, S = 300, 12
    x0, U, g_x = open_inputs(B, S)
    leaf = gpu(pt.oracle_row()).requires_grad_(True)
    X = fca.forging_rk4(gpu(x0), gpu(U), smooth=True, params=leaf)
    g1, = torch.autograd.grad(X, leaf, gpu(g_x), retain_graph=True)
    g2, = torch.autograd.grad(X, leaf, gpu(g_x))
    assert g1.shape == (28,) and torch.equal(g1, g2) and float(g1.abs().min()) > 0
    x0l, ref, (gx, gu) = loop_inputs(B, S)
    loop = fca.ClosedLoop(controller_of(pt.ctrl_weights(50, 2.0)), pt.SCALERS)
    x, u = loop.run(gpu(x0l), gpu(ref), plant_params=leaf.detach())
    r = [fca.closed_loop.loop_vjp(loop, x, u, gpu(ref), gpu(gx), gpu(gu), plant_params=leaf.detach(), press_grad=True)
         for _ in range(2)]
    assert all(torch.equal(r[0][k], r[1][k]) for k in r[0])


def test_press_grad_sum_adds_the_blocks_in_order():
    """B = 300: two partial records; B = 0 is zeros; against the same order of additions on the host."""
    g = np.random.default_rng(2).standard_normal((300, 28)) * 10.0 ** np.arange(-9, 19)
    got = host(fca.plant.press_grad_sum(gpu(g)))
    part = [functools.reduce(lambda s, r: s + r, blk, np.zeros(28)) for blk in (g[:256], g[256:])]
    assert np.array_equal(got, part[0] + part[1])
    assert np.array_equal(host(fca.plant.press_grad_sum(gpu(np.zeros((0, 28))))), np.zeros(28))


def test_the_gradient_has_the_leafs_shape_dtype_and_device():
    B, S = 300, 12
    x0, U, g_x = open_inputs(B, S)
    row32 = torch.tensor(pt.oracle_row(), dtype=torch.float32, device=DEV, requires_grad=True)
    X = fca.forging_rk4(gpu(x0), gpu(U), smooth=True, params=row32)
    assert X.requires_grad
    X.backward(gpu(g_x))
    assert row32.grad.shape == (28,) and row32.grad.dtype == torch.float32 and row32.grad.device == row32.device
    assert bool(torch.isfinite(row32.grad).all()) and float(row32.grad.abs().max()) > 0
    with torch.no_grad():
        assert not fca.forging_rk4(gpu(x0), gpu(U), smooth=True, params=row32).requires_grad


def test_a_constant_press_leaves_the_graph_as_it_is():
    """A PressParams and a tensor without grad: the result is attached to nothing and equals the plain call's bits; with
    x0 requiring grad the backward is the existing one (no gradient for the press)."""
    B, S = 300, 12
    x0, U, g_x = open_inputs(B, S)
    plain = fca.forging_rk4(gpu(x0), gpu(U), smooth=True, params=gpu(pt.oracle_row()))
    for params in (fca.PressParams(), gpu(pt.oracle_row())):
        X = fca.forging_rk4(gpu(x0), gpu(U), smooth=True, params=params)
        assert not X.requires_grad and torch.equal(X, plain)
    const = gpu(pt.oracle_row())
    a = gpu(x0).requires_grad_(True)
    fca.forging_rk4(a, gpu(U), smooth=True, params=const).backward(gpu(g_x))
    assert const.grad is None and a.grad is not None


def test_fit_press_recovers_the_press_of_the_cpu_yardstick():
    """The inputs of tests/golden/press_fit_cpu.json (B = 16, S = 12, smooth; CD x 0.85, M0 x 0.9, KB x 1.1): every
    field's error <= 10 x the recorded CPU error and loss / loss0 <= 100 x the recorded ratio (L-BFGS paths differ with
    rounding; the minimum is the same)."""
    rec = json.load(open(os.path.join(pt.GOLDEN, pp.FIT_GOLDEN)))
    x_obs, U = pp.fit_inputs(rec["B"], rec["S"], rec["smooth"])
    fitted, info = fca.fit_press(gpu(x_obs), gpu(U), pp.FIT_FIELDS, smooth=rec["smooth"])
    errors = pp.fit_errors([info["multipliers"][f] for f in pp.FIT_FIELDS])
    ratio = info["loss"] / info["loss0"]
    print("errors:", errors, "recorded:", rec["errors"], "loss/loss0:", ratio, "recorded:", rec["loss_ratio"], "evals:", info["evals"])
    assert isinstance(fitted, fca.PressParams) and fitted.B_DAMP == fca.PressParams().B_DAMP
    assert abs(fitted.CD / (0.63 * info["multipliers"]["CD"]) - 1) < 1e-15
    assert abs(info["loss0"] / rec["loss0"] - 1) < 1e-6
    for name, e, e0 in zip(pp.FIT_FIELDS, errors, rec["errors"]):
        assert e <= 10 * e0, (name, e, e0)
    assert ratio <= 100 * rec["loss_ratio"], (ratio, rec["loss_ratio"])
