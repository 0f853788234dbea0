"""GPU: every kernel instantiation the press rows' host code picks from run-time flags (csrc/fcr_press_host.h: select)
is the one its flags name. A swapped index there leaves every kernel's code as it was and every existing test of one
flag combination possibly passing, so each combination is run once, at the smallest shapes, against the CPU oracles
(oracle/closed_loop_np.py, tests/feasibility_np.py, tests/press_np.py, tests/press_torch.py) at the bars of
tests/test_gpu_loop_bank.py (1e-5 of a state's largest magnitude, 1e-5 of the largest command), tests/test_gpu_press_params.py
(the plant: 1e-9) and tests/test_gpu_press_grad.py (press_torch.BAR = 1e-5 per gradient tensor).

The inputs make every flag matter: p2 starts at or below 0 (the smooth floor acts), the commands saturate and the
projection's p1 bound lies inside what the loop reaches (recovery acts, with flags 1 and 2), w and v are the harness's noise, and the table's rows
are 28 fields drawn in +-5 %. The `every_*_flag_matters` functions show on the oracles alone that flipping any one flag
of any case moves the oracle's result by at least 100 x the bar it is compared at; every test begins with its family's."""
import functools
import itertools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import press_np
import press_torch as pt
from test_loop_host import MEAS_STD, PROCESS_STD

M, B, T, HIDDEN, SUBSTEPS, TS = 2, 5, 3, 3, 2, 1e-3
FEAS = dict(p1=(0.0, 9e6), ts=TS, substeps=SUBSTEPS, expand=3, bisect=4)   # p1: inside what the loop reaches
SCALE_ARGS = (pt.SCALERS["input"][:2], pt.SCALERS["y_dot"], pt.SCALERS["output"])
LOOP_BAR, PLANT_BAR = 1e-5, 1e-9
DEV = "cuda:0"
FLAGS = list(itertools.product([False, True], repeat=4))          # (table, recover, smooth, noise)


# ---------------------------------------------------------------------------------------------
# inputs and oracles (CPU, shared, read-only)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs():
    """x0 (M,B,5) with p2 from 0 down to -2 MPa, ref (M,B,T) of either sign, w and v (M,B,T,5), commands U (B,T)."""
    rng = np.random.default_rng(12)
    x0 = np.empty((M, B, 5))
    x0[..., 0] = rng.uniform(0.02, 0.06, (M, B))
    x0[..., 1] = rng.uniform(0.05, 0.3, (M, B))
    x0[..., 2] = rng.uniform(2e6, 1e7, (M, B))
    x0[..., 3] = -np.linspace(0.0, 2e6, B)
    x0[..., 4] = rng.uniform(-0.05, 0.08, (M, B))
    ref = rng.uniform(0.2, 0.9, (M, B, T)) * rng.choice([-1.0, 1.0], (M, B, 1))
    w, v = fca.closed_loop.harness_noise(M * B, T, PROCESS_STD, MEAS_STD, np.random.RandomState(3))
    U = rng.uniform(-0.2, 0.2, (B, T))
    return x0, ref, w.reshape(M, B, T, 5), v.reshape(M, B, T, 5), U


@functools.lru_cache(maxsize=None)
def weights():
    """(W_inp (M,H,3), b_inp (M,H), W_out (M,H)) fp32: model 0 is press_torch's 3-unit controller with W_out x 2 (it
    saturates), model 1 the same units moved by up to 20 %."""
    W_inp, b_inp, W_out = pt.ctrl_weights(HIDDEN, 2.0)
    rng = np.random.default_rng(8)
    return tuple(np.stack([a, (a * (1 + rng.uniform(-0.2, 0.2, a.shape))).astype(np.float32)])
                 for a in (W_inp, b_inp, W_out.reshape(-1)))


def model_weights(m):
    W = weights()
    return W[0][m], W[1][m], W[2][m][None, :]


def adjoint_weights():
    """The adjoints' controller: the same units with W_out x 1, which clamps 6 of the 15 (trajectory, step) pairs, so the
    Hardtanh's mask is met on both sides."""
    return pt.ctrl_weights(HIDDEN, 1.0)


@functools.lru_cache(maxsize=None)
def tables():
    """{False: the oracle's own press for every trajectory, True: 28 fields in +-5 % per trajectory}, each (B,28)."""
    spread = fca.PressParams().sample(B, {n: 0.05 for n in fca.PressParams.NAMES}, rng=np.random.RandomState(2))
    assert fca.PressParams.validate(spread)
    return {False: np.tile(press_np.oracle_row(), (B, 1)), True: spread.numpy()}


@functools.lru_cache(maxsize=None)
def loop_oracle(m, table, recover, smooth, noise):
    """Model m's loop under the four flags: (x, u) or (x, u, u_nn, flag)."""
    x0, ref, w, v, _ = inputs()
    return press_np.closed_loop_press(tables()[table], x0[m], ref[m], *model_weights(m), *SCALE_ARGS, TS, SUBSTEPS, smooth,
                                      w[m] if noise else None, v[m] if noise else None, FEAS if recover else None)


@functools.lru_cache(maxsize=None)
def plant_oracle(table, smooth):
    x0, _, _, _, U = inputs()
    return press_np.trajectory(tables()[table], x0[0], U, TS, SUBSTEPS, smooth)


def state_err(x, xr):
    return (np.abs(x - xr).reshape(-1, 5) / np.abs(xr).reshape(-1, 5).max(0)).max(0)


def loop_err(got, want):
    """The figures of the bank's oracle tests: the worst state's error over its largest magnitude, and the command's."""
    return max(state_err(got[0], want[0]).max(), np.abs(got[1] - want[1]).max() / np.abs(want[1]).max())


def cotangents():
    return pt.cotangents(B, T, seed=5)


def adjoint(x, u, smooth, substeps, table, closed, ts=TS):
    """press_torch's stepwise adjoint on a stored run: the open loop's, or the closed loop's under adjoint_weights()."""
    g_x, g_u = cotangents()
    if not closed:
        return pt.stepwise_adjoint(x, u, g_x, smooth, ts=ts, substeps=substeps, table=tables()[table] if table else None)
    return pt.stepwise_adjoint(x, u, g_x, smooth, g_u, adjoint_weights(), inputs()[1][0], ts=ts, substeps=substeps,
                               table=tables()[table] if table else None)


@functools.lru_cache(maxsize=None)
def stored_run(closed, smooth, substeps, table):
    """The oracle's forward run the adjoint's input condition is shown on: (x, u)."""
    x0, ref, _, _, U = inputs()
    if not closed:
        return press_np.trajectory(tables()[table], x0[0], U, TS, substeps, smooth), U
    return press_np.closed_loop_press(tables()[table], x0[0], ref[0], *adjoint_weights(), *SCALE_ARGS, TS, substeps, smooth)


# The condition on the inputs, on the oracles alone: one flag flipped moves the result by >= 100 x its bar. `store`
# changes no number; its cases compare the statistics bit for bit. Each part is evaluated once.
@functools.lru_cache(maxsize=None)
def every_loop_flag_matters():
    """Each of (table, recover, smooth, noise), for each model, from every one of the 16 combinations (the single-model
    loop's cases are model 0's without a table); and every model's command saturates."""
    for m in range(M):
        for flags in FLAGS:
            base = loop_oracle(m, *flags)
            assert np.isfinite(base[0]).all(), (m, flags)
            for i, name in enumerate(("table", "recover", "smooth", "noise")):
                moved = loop_err(loop_oracle(m, *(f != (i == j) for j, f in enumerate(flags))), base)
                assert moved >= 100 * LOOP_BAR, (m, flags, name, moved)
        assert np.abs(loop_oracle(m, False, False, True, False)[1]).max() == np.float32(pt.SCALERS["output"])
    return True


@functools.lru_cache(maxsize=None)
def every_plant_flag_matters():
    for table, smooth in itertools.product([False, True], repeat=2):
        base = plant_oracle(table, smooth)
        assert state_err(plant_oracle(not table, smooth), base).max() >= 100 * PLANT_BAR
        assert state_err(plant_oracle(table, not smooth), base).max() >= 100 * PLANT_BAR
    return True


@functools.lru_cache(maxsize=None)
def every_adjoint_flag_matters(closed):
    """smooth and table, flipped on the same stored run; and, at substeps = 2, the kept path's arithmetic (four sub-steps
    of the same dt) in place of the general path's. At substeps = 4 the general path computes the same function as the
    kept one, so a swap there has no wrong result to show."""
    for smooth, substeps, table in itertools.product([False, True], (4, 2), [False, True]):
        x, u = stored_run(closed, smooth, substeps, table)
        want = adjoint(x, u, smooth, substeps, table, closed)
        flips = {"smooth": adjoint(x, u, not smooth, substeps, table, closed),
                 "table": adjoint(x, u, smooth, substeps, not table, closed)}
        if substeps != 4:
            flips["kept"] = adjoint(x, u, smooth, 4, table, closed, ts=TS * 4 / substeps)
        for name, other in flips.items():
            moved = max(pt.figures(other, want).values())
            assert moved >= 100 * pt.BAR, (closed, smooth, substeps, table, name, moved)
        assert not closed or 5 <= np.count_nonzero(want["dv"]) <= 10          # the clamp's mask, both ways
    return True


# ---------------------------------------------------------------------------------------------
# the GPU side
# ---------------------------------------------------------------------------------------------
def gpu(a):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV)


def host(a):
    return a.detach().cpu().numpy()


def recovery():
    return fca.FeasibilityRecovery(**FEAS)


def controller(w):
    W_inp, b_inp, W_out = w
    ctrl = fca.FNNModel(3, HIDDEN, 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(W_inp))
        ctrl.fc_inp.bias.copy_(torch.tensor(b_inp))
        ctrl.fc_out.weight.copy_(torch.tensor(W_out))
    return ctrl


def assert_loop(got, want, what):
    err = loop_err(got, want)
    print(f"{what}: err {err:.3g}")
    assert err <= LOOP_BAR, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("table,recover,smooth,noise", FLAGS,
                         ids=["-".join(n for n, f in zip(("table", "recover", "smooth", "noise"), fl) if f) or "plain" for fl in FLAGS])
def test_bank_runs_the_instantiation_its_flags_name(table, recover, smooth, noise):
    """bank, bank_press, bank_recover, bank_recover_press x smooth x noise, each with store and without: 32 launches."""
    from test_gpu_loop_bank import assert_same_numbers, make_bank
    assert every_loop_flag_matters()
    x0, ref, w, v, _ = inputs()
    clb = fca.ClosedLoopBank(make_bank(weights()), pt.SCALERS, TS, SUBSTEPS, smooth)
    kw = dict(process_noise=gpu(w) if noise else None, meas_noise=gpu(v) if noise else None,
              feasibility=recovery() if recover else None, plant_params=gpu(tables()[True]) if table else None)
    full = clb.run(gpu(x0), gpu(ref), **kw)
    for m in range(M):
        assert_loop((host(full["x"][m]), host(full["u"][m])), loop_oracle(m, table, recover, smooth, noise), f"model {m}")
    lean = clb.run(gpu(x0), gpu(ref), store=False, **kw)
    assert all(lean[k] is None for k in ("x", "u", "u_nn", "flag"))
    assert_same_numbers(full, lean)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("recover", [False, True])
def test_single_model_loop_runs_the_instantiation_its_flags_name(recover, smooth, noise):
    """closed_loop_kernel, closed_loop_noise_kernel and closed_loop_recover_kernel<*, noise>, each x smooth."""
    assert every_loop_flag_matters()
    x0, ref, w, v, _ = inputs()
    r = fca.ClosedLoop(controller(model_weights(0)), pt.SCALERS, TS, SUBSTEPS, smooth).run(
        gpu(x0[0]), gpu(ref[0]), gpu(w[0]) if noise else None, gpu(v[0]) if noise else None, recovery() if recover else None)
    assert_loop((host(r[0]), host(r[1])), loop_oracle(0, False, recover, smooth, noise), "single model")


@pytest.mark.gpu
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_plant_runs_the_instantiation_its_flags_name(smooth, table):
    assert every_plant_flag_matters()
    x0, _, _, _, U = inputs()
    got = fca.forging_rk4(gpu(x0[0]), gpu(U), TS, SUBSTEPS, smooth, params=gpu(tables()[True]) if table else None)
    err = state_err(host(got), plant_oracle(table, smooth))
    print(f"plant: err {err}")
    assert np.all(err < PLANT_BAR), err


@pytest.mark.gpu
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("substeps", [4, 2], ids=["kept", "general"])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("closed", [False, True], ids=["plant_rk4_vjp", "closed_loop_vjp"])
def test_adjoints_run_the_instantiation_their_flags_name(closed, smooth, substeps, table):
    """The oracle runs on the GPU's own stored x, u, as in tests/test_gpu_press_grad.py."""
    assert every_adjoint_flag_matters(closed)
    x0, ref, _, _, U = inputs()
    g_x, g_u = cotangents()
    tab = gpu(tables()[True]) if table else None
    if closed:
        loop = fca.ClosedLoop(controller(adjoint_weights()), pt.SCALERS, TS, substeps, smooth)
        x, u = loop.run(gpu(x0[0]), gpu(ref[0]), plant_params=tab)
        got = fca.closed_loop.loop_vjp(loop, x, u, gpu(ref[0]), gpu(g_x), gpu(g_u), plant_params=tab)
        got = {k: host(a) for k, a in got.items()}
        u = host(u)
    else:
        a, b = gpu(x0[0]).requires_grad_(True), gpu(U).requires_grad_(True)
        x = fca.forging_rk4(a, b, TS, substeps, smooth, params=tab)
        x.backward(gpu(g_x))
        got, u = {"g_x0": host(a.grad), "g_u": host(b.grad)}, U
    want = adjoint(host(x), u, smooth, substeps, table, closed)
    f = pt.figures(got, want)
    print("figures:", {k: f"{e:.2e}" for k, e in f.items()})
    assert not pt.refused(got, want), f
