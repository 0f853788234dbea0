"""GPU: the batched harness loop (NeuralNetwork.loop, Functions.py:1014-1289) — the press under process and
measurement noise in the one-launch closed loop, the surrogate's command-driven free run (fcr_lstm_rollout) and
``ClosedLoop.loop`` — against fp64 oracles built here from oracle/plant_np.py, closed_loop_np.py and rollout_np.py."""
import functools
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
from conftest import GOLDEN
from oracle.closed_loop_np import closed_loop
from oracle.rollout_np import lstm_forward
from test_closed_loop import SCALERS, ctrl_weights
from test_harness import OUT_MAXABS

pytestmark = pytest.mark.gpu

PROCESS_STD = np.array([0.5, 2.0, 5e7, 5e7, 2.0])     # UL/Main.py:88-112
MEAS_STD = np.array([1e-4, 1e-2, 1e4, 1e4, 1e-3])
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------
# the press under noise
# ---------------------------------------------------------------------------------------------
def noisy_loop_oracle(x0, ref, w, v, smooth):
    """closed_loop_np.closed_loop with the harness's noise: process noise w (or None) at every RK4 stage, measurement
    noise v (or None) on the record the controller reads."""
    return closed_loop(x0, ref, *ctrl_weights(), SCALERS["input"][:2], SCALERS["y_dot"], SCALERS["output"], smooth=smooth,
                       process_noise=w, meas_noise=v)


@functools.lru_cache(maxsize=None)
def press_case():
    B, T = 300, 40                                  # crosses the 256-lane block
    rng = np.random.default_rng(4)
    x0 = np.zeros((B, 5))
    x0[:, 2] = rng.uniform(1e6, 4e6, B)
    x0[:, 3] = rng.uniform(1e6, 4e6, B)
    ref = fca.closed_loop.reference_speeds(B, T, 1e-3, 1, 100)
    w, v = fca.closed_loop.harness_noise(B, T, PROCESS_STD, MEAS_STD, np.random.RandomState(7))
    return x0, ref, w, v


def gpu_controller():
    W_inp, b_inp, W_out = ctrl_weights()
    ctrl = fca.FNNModel(3, 50, 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(W_inp))
        ctrl.fc_inp.bias.copy_(torch.tensor(b_inp))
        ctrl.fc_out.weight.copy_(torch.tensor(W_out))
    return ctrl


@pytest.mark.parametrize("smooth", [True, False])
def test_noisy_press_matches_oracle(smooth):
    x0, ref, w, v = press_case()
    cl = fca.ClosedLoop(gpu_controller(), SCALERS, smooth=smooth)
    t = lambda a: torch.tensor(a, device=DEV)
    xc, uc = cl.run(t(x0), t(ref))
    xz, uz = cl.run(t(x0), t(ref), process_noise=torch.zeros(300, 40, 5, dtype=torch.float64, device=DEV))
    assert torch.equal(xz, xc) and torch.equal(uz, uc)          # zero noise: the clean run, bit for bit
    xr0, ur0 = closed_loop(x0, ref, *ctrl_weights(), SCALERS["input"][:2], SCALERS["y_dot"], SCALERS["output"],
                           smooth=smooth)
    xo0, uo0 = noisy_loop_oracle(x0, ref, np.zeros_like(w), np.zeros_like(v), smooth)
    assert np.array_equal(xo0, xr0) and np.array_equal(uo0, ur0)   # the oracle without noise is closed_loop_np
    for name, vv in (("w", None), ("w+v", v)):
        x, u = cl.run(t(x0), t(ref), process_noise=t(w), meas_noise=None if vv is None else t(vv))
        xr, ur = noisy_loop_oracle(x0, ref, w, np.zeros_like(v) if vv is None else vv, smooth)
        assert np.isfinite(xr).all() and xr[:, :, 1].min() > -0.5   # away from the plant's one discontinuity
        x, u = x.cpu().numpy(), u.cpu().numpy()
        assert np.array_equal(x[:, 0], x0)
        scale = np.abs(xr).reshape(-1, 5).max(0)
        err = (np.abs(x - xr).reshape(-1, 5) / scale).max(0)
        uerr = np.abs(u - ur).max() / np.abs(ur).max()
        moved = (np.abs(x - xc.cpu().numpy()).reshape(-1, 5) / scale).max(0)
        print(f"smooth={smooth} {name}: state err {err}, u err {uerr:.3g}, moved by the noise {moved}")
        assert np.all(err < 1e-5), (name, err)
        assert uerr <= 1e-5, (name, uerr)
        assert np.all(moved > 1e-3), (name, moved)               # a kernel that ignores the noise does not pass


@pytest.mark.parametrize("smooth", [True, False])
def test_measurement_noise_alone_matches_oracle(smooth):
    """process_noise=None, meas_noise=v: the first 20 steps of press_case(). MEAS_STD is small beside the states, so
    "moved by the noise" is measured against the oracle's own two runs, not a fixed floor: on the CPU the oracle with v
    is away from the oracle without it by [0.068, 0.096, 0.0099, 0.019, 0.027] of each state's range and 0.017 of
    u's (both plant models, to these digits); the GPU runs must be at least half that apart."""
    x0, ref, _, v = press_case()
    ref, v = ref[:, :20], v[:, :20]
    cl = fca.ClosedLoop(gpu_controller(), SCALERS, smooth=smooth)
    t = lambda a: torch.tensor(a, device=DEV)
    xc, uc = (a.cpu().numpy() for a in cl.run(t(x0), t(ref)))
    x, u = (a.cpu().numpy() for a in cl.run(t(x0), t(ref), meas_noise=t(v)))
    xrc, urc = noisy_loop_oracle(x0, ref, None, None, smooth)
    xr, ur = noisy_loop_oracle(x0, ref, None, v, smooth)
    assert np.isfinite(xr).all() and xr[:, :, 1].min() > -0.5
    assert np.array_equal(x[:, 0], x0)
    scale, uscale = np.abs(xr).reshape(-1, 5).max(0), np.abs(ur).max()
    err = (np.abs(x - xr).reshape(-1, 5) / scale).max(0)
    uerr = np.abs(u - ur).max() / uscale
    moved, moved_ref = (np.abs(x - xc).reshape(-1, 5) / scale).max(0), (np.abs(xr - xrc).reshape(-1, 5) / scale).max(0)
    umoved, umoved_ref = np.abs(u - uc).max() / uscale, np.abs(ur - urc).max() / uscale
    print(f"smooth={smooth} v: state err {err}, u err {uerr:.3g}, moved by the noise {moved} / {umoved:.3g}, "
          f"the oracle {moved_ref} / {umoved_ref:.3g}")
    assert np.all(err < 1e-5), err
    assert uerr <= 1e-5, uerr
    assert np.all(moved_ref > 0) and umoved_ref > 0
    assert np.all(moved >= 0.5 * moved_ref) and umoved >= 0.5 * umoved_ref   # a kernel that ignores v does not pass


@pytest.mark.parametrize("smooth", [True, False])
def test_saturating_controller_fires_both_clamps(smooth):
    """The controller's Hardtanh in the closed loop (fcr_closed_loop.h): on press_case() the command stays within
    [-0.71, 0.52] of the output scale, clean and noisy, so neither clamp fires in any other test here. With W_out doubled,
    over the 20 steps 10..29 of press_case() — the ten before and the ten after the reference changes sign — the fp64
    oracle commands +out_scale in 6 % of the steps and -out_scale in 2 %, every state stays finite and y_dot stays above
    -0.46 (both plant models; over the first 20 steps alone the reference is positive and the lower clamp never
    fires, over all 40 y_dot passes -0.5). Same bounds as the tests above."""
    x0, ref, _, _ = press_case()
    ref = np.ascontiguousarray(ref[:, 10:30])
    W_inp, b_inp, W_out = ctrl_weights()
    W_out = np.float32(2) * W_out
    ctrl = gpu_controller()
    with torch.no_grad():
        ctrl.fc_out.weight.copy_(torch.tensor(W_out))
    xr, ur = closed_loop(x0, ref, W_inp, b_inp, W_out, SCALERS["input"][:2], SCALERS["y_dot"], SCALERS["output"],
                         smooth=smooth)
    top = float(np.float32(SCALERS["output"]))
    hi, lo = float((ur >= top).mean()), float((ur <= -top).mean())
    assert np.isfinite(xr).all() and xr[:, :, 1].min() > -0.5
    assert hi >= 0.01 and lo >= 0.01, (hi, lo)                   # both clamps fire in the oracle
    t = lambda a: torch.tensor(a, device=DEV)
    x, u = (a.cpu().numpy() for a in fca.ClosedLoop(ctrl, SCALERS, smooth=smooth).run(t(x0), t(ref)))
    assert np.array_equal(x[:, 0], x0)
    scale = np.abs(xr).reshape(-1, 5).max(0)
    err = (np.abs(x - xr).reshape(-1, 5) / scale).max(0)
    uerr = np.abs(u - ur).max() / np.abs(ur).max()
    print(f"smooth={smooth} W_out x 2: +clamp {hi:.3f}, -clamp {lo:.3f}, state err {err}, u err {uerr:.3g}")
    assert np.all(err < 1e-5), err
    assert uerr <= 1e-5, uerr


def test_noise_arguments_are_checked():
    cl = fca.ClosedLoop(gpu_controller(), SCALERS)
    x0 = torch.zeros(4, 5, dtype=torch.float64, device=DEV)
    ref = torch.zeros(4, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="process_noise"):
        cl.run(x0, ref, process_noise=torch.zeros(4, 3, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="meas_noise"):
        cl.run(x0, ref, meas_noise=torch.zeros(4, 2, 5, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="meas_noise"):
        cl.run(x0, ref, meas_noise=torch.zeros(4, 3, 5, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------
# the surrogate's command-driven rollout
# ---------------------------------------------------------------------------------------------
def load_weights(name):
    w = np.load(os.path.join(GOLDEN, f"weights_{name}.npz"))
    return {k: w[k].astype(np.float32) for k in w.files}


def lstm_model(w, dev=DEV):
    H = w["Whh0"].shape[1]
    m = fca.LSTMModel(5, H, 4, 3)
    with torch.no_grad():
        for k in range(3):
            getattr(m.lstm, f"weight_ih_l{k}").copy_(torch.as_tensor(w[f"Wih{k}"]))
            getattr(m.lstm, f"weight_hh_l{k}").copy_(torch.as_tensor(w[f"Whh{k}"]))
        m.fc.weight.copy_(torch.as_tensor(w["fcW"]))
        m.fc.bias.copy_(torch.as_tensor(w["fcb"]))
    return m.to(dev)


def rollout_inputs(B, T, seed):
    """Row 0: y_dot and z uniform in [-0.5, 0.5], the pressures in [0.05, 0.9], the command in [-1, 1], repeated over
    the 10 rows; piecewise-constant commands in [-1, 1]."""
    rng = np.random.default_rng(seed)
    row = np.empty((B, 5))
    row[:, [0, 3]] = rng.uniform(-0.5, 0.5, (B, 2))
    row[:, 1:3] = rng.uniform(0.05, 0.9, (B, 2))
    row[:, 4] = rng.uniform(-1, 1, B)
    window0 = np.repeat(row[:, None, :], 10, axis=1).astype(np.float32)
    levels = rng.uniform(-1, 1, (B, (T + 3) // 4))
    cmd = np.repeat(levels, 4, axis=1)[:, :T].astype(np.float32)
    return window0, cmd


def rollout_oracle(w, window0, cmd, gain=None, noise=None, lstm=None):
    """fp64: step 0 on window0 with its last command replaced by cmd[:,0]; step t >= 1 drops the oldest row and appends
    [gain * x̂_{t-1}, cmd[:,t]]; x̂_t = LSTM(window_t) + noise[:,t]. lstm: another evaluator of one window."""
    f64 = np.float64
    if lstm is None:
        Wih, Whh = [w[f"Wih{k}"].astype(f64) for k in range(3)], [w[f"Whh{k}"].astype(f64) for k in range(3)]
        lstm = lambda win: lstm_forward(win, Wih, Whh, w["fcW"].astype(f64), w["fcb"].astype(f64))[0]
    g = np.ones(4) if gain is None else np.asarray(gain, np.float32).astype(f64)
    win = window0.astype(f64).copy()
    win[:, -1, 4] = cmd[:, 0]
    B, T = cmd.shape
    out = np.empty((B, T, 4))
    for t in range(T):
        if t > 0:
            row = np.concatenate([g * out[:, t - 1], cmd[:, t:t + 1].astype(f64)], axis=1)
            win = np.concatenate([win[:, 1:], row[:, None, :]], axis=1)
        out[:, t] = lstm(win) + (0.0 if noise is None else noise[:, t].astype(f64))
    return out


def col_err(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    return np.abs(a - b).max(0) / np.abs(b).max(0)


def run_rollout(w, window0, cmd, gain=None, noise=None):
    t = lambda a: None if a is None else torch.tensor(a, device=DEV)
    out = fca.simulate_rollout(lstm_model(w), t(window0), t(cmd), gain=gain, noise=t(noise))
    assert out.shape == cmd.shape + (4,) and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("name,B,T,extras", [
    ("ref", 33, 12, False),      # a partial wave; the window fully regenerated after step 10
    ("ref", 33, 12, True),       # ... with a gain and output noise
    ("ref", 130, 3, False),      # crosses a workgroup
    ("h16", 17, 12, False),      # HS = 4
    ("h32", 16, 11, False),      # HS = 8
    ("ref", 1, 1, False),
])
def test_surrogate_rollout_matches_fp64_oracle(name, B, T, extras):
    w = load_weights(name)
    window0, cmd = rollout_inputs(B, T, 100 + B + T)
    gain = np.array([1.02, 0.97, 1.01, 0.99], np.float32) if extras else None
    noise = np.random.default_rng(9).normal(0, 0.01, (B, T, 4)).astype(np.float32) if extras else None
    got = run_rollout(w, window0, cmd, gain, noise)
    exp = rollout_oracle(w, window0, cmd, gain, noise)
    err = col_err(got, exp)
    print(f"{name} B={B} T={T} extras={extras}: per-column error {err}")
    assert np.isfinite(got).all()
    assert np.all(err <= 1e-5), err
    if extras:   # the gain and the noise are really applied
        plain = rollout_oracle(w, window0, cmd)
        assert np.all(col_err(got, plain) > 1e-3)


def test_surrogate_rollout_range_guard():
    """Pressure columns of the window at ~3e4 (beyond the f16 split's range once generated rows reach gain x x̂), W_ih0's
    pressure columns divided by the same 3e4: the same function of the same inputs, on windows whose values the guard
    (fcr_pack.h) must scale — from window0 AND from gain x the readout's bound. The rule of
    test_unscaled_window_values_stay_finite_like_torch_fp32: finite, and within max(1e-5, 4 x torch fp32's own distance
    to fp64)."""
    from oracle.rollout_torch import TorchLSTM
    B, T = 33, 12
    w = load_weights("ref")
    window0, cmd = rollout_inputs(B, T, 5)
    window0[:, :, 1:3] *= np.float32(3e4)
    gain = np.array([1.0, 3e4, 3e4, 1.0], np.float32)
    w = dict(w)
    w["Wih0"] = w["Wih0"].copy()
    w["Wih0"][:, 1:3] = (w["Wih0"][:, 1:3].astype(np.float64) / 3e4).astype(np.float32)
    got = run_rollout(w, window0, cmd, gain)
    exp = rollout_oracle(w, window0, cmd, gain)
    sim = TorchLSTM(5, 50, 4, 3)
    with torch.no_grad():
        for k in range(3):
            getattr(sim.lstm, f"weight_ih_l{k}").copy_(torch.as_tensor(w[f"Wih{k}"]))
            getattr(sim.lstm, f"weight_hh_l{k}").copy_(torch.as_tensor(w[f"Whh{k}"]))
        sim.fc.weight.copy_(torch.as_tensor(w["fcW"]))
        sim.fc.bias.copy_(torch.as_tensor(w["fcb"]))
        t32 = rollout_oracle(w, window0, cmd, gain,
                             lstm=lambda win: sim(torch.as_tensor(win, dtype=torch.float32)).numpy().astype(np.float64))
    e_hip, e_t32 = col_err(got, exp), col_err(t32, exp)
    print(f"guard: kernel {e_hip}, torch fp32 {e_t32}")
    assert np.isfinite(got).all()
    assert np.all(e_hip <= np.maximum(1e-5, 4 * e_t32)), (e_hip, e_t32)


# ---------------------------------------------------------------------------------------------
# ClosedLoop.loop: both tracks
# ---------------------------------------------------------------------------------------------
def test_closed_loop_loop_returns_both_tracks():
    B, T = 40, 30
    rng = np.random.default_rng(4)
    x0 = np.zeros((B, 5))
    x0[:, 2] = rng.uniform(1e6, 4e6, B)
    x0[:, 3] = rng.uniform(1e6, 4e6, B)
    ref = fca.closed_loop.reference_speeds(B, T, 1e-3, 1, 100)
    in_scale, out_scale = np.append(OUT_MAXABS, 0.3), OUT_MAXABS
    w = load_weights("ref")
    cl = fca.ClosedLoop(gpu_controller(), SCALERS)
    t = lambda a: torch.tensor(a, device=DEV)
    res, res_lstm = cl.loop(t(x0), t(ref), lstm_model(w), {"input": in_scale, "output": out_scale})
    x, u = cl.run(t(x0), t(ref))
    assert set(res) == {"y", "y_dot", "p1", "p2", "z", "ref", "u"} and set(res_lstm) == {"y_dot", "p1", "p2", "z"}
    for i, k in enumerate(("y", "y_dot", "p1", "p2", "z")):
        assert res[k].shape == (B, T + 1) and res[k].dtype == torch.float64 and torch.equal(res[k], x[:, :, i])
    assert torch.equal(res["u"], u) and res["u"].shape == (B, T)
    assert torch.equal(res["ref"], t(ref)) and res["ref"].dtype == torch.float64
    # fp64 restatement of Functions.py:1196-1231 on the GPU's own u (plant differences do not leak in)
    un = u.cpu().numpy()
    x_next = x0[:, 1:5]
    track = np.empty((B, T + 1, 4))
    track[:, 0] = x_next
    Wih, Whh = [w[f"Wih{k}"].astype(np.float64) for k in range(3)], [w[f"Whh{k}"].astype(np.float64) for k in range(3)]
    for s in range(T):
        row = np.concatenate([x_next, un[:, s:s + 1]], axis=1) / in_scale                  # :1196-1198
        win = np.repeat(row[:, None, :], 10, axis=1) if s == 0 else np.concatenate([win[:, 1:], row[:, None, :]], axis=1)
        y = lstm_forward(win, Wih, Whh, w["fcW"].astype(np.float64), w["fcb"].astype(np.float64))[0]
        x_next = y * out_scale                                                             # :1009
        track[:, s + 1] = x_next
    for i, k in enumerate(("y_dot", "p1", "p2", "z")):
        got = res_lstm[k]
        assert got.shape == (B, T + 1) and got.dtype == torch.float64 and got.device == x.device
        assert np.array_equal(got[:, 0].cpu().numpy(), x0[:, 1 + i])
        err = np.abs(got.cpu().numpy() - track[:, :, i]).max() / np.abs(track[:, :, i]).max()
        print(f"results_LSTM[{k}]: {err:.3g}")
        assert err <= 1e-5, (k, err)


# ---------------------------------------------------------------------------------------------
# the single-model closed loop at other controller widths than 50
# ---------------------------------------------------------------------------------------------
def _cl_constants():
    """kClBlock and kClMaxHidden of csrc/fcr_closed_loop.h: the lanes of a block, which also load the controller into
    LDS (``for i = threadIdx.x; i < hidden; i += kClBlock``), and the widest controller the kernels take."""
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "forging-control_amd", "csrc", "fcr_closed_loop.h")).read()
    return tuple(int(re.search(rf"constexpr int {k} = (\d+);", text).group(1)) for k in ("kClBlock", "kClMaxHidden"))


def loop_widths():
    """1, the widest, and 65 (past the 64 of the stand-alone FNN kernels; it takes the LDS loader past one pass only if
    a block has fewer than 65 lanes, else kClBlock + 1 does where the kernels accept it)."""
    block, widest = _cl_constants()
    second_pass = 65 if block < 65 else block + 1
    return sorted({1, 65, widest} | ({second_pass} if second_pass <= widest else set()))


def widened_controller(hidden):
    """The reference's 50-unit controller retold with ``hidden`` units: unit j is a copy of unit j mod 50 with its
    output weight divided by the number of copies and its bias moved by a seeded 1e-3, so the commands stay those of
    a controller the press was trained with and no two units are the same. One unit: the reference's unit of largest
    |W_out|."""
    W_inp, b_inp, W_out = (np.asarray(a, np.float64) for a in ctrl_weights())
    if hidden == 1:
        j = int(np.abs(W_out[0]).argmax())
        return tuple(a.astype(np.float32) for a in (W_inp[j:j + 1], b_inp[j:j + 1], 4.0 * W_out[:, j:j + 1]))
    src = np.arange(hidden) % 50
    copies = np.bincount(src, minlength=50)[src]
    b = b_inp[src] + 1e-3 * np.random.default_rng(hidden).standard_normal(hidden)
    return tuple(a.astype(np.float32) for a in (W_inp[src], b, W_out[:, src] / copies))


@pytest.mark.parametrize("hidden", loop_widths())
def test_single_model_loop_at_other_controller_widths(hidden):
    """ClosedLoop.run, plain and under process and measurement noise, B = 5 and T = 6: only width 50 runs in the tests
    above (7 in the bank's). Same bounds as there; the commands must really depend on the controller (they move, and
    differ between the trajectories)."""
    assert 1 <= hidden <= _cl_constants()[1]
    B, T = 5, 6
    x0, ref, w, v = press_case()
    x0, ref, w, v = x0[:B], np.ascontiguousarray(ref[:B, 17:17 + T]), w[:B, :T], v[:B, :T]   # the reference changes sign
    W_inp, b_inp, W_out = widened_controller(hidden)
    assert W_inp.shape == (hidden, 3) and W_out.shape == (1, hidden)
    ctrl = fca.FNNModel(3, hidden, 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(W_inp))
        ctrl.fc_inp.bias.copy_(torch.tensor(b_inp))
        ctrl.fc_out.weight.copy_(torch.tensor(W_out))
    cl = fca.ClosedLoop(ctrl, SCALERS)
    t = lambda a: torch.tensor(a, device=DEV)
    for name, ww, vv in (("plain", None, None), ("w+v", w, v)):
        xr, ur = closed_loop(x0, ref, W_inp, b_inp, W_out, SCALERS["input"][:2], SCALERS["y_dot"], SCALERS["output"],
                             process_noise=ww, meas_noise=vv)
        assert np.isfinite(xr).all() and xr[:, :, 1].min() > -0.5
        assert (ur != 0).mean() >= 0.25 and np.ptp(ur, axis=1).min() > 0       # every trajectory's command moves
        x, u = cl.run(t(x0), t(ref), process_noise=None if ww is None else t(ww), meas_noise=None if vv is None else t(vv))
        x, u = x.cpu().numpy(), u.cpu().numpy()
        assert x.shape == (B, T + 1, 5) and u.shape == (B, T) and np.array_equal(x[:, 0], x0)
        scale = np.abs(xr).reshape(-1, 5).max(0)
        err = (np.abs(x - xr).reshape(-1, 5) / scale).max(0)
        uerr = np.abs(u - ur).max() / np.abs(ur).max()
        print(f"hidden={hidden} {name}: state err {err}, u err {uerr:.3g}")
        assert np.all(err < 1e-5), (name, err)
        assert uerr <= 1e-5, (name, uerr)
