"""CPU: the batched harness loop's host side — the noise draws in the reference's order
(``closed_loop.harness_noise``, Functions.py:1176-1179, 1209-1210) and the host validation of
``fcr_lstm_rollout`` / ``fcr_closed_loop_run`` (no compute calls: there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

import forging_control_amd as fca

PROCESS_STD = np.array([0.5, 2.0, 5e7, 5e7, 2.0])     # UL/Main.py:88-112
MEAS_STD = np.array([1e-4, 1e-2, 1e4, 1e4, 1e-3])


def literal_draws(rs, n_traj, t_traj, process_std, meas_std):
    w, v = np.empty((n_traj, t_traj, 5)), np.empty((n_traj, t_traj, 5))
    for i in range(n_traj):
        for t in range(t_traj):
            w[i, t] = rs.normal(loc=0.0, scale=process_std)                  # Functions.py:1176
            v[i, t] = rs.normal(loc=0.0, scale=meas_std)                     # :1179
            rs.normal(loc=0.0, scale=np.array([0.0, 0.0, 0.0, 0.0]))         # w0_NN, :1209-1210
    return w, v


def test_harness_noise_draws_in_the_reference_order():
    w, v = fca.closed_loop.harness_noise(2, 3, PROCESS_STD, MEAS_STD, np.random.RandomState(42))
    we, ve = literal_draws(np.random.RandomState(42), 2, 3, PROCESS_STD, MEAS_STD)
    assert w.shape == v.shape == (2, 3, 5) and w.dtype == v.dtype == np.float64
    assert np.array_equal(w, we) and np.array_equal(v, ve)
    assert np.abs(w).min() > 0 and np.abs(v).min() > 0


def test_harness_noise_zero_std_still_consumes_the_stream():
    rs, rl = np.random.RandomState(42), np.random.RandomState(42)
    w, v = fca.closed_loop.harness_noise(2, 3, PROCESS_STD, 0.0, rs)
    we, ve = literal_draws(rl, 2, 3, PROCESS_STD, np.zeros(5))
    assert np.array_equal(w, we) and np.array_equal(v, ve) and not v.any()
    assert rs.normal() == rl.normal()      # a fourth draw after it matches


def lro_dims(**kw):
    base = dict(B=64, N=12, H=50, precision=0)
    base.update(kw)
    return fca.rollout.make_dims(base["B"], base["N"], base["H"], 3, 1, 0.0, precision=base["precision"])


def lro_size(**kw):
    lib = fca._native.load()
    out = ctypes.c_size_t(0)
    d = lro_dims(**kw)
    return lib.fcr_lstm_rollout_workspace_size(ctypes.byref(d), ctypes.byref(out)), out.value


@pytest.mark.parametrize("kw,code", [(dict(H=64), -4), (dict(precision=1), -4), (dict(N=0), -1), (dict(B=-1), -1)])
def test_lstm_rollout_refuses_what_it_is_not_built_for(kw, code):
    lib = fca._native.load()
    assert lro_size(**kw)[0] == code
    assert lib.fcr_last_error().decode()
    d, w = lro_dims(**kw), fca._native.FcrWeights()
    assert lib.fcr_lstm_rollout(ctypes.byref(d), ctypes.byref(w), None, None, None, None, None, None, 0, None) == code


def test_lstm_rollout_validates_before_any_device_call():
    lib = fca._native.load()
    d, w = lro_dims(), fca._native.FcrWeights()
    rc = lib.fcr_lstm_rollout(ctypes.byref(d), ctypes.byref(w), None, None, None, None, None, None, 0, None)
    assert rc == -1 and "NULL" in lib.fcr_last_error().decode()
    assert lib.fcr_lstm_rollout(None, ctypes.byref(w), None, None, None, None, None, None, 0, None) == -1
    assert "NULL" in lib.fcr_last_error().decode()
    assert lib.fcr_lstm_rollout_workspace_size(ctypes.byref(d), None) == -1 and "NULL" in lib.fcr_last_error().decode()
    # an empty batch is a no-op, whatever the pointers
    d0 = lro_dims(B=0)
    assert lib.fcr_lstm_rollout(ctypes.byref(d0), ctypes.byref(w), None, None, None, None, None, None, 0, None) == 0


def test_lstm_rollout_workspace_does_not_grow_with_the_steps():
    (rc1, n1), (rc300, n300) = lro_size(B=4096, N=1), lro_size(B=4096, N=300)
    assert rc1 == 0 and rc300 == 0 and n1 == n300 > 0
    # layer 1's h records of ONE window per 16-trajectory wave (10 cells x 64 lanes x 13 slots x 4 B) and the packs
    assert 256 * 10 * 64 * 13 * 4 <= n1 < 256 * 10 * 64 * 13 * 4 + (1 << 20)
    assert lro_size(B=64, N=300)[1] < n1


def test_closed_loop_zeroed_struct_still_means_no_noise():
    lib = fca._native.load()
    a = fca._native.FcrClosedLoop()
    assert a.process_noise is None and a.meas_noise is None
    a.B, a.T, a.ts, a.substeps, a.ctrl_hidden = 4, 3, 1e-3, 4, 50
    a.in_scale[0] = a.in_scale[1] = a.ref_scale = a.out_scale = 1.0
    assert lib.fcr_closed_loop_run(ctypes.byref(a), None) == -1 and "NULL" in lib.fcr_last_error().decode()
    a.process_noise = 12                                   # fp64 buffers are 8-byte aligned
    a.x0 = a.ref = a.x = a.u = a.ctrl_w_inp = a.ctrl_b_inp = a.ctrl_w_out = 64
    assert lib.fcr_closed_loop_run(ctypes.byref(a), None) == -1 and "aligned" in lib.fcr_last_error().decode()


def test_python_entry_points_check_their_arguments_on_the_host():
    ctrl = fca.FNNModel(3, 50, 1, 1)
    cl = fca.ClosedLoop(ctrl, {"input": np.ones(3), "y_dot": 1.0, "output": 1.0})
    with pytest.raises(RuntimeError, match="ROCm device only"):    # the existing checks come first
        cl.run(torch.zeros(2, 5), torch.zeros(2, 3), process_noise=torch.zeros(2, 3, 4))
    sim = fca.LSTMModel(5, 50, 4, 3)
    with pytest.raises(ValueError, match="window0"):
        fca.simulate_rollout(sim, torch.zeros(2, 9, 5), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="cmd"):
        fca.simulate_rollout(sim, torch.zeros(2, 10, 5), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="noise"):
        fca.simulate_rollout(sim, torch.zeros(2, 10, 5), torch.zeros(2, 3), noise=torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match="gain"):
        fca.simulate_rollout(sim, torch.zeros(2, 10, 5), torch.zeros(2, 3), gain=[1.0, 1.0])
    with pytest.raises(RuntimeError, match="ROCm device only"):
        fca.simulate_rollout(sim, torch.zeros(2, 10, 5), torch.zeros(2, 3))
