"""Training the surrogate on its free run, the parts that need no GPU: the fp64 references (tests/free_run_ref.py)
against finite differences and against each other, the batch producer, the CPU route of ``free_run`` and the argument
checks of fcr_lstm_rollout_backward."""
import ctypes
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import free_run_ref as R
from conftest import ROOT
from test_gpu_loop import load_weights
from test_surrogate import params_for

GAIN = (1.1, 0.9, 1.05, 0.8)


def test_autograd_matches_finite_differences():
    p = params_for(3, seed=1)
    d = R.inputs(2, 3, 0)
    noise = 0.01 * np.random.default_rng(1).standard_normal((2, 3, 4))
    args = (d["window0"], d["cmd"], GAIN, noise)
    g = R.autograd_free_run(p, *args, target=d["target"])
    rng = np.random.default_rng(0)
    for key, k in (("Wih", 0), ("Whh", 2), ("Wih", 1), ("Whh", 0)):
        W = p[key][k]
        for _ in range(3):
            i = tuple(rng.integers(0, s) for s in W.shape)
            eps = 1e-6
            W[i] += eps
            lp = R.autograd_free_run(p, *args, target=d["target"])["loss"]
            W[i] -= 2 * eps
            lm = R.autograd_free_run(p, *args, target=d["target"])["loss"]
            W[i] += eps
            assert (lp - lm) / (2 * eps) == pytest.approx(g[f"{key}{k}"][i], rel=1e-6, abs=1e-10)


@pytest.mark.parametrize("T", [1, 2, 10, 12])
@pytest.mark.parametrize("H", [7, 50])
def test_recursion_matches_autograd(H, T):
    p = params_for(H, seed=H)
    d = R.inputs(3, T, 10 * T + H)
    noise = 0.01 * np.random.default_rng(T).standard_normal((3, T, 4))
    a = R.autograd_free_run(p, d["window0"], d["cmd"], GAIN, noise, G=d["G"])
    r = R.recursion(p, d["window0"], d["cmd"], GAIN, noise, G=d["G"])
    for k in R.KEYS:
        assert R.rel(r[k], a[k]) <= 1e-9, (k, R.rel(r[k], a[k]))
    assert np.all(a["window0"][:, 9, 4] == 0.0) and np.all(r["window0"][:, 9, 4] == 0.0)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_moves_a_gradient(mutant):
    """On the inputs of the GPU parity test's ring-wrapping case (the reference's weights, B = 33, T = 12, a gain)."""
    p = R.params_of(load_weights("ref"))
    d = R.inputs(33, 12, 33 * 12)
    noise = 0.01 * np.random.default_rng(12).standard_normal((33, 12, 4))
    good = R.recursion(p, d["window0"], d["cmd"], GAIN, noise, G=d["G"])
    bad = R.recursion(p, d["window0"], d["cmd"], GAIN, noise, G=d["G"], mutant=mutant)
    moved = {k: np.abs(bad[k] - good[k]).max() / np.abs(good[k]).max() for k in R.KEYS}
    print(mutant, {k: f"{v:.2e}" for k, v in moved.items()})
    assert max(moved.values()) > 1e-3, moved


# ---------------------------------------------------------------------------------------------------- batch producer

def plain_batches(Z, Y, traj_len, T, lookback, order, batch_size):
    samples = []
    for g in order:
        k, i = divmod(int(g), traj_len - T)
        base = k * traj_len
        w = np.stack([Z[base + max(i - lookback + 1 + j, 0)] for j in range(lookback)])
        c = np.array([Z[base + i + t, 4] for t in range(T)])
        y = np.stack([Y[base + i + 1 + t] for t in range(T)])
        samples.append((w, c, y))
    for s in range(0, len(samples), batch_size):
        chunk = samples[s:s + batch_size]
        yield tuple(np.stack([c[n] for c in chunk]) for n in range(3))


def test_free_run_batches_against_a_plain_loop():
    rng = np.random.default_rng(3)
    traj_len, ntraj, T = 17, 3, 4
    Z = rng.standard_normal((traj_len * ntraj, 5)).astype(np.float32)
    Y = rng.standard_normal((traj_len * ntraj, 4)).astype(np.float32)
    n = ntraj * (traj_len - T)
    got = list(fca.free_run_batches(torch.tensor(Z), traj_len, T, 8, Y=torch.tensor(Y)))
    want = list(plain_batches(Z, Y, traj_len, T, 10, range(n), 8))
    assert len(got) == len(want) == (n + 7) // 8 and got[-1][0].shape[0] == n - 8 * (len(got) - 1)
    for g, w in zip(got, want):
        assert g[0].shape[1:] == (10, 5) and g[1].shape[1:] == (T,) and g[2].shape[1:] == (T, 4)
        for a, b in zip(g, w):
            assert np.array_equal(a.numpy(), b)
    # sample 0 (i = 0 < 9): the window is row 0 repeated; the last admissible start row reads the trajectory's last row
    assert np.array_equal(got[0][0][0].numpy(), np.repeat(Z[:1], 10, 0))
    last = traj_len - T - 1
    w, c, y = (t[last] for t in (torch.cat([g[i] for g in got]) for i in range(3)))
    assert np.array_equal(y[-1].numpy(), Y[traj_len - 1]) and np.array_equal(c.numpy(), Z[last:last + T, 4])
    # Y defaults to the state columns of Z
    d = next(iter(fca.free_run_batches(torch.tensor(Z), traj_len, T, 5)))
    assert np.array_equal(d[2][2].numpy(), Z[3:3 + T, :4])
    # the longest horizon with a sample, and the first without
    assert sum(b[0].shape[0] for b in fca.free_run_batches(Z, traj_len, traj_len - 1, 2)) == ntraj
    with pytest.raises(ValueError, match="leaves no sample"):
        fca.free_run_batches(Z, traj_len, traj_len, 2)
    with pytest.raises(ValueError, match="multiple of traj_len"):
        fca.free_run_batches(Z[:-1], traj_len, T, 2)


def test_free_run_batches_shuffle_is_reproducible():
    rng = np.random.default_rng(4)
    Z = rng.standard_normal((40, 5)).astype(np.float32)
    run = lambda seed: list(fca.free_run_batches(Z, 20, 3, 7, shuffle=True, generator=torch.Generator().manual_seed(seed)))
    a, b, c = run(5), run(5), run(6)
    assert all(torch.equal(x, y) for ba, bb in zip(a, b) for x, y in zip(ba, bb))
    assert not all(torch.equal(x, y) for ba, bc in zip(a, c) for x, y in zip(ba, bc))
    order = torch.randperm(2 * 17, generator=torch.Generator().manual_seed(5)).tolist()
    want = list(plain_batches(Z, Z[:, :4], 20, 3, 10, order, 7))
    for g, w in zip(a, want):
        for x, y in zip(g, w):
            assert np.array_equal(x.numpy(), y)


# ---------------------------------------------------------------------------------------------------- CPU route

def test_free_run_on_cpu_tensors_is_the_modules_own_lstm():
    w = load_weights("ref")
    from test_gpu_loop import lstm_model
    m = lstm_model(w, "cpu")
    d = R.inputs(5, 4, 7)
    noise = 0.01 * np.random.default_rng(2).standard_normal((5, 4, 4))
    ref = R.autograd_free_run(R.params_of(w), d["window0"], d["cmd"], GAIN, noise, target=d["target"])
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    w0, c = f(d["window0"]).requires_grad_(True), f(d["cmd"]).requires_grad_(True)
    xhat = fca.free_run(m, w0, c, GAIN, f(noise))
    assert fca.free_run.last_route == "host" and xhat.shape == (5, 4, 4)
    torch.nn.functional.mse_loss(xhat, f(d["target"])).backward()
    got = {"window0": w0.grad, "cmd": c.grad, "fcW": m.fc.weight.grad, "fcb": m.fc.bias.grad}
    for k in range(3):
        got[f"Wih{k}"], got[f"Whh{k}"] = getattr(m.lstm, f"weight_ih_l{k}").grad, getattr(m.lstm, f"weight_hh_l{k}").grad
    assert R.rel(xhat.detach().numpy(), ref["xhat"]) <= 1e-5
    for k in R.KEYS:
        assert R.rel(got[k].numpy(), ref[k]) <= 1e-5, (k, R.rel(got[k].numpy(), ref[k]))
    assert torch.all(w0.grad[:, 9, 4] == 0)


def test_free_run_checks_its_arguments():
    m = fca.LSTMModel(5, 8, 4, 3)
    w0, c = torch.zeros(3, 10, 5), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="window0"):
        fca.free_run(m, torch.zeros(3, 9, 5), c)
    with pytest.raises(ValueError, match="cmd"):
        fca.free_run(m, w0, torch.zeros(2, 2))
    with pytest.raises(ValueError, match="cmd"):
        fca.free_run(m, w0, torch.zeros(3, 0))
    with pytest.raises(ValueError, match="noise"):
        fca.free_run(m, w0, c, noise=torch.zeros(3, 2, 3))
    with pytest.raises(ValueError, match="gain"):
        fca.free_run(m, w0, c, gain=(1.0, 2.0))


# ---------------------------------------------------------------------------------------------------- ABI

def _sizes(B, T, H=50, layers=3, precision=0):
    lib = fca._native.load()
    d = fca.rollout.make_dims(B, T, H, layers, 1, 0.0)
    d.precision = precision
    fwd, bwd = ctypes.c_size_t(0), ctypes.c_size_t(0)
    return (lib.fcr_lstm_rollout_workspace_size(ctypes.byref(d), ctypes.byref(fwd)), fwd.value,
            lib.fcr_lstm_rollout_backward_workspace_size(ctypes.byref(d), ctypes.byref(bwd)), bwd.value)


def test_backward_abi_validates_before_any_device_call():
    N = fca._native
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "fcr.h")).read()
    for name in ("fcr_lstm_rollout_backward_workspace_size", "fcr_lstm_rollout_backward"):
        assert name in N.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    rc_f, fwd, rc_b, b10 = _sizes(256, 10)
    assert rc_f == 0 and rc_b == 0 and b10 > fwd > 0
    assert _sizes(256, 11)[3] > b10 > _sizes(256, 9)[3] > _sizes(256, 1)[3] > fwd
    assert _sizes(241, 10)[3] == b10                      # whole waves of 16 trajectories per step
    assert _sizes(0, 10)[2] == 0
    assert _sizes(16, 3, H=64)[2] == -4 and "H=64" in lib.fcr_last_error().decode()
    assert _sizes(16, 3, precision=N.PRECISION_F16)[2] == -4 and "precision" in lib.fcr_last_error().decode()
    assert _sizes(16, 3, layers=2)[2] == -4
    assert _sizes(16, 0)[2] == -1
    assert _sizes(2 ** 30, 2)[2] == -1 and "too large" in lib.fcr_last_error().decode()
    d = fca.rollout.make_dims(16, 3, 50, 3, 1, 0.0)
    assert lib.fcr_lstm_rollout_backward_workspace_size(ctypes.byref(d), None) == -1
    assert lib.fcr_lstm_rollout_backward_workspace_size(None, ctypes.byref(ctypes.c_size_t(0))) == -1

    w, out = N.FcrWeights(), N.FcrLstmRolloutGrads()
    one = ctypes.c_void_p(256)   # a non-NULL, aligned address that no check may dereference
    call = lambda dims, w_, a, out_, ws, nbytes: lib.fcr_lstm_rollout_backward(
        ctypes.byref(dims), ctypes.byref(w_), a, a, None, a, a, ctypes.byref(out_) if out_ is not None else None, ws,
        nbytes, None)
    assert call(d, w, None, out, one, 1 << 40) == -1 and "NULL" in lib.fcr_last_error().decode()
    assert call(d, w, one, None, one, 1 << 40) == -1
    assert call(d, w, one, out, one, 1 << 40) == -1 and "gradient of layer 0" in lib.fcr_last_error().decode()
    for l in range(3):
        out.g_w_ih[l] = out.g_w_hh[l] = 256
    assert call(d, w, one, out, one, 1 << 40) == -1 and "readout" in lib.fcr_last_error().decode()
    out.g_fc_w = out.g_fc_b = 256
    assert call(d, w, one, out, one, 1 << 40) == -1 and "weight pointer" in lib.fcr_last_error().decode()
    for l in range(3):
        w.w_ih[l] = w.w_hh[l] = 256
    w.fc_w = w.fc_b = 256
    assert call(d, w, one, out, None, 1 << 40) == -1
    assert call(d, w, one, out, ctypes.c_void_p(264), 1 << 40) == -1 and "aligned" in lib.fcr_last_error().decode()
    need = _sizes(16, 3)[3]
    assert call(d, w, one, out, one, need - 1) == -2 and str(need) in lib.fcr_last_error().decode()
    for bad in (fca.rollout.make_dims(16, 3, 64, 3, 1, 0.0), fca.rollout.make_dims(16, 3, 50, 2, 1, 0.0)):
        assert call(bad, w, one, out, one, 1 << 40) == -4
    assert call(fca.rollout.make_dims(16, 0, 50, 3, 1, 0.0), w, one, out, one, 1 << 40) == -1
    d0 = fca.rollout.make_dims(0, 3, 50, 3, 1, 0.0)
    assert call(d0, N.FcrWeights(), None, None, None, 0) == 0   # B = 0: a no-op
