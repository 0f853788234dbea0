"""Batched closed-loop inference on the rollout kernel.

The reference's closed-loop harness steps, per trajectory and per sampling instant, the LSTM surrogate
on a 10-row window (``NeuralNetwork.simulator_make_step``, Functions.py:969-1011, window built at
:1196-1207) and the FNN controller (``FeasibilityRecovery.NN_make_step``, :1560-1613, without the
CasADi feasibility recovery). Here the LSTM step is one window of the fused gfx950 forward
(``fcr_forward`` with N = 1 and u0 = the window's last command, no backward state) over a whole batch
of trajectories; the controller is the 3->50->1 FNN.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native
from .functions import _simulator_params
from .rollout import WINDOW_ROWS, _ptr, _stream, make_dims, rollout


def simulate_step(simulator, windows: torch.Tensor, noise: torch.Tensor | None = None) -> torch.Tensor:
    """x̂ = LSTMModel(window) (+ noise) for every window of a (B, 10, 5) batch on a ROCm device: the
    scaled prediction of ``simulator_make_step`` before ``scalers['output'].inverse_transform``."""
    if windows.dim() != 3 or windows.shape[1:] != (WINDOW_ROWS, 5):
        raise ValueError(f"windows must be (B, 10, 5), got {tuple(windows.shape)}")
    B, dev = windows.shape[0], windows.device
    f32 = dict(dtype=torch.float32, device=dev)
    zero_ctrl = (torch.zeros(1, 3, **f32), torch.zeros(1, **f32), torch.zeros(1, 1, **f32))   # unused at N = 1
    with torch.no_grad():
        w = windows.to(torch.float32).contiguous()
        out = rollout(torch.zeros(B, 3, **f32), w[:, WINDOW_ROWS - 1, 4].contiguous(), w, zero_ctrl,
                      tuple(_to(p, dev) for p in _flat(_simulator_params(simulator))), 1, 0.0,
                      None if noise is None else noise.to(**f32).reshape(B, 1, 4))
    return out[5][:, 0, :]


def simulate_rollout(simulator, window0: torch.Tensor, cmd: torch.Tensor, gain=None,
                     noise: torch.Tensor | None = None) -> torch.Tensor:
    """The surrogate free-running for T steps on its own predictions and a given command sequence — the
    ``results_LSTM`` track of ``NeuralNetwork.loop`` (Functions.py:1196-1231) — for a batch, in scaled units.

    ``window0`` (B,10,5) and ``cmd`` (B,T) on a ROCm device; ``gain``: 4 host numbers (None = 1), what the harness's
    ``scalers['output'].inverse_transform`` then ``scalers['input'].transform`` amount to between steps
    (out_scale / in_scale[:4]); ``noise`` (B,T,4) or None. Step 0 runs ``window0`` with its last row's command
    replaced by ``cmd[:,0]``; step t >= 1 drops the oldest row and appends ``[gain * x̂_{t-1}, cmd[:,t]]``;
    ``x̂_t = LSTM(window_t) + noise[:,t]``. Returns x̂ (B,T,4).

    H <= 52 runs all T steps in ONE launch (``fcr_lstm_rollout``, csrc/fcr_lstm_rollout.h); a wider surrogate
    composes T calls of :func:`simulate_step` with the window update in torch."""
    if window0.dim() != 3 or window0.shape[1:] != (WINDOW_ROWS, 5):
        raise ValueError(f"window0 must be (B, 10, 5), got {tuple(window0.shape)}")
    B, dev = window0.shape[0], window0.device
    if cmd.dim() != 2 or cmd.shape[0] != B or cmd.shape[1] < 1:
        raise ValueError(f"cmd must be (B, T) with T >= 1 and B = {B}, got {tuple(cmd.shape)}")
    T = cmd.shape[1]
    if noise is not None and tuple(noise.shape) != (B, T, 4):
        raise ValueError(f"noise must be (B, T, 4) = {(B, T, 4)}, got {tuple(noise.shape)}")
    g = np.ones(4, np.float32) if gain is None else np.asarray(gain, np.float32).reshape(-1)
    if g.shape != (4,):
        raise ValueError(f"gain must hold 4 numbers, got {g.shape[0]}")
    if dev.type != "cuda":
        raise RuntimeError(f"simulate_rollout runs on a ROCm device only (window0 on {dev})")
    for name, t in (("cmd", cmd), ("noise", noise)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on {dev}, found it on {t.device}")
    f32 = dict(dtype=torch.float32, device=dev)
    w_ih, w_hh, fc_w, fc_b = _flat(_simulator_params(simulator))
    H = w_hh[0].shape[1]
    with torch.no_grad():
        w = window0.to(**f32).contiguous()
        c = cmd.to(**f32).contiguous()
        nz = None if noise is None else noise.to(**f32).contiguous()
        if H > 52:
            return _rollout_by_steps(simulator, w, c, torch.as_tensor(g, device=dev), nz)
        keep = [t.detach().to(**f32).contiguous() for t in list(w_ih) + list(w_hh) + [fc_w, fc_b]]
        fw = _native.FcrWeights()
        for l in range(3):
            fw.w_ih[l], fw.w_hh[l] = keep[l].data_ptr(), keep[3 + l].data_ptr()
        fw.fc_w, fw.fc_b = keep[6].data_ptr(), keep[7].data_ptr()
        dims = make_dims(B, T, H, 3, 1, 0.0)
        lib = _native.load()
        nbytes = ctypes.c_size_t(0)
        _native.check(lib.fcr_lstm_rollout_workspace_size(ctypes.byref(dims), ctypes.byref(nbytes)),
                      "fcr_lstm_rollout_workspace_size")
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        xhat = torch.empty(B, T, 4, **f32)
        _native.check(lib.fcr_lstm_rollout(ctypes.byref(dims), ctypes.byref(fw), _ptr(w), _ptr(c),
                                           (ctypes.c_float * 4)(*g.tolist()), _ptr(nz), _ptr(xhat), _ptr(ws),
                                           ws.numel(), _stream(dev)), "fcr_lstm_rollout")
    return xhat


def _rollout_by_steps(simulator, window0, cmd, gain, noise):
    """simulate_rollout as T launches of simulate_step with the window shuffled in torch between them."""
    B, T = cmd.shape
    win = window0.clone()
    win[:, WINDOW_ROWS - 1, 4] = cmd[:, 0]
    out = torch.empty(B, T, 4, dtype=torch.float32, device=window0.device)
    for t in range(T):
        if t > 0:
            row = torch.cat([gain * out[:, t - 1], cmd[:, t:t + 1]], dim=1)
            win = torch.cat([win[:, 1:], row[:, None, :]], dim=1)
        out[:, t] = simulate_step(simulator, win, None if noise is None else noise[:, t])
    return out


def controller_step(controller, X: torch.Tensor) -> torch.Tensor:
    """u = FNNModel(X) for a (B, 3) batch of scaled controller inputs (the NN part of NN_make_step)."""
    with torch.no_grad():
        return controller(X)


def simulator_make_step(X: np.ndarray, model, scalers: dict, noise: np.ndarray, device=None) -> np.ndarray:
    """Drop-in for ``NeuralNetwork.simulator_make_step`` (Functions.py:969-1011) with the same arguments:
    X (B, 10, 5) or (10, 5) scaled LSTM inputs, noise (4,) or (B, 4) in scaled units; returns the unscaled
    prediction ``scalers['output'].inverse_transform(model(X) + noise)``.

    ``device`` defaults to where the model's weights are. A model on a ROCm device runs the whole batch
    through the fused gfx950 forward; a model the harness moved to the CPU (UL/Main.py:347-348) runs
    ``model(X_new, "cpu")`` exactly as the reference does — its own ``nn.LSTM`` (LSTMModel.forward)."""
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    Xt = torch.as_tensor(np.asarray(X, np.float32), device=device)
    if Xt.dim() == 2:
        Xt = Xt.unsqueeze(0)
    nz = torch.as_tensor(np.broadcast_to(np.asarray(noise, np.float32), (Xt.shape[0], 4)).copy(), device=device)
    if device.type == "cpu":
        model.eval()
        with torch.no_grad():
            y = (model(Xt, "cpu") + nz).numpy()
        return scalers["output"].inverse_transform(y)
    y = simulate_step(model, Xt, nz).cpu().numpy().astype(np.float64)
    return scalers["output"].inverse_transform(y)


def _flat(params):
    w_ih, w_hh, fc_w, fc_b = params
    return (list(w_ih), list(w_hh), fc_w, fc_b)


def _to(p, dev):
    if isinstance(p, list):
        return [t.detach().to(dev) for t in p]
    return p.detach().to(dev)
