"""LSTM surrogate training on the gfx950 path.

The reference trains the plant surrogate ``LSTMModel(5, 50, 4, 3)`` with ``nn.MSELoss`` and AdamW
(Model_NN/Main.py:218-242) through ``NeuralNetwork.train_model`` (Model_NN/Functions.py:520-569), i.e.
``output = model(X, device); loss = loss_function(output, y.squeeze()); loss.backward();
optimizer.step()`` per batch. Here ``LSTMModel.forward`` on a ROCm device runs :class:`LSTMFunction`:
``fcr_lstm_forward`` and, on ``backward``, ``fcr_lstm_backward``. For H <= 52 (the reference's H = 50)
they are the rollout's fused split-f16 cell kernels over one window (csrc/fcr_sur.h: one forward launch,
one backward launch that also keeps every cell's dgates, and one hand-written weight-gradient product per
layer over all 10·B (step, sample) rows); wider models run the per-cell path (csrc/fcr_wide.h). Every
LSTM weight, the readout and — when it requires grad — the input window receive gradients, so the
reference's loop and optimizer run unchanged.

:func:`free_run` / :func:`train_free_run` train the same model on its T-step free run instead of one step ahead
(``fcr_lstm_rollout`` forward, ``fcr_lstm_rollout_backward`` backward, csrc/fcr_lro_bwd.h).
"""
from __future__ import annotations

import ctypes

import torch

from . import _native
from .rollout import WINDOW_ROWS, make_dims


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _weights(w_ih, w_hh, fc_w, fc_b):
    w = _native.FcrWeights()
    w.w_ih = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in w_ih])
    w.w_hh = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in w_hh])
    w.fc_w, w.fc_b = fc_w.data_ptr(), fc_b.data_ptr()
    return w


class LSTMFunction(torch.autograd.Function):
    """y = LSTMModel(x) with gradients for x and every weight (fcr_lstm_forward / fcr_lstm_backward)."""

    @staticmethod
    def forward(ctx, x, w_ih0, w_ih1, w_ih2, w_hh0, w_hh1, w_hh2, fc_w, fc_b):
        dev = x.device
        B, H = x.shape[0], w_hh0.shape[1]
        dims = make_dims(B, 1, H, 3, 1, 0.0)
        ts = [t.detach().to(torch.float32).contiguous() for t in (x, w_ih0, w_ih1, w_ih2, w_hh0, w_hh1, w_hh2, fc_w, fc_b)]
        xc, w_ih, w_hh, fcw, fcb = ts[0], ts[1:4], ts[4:7], ts[7], ts[8]
        w = _weights(w_ih, w_hh, fcw, fcb)
        need_grad = any(ctx.needs_input_grad)
        lib = _native.load()
        nbytes = ctypes.c_size_t(0)
        _native.check(lib.fcr_lstm_workspace_size(ctypes.byref(dims), int(need_grad), ctypes.byref(nbytes)),
                      "fcr_lstm_workspace_size")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        y = torch.empty(B, 4, dtype=torch.float32, device=dev)
        stream = _native.stream(dev)
        _native.check(lib.fcr_lstm_forward(ctypes.byref(dims), ctypes.byref(w), _p(xc), _p(y), int(need_grad),
                                           _p(ws), ws.numel(), stream), "fcr_lstm_forward")
        if need_grad:
            ctx.dims, ctx.ws, ctx.tensors = dims, ws, ts
        return y

    @staticmethod
    def backward(ctx, dy):
        ts = ctx.tensors
        xc, w_ih, w_hh, fcw, fcb = ts[0], ts[1:4], ts[4:7], ts[7], ts[8]
        dev = xc.device
        g = [torch.empty_like(t) for t in ts]
        w = _weights(w_ih, w_hh, fcw, fcb)
        g_ih = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in g[1:4]])
        g_hh = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in g[4:7]])
        dyc = dy.to(torch.float32).contiguous()
        lib = _native.load()
        _native.check(lib.fcr_lstm_backward(ctypes.byref(ctx.dims), ctypes.byref(w), _p(dyc), g_ih, g_hh, _p(g[7]),
                                            _p(g[8]), _p(g[0]) if ctx.needs_input_grad[0] else None, _p(ctx.ws),
                                            ctx.ws.numel(), _native.stream(dev)),
                      "fcr_lstm_backward")
        return tuple(gi if need else None for gi, need in zip(g, ctx.needs_input_grad))


def hip_shape_ok(model, x) -> bool:
    """True when ``model(x)`` is the shape the gfx950 LSTM path is built for: LSTM(5, H, 3) without LSTM
    bias -> Linear(H, 4), fp32 (B, 10, 5) windows on the device the weights live on."""
    lstm = model.lstm
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and tuple(x.shape[1:]) == (WINDOW_ROWS, 5)
            and not lstm.bias and lstm.num_layers == 3 and lstm.input_size == 5 and model.fc.out_features == 4
            and lstm.batch_first and all(p.dtype == torch.float32 and p.device == x.device for p in model.parameters()))


def lstm_apply(model, x: torch.Tensor) -> torch.Tensor:
    """LSTMModel forward on the HIP path (x (B, 10, 5) on a ROCm device); :func:`hip_shape_ok` must hold."""
    if not hip_shape_ok(model, x):
        raise RuntimeError("the gfx950 LSTM path is built for LSTMModel(5, H, 4, 3) without LSTM bias on fp32 "
                           f"(B, 10, 5) device windows (Model_NN/Main.py:225, UL/Main.py:144-154); got {tuple(x.shape)} "
                           f"on {x.device}")
    lstm = model.lstm
    p = [getattr(lstm, f"weight_ih_l{k}") for k in range(3)] + [getattr(lstm, f"weight_hh_l{k}") for k in range(3)]
    return LSTMFunction.apply(x, *p, model.fc.weight, model.fc.bias)


def captured_step(model, loss_function, optimizer, device, warmup=2):
    """The batch step of :func:`train_model` as a :class:`~.graphed.CapturedStep` (one HIP graph replay
    per batch; pass it as ``train_model(..., step=...)``)."""
    from .graphed import CapturedStep

    def body(X, y):
        loss = loss_function(model(X, device), y.squeeze())
        loss.backward()
        return (loss.detach(),)

    return CapturedStep(model.parameters(), optimizer, body, None, warmup)


def train_model(data_loader, model, loss_function, optimizer, device, step=None):
    """Model_NN/Functions.py:520-569 with the same arguments and return value (average batch loss).
    ``step`` (optional, from :func:`captured_step`) replays each batch from a HIP graph and reads the
    summed loss once per epoch instead of once per batch."""
    model.train()
    if step is not None:
        total_dev = None
        for X, y in data_loader:
            (loss,) = step(X.to(device), y.to(device))
            total_dev = loss.clone() if total_dev is None else total_dev + loss
        return (float(total_dev.item()) if total_dev is not None else 0.0) / len(data_loader)
    total = 0.0
    for X, y in data_loader:
        X, y = X.to(device), y.to(device)
        optimizer.zero_grad()
        output = model(X, device)
        loss = loss_function(output, y.squeeze())
        loss.backward()
        optimizer.step()
        total += loss.item()
    return total / len(data_loader)


# ---------------------------------------------------------------------------------------------------------------------
# Training the surrogate on its free run: x̂ (B,T,4) of the command-driven rollout (inference.simulate_rollout), attached
# to the graph. H <= 52 on a ROCm device: fcr_lstm_rollout forward, fcr_lstm_rollout_backward (csrc/fcr_lro_bwd.h)
# backward, a number of launches that does not depend on T.


class FreeRunFunction(torch.autograd.Function):
    """x̂ = free run of LSTMModel from ``window0`` under ``cmd`` with gradients for every weight, ``window0`` and ``cmd``
    (fcr_lstm_rollout / fcr_lstm_rollout_backward). ``gain``: 4 host floats; ``noise`` (B,T,4) or None (no gradient)."""

    @staticmethod
    def forward(ctx, gain, noise, window0, cmd, w_ih0, w_ih1, w_ih2, w_hh0, w_hh1, w_hh2, fc_w, fc_b):
        dev = window0.device
        B, T, H = window0.shape[0], cmd.shape[1], w_hh0.shape[1]
        ts = [t.detach().to(torch.float32).contiguous()
              for t in (window0, cmd, w_ih0, w_ih1, w_ih2, w_hh0, w_hh1, w_hh2, fc_w, fc_b)]
        nz = None if noise is None else noise.detach().to(torch.float32).contiguous()
        dims = make_dims(B, T, H, 3, 1, 0.0)
        w = _weights(ts[2:5], ts[5:8], ts[8], ts[9])
        g4 = (ctypes.c_float * 4)(*[float(v) for v in gain])
        lib = _native.load()
        nbytes = ctypes.c_size_t(0)
        _native.check(lib.fcr_lstm_rollout_workspace_size(ctypes.byref(dims), ctypes.byref(nbytes)),
                      "fcr_lstm_rollout_workspace_size")
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        xhat = torch.empty(B, T, 4, dtype=torch.float32, device=dev)
        _native.check(lib.fcr_lstm_rollout(ctypes.byref(dims), ctypes.byref(w), _p(ts[0]), _p(ts[1]), g4, _p(nz),
                                           _p(xhat), _p(ws), ws.numel(), _native.stream(dev)), "fcr_lstm_rollout")
        if any(ctx.needs_input_grad):
            ctx.dims, ctx.gain, ctx.tensors, ctx.xhat = dims, g4, ts, xhat
        return xhat

    @staticmethod
    def backward(ctx, g_xhat):
        ts = ctx.tensors
        dev = ts[0].device
        need_w0, need_cmd = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        g = [torch.empty_like(t) if (i >= 2 or (need_w0, need_cmd)[i]) else None for i, t in enumerate(ts)]
        out = _native.FcrLstmRolloutGrads()
        out.g_w_ih = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in g[2:5]])
        out.g_w_hh = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in g[5:8]])
        out.g_fc_w, out.g_fc_b = g[8].data_ptr(), g[9].data_ptr()
        out.g_window0 = g[0].data_ptr() if need_w0 else None
        out.g_cmd = g[1].data_ptr() if need_cmd else None
        w = _weights(ts[2:5], ts[5:8], ts[8], ts[9])
        gx = g_xhat.to(torch.float32).contiguous()
        lib = _native.load()
        nbytes = ctypes.c_size_t(0)
        _native.check(lib.fcr_lstm_rollout_backward_workspace_size(ctypes.byref(ctx.dims), ctypes.byref(nbytes)),
                      "fcr_lstm_rollout_backward_workspace_size")
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        _native.check(lib.fcr_lstm_rollout_backward(ctypes.byref(ctx.dims), ctypes.byref(w), _p(ts[0]), _p(ts[1]), ctx.gain,
                                                    _p(ctx.xhat), _p(gx), ctypes.byref(out), _p(ws), ws.numel(),
                                                    _native.stream(dev)), "fcr_lstm_rollout_backward")
        return (None, None) + tuple(gi if need else None for gi, need in zip(g, ctx.needs_input_grad[2:]))


def _free_run_composed(step, window0, cmd, gain, noise):
    """The free run as T window evaluations under autograd: ``step(window) -> (B,4)``; the window is cloned, its last
    command overwritten in place by cmd[:,0] and shifted with torch.cat, as the fused rollout does it."""
    T = cmd.shape[1]
    win = window0.clone()
    win[:, WINDOW_ROWS - 1, 4] = cmd[:, 0]
    out = []
    for t in range(T):
        if t > 0:
            row = torch.cat([gain * out[-1], cmd[:, t:t + 1]], dim=1)
            win = torch.cat([win[:, 1:], row[:, None, :]], dim=1)
        y = step(win)
        out.append(y if noise is None else y + noise[:, t])
    return torch.stack(out, dim=1)


def free_run(model, window0: torch.Tensor, cmd: torch.Tensor, gain=None, noise: torch.Tensor | None = None):
    """x̂ (B,T,4): ``model`` free-running for T steps on its own predictions and the commands ``cmd`` (B,T) from the
    window ``window0`` (B,10,5) — :func:`~.inference.simulate_rollout`'s semantics and, on the fused route, its bits —
    attached to the autograd graph: the six LSTM weights, the readout, and ``window0`` / ``cmd`` where they require grad.
    ``gain`` (4 host numbers, None = 1) and ``noise`` (B,T,4) receive no gradient.

    ``free_run.last_route`` names what ran: ``"fused"`` (H <= 52 on a ROCm device: one forward launch, a backward whose
    launch count does not depend on T), ``"steps"`` (a wider model on the device: :func:`lstm_apply` per step under
    autograd) or ``"host"`` (CPU tensors: the module's own ``nn.LSTM``)."""
    if window0.dim() != 3 or window0.shape[1:] != (WINDOW_ROWS, 5):
        raise ValueError(f"window0 must be (B, 10, 5), got {tuple(window0.shape)}")
    B, dev = window0.shape[0], window0.device
    if cmd.dim() != 2 or cmd.shape[0] != B or cmd.shape[1] < 1:
        raise ValueError(f"cmd must be (B, T) with T >= 1 and B = {B}, got {tuple(cmd.shape)}")
    T = cmd.shape[1]
    if noise is not None and tuple(noise.shape) != (B, T, 4):
        raise ValueError(f"noise must be (B, T, 4) = {(B, T, 4)}, got {tuple(noise.shape)}")
    g = [1.0] * 4 if gain is None else [float(v) for v in torch.as_tensor(gain, dtype=torch.float64).reshape(-1).tolist()]
    if len(g) != 4:
        raise ValueError(f"gain must hold 4 numbers, got {len(g)}")
    for name, t in (("cmd", cmd), ("noise", noise)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on {dev}, found it on {t.device}")
    if dev.type != "cuda":
        free_run.last_route = "host"
        gt = torch.tensor(g, dtype=window0.dtype)
        return _free_run_composed(lambda w: model(w, dev), window0, cmd, gt, noise)
    f32 = dict(dtype=torch.float32, device=dev)
    window0, cmd = window0.to(**f32), cmd.to(**f32)
    noise = None if noise is None else noise.to(**f32)
    if not hip_shape_ok(model, window0):
        raise RuntimeError("free_run on a ROCm device is built for LSTMModel(5, H, 4, 3) without LSTM bias, its fp32 "
                           f"weights on the windows' device; got window0 {tuple(window0.shape)} on {dev}")
    lstm = model.lstm
    if lstm.hidden_size > 52:
        free_run.last_route = "steps"
        return _free_run_composed(lambda w: lstm_apply(model, w), window0, cmd, torch.tensor(g, **f32), noise)
    free_run.last_route = "fused"
    p = [getattr(lstm, f"weight_ih_l{k}") for k in range(3)] + [getattr(lstm, f"weight_hh_l{k}") for k in range(3)]
    return FreeRunFunction.apply(tuple(g), noise, window0, cmd, *p, model.fc.weight, model.fc.bias)


free_run.last_route = None


def train_free_run(batches, model, loss_function, optimizer, gain=None):
    """:func:`train_model`'s loop over ``(window0, cmd, target)`` batches (:func:`~.data.free_run_batches`) with
    ``loss_function(free_run(model, window0, cmd, gain), target)``; returns the average batch loss."""
    model.train()
    total, n = 0.0, 0
    for window0, cmd, target in batches:
        optimizer.zero_grad()
        loss = loss_function(free_run(model, window0, cmd, gain), target)
        loss.backward()
        optimizer.step()
        total += loss.item()
        n += 1
    return total / max(n, 1)
