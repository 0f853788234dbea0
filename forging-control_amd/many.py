"""M controllers side by side against one shared LSTM surrogate.

The reference does not train one controller: it ships ten seeds of the unsupervised controller
(``Unsupervised Learning/results/NN_controller_N_10_{0..9}.pt``), every one trained at batch 15 (UL/Main.py:84, 297).
At that batch one training step fills a single 16-trajectory group — one workgroup of a chip with 256 CUs — so ten
seeds trained one after the other leave the chip idle ten times over. Here the M controllers are ONE stacked set of
parameters (:class:`ControllerBank`), and one rollout launch per pass runs a workgroup per (model, group)
(``fcr_forward_many`` / ``fcr_backward_many``, include/fcr.h; csrc/fcr_small.h, the ``MANY`` instantiations).

Layout: everything is stacked model-major — ``X (M,B,3)``, ``u0 (M,B,1)``, ``states (M,B,10,5)``, ``noise (M,B,N,4)``
— and every model has the same B. Model m's results are what the single-model call returns for
``(controller_m, X[m], u0[m], states[m], noise[m])``; nothing sums over models.

* :class:`ControllerBank`         the M controllers as three stacked ``nn.Parameter``s
* :func:`forward_many`            the body of :meth:`MPCLoss.forward_many`
* :func:`train_models`            the body of :meth:`NeuralNetwork.train_models`
* :func:`zip_loaders`             M loaders -> stacked batches
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import torch
from torch import nn

from . import _native
from .controller import MAX_HIDDEN
from .rollout import WINDOW_ROWS, _dev_f32, _ptr, _stream, make_dims

# forward_many runs the many-model kernels from this many models on; below it, the loop over the single-model path
# (whose layer-pipelined kernels spread ONE model over six CUs). The measured crossover of scripts/bench_many.py
# (profiles/many_controllers_bench.log), set the way supervised.EPOCH_KERNEL_MAX_BATCH was.
MANY_MIN_MODELS = 3


class _BankFNN(torch.autograd.Function):
    """u[m] = Hardtanh(W_out[m] · ReLU(W_inp[m] · x + b_inp[m])) for X (M,B,3) -> (M,B,1): one launch for all models."""

    @staticmethod
    def forward(ctx, X, W_inp, b_inp, W_out):
        lib = _native.load()
        Xc, Wi, bi, Wo = (t.contiguous() for t in (X, W_inp, b_inp, W_out))
        M, B, hidden = Xc.shape[0], Xc.shape[1], Wi.shape[1]
        u = torch.empty(M, B, 1, dtype=torch.float32, device=Xc.device)
        _native.check(lib.fcr_fnn_forward_many(M, B, Xc.shape[2], hidden, _ptr(Xc), _ptr(Wi), _ptr(bi), _ptr(Wo), _ptr(u),
                                               _stream(Xc.device)), "fcr_fnn_forward_many")
        ctx.save_for_backward(Xc, Wi, bi, Wo)
        return u

    @staticmethod
    def backward(ctx, g_u):
        lib = _native.load()
        Xc, Wi, bi, Wo = ctx.saved_tensors
        M, B, hidden = Xc.shape[0], Xc.shape[1], Wi.shape[1]
        dev = Xc.device
        g_X = torch.empty_like(Xc) if ctx.needs_input_grad[0] else None
        g_Wi, g_bi, g_Wo = torch.empty_like(Wi), torch.empty_like(bi), torch.empty_like(Wo)
        nbytes = ctypes.c_size_t(0)
        _native.check(lib.fcr_fnn_workspace_size(B, hidden, ctypes.byref(nbytes)), "fcr_fnn_workspace_size")
        ws = torch.empty(max(M * int(nbytes.value), 4), dtype=torch.uint8, device=dev)
        gu = g_u.detach().to(torch.float32).contiguous()
        _native.check(lib.fcr_fnn_backward_many(M, B, Xc.shape[2], hidden, _ptr(Xc), _ptr(Wi), _ptr(bi), _ptr(Wo), _ptr(gu),
                                                _ptr(g_X), _ptr(g_Wi), _ptr(g_bi), _ptr(g_Wo), _ptr(ws), ws.numel(),
                                                _stream(dev)), "fcr_fnn_backward_many")
        return g_X, g_Wi, g_bi, g_Wo


class _BankMember:
    """Controller m of a bank with the attributes the single-model path reads (``fc_inp.weight``, ``fc_inp.bias``,
    ``fc_out.weight``, ``width_dim``, ``activation``): views of the bank's stacked parameters, so a gradient through
    them lands in row m of the bank's. Calling it is FNNModel.forward."""

    width_dim = 1

    def __init__(self, bank, m):
        self.activation = nn.ReLU()
        self.fc_inp = SimpleNamespace(weight=bank.w_inp[m], bias=bank.b_inp[m], out_features=bank.hidden)
        self.fc_out = SimpleNamespace(weight=bank.w_out[m].unsqueeze(0), out_features=1)

    def __call__(self, x):
        from .controller import FNNFunction
        if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and self.fc_inp.out_features <= MAX_HIDDEN:
            return FNNFunction.apply(x, self.fc_inp.weight, self.fc_inp.bias, self.fc_out.weight)
        y = torch.relu(nn.functional.linear(x, self.fc_inp.weight, self.fc_inp.bias))
        return nn.functional.hardtanh(nn.functional.linear(y, self.fc_out.weight))


class ControllerBank(nn.Module):
    """M controllers 3 -> hidden -> 1 (the reference's FNNModel at width_dim = 1, ReLU, UL/Main.py:183-188) as three
    stacked parameters: ``w_inp (M,hidden,3)``, ``b_inp (M,hidden)``, ``w_out (M,hidden)``. The unused ``fc_int`` layer
    an FNNModel carries at width 1 is kept as buffers, so :meth:`state_dicts` load into the reference's FNNModel
    unchanged (strict).

    ``bank(X)`` with ``X (M,B,3)`` returns ``(M,B,1)`` under autograd: one launch of the many-model FNN kernels on a
    ROCm device, plain torch on the CPU."""

    def __init__(self, n_models: int, hidden_dim: int, dtype=torch.float32):
        super().__init__()
        self.w_inp = nn.Parameter(torch.zeros(n_models, hidden_dim, 3, dtype=dtype))
        self.b_inp = nn.Parameter(torch.zeros(n_models, hidden_dim, dtype=dtype))
        self.w_out = nn.Parameter(torch.zeros(n_models, hidden_dim, dtype=dtype))
        self.register_buffer("w_int", torch.zeros(n_models, hidden_dim, hidden_dim, dtype=dtype))
        self.register_buffer("b_int", torch.zeros(n_models, hidden_dim, dtype=dtype))

    @property
    def n_models(self) -> int:
        return self.w_inp.shape[0]

    @property
    def hidden(self) -> int:
        return self.w_inp.shape[1]

    @classmethod
    def from_models(cls, models):
        """A bank of the given FNNModels (or of their state_dicts): same hidden width, width_dim = 1, ReLU, biased."""
        sds = []
        for m in models:
            if isinstance(m, nn.Module):
                if getattr(m, "width_dim", 1) != 1 or not isinstance(getattr(m, "activation", nn.ReLU()), nn.ReLU):
                    raise NotImplementedError("ControllerBank holds width_dim = 1 ReLU controllers (UL/Main.py:183-188)")
                m = m.state_dict()
            sds.append(m)
        if not sds:
            raise ValueError("ControllerBank.from_models: no models")
        w0 = sds[0]["fc_inp.weight"]
        if any(sd["fc_inp.weight"].shape != w0.shape for sd in sds) or w0.shape[1] != 3:
            raise ValueError("ControllerBank: every controller must be 3 -> the same hidden width -> 1")
        if any("fc_inp.bias" not in sd for sd in sds):
            raise NotImplementedError("ControllerBank expects fc_inp with bias (UL/Main.py:188)")
        bank = cls(len(sds), w0.shape[0], w0.dtype).to(w0.device)
        with torch.no_grad():
            for i, sd in enumerate(sds):
                bank.w_inp[i].copy_(sd["fc_inp.weight"])
                bank.b_inp[i].copy_(sd["fc_inp.bias"])
                bank.w_out[i].copy_(sd["fc_out.weight"].reshape(-1))
                if "fc_int.weight" in sd:
                    bank.w_int[i].copy_(sd["fc_int.weight"])
                    bank.b_int[i].copy_(sd["fc_int.bias"])
        return bank

    def state_dicts(self):
        """One FNNModel state_dict per model (copies)."""
        c = lambda t: t.detach().clone()
        return [{"fc_inp.weight": c(self.w_inp[m]), "fc_inp.bias": c(self.b_inp[m]), "fc_int.weight": c(self.w_int[m]),
                 "fc_int.bias": c(self.b_int[m]), "fc_out.weight": c(self.w_out[m]).unsqueeze(0)}
                for m in range(self.n_models)]

    def to_models(self):
        """One FNNModel per model, on the bank's device, holding copies of its parameters."""
        from .functions import FNNModel
        out = []
        for sd in self.state_dicts():
            m = FNNModel(3, self.hidden, 1, 1).to(device=self.w_inp.device, dtype=self.w_inp.dtype)
            m.load_state_dict(sd)
            out.append(m)
        return out

    def member(self, m: int) -> _BankMember:
        """Controller m as the single-model path sees one (views of the stacked parameters, gradients included)."""
        return _BankMember(self, m)

    def forward(self, X):
        if X.dim() != 3 or X.shape[0] != self.n_models or X.shape[2] != 3:
            raise ValueError(f"ControllerBank: X must be (M={self.n_models}, B, 3), got {tuple(X.shape)}")
        if (X.is_cuda and X.dtype == torch.float32 and self.w_inp.dtype == torch.float32 and self.w_inp.device == X.device
                and self.hidden <= MAX_HIDDEN):
            return _BankFNN.apply(X, self.w_inp, self.b_inp, self.w_out)
        y = torch.relu(torch.baddbmm(self.b_inp.unsqueeze(1), X, self.w_inp.transpose(1, 2)))   # Functions.py:275-289
        return nn.functional.hardtanh(torch.bmm(y, self.w_out.unsqueeze(2)))


class ManyCallInfo:
    """What one :meth:`MPCLoss.forward_many` ran. ``route``: "many" (one launch per pass for all models) or "loop" (M
    single-model calls, whose own :class:`~.rollout.CallInfo` are in ``calls``); ``forward`` / ``backward``: the kernel
    family of the many route's passes ("small"); ``why``: what sent the call to the loop."""

    def __init__(self, route, n_models, why=None):
        self.route, self.n_models, self.why = route, n_models, why
        self.forward = self.backward = None
        self.workspace_bytes = 0
        self.calls = []


class ManyRolloutFn(torch.autograd.Function):
    """RolloutFn for M stacked models. Inputs: X (M,B,3), u0 (M,B,1), states (M,B,10,5), noise (M,B,N,4) or None, the
    bank's (M,hidden,3), (M,hidden), (M,hidden), the LSTM weights, N, alpha, the small-batch limit, a ManyCallInfo; then,
    optionally, the table of the models' terms ((M,6) or, shared, (1,6) float32 on the device) and ref_h (M,B,N).
    Outputs: loss (M,), cost / command / error (M,B), prediction (M,B*N), xhat (M,B,N,4)."""

    @staticmethod
    def forward(ctx, X, u0, states, noise, W_inp, b_inp, W_out, w_ih0, w_ih1, w_ih2, w_hh0, w_hh1, w_hh2, fc_w, fc_b,
                N, alpha, small_limit, info, table=None, ref_h=None):
        lib = _native.load()
        dev = X.device
        M, B = X.shape[0], X.shape[1]
        dims = make_dims(B, N, w_hh0.shape[1], 3, W_inp.shape[1], alpha)
        need_grad = any(ctx.needs_input_grad[i] for i in (1, 4, 5, 6))
        opts = _native.FcrOptions(int(small_limit), 0, _native.OPT_INHERIT)
        ws = torch.empty(_native.many_workspace_bytes(dims, M, need_grad, opts), dtype=torch.uint8, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        loss = torch.empty(M, **f32)
        cost, command, error = (torch.empty(M, B, **f32) for _ in range(3))
        prediction = torch.empty(M, B * N, **f32)
        xhat = torch.empty(M, B, N, 4, **f32)
        w = _native.FcrWeights()
        keep = [t.contiguous() for t in (W_inp, b_inp, W_out, w_ih0, w_ih1, w_ih2, w_hh0, w_hh1, w_hh2, fc_w, fc_b)]
        w.ctrl_w_inp, w.ctrl_b_inp, w.ctrl_w_out = (t.data_ptr() for t in keep[0:3])
        for l in range(3):
            w.w_ih[l] = keep[3 + l].data_ptr()
            w.w_hh[l] = keep[6 + l].data_ptr()
        w.fc_w, w.fc_b = keep[9].data_ptr(), keep[10].data_ptr()
        Xc, u0c, stc = X.contiguous(), u0.contiguous(), states.contiguous()
        nzc = noise.contiguous() if noise is not None else None
        terms = None
        if table is not None or ref_h is not None:
            rhc = ref_h.contiguous() if ref_h is not None else None
            terms = (table, rhc)
            ft = ManyRolloutFn._terms(terms, alpha, B, N)
            _native.check(lib.fcr_forward_many_terms(ctypes.byref(dims), ctypes.byref(opts), M, ctypes.byref(w),
                                                     ctypes.byref(ft), _ptr(Xc), _ptr(u0c), _ptr(stc), _ptr(nzc), _ptr(loss),
                                                     _ptr(cost), _ptr(command), _ptr(error), _ptr(prediction), _ptr(xhat),
                                                     int(need_grad), _ptr(ws), ws.numel(), _stream(dev)),
                          "fcr_forward_many_terms")
        else:
            _native.check(lib.fcr_forward_many(ctypes.byref(dims), ctypes.byref(opts), M, ctypes.byref(w), _ptr(Xc),
                                               _ptr(u0c), _ptr(stc), _ptr(nzc), _ptr(loss), _ptr(cost), _ptr(command),
                                               _ptr(error), _ptr(prediction), _ptr(xhat), int(need_grad), _ptr(ws),
                                               ws.numel(), _stream(dev)), "fcr_forward_many")
        info.forward, info.backward = _native.KERNEL_FAMILIES[opts.kernels], None
        info.workspace_bytes = ws.numel()
        ctx.mark_non_differentiable(cost, command, error, prediction, xhat)
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.ws, ctx.dims, ctx.info, ctx.small_limit, ctx.M = ws, dims, info, int(small_limit), M
            ctx.terms, ctx.alpha = terms, alpha
            ctx.save_for_backward(Xc, stc, prediction)
            ctx.ctrl_shapes = (W_inp.shape, b_inp.shape, W_out.shape)
        return loss, cost, command, error, prediction, xhat

    @staticmethod
    def _terms(terms, alpha, B, N):
        """fcr_loss_terms of a many call: the table's row stride is 0 for one shared row; ref_h is (M,B,N)."""
        table, ref_h = terms
        return _native.make_loss_terms(_native.default_terms_row(alpha), ref_h, (B * N, N, 1), table,
                                       0 if table is None or table.shape[0] == 1 else table.stride(0))

    @staticmethod
    def backward(ctx, g_loss, *unused):
        if g_loss is None:
            ctx.ws = None
            return (None,) * 21
        if ctx.ws is None:
            raise RuntimeError("MPCLoss.forward_many: trying to backward through the same rollout a second time; its "
                               "workspace was released by the first backward: recompute the losses")
        lib = _native.load()
        Xc, stc, prediction = ctx.saved_tensors
        dev = Xc.device
        M, B = Xc.shape[0], Xc.shape[1]
        f32 = dict(dtype=torch.float32, device=dev)
        g_u0 = torch.empty(M, B, 1, **f32)
        g_wi, g_bi, g_wo = (torch.empty(s, **f32) for s in ctx.ctrl_shapes)
        dl = g_loss.detach().to(torch.float32).reshape(M).contiguous()
        opts = _native.FcrOptions(ctx.small_limit, 0, _native.OPT_INHERIT)
        if ctx.terms is not None:
            ft = ManyRolloutFn._terms(ctx.terms, ctx.alpha, B, ctx.dims.N)
            _native.check(lib.fcr_backward_many_terms(ctypes.byref(ctx.dims), ctypes.byref(opts), M, ctypes.byref(ft),
                                                      _ptr(Xc), _ptr(stc), _ptr(prediction), _ptr(dl), _ptr(g_u0), _ptr(g_wi),
                                                      _ptr(g_bi), _ptr(g_wo), _ptr(ctx.ws), ctx.ws.numel(), _stream(dev)),
                          "fcr_backward_many_terms")
        else:
            _native.check(lib.fcr_backward_many(ctypes.byref(ctx.dims), ctypes.byref(opts), M, _ptr(Xc), _ptr(stc),
                                                _ptr(prediction), _ptr(dl), _ptr(g_u0), _ptr(g_wi), _ptr(g_bi), _ptr(g_wo),
                                                _ptr(ctx.ws), ctx.ws.numel(), _stream(dev)), "fcr_backward_many")
        ctx.info.backward = _native.KERNEL_FAMILIES[opts.kernels]
        ctx.ws = None
        return (None, g_u0, None, None, g_wi, g_bi, g_wo) + (None,) * 14


def _loop_reason(loss_fn, simulator, bank, X):
    """None when the many-model kernels cover this call, else what sends it to the loop over the single-model path."""
    if X.device.type != "cuda":
        return "CPU tensors"
    if loss_fn.precision != "fp32":
        return f"precision {loss_fn.precision!r}"
    H = simulator.lstm.hidden_size
    if not 17 <= H <= 52:
        return f"H = {H} outside the slot tiers 8 and 13 (17..52)"
    if any(t.dtype != torch.float32 for t in (X, bank.w_inp)):
        return "not float32"
    limit = loss_fn.small_batch_limit if loss_fn.small_batch_limit is not None else _native.small_batch_limit()
    if X.shape[1] > limit:
        return f"B = {X.shape[1]} above the small-batch limit {limit}"
    least = loss_fn.many_min_models if getattr(loss_fn, "many_min_models", None) is not None else MANY_MIN_MODELS
    if bank.n_models < least:
        return f"M = {bank.n_models} below MANY_MIN_MODELS = {least}"
    return None


def forward_many(loss_fn, simulator, bank, X, u0, states, device, enable_noise=False, noise=None, ref_horizon=None):
    """:meth:`MPCLoss.forward_many` (see there)."""
    from .functions import _simulator_params
    from .loss_terms import resolve
    dev = torch.device(device)
    if dev.type != X.device.type or (dev.index is not None and dev.index != X.device.index):
        raise RuntimeError(f"MPCLoss: inputs are on {X.device}, device argument is {device}")
    M, N = bank.n_models, loss_fn.N
    if X.dim() != 3 or X.shape[0] != M or X.shape[2] != 3:
        raise ValueError(f"forward_many: X must be (M={M}, B, 3), got {tuple(X.shape)}")
    B = X.shape[1]
    if u0.numel() != M * B or tuple(states.shape) != (M, B, WINDOW_ROWS, 5):
        raise ValueError(f"forward_many: u0 must be (M,B,1) and states (M,B,10,5); got {tuple(u0.shape)}, "
                         f"{tuple(states.shape)}")
    if noise is not None and tuple(noise.shape) != (M, B, N, 4):
        raise ValueError(f"forward_many: noise must be (M,B,N,4) = {(M, B, N, 4)}, got {tuple(noise.shape)}")
    if ref_horizon is not None and tuple(ref_horizon.shape) != (M, B, N):
        raise ValueError(f"forward_many: ref_horizon must be (M,B,N) = {(M, B, N)}, got {tuple(ref_horizon.shape)}")
    terms = loss_fn.terms
    if terms is not None and not hasattr(terms, "as_row"):
        terms = resolve(terms, M)   # one LossTerms per model
    u0 = u0.reshape(M, B, 1)
    why = _loop_reason(loss_fn, simulator, bank, X)
    if why is not None:
        # the single-model path per model, model 0 first (so drawn noise is that of M successive calls)
        info = ManyCallInfo("loop", M, why)
        losses, feats, traj = [], [], []
        for m in range(M):
            l, f = loss_fn.forward(simulator, bank.member(m), X[m], u0[m], states[m], device, enable_noise,
                                   None if noise is None else noise[m],
                                   None if ref_horizon is None else ref_horizon[m],
                                   terms[m] if isinstance(terms, tuple) else None)
            losses.append(l)
            feats.append(f)
            traj.append(loss_fn.last_trajectory)
            info.calls.append(loss_fn.last_call)
        loss_fn.last_trajectory = torch.stack(traj, dim=0)
        loss_fn.last_call = info
        return torch.stack(losses), {k: torch.stack([f[k] for f in feats], dim=0)
                                     for k in ("loss", "command", "error", "prediction")}
    if enable_noise and noise is None:   # the draws of M successive single-model calls (MPCLoss.forward)
        noise = torch.stack([torch.stack([torch.randn(B, 4, device=X.device) * 0.01 for _ in range(N)], dim=1)
                             for _ in range(M)], dim=0)
    elif not enable_noise:
        noise = None
    w_ih, w_hh, fc_w, fc_b = _simulator_params(simulator)
    if ref_horizon is not None:
        ref_horizon = _dev_f32(ref_horizon.detach(), "ref_horizon")
    for t in ([u0, states, bank.w_inp] + list(w_ih) + list(w_hh) + [fc_w, fc_b] + ([] if noise is None else [noise])
              + ([] if ref_horizon is None else [ref_horizon])):
        if t.device != X.device:
            raise RuntimeError(f"all rollout tensors must be on {X.device}, found one on {t.device}")
    limit = loss_fn.small_batch_limit if loss_fn.small_batch_limit is not None else _native.small_batch_limit()
    info = ManyCallInfo("many", M)
    loss, cost, command, error, prediction, xhat = ManyRolloutFn.apply(
        _dev_f32(X, "X"), _dev_f32(u0, "u0"), _dev_f32(states, "states"),
        None if noise is None else _dev_f32(noise, "noise"), bank.w_inp, bank.b_inp, bank.w_out,
        *[_dev_f32(t, "lstm weight") for t in list(w_ih) + list(w_hh) + [fc_w, fc_b]], int(N), float(loss_fn.alpha),
        int(limit), info, loss_fn.terms_table(M, X.device), ref_horizon)
    loss_fn.last_trajectory = xhat
    loss_fn.last_call = info
    return loss, {"loss": cost, "command": command, "error": error, "prediction": prediction}


def zip_loaders(loaders):
    """M loaders (``DataLoader`` or :class:`~.data.DeviceLoader`, one per model, each with its own shuffling) as one
    iterable of stacked batches ``(X (M,B,3), y (M,B,...), states (M,B,10,5))`` — and ``ref_h (M,B,N)`` when the loaders
    yield a fourth element (a reference preview). Refuses loaders whose batch sizes
    differ within a step, or that run out at different steps: every model of a bank has the same B."""
    loaders = list(loaders)
    if not loaders:
        raise ValueError("zip_loaders: no loaders")
    its = [iter(l) for l in loaders]
    step = 0
    while True:
        batches = []
        for it in its:
            try:
                batches.append(next(it))
            except StopIteration:
                batches.append(None)
        if all(b is None for b in batches):
            return
        if any(b is None for b in batches):
            raise ValueError(f"zip_loaders: step {step}: loaders {[i for i, b in enumerate(batches) if b is None]} ran out "
                             "before the others")
        sizes = [b[0].shape[0] for b in batches]
        if len(set(sizes)) != 1:
            raise ValueError(f"zip_loaders: step {step}: batch sizes differ between the models: {sizes}")
        width = {len(b) for b in batches}
        if len(width) != 1 or width.pop() not in (3, 4):
            raise ValueError(f"zip_loaders: step {step}: batches must all be (X, y, z) or all (X, y, z, ref_h)")
        yield tuple(torch.stack([b[k] for b in batches], dim=0) for k in range(len(batches[0])))
        step += 1


FEATURE_KEYS = ("loss", "command", "error", "prediction")


def captured_models_step(simulator, bank, loss_function, optimizer, device, enable_noise=False, warmup=2):
    """The body of :func:`train_models`' batch loop as a :class:`~.graphed.CapturedStep` (one HIP graph replay per
    stacked batch; pass it as ``train_models(..., step=...)``)."""
    from .graphed import CapturedStep

    def body(X, z):
        output = bank(X)
        losses, f = loss_function.forward_many(simulator, bank, X, output, z, device, enable_noise)
        losses.sum().backward()
        return (losses.detach(),) + tuple(f[k] for k in FEATURE_KEYS)

    return CapturedStep(bank.parameters(), optimizer, body, None, warmup)


def train_models(batches, simulator, bank, loss_function, optimizer, device, enable_noise=False, step=None):
    """:meth:`NeuralNetwork.train_models` (see there)."""
    bank.train()
    feats = {k: [] for k in FEATURE_KEYS}
    total, n_batches = None, 0
    for X, _, z, *more in batches:
        X, z = X.to(device), z.to(device)
        ref_h = more[0].to(device) if more else None   # (X, y, z, ref_h): the reference over the horizon, (M,B,N)
        if step is not None:
            if ref_h is not None:
                raise NotImplementedError("train_models(step=...): batches with a reference preview (a fourth element) "
                                          "are not replayed from a graph; train them without step")
            losses, *f = step(X, z)
            f = dict(zip(FEATURE_KEYS, (v.clone() for v in f)))
            losses = losses.clone()
        else:
            optimizer.zero_grad()
            output = bank(X)
            losses, f = loss_function.forward_many(simulator, bank, X, output, z, device, enable_noise, None, ref_h)
            losses.sum().backward()   # the models are independent: d sum / d (model m's parameters) = d losses[m] / d them
            optimizer.step()
            losses = losses.detach()
        for k in FEATURE_KEYS:
            feats[k].append(f[k])
        total = losses if total is None else total + losses
        n_batches += 1
    M = bank.n_models
    avg = (total / n_batches).tolist() if n_batches else [0.0] * M
    empty = torch.empty(M, 0, device=device)
    return avg, {k: torch.cat(v, dim=1) if v else empty for k, v in feats.items()}
