"""The supervised (behaviour-cloning) baseline on gfx950: the reference's Supervised Learning/ trains the same
3 -> 50 -> 1 ``FNNModel`` as the unsupervised side against the MPC's command with ``nn.L1Loss`` and
``AdamW(lr=1e-3)`` at batch 256, shuffled, once per seed (SL/Main.py:143-159, SL/Functions.py:396-464, 564-630).

One optimizer step there is 256 samples x 250 parameters: a few microseconds of arithmetic behind ~10 launches and
a host ``.item()``. :func:`train_epoch` runs every step of an epoch, optimizer included, in ONE launch
(``fcr_supervised_epoch``, csrc/fcr_supervised.h): one workgroup per model keeps parameters, AdamW moments and step
counter on the chip, so many independent models (the reference's ten seeds) train side by side at the price of one.
:func:`evaluate` is ``validate_model``; :func:`train_loop` has the reference's signature and dispatches to the kernel
when the call is the reference's shape, and to the reference's eager loop otherwise.
"""
from __future__ import annotations

import ctypes
from time import time

import torch
from torch import nn
from torch.utils.data import DataLoader, RandomSampler, SequentialSampler, TensorDataset

from . import _native
from .controller import MAX_HIDDEN, _stream
from .functions import FNNModel

# Batches above this run train_loop's eager loop: one workgroup per model walks a batch 256 samples at a time, so a
# very large batch is better served by the batch-wide fnn kernels (scripts/bench_supervised.py measures the crossover).
EPOCH_KERNEL_MAX_BATCH = 8192

_LOSSES = {"l1": _native.LOSS_L1, "mse": _native.LOSS_MSE}


def _as_list(x):
    return (list(x), True) if isinstance(x, (list, tuple)) else ([x], False)


def _params(model):
    """The three tensors the kernel trains; fc_int gets no gradient at width_dim = 1 and is left alone."""
    return model.fc_inp.weight, model.fc_inp.bias, model.fc_out.weight


def model_reason(model) -> str | None:
    """None when the epoch kernel can train ``model``, else why not."""
    if not isinstance(model, FNNModel):
        return "not an FNNModel"
    if model.width_dim != 1:
        return f"width_dim={model.width_dim} (the kernel is built for 1)"
    if not isinstance(model.activation, nn.ReLU):
        return "activation is not ReLU"
    if model.fc_inp.bias is None or model.fc_inp.in_features != 3 or model.fc_out.out_features != 1:
        return "not the 3 -> hidden -> 1 shape with an input bias"
    if not 1 <= model.fc_inp.out_features <= MAX_HIDDEN:
        return f"hidden={model.fc_inp.out_features} (the kernel is built for 1..{MAX_HIDDEN})"
    dev = model.fc_inp.weight.device
    if dev.type != "cuda" or torch.version.hip is None:
        return f"model is on {dev}, not a ROCm device"
    if any(p.dtype != torch.float32 or p.device != dev for p in _params(model)):
        return "parameters are not float32 on one device"
    return None


def optimizer_reason(optimizer, model) -> str | None:
    """None when ``optimizer`` is a plain AdamW over the model's trained tensors, else why not."""
    if type(optimizer) is not torch.optim.AdamW:
        return f"optimizer is {type(optimizer).__name__}, not torch.optim.AdamW"
    try:
        groups = [_group_of(optimizer, p) for p in _params(model)]
    except ValueError as e:
        return str(e)
    g = groups[0]
    for k in ("amsgrad", "maximize", "capturable", "differentiable"):
        if any(gr.get(k) for gr in groups):
            return f"AdamW with {k}"
    if any(gr.get("fused") for gr in groups):
        return "fused AdamW (its state lives on the device)"
    if any(isinstance(gr[k], torch.Tensor) for gr in groups for k in ("lr", "eps", "weight_decay")) or \
            any(isinstance(b, torch.Tensor) for gr in groups for b in gr["betas"]):
        return "tensor hyper-parameters"
    if any(_hyper(gr) != _hyper(g) for gr in groups[1:]):
        return "the model's tensors sit in parameter groups with different hyper-parameters"
    return None


def _group_of(optimizer, p):
    for g in optimizer.param_groups:
        if any(q is p for q in g["params"]):
            return g
    raise ValueError("a trained tensor of the model is not in the optimizer")


def _hyper(g):
    return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])


def _loss_kind(loss) -> int:
    if isinstance(loss, str):
        if loss.lower() not in _LOSSES:
            raise ValueError(f"loss must be 'l1' or 'mse', got {loss!r}")
        return _LOSSES[loss.lower()]
    kind = loss_reason(loss)
    if isinstance(kind, str):
        raise ValueError(kind)
    return _native.LOSS_L1 if type(loss) is nn.L1Loss else _native.LOSS_MSE


def loss_reason(loss_function) -> str | None:
    if type(loss_function) not in (nn.L1Loss, nn.MSELoss):
        return f"loss is {type(loss_function).__name__}, not L1Loss or MSELoss"
    if loss_function.reduction != "mean":
        return f"loss reduction is {loss_function.reduction!r}, not 'mean'"
    return None


def _tables(X, y, device):
    X = torch.as_tensor(X).to(device=device, dtype=torch.float32).contiguous()
    y = torch.as_tensor(y).to(device=device, dtype=torch.float32)
    if X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"X must be (n, 3), got {tuple(X.shape)}")
    if y.dim() == 2 and y.shape[1] == 1:
        y = y[:, 0]
    y = y.contiguous()
    if y.dim() != 1 or y.shape[0] != X.shape[0]:
        raise ValueError(f"y must be (n,) or (n, 1) with X's n={X.shape[0]}, got {tuple(y.shape)}")
    if X.shape[0] < 1:
        raise ValueError("no samples")
    return X, y


def _stack(models):
    for m in models:
        why = model_reason(m)
        if why:
            raise ValueError(f"fcr_supervised_epoch cannot run this model: {why}")
    dev = models[0].fc_inp.weight.device
    hidden = models[0].fc_inp.out_features
    if any(m.fc_inp.out_features != hidden or m.fc_inp.weight.device != dev for m in models):
        raise ValueError("all models of one call must have the same hidden size and device")
    with torch.no_grad():
        wi = torch.stack([m.fc_inp.weight for m in models]).contiguous()
        bi = torch.stack([m.fc_inp.bias for m in models]).contiguous()
        wo = torch.stack([m.fc_out.weight.reshape(-1) for m in models]).contiguous()
    return dev, hidden, wi, bi, wo


def _launch(dev, hidden, wi, bi, wo, X, y, batch_size, kind, perm=None, hyper=None, moments=None, step=None):
    n, M = X.shape[0], wi.shape[0]
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    nb = (n + batch_size - 1) // batch_size
    loss = torch.empty(M, nb, dtype=torch.float32, device=dev)
    a = _native.FcrSupervised()
    a.n_models, a.n_samples, a.batch_size, a.hidden, a.loss_kind, a.train = M, n, batch_size, hidden, kind, int(hyper is not None)
    if hyper is not None:
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = hyper
        (a.exp_avg_w_inp, a.exp_avg_b_inp, a.exp_avg_w_out, a.exp_avg_sq_w_inp, a.exp_avg_sq_b_inp,
         a.exp_avg_sq_w_out) = (t.data_ptr() for t in moments)
        a.step = step.data_ptr()
    a.X, a.y, a.perm = X.data_ptr(), y.data_ptr(), perm.data_ptr() if perm is not None else None
    a.w_inp, a.b_inp, a.w_out, a.loss = wi.data_ptr(), bi.data_ptr(), wo.data_ptr(), loss.data_ptr()
    with torch.cuda.device(dev):
        _native.check(_native.load().fcr_supervised_epoch(ctypes.byref(a), _stream(dev)), "fcr_supervised_epoch")
    return loss


def _averages(loss, many, return_batch_losses):
    avg = loss.double().mean(dim=1).tolist()          # train_model's total_loss / len(data_loader)
    out = avg if many else avg[0]
    if return_batch_losses:
        return out, (loss if many else loss[0])
    return out


def train_epoch(models, optimizers, X, y, batch_size=256, generator=None, loss="l1", perm=None,
                return_batch_losses=False):
    """One epoch of ``NeuralNetwork.train_model`` (SL/Functions.py:396-422) for one FNNModel or a list of them, each
    with its own ``torch.optim.AdamW``, over the table ``X`` (n,3), ``y`` (n,) or (n,1), in one launch.

    Each model's sample order is drawn on the host with ``torch.randperm(n, generator=generator)`` as a shuffling
    DataLoader draws it (``perm`` (M,n) gives the orders instead). Parameters are written back into the modules, and
    ``step`` / ``exp_avg`` / ``exp_avg_sq`` into every optimizer's ``state`` in torch's own layout, so a following
    ``optimizer.step()`` continues the same run and ``state_dict()`` looks as torch's own; an optimizer with empty
    state starts from zero moments at step 0. ``fc_int`` gets no gradient at width_dim = 1: no state, untouched.
    Returns each model's average of per-batch losses (a float for one model, a list for a list); with
    ``return_batch_losses`` also the (M, n_batches) device tensor of them."""
    models, many = _as_list(models)
    optimizers, _ = _as_list(optimizers)
    if len(models) != len(optimizers) or not models:
        raise ValueError("one optimizer per model")
    kind = _loss_kind(loss)
    dev, hidden, wi, bi, wo = _stack(models)
    for m, o in zip(models, optimizers):
        why = optimizer_reason(o, m)
        if why:
            raise ValueError(f"fcr_supervised_epoch cannot run this optimizer: {why}")
    hypers = [_hyper(_group_of(o, m.fc_inp.weight)) for m, o in zip(models, optimizers)]
    if any(h != hypers[0] for h in hypers[1:]):
        raise ValueError("all optimizers of one call must share lr, betas, eps and weight_decay")
    X, y = _tables(X, y, dev)
    n, M = X.shape[0], len(models)
    if perm is None:
        perm = torch.stack([torch.randperm(n, generator=generator) for _ in models])
    perm = torch.as_tensor(perm)
    if perm.dim() == 1:
        perm = perm.unsqueeze(0)
    if tuple(perm.shape) != (M, n):
        raise ValueError(f"perm must be ({M}, {n}), got {tuple(perm.shape)}")
    if perm.device.type == "cpu" and (int(perm.min()) < 0 or int(perm.max()) >= n):
        raise IndexError(f"perm has entries outside [0, {n})")
    perm = perm.to(device=dev, dtype=torch.int32).contiguous()
    # optimizer state -> stacked moments and step counters (an empty state: zero moments at step 0)
    steps, mom = [], [[] for _ in range(6)]
    for m, o in zip(models, optimizers):
        st = [o.state.get(p, {}) for p in _params(m)]
        if any(bool(s) != bool(st[0]) for s in st) or any(s and float(s["step"]) != float(st[0]["step"]) for s in st):
            raise ValueError("the optimizer's state covers only some of the model's tensors, or at different steps")
        steps.append(float(st[0]["step"]) if st[0] else 0.0)
        for i, (p, s) in enumerate(zip(_params(m), st)):
            shape = (hidden, 3) if i == 0 else (hidden,)
            for k, key in enumerate(("exp_avg", "exp_avg_sq")):
                mom[3 * k + i].append(s[key].detach().to(dev, torch.float32).reshape(shape) if s
                                      else torch.zeros(shape, dtype=torch.float32, device=dev))
    moments = [torch.stack(ts).contiguous() for ts in mom]
    step = torch.tensor(steps, dtype=torch.float32).to(dev)
    losses = _launch(dev, hidden, wi, bi, wo, X, y, batch_size, kind, perm, hypers[0], moments, step)
    nb = losses.shape[1]
    # back into the modules and the optimizers' state: one batched copy for all models (a copy per tensor would cost
    # many times the epoch's launch)
    dst, src = [], []
    for i, (m, o) in enumerate(zip(models, optimizers)):
        for j, p in enumerate(_params(m)):
            s = o.state[p]                           # (a defaultdict: creates the entry)
            # torch's AdamW keeps `step` as an fp32 scalar on the host: known here without reading the device
            s["step"] = torch.tensor(steps[i] + nb, dtype=torch.float32)
            s["exp_avg"] = torch.empty_like(p, memory_format=torch.preserve_format)
            s["exp_avg_sq"] = torch.empty_like(p, memory_format=torch.preserve_format)
            dst += [p, s["exp_avg"], s["exp_avg_sq"]]
            src += [t[i].reshape(p.shape) for t in ((wi, bi, wo)[j], moments[j], moments[3 + j])]
    with torch.no_grad():
        torch._foreach_copy_(dst, src)
    return _averages(losses, many, return_batch_losses)


def evaluate(models, X, y, batch_size=256, loss="l1", return_batch_losses=False):
    """``NeuralNetwork.validate_model`` (SL/Functions.py:425-464): the samples in order, no update; each model's
    average of per-batch losses (with ``return_batch_losses`` also the (M, n_batches) device tensor)."""
    models, many = _as_list(models)
    if not models:
        raise ValueError("no model")
    kind = _loss_kind(loss)
    dev, hidden, wi, bi, wo = _stack(models)
    X, y = _tables(X, y, dev)
    return _averages(_launch(dev, hidden, wi, bi, wo, X, y, batch_size, kind), many, return_batch_losses)


# ---- train_loop: the reference's entry point -----------------------------------------------------------------------

def _loader_reason(loader) -> str | None:
    if not isinstance(loader, DataLoader):
        return "not a torch DataLoader"
    ds = loader.dataset
    if not isinstance(ds, TensorDataset) or len(ds.tensors) != 2:
        return "dataset is not a plain (X, y) TensorDataset"
    X, y = ds.tensors
    if X.dim() != 2 or X.shape[1] != 3 or X.shape[0] < 1 or not (y.dim() == 1 or (y.dim() == 2 and y.shape[1] == 1)):
        return "tensors are not X (n, 3) and y (n,) or (n, 1)"
    if X.dtype != torch.float32 or y.dtype != torch.float32:
        return "tensors are not float32"
    if loader.batch_size is None or loader.drop_last or loader.batch_sampler is None:
        return "no automatic batching, or drop_last"
    if type(loader.batch_sampler) is not torch.utils.data.BatchSampler:
        return "custom batch sampler"
    s = loader.sampler
    if type(s) is SequentialSampler:
        return None
    if type(s) is RandomSampler and not s.replacement and s.num_samples == len(ds):
        return None
    return "sampler is neither sequential nor a full shuffle without replacement"


def dispatch_reason(controller, train_loader, val_loader, loss_function, optimizer) -> str | None:
    """None when :func:`train_loop` runs the epoch kernel for this call, else the reason it runs the eager loop."""
    why = model_reason(controller) or loss_reason(loss_function) or optimizer_reason(optimizer, controller)
    if why:
        return why
    for name, loader in (("train", train_loader), ("validation", val_loader)):
        why = _loader_reason(loader)
        if why:
            return f"{name} loader: {why}"
        if loader.batch_size > EPOCH_KERNEL_MAX_BATCH:
            return f"{name} batch size {loader.batch_size} > EPOCH_KERNEL_MAX_BATCH={EPOCH_KERNEL_MAX_BATCH}"
    return None


def _draw_order(loader):
    """The sample order one pass over ``loader`` would take, drawing from the same generators in the same order as
    ``iter(loader)`` does (its base seed, then RandomSampler's seed and permutation), or None for the index order."""
    torch.empty((), dtype=torch.int64).random_(generator=loader.generator)      # _BaseDataLoaderIter._base_seed
    s = loader.sampler
    if type(s) is SequentialSampler:
        return None
    gen = s.generator
    if gen is None:
        gen = torch.Generator()
        gen.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    n = len(loader.dataset)
    order = torch.randperm(n, generator=gen)
    torch.randperm(n, generator=gen)      # RandomSampler draws a second permutation for its (empty) remainder
    return order


def _train_model_eager(data_loader, model, loss_function, optimizer, device):
    """SL/Functions.py:396-422."""
    model.train()
    total_loss = 0
    for X, y in data_loader:
        X, y = X.to(device), y.to(device)
        optimizer.zero_grad()
        output = model(X)
        loss = loss_function(output, y)
        loss.backward()
        optimizer.step()
        total_loss += loss.item()
    return total_loss / len(data_loader)


def _validate_model_eager(data_loader, model, loss_function, device):
    """SL/Functions.py:425-464."""
    model.eval()
    total_loss = 0
    with torch.no_grad():
        for X, y in data_loader:
            X, y = X.to(device), y.to(device)
            output = model(X)
            total_loss += loss_function(output, y).item()
    return total_loss / len(data_loader)


def train_loop(controller, train_loader, val_loader, loss_function, optimizer, n_epochs, device):
    """``NeuralNetwork.train_loop`` (SL/Functions.py:564-630) without its plotting and logging: returns
    ``(controller, vec_t_loss, vec_v_loss, comp_time)``.

    The reference's shape (:func:`dispatch_reason` is None) runs one launch per training epoch and one per
    validation pass, over tables moved to the device once, with the sample order drawn as the loaders would draw
    it; anything else runs the reference's eager loop (on a ROCm device ``FNNModel.forward`` is already the HIP
    controller kernel there)."""
    if dispatch_reason(controller, train_loader, val_loader, loss_function, optimizer) is not None:
        _validate_model_eager(val_loader, controller, loss_function, device)
        vec_t_loss, vec_v_loss = [], []
        t0 = time()
        for _ in range(n_epochs):
            training_loss = _train_model_eager(train_loader, controller, loss_function, optimizer, device)
            validation_loss = _validate_model_eager(val_loader, controller, loss_function, device)
            vec_t_loss.append(training_loss)
            vec_v_loss.append(validation_loss)
        return controller, vec_t_loss, vec_v_loss, time() - t0
    dev = controller.fc_inp.weight.device
    Xt, yt = _tables(*train_loader.dataset.tensors, dev)
    Xv, yv = _tables(*val_loader.dataset.tensors, dev)

    def validate():
        order = _draw_order(val_loader)
        if order is None:
            return evaluate(controller, Xv, yv, val_loader.batch_size, loss_function)
        return evaluate(controller, Xv[order.to(dev)], yv[order.to(dev)], val_loader.batch_size, loss_function)

    validate()
    vec_t_loss, vec_v_loss = [], []
    t0 = time()
    for _ in range(n_epochs):
        controller.train()
        order = _draw_order(train_loader)
        if order is None:
            order = torch.arange(Xt.shape[0])
        vec_t_loss.append(train_epoch(controller, optimizer, Xt, yt, train_loader.batch_size, loss=loss_function,
                                      perm=order))
        controller.eval()
        vec_v_loss.append(validate())
    return controller, vec_t_loss, vec_v_loss, time() - t0
