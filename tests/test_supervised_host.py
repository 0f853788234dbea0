"""CPU: the supervised baseline's host side — fcr_supervised's layout and argument checks (every call here is refused,
or empty, before any launch), train_loop's dispatch predicate, and its eager fall-back, which must stay the
reference's loop bit for bit."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

import forging_control_amd as fca
from conftest import ROOT
from forging_control_amd import supervised as sl

N = fca._native


def test_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "fcr.h")).read()
    body = re.search(r"typedef struct fcr_supervised \{(.*?)\} fcr_supervised;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "p" if "*" in decl else ("d" if decl.startswith("double") else "i")
        for name in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(","):
            fields.append((name.replace("*", "").strip(), kind))
    ctype = {"p": ctypes.c_void_p, "d": ctypes.c_double, "i": ctypes.c_int32}
    assert [(n, ctype[k]) for n, k in fields] == list(N.FcrSupervised._fields_)
    assert [n for n, _ in fields[:11]] == ["n_models", "n_samples", "batch_size", "hidden", "loss_kind", "train",
                                           "lr", "beta1", "beta2", "eps", "weight_decay"]
    assert ctypes.sizeof(N.FcrSupervised) == 6 * 4 + 5 * 8 + 14 * 8
    assert N.FcrSupervised.lr.offset == 24 and N.FcrSupervised.X.offset == 64 and N.FcrSupervised.loss.offset == 168
    # an addition to the ABI: no existing call or struct changed, so the version number did not move
    assert f"#define FCR_ABI_VERSION {N.ABI_VERSION} " in text and N.load().fcr_abi_version() == N.ABI_VERSION
    assert "fcr_supervised_epoch" in N.EXPORTS and (N.LOSS_L1, N.LOSS_MSE) == (0, 1)


def args(**kw):
    a = N.FcrSupervised()
    a.n_models, a.n_samples, a.batch_size, a.hidden, a.loss_kind, a.train = 2, 37, 16, 50, 0, 1
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    for name, _ in N.FcrSupervised._fields_[11:]:
        setattr(a, name, 64)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


POINTERS = [n for n, _ in N.FcrSupervised._fields_[11:]]
BAD = ([(dict(hidden=65), -4, "hidden=65"), (dict(hidden=0), -4, "hidden=0"), (dict(batch_size=0), -1, "batch_size=0"),
        (dict(n_samples=0), -1, "n_samples=0"), (dict(n_models=-1), -1, "n_models=-1"), (dict(loss_kind=2), -1, "loss_kind=2"),
        (dict(train=2), -1, "train=2"), (dict(beta1=1.0), -1, "betas"), (dict(lr=float("nan")), -1, "lr"),
        (dict(train=0, X=None), -1, "NULL"), (dict(train=0, loss=None), -1, "NULL")]
       + [({p: None}, -1, "NULL") for p in POINTERS])


@pytest.mark.parametrize("kw,code,word", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _, _ in BAD])
def test_epoch_abi_rejects_bad_arguments_without_launching(kw, code, word):
    lib = N.load()
    assert lib.fcr_supervised_epoch(ctypes.byref(args(**kw)), None) == code
    msg = lib.fcr_last_error().decode()
    assert msg.startswith("fcr_supervised_epoch") and word in msg, msg


def test_epoch_abi_null_struct_and_empty_call():
    lib = N.load()
    assert lib.fcr_supervised_epoch(None, None) == -1 and "NULL" in lib.fcr_last_error().decode()
    assert lib.fcr_supervised_epoch(ctypes.byref(args(n_models=0, X=None, loss=None)), None) == 0      # no model: no launch
    # (every call of this file is refused or empty: none may reach a launch, its pointers are made up)


# ---- dispatch ------------------------------------------------------------------------------------------------------

def loaders(n=37, nv=21, bs=16, **kw):
    g = torch.Generator().manual_seed(3)
    X, y = torch.randn(n + nv, 3, generator=g), torch.rand(n + nv, 1, generator=g) - 0.5
    return (DataLoader(TensorDataset(X[:n], y[:n]), batch_size=bs, shuffle=True, **kw),
            DataLoader(TensorDataset(X[n:], y[n:]), batch_size=bs, shuffle=False))


def test_model_loss_and_optimizer_predicates():
    ok = fca.FNNModel(3, 50, 1, 1)
    assert "width_dim=2" in sl.model_reason(fca.FNNModel(3, 50, 1, 2))
    assert "hidden=65" in sl.model_reason(fca.FNNModel(3, 65, 1, 1))
    assert "ReLU" in sl.model_reason(fca.FNNModel(3, 50, 1, 1, nn.Tanh))
    assert "shape" in sl.model_reason(fca.FNNModel(4, 50, 1, 1)) and "shape" in sl.model_reason(fca.FNNModel(3, 50, 2, 1))
    assert "shape" in sl.model_reason(fca.FNNModel(3, 50, 1, 1, bias=False))
    assert "FNNModel" in sl.model_reason(nn.Linear(3, 1))
    assert "ROCm" in sl.model_reason(ok)                                   # the last check: a CPU model
    assert sl.loss_reason(nn.L1Loss()) is None and sl.loss_reason(nn.MSELoss()) is None
    assert "reduction" in sl.loss_reason(nn.L1Loss(reduction="sum")) and "HuberLoss" in sl.loss_reason(nn.HuberLoss())
    assert sl.optimizer_reason(torch.optim.AdamW(ok.parameters(), lr=1e-3), ok) is None
    assert "Adam," in sl.optimizer_reason(torch.optim.Adam(ok.parameters()), ok)
    assert "SGD" in sl.optimizer_reason(torch.optim.SGD(ok.parameters(), lr=0.1), ok)
    for flag in ("amsgrad", "maximize", "capturable"):
        assert flag in sl.optimizer_reason(torch.optim.AdamW(ok.parameters(), **{flag: True}), ok)
    assert "not in the optimizer" in sl.optimizer_reason(torch.optim.AdamW([ok.fc_inp.weight]), ok)
    split = torch.optim.AdamW([{"params": [ok.fc_inp.weight, ok.fc_inp.bias]}, {"params": [ok.fc_out.weight], "lr": 1e-2}])
    assert "groups" in sl.optimizer_reason(split, ok)


def test_train_loop_dispatch_on_each_disqualifying_case(monkeypatch):
    model = fca.FNNModel(3, 50, 1, 1)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    tl, vl = loaders()
    assert "ROCm" in sl.dispatch_reason(model, tl, vl, nn.L1Loss(), opt)
    monkeypatch.setattr(sl, "model_reason", lambda m: None)                # as if the model sat on a ROCm device
    assert sl.dispatch_reason(model, tl, vl, nn.L1Loss(), opt) is None
    assert sl.dispatch_reason(model, tl, vl, nn.MSELoss(), opt) is None
    assert "reduction" in sl.dispatch_reason(model, tl, vl, nn.MSELoss(reduction="sum"), opt)
    assert "amsgrad" in sl.dispatch_reason(model, tl, vl, nn.L1Loss(), torch.optim.AdamW(model.parameters(), amsgrad=True))
    X, y = tl.dataset.tensors

    class Rows(torch.utils.data.Dataset):
        def __len__(self):
            return len(X)

        def __getitem__(self, i):
            return X[i], y[i]

    for bad, word in ((DataLoader(Rows(), batch_size=16), "TensorDataset"),
                      (DataLoader(TensorDataset(X, y, y), batch_size=16), "TensorDataset"),
                      (DataLoader(TensorDataset(X.double(), y.double()), batch_size=16), "float32"),
                      (DataLoader(TensorDataset(X[:, :2], y), batch_size=16), "(n, 3)"),
                      (DataLoader(TensorDataset(X, y), batch_size=16, drop_last=True), "drop_last"),
                      (DataLoader(TensorDataset(X, y), batch_size=None), "batching"),
                      (DataLoader(TensorDataset(X, y), batch_size=16,
                                  sampler=torch.utils.data.RandomSampler(range(len(X)), replacement=True)), "sampler"),
                      (DataLoader(TensorDataset(X, y), batch_size=sl.EPOCH_KERNEL_MAX_BATCH + 1), "EPOCH_KERNEL_MAX_BATCH"),
                      ([(X, y)], "DataLoader")):
        assert word in sl.dispatch_reason(model, bad, vl, nn.L1Loss(), opt), word
        assert word in sl.dispatch_reason(model, tl, bad, nn.L1Loss(), opt), word
    assert sl.dispatch_reason(model, DataLoader(TensorDataset(X, y), batch_size=sl.EPOCH_KERNEL_MAX_BATCH), vl,
                              nn.L1Loss(), opt) is None


def test_loader_order_is_drawn_as_the_loader_draws_it():
    """_draw_order consumes the generators exactly as iter(loader) does, so the kernel path of train_loop sees the
    batches the eager loop would see under the same seed."""
    for own in (False, True):
        def make():
            tl, _ = loaders(generator=torch.Generator().manual_seed(9)) if own else loaders()
            return tl
        torch.manual_seed(4)
        tl = make()
        want = [torch.cat([x for x, _ in tl]) for _ in range(2)]
        after = torch.rand(1)
        torch.manual_seed(4)
        tl = make()
        got = [tl.dataset.tensors[0][sl._draw_order(tl)] for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(want, got)) and torch.equal(after, torch.rand(1))
    torch.manual_seed(4)
    _, vl = loaders()
    assert sl._draw_order(vl) is None


# ---- the fall-back -------------------------------------------------------------------------------------------------

def reference_train_loop(controller, train_loader, val_loader, loss_function, optimizer, n_epochs, device):
    """SL/Functions.py:396-422, 425-464 and 564-630, restated literally (without the logging and the progress bar)."""
    def train_model(data_loader, model, loss_function, optimizer, device):
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
        avg_loss = total_loss / len(data_loader)
        return avg_loss

    def validate_model(data_loader, model, loss_function, device):
        model.eval()
        total_loss = 0
        with torch.no_grad():
            for X, y in data_loader:
                X, y = X.to(device), y.to(device)
                output = model(X)
                total_loss += loss_function(output, y).item()
        avg_loss = total_loss / len(data_loader)
        return avg_loss

    validation_loss = validate_model(val_loader, controller, loss_function, device)
    vec_t_loss, vec_v_loss = [], []
    for ix_epoch in range(n_epochs):
        training_loss = train_model(train_loader, controller, loss_function, optimizer, device)
        validation_loss = validate_model(val_loader, controller, loss_function, device)
        vec_t_loss.append(training_loss)
        vec_v_loss.append(validation_loss)
    return controller, vec_t_loss, vec_v_loss


@pytest.mark.parametrize("width", [1, 2])
def test_train_loop_on_the_cpu_is_the_references_loop_bit_for_bit(width):
    runs = []
    for loop in (reference_train_loop, sl.train_loop):
        torch.manual_seed(17)
        model = fca.FNNModel(3, 50, 1, width)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        tl, vl = loaders()
        out = loop(model, tl, vl, nn.L1Loss(), opt, 3, torch.device("cpu"))
        assert out[0] is model
        runs.append((out[1], out[2], [p.detach().clone() for p in model.parameters()], torch.rand(1)))
    assert len(runs[1][0]) == 3
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2])) and torch.equal(runs[0][3], runs[1][3])


def test_train_loop_returns_the_references_four_values():
    torch.manual_seed(1)
    model = fca.FNNModel(3, 8, 1, 1)
    tl, vl = loaders()
    out = sl.train_loop(model, tl, vl, nn.MSELoss(), torch.optim.AdamW(model.parameters()), 2, torch.device("cpu"))
    assert len(out) == 4 and out[0] is model and len(out[1]) == len(out[2]) == 2 and isinstance(out[3], float)
    assert all(isinstance(v, float) for v in out[1] + out[2])


def test_entry_points_refuse_what_the_kernel_cannot_run():
    model = fca.FNNModel(3, 50, 1, 1)
    X, y = loaders()[0].dataset.tensors
    with pytest.raises(ValueError, match="ROCm"):
        sl.train_epoch(model, torch.optim.AdamW(model.parameters()), X, y)
    with pytest.raises(ValueError, match="ROCm"):
        sl.evaluate(model, X, y)
    with pytest.raises(ValueError, match="one optimizer per model"):
        sl.train_epoch([model, model], [torch.optim.AdamW(model.parameters())], X, y)
    with pytest.raises(ValueError, match="'l1' or 'mse'"):
        sl.evaluate(model, X, y, loss="huber")
    assert fca.supervised is sl and "supervised" in fca.__all__
