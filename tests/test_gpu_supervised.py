"""GPU: the supervised baseline's epoch kernel (fcr_supervised_epoch, csrc/fcr_supervised.h) against the same model in
float64 on the CPU — torch autograd and torch.optim.AdamW, fed the same permutation, written here.

Bar: 1e-5 of each tensor's max-abs (the project's bar for fp32 paths) wherever no sample sits on a kink (|pre| = 1,
z_k = 0, out = y); the kinks themselves are checked exactly; the multi-step runs are held to what torch's own fp32 run
of the same steps achieves (4x its distance to fp64, or 1e-5)."""
import copy

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

import forging_control_amd as fca
from forging_control_amd import supervised as sl

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-5
CLEAR = 1e-4          # no sample of a one-step case lies this close to a kink (asserted on the fp64 side)
LOSS = {"l1": nn.L1Loss, "mse": nn.MSELoss}
NAMES = ("fc_inp.weight", "fc_inp.bias", "fc_out.weight")


def trained(m):
    return m.fc_inp.weight, m.fc_inp.bias, m.fc_out.weight


def rel(a, b):
    """max |a - b| over max |b| (b: the fp64 side)."""
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def make_models(M, hidden, seed, out_gain=1.0):
    """M different FNNModels (CPU, fp32): Xavier weights, a non-zero bias, fc_out scaled by out_gain."""
    g = torch.Generator().manual_seed(seed)
    models = []
    for _ in range(M):
        m = fca.FNNModel(3, hidden, 1, 1)
        with torch.no_grad():
            m.fc_inp.weight.copy_(torch.randn(hidden, 3, generator=g) * 0.7)
            m.fc_inp.bias.copy_(torch.randn(hidden, generator=g) * 0.3)
            m.fc_out.weight.copy_(torch.randn(1, hidden, generator=g) * out_gain / hidden ** 0.5)
        models.append(m)
    return models


def forward64(m, X):
    z = X @ m.fc_inp.weight.T + m.fc_inp.bias
    pre = torch.relu(z) @ m.fc_out.weight.T
    return z, pre, torch.clamp(pre, -1.0, 1.0)


def clearance(models64, X, y):
    """Distance of the nearest sample to a kink, over the models: min(|z_k|, ||pre| - 1|, |out - y|)."""
    d = float("inf")
    with torch.no_grad():
        for m in models64:
            z, pre, out = forward64(m, X)
            d = min(d, float(z.abs().min()), float((pre.abs() - 1).abs().min()), float((out - y).abs().min()))
    return d


def draw_clear(models, n, seed, margin=CLEAR):
    """(X (n,3), y (n,1)) fp32 with every sample at least `margin` from every kink of every model (rows that come
    closer are redrawn; judged in fp64)."""
    g = torch.Generator().manual_seed(seed)
    m64 = [copy.deepcopy(m).double() for m in models]
    X = torch.randn(n, 3, generator=g)
    y = torch.rand(n, 1, generator=g) * 1.6 - 0.8
    for _ in range(200):
        with torch.no_grad():
            bad = torch.zeros(n, dtype=torch.bool)
            for m in m64:
                z, pre, out = forward64(m, X.double())
                bad |= (z.abs().min(dim=1).values < margin) | ((pre.abs() - 1).abs()[:, 0] < margin) | \
                       ((out - y.double()).abs()[:, 0] < margin)
        if not bad.any():
            return X, y
        k = int(bad.sum())
        X[bad] = torch.randn(k, 3, generator=g)
        y[bad] = torch.rand(k, 1, generator=g) * 1.6 - 0.8
    raise AssertionError("could not draw samples clear of the kinks")


def make_state(models, seed, step=5):
    """Per model {name: (exp_avg, exp_avg_sq)} fp32 non-zero moments, as after `step` steps."""
    g = torch.Generator().manual_seed(seed)
    return [{n: (torch.randn(p.shape, generator=g) * 0.05, torch.rand(p.shape, generator=g) * 0.01 + 1e-4)
             for n, p in zip(NAMES, trained(m))} for m in models], float(step)


def optimizer_for(m, state=None, step=0.0, **kw):
    opt = torch.optim.AdamW(m.parameters(), lr=kw.pop("lr", 1e-3), **kw)
    if state is not None:
        for n, p in zip(NAMES, trained(m)):
            opt.state[p] = {"step": torch.tensor(step, dtype=torch.float32),
                            "exp_avg": state[n][0].to(p.device, p.dtype).clone(),
                            "exp_avg_sq": state[n][1].to(p.device, p.dtype).clone()}
    return opt


def reference_epochs(models, states, step, X, y, perms, bs, loss, dtype, epochs=1, tie=None, **kw):
    """The same run on the CPU in `dtype` (torch autograd + AdamW): returns the models, optimizers, per-epoch
    (M, n_batches) losses and the ReLU / Hardtanh masks of every step (to compare two precisions' paths).
    perms: per epoch a (M, n) index tensor. tie: (n,) bool — samples whose |out - y| is exactly 0 in the kernel's
    arithmetic: their loss term is cut from the graph, as torch's sign(0) = 0 cuts it."""
    ms = [copy.deepcopy(m).to(dtype) for m in models]
    opts = [optimizer_for(m, None if states is None else states[i], step, **kw) for i, m in enumerate(ms)]
    Xd, yd = X.to(dtype), y.to(dtype).reshape(-1, 1)
    losses, masks = [], []
    for e in range(epochs):
        ep = []
        for i, (m, o) in enumerate(zip(ms, opts)):
            row = []
            for s in range(0, X.shape[0], bs):
                idx = perms[e][i, s:s + bs].long()
                o.zero_grad()
                z, pre, out = forward64(m, Xd[idx])
                if tie is None:
                    l = LOSS[loss]()(out, yd[idx])
                else:
                    l = ((out - yd[idx]).abs() * (~tie[idx]).reshape(-1, 1)).sum() / idx.numel()
                l.backward()
                o.step()
                row.append(float(l.detach()))
                masks.append(((z > 0).clone(), ((pre > -1) & (pre < 1)).clone()))
            ep.append(row)
        losses.append(torch.tensor(ep, dtype=torch.float64))
    return ms, opts, losses, masks


def to_gpu(models, states=None, step=0.0, **kw):
    ms = [copy.deepcopy(m).to(DEV) for m in models]
    return ms, [optimizer_for(m, None if states is None else states[i], step, **kw) for i, m in enumerate(ms)]


def check_against(ms, opts, ref_ms, ref_opts, bar, what):
    errs = {}
    for i, (m, o, rm, ro) in enumerate(zip(ms, opts, ref_ms, ref_opts)):
        for n, p, rp in zip(NAMES, trained(m), trained(rm)):
            errs[f"{what} m{i} {n}"] = rel(p, rp)
            errs[f"{what} m{i} {n} exp_avg"] = rel(o.state[p]["exp_avg"], ro.state[rp]["exp_avg"])
            errs[f"{what} m{i} {n} exp_avg_sq"] = rel(o.state[p]["exp_avg_sq"], ro.state[rp]["exp_avg_sq"])
            assert float(o.state[p]["step"]) == float(ro.state[rp]["step"]), (what, i, n)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= bar}
    assert not bad, bad


def perms_for(M, n, seed, epochs=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.stack([torch.randperm(n, generator=g) for _ in range(M)]) for _ in range(epochs)]


# ---- one step from a given state -----------------------------------------------------------------------------------
# one batch each: a short one, one larger than a pass of the 256 lanes, the wave boundary, hidden 7 / 50 / 64, M 1 / 3
ONE_STEP = [(5, 16, 50, 1), (16, 16, 50, 3), (300, 300, 50, 3), (64, 64, 7, 1), (65, 65, 64, 3)]


@pytest.mark.parametrize("loss", ["l1", "mse"])
@pytest.mark.parametrize("n,bs,hidden,M", ONE_STEP)
def test_one_step_from_a_given_state(n, bs, hidden, M, loss):
    models = make_models(M, hidden, seed=11)
    X, y = draw_clear(models, n, seed=12)
    states, step = make_state(models, seed=13)
    perms = perms_for(M, n, seed=14)
    kw = dict(weight_decay=0.05)
    r64, o64, l64, _ = reference_epochs(models, states, step, X, y, perms, bs, loss, torch.float64, **kw)
    assert clearance([copy.deepcopy(m).double() for m in models], X.double(), y.double()) >= CLEAR
    # torch's own fp32 step passes the same bar on these inputs
    r32, o32, l32, _ = reference_epochs(models, states, step, X, y, perms, bs, loss, torch.float32, **kw)
    check_against(r32, o32, r64, o64, BAR, "torch-fp32")
    ms, opts = to_gpu(models, states, step, **kw)
    avg, batch = sl.train_epoch(ms, opts, X, y, bs, loss=loss, perm=perms[0], return_batch_losses=True)
    assert batch.shape == (M, 1) and rel(batch, l64[0]) <= BAR, (batch, l64[0])
    assert rel(torch.tensor(avg), l64[0].mean(dim=1)) <= BAR
    check_against(ms, opts, r64, o64, BAR, "kernel")
    assert all(float(o.state[p]["step"]) == 6.0 for m, o in zip(ms, opts) for p in trained(m))


# ---- the kinks themselves, exactly ---------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["l1", "mse"])
def test_saturated_samples_and_a_dead_unit(loss):
    """Samples with pre >= 1 and pre <= -1 give no gradient; a hidden unit dead for every sample has gradient exactly
    0, and AdamW still decays its moments and its weights."""
    n, hidden, dead = 48, 50, 3
    models = make_models(1, hidden, seed=21, out_gain=6.0)
    with torch.no_grad():
        models[0].fc_inp.bias[dead] = -100.0
    X, y = draw_clear(models, n, seed=22)
    m64 = copy.deepcopy(models[0]).double()
    with torch.no_grad():
        z, pre, _ = forward64(m64, X.double())
    assert int((pre >= 1).sum()) >= 3 and int((pre <= -1).sum()) >= 3 and int((pre.abs() < 1).sum()) >= 3
    assert bool((z[:, dead] < 0).all())
    perms = perms_for(1, n, seed=23)
    states, step = make_state(models, seed=24)
    kw = dict(weight_decay=0.05)
    r64, o64, l64, _ = reference_epochs(models, states, step, X, y, perms, n, loss, torch.float64, **kw)
    ms, opts = to_gpu(models, states, step, **kw)
    _, batch = sl.train_epoch(ms, opts, X, y, n, loss=loss, perm=perms[0], return_batch_losses=True)
    assert rel(batch, l64[0]) <= BAR
    check_against(ms, opts, r64, o64, BAR, "kernel")
    # from a fresh optimizer the dead unit's step is exact: zero moments, and only the decoupled decay moves it
    ms, opts = to_gpu(models, None, **kw)
    sl.train_epoch(ms, opts, X, y, n, loss=loss, perm=perms[0])
    decay = torch.tensor(1.0 - 1e-3 * 0.05, dtype=torch.float32)
    for p, p0 in zip(trained(ms[0]), trained(models[0])):
        row = (lambda t: t[dead] if t.dim() == 1 else (t[dead] if t.shape[0] == hidden else t[0, dead]))
        assert torch.equal(row(p.detach().cpu()), row(p0.detach()) * decay)
        st = opts[0].state[p]
        assert float(row(st["exp_avg"]).abs().max()) == 0.0 and float(row(st["exp_avg_sq"]).abs().max()) == 0.0


def test_l1_gradient_of_an_exact_tie_is_zero():
    """Samples with out == y bit for bit (y built from the kernel's own fp32 outputs) add nothing to the L1 gradient:
    sign(0) = 0, as torch's L1 backward."""
    n, hidden = 40, 50
    models = make_models(1, hidden, seed=31)
    X, y = draw_clear(models, n, seed=32, margin=1e-3)
    gm = copy.deepcopy(models[0]).to(DEV)
    # batch size 1 against y = 0: each "batch" loss is |out| of one sample, exactly (a sum of one term, times 1)
    _, mag = sl.evaluate(gm, X, torch.zeros(n), 1, "l1", return_batch_losses=True)
    with torch.no_grad():
        _, pre64, out64 = (t[:, 0] if t.shape[1] == 1 else t for t in forward64(copy.deepcopy(models[0]).double(), X.double()))
    assert float(out64.abs().min()) >= 1e-3            # so the sign of every fp32 out is the fp64 one's
    out32 = torch.sign(out64).float() * mag.cpu()
    assert rel(out32, out64) <= BAR
    tie = (torch.arange(n) % 2 == 0) & (pre64.abs() < 1 - 1e-3)        # ties among the samples that carry a gradient
    assert int(tie.sum()) >= 8
    y = torch.where(tie, out32, y[:, 0])
    _, batch = sl.evaluate(gm, X, y, 1, "l1", return_batch_losses=True)
    assert bool((batch.cpu()[tie] == 0).all()) and bool((batch.cpu()[~tie] > 0).all())      # the ties are exact
    perms = perms_for(1, n, seed=33)
    states, step = make_state(models, seed=34)
    r64, o64, l64, _ = reference_epochs(models, states, step, X, y, perms, n, "l1", torch.float64, tie=tie)
    ms, opts = to_gpu(models, states, step)
    _, batch = sl.train_epoch(ms, opts, X, y, n, loss="l1", perm=perms[0], return_batch_losses=True)
    assert rel(batch, l64[0]) <= BAR
    check_against(ms, opts, r64, o64, BAR, "kernel")
    # and the bar sees it: counting the ties as sign = +1 moves the first moment well beyond it
    rp, op, _, _ = reference_epochs(models, states, step, X, y.double() - tie * 1e-6, perms, n, "l1", torch.float64)
    assert rel(op[0].state[rp[0].fc_out.weight]["exp_avg"], o64[0].state[r64[0].fc_out.weight]["exp_avg"]) > 100 * BAR


# ---- short runs ----------------------------------------------------------------------------------------------------
# (n, bs, hidden, M, epochs, seed): two full batches and a short one of 5 for three epochs; the wave boundary
# (64 | 64 | 2 and 65 | 65); hidden 7 and 64. Seeds: torch's fp32 run takes the same ReLU / Hardtanh branches as its fp64
# run in every step (asserted below), and ends within 1e-6 of it under both losses, so the bar below is 1e-5. (Other
# seeds leave torch's fp32 L1 run 1e-4 away: a gradient that cancels to rounding noise, which Adam's first steps
# normalise to a full-size move.)
SHORT = [(37, 16, 50, 3, 3, 3), (130, 64, 50, 1, 1, 1), (130, 65, 7, 3, 1, 2), (130, 65, 64, 1, 1, 4)]


@pytest.mark.parametrize("loss", ["l1", "mse"])
@pytest.mark.parametrize("n,bs,hidden,M,epochs,seed", SHORT)
def test_short_run_stays_as_close_to_fp64_as_torch_fp32(n, bs, hidden, M, epochs, seed, loss):
    models = make_models(M, hidden, seed=40 + seed)
    X, y = draw_clear(models, n, seed=50 + seed)
    perms = perms_for(M, n, seed=60 + seed, epochs=epochs)
    r64, o64, l64, k64 = reference_epochs(models, None, 0.0, X, y, perms, bs, loss, torch.float64, epochs=epochs)
    r32, o32, l32, k32 = reference_epochs(models, None, 0.0, X, y, perms, bs, loss, torch.float32, epochs=epochs)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(k64, k32)), \
        "a sample crosses a kink between fp32 and fp64: pick another seed"
    d32 = max(rel(p, q) for a, b in zip(r32, r64) for p, q in zip(trained(a), trained(b)))
    ms, opts = to_gpu(models)
    got = [sl.train_epoch(ms, opts, X, y, bs, loss=loss, perm=perms[e], return_batch_losses=True)[1]
           for e in range(epochs)]
    dk = max(rel(p, q) for a, b in zip(ms, r64) for p, q in zip(trained(a), trained(b)))
    print(f"parameters vs fp64: torch fp32 {d32:.3e}, kernel {dk:.3e}")
    bar = max(4 * d32, BAR)
    assert dk <= bar, (dk, d32)
    for e in range(epochs):
        assert got[e].shape == l64[e].shape and rel(got[e], l64[e]) <= bar, (e, got[e], l64[e])
    check_against(ms, opts, r64, o64, bar, "kernel")


def test_the_same_call_twice_is_bit_identical():
    models = make_models(3, 50, seed=71)
    X, y = draw_clear(models, 300, seed=72)
    perms = perms_for(3, 300, seed=73)
    runs = []
    for _ in range(2):
        ms, opts = to_gpu(models)
        _, batch = sl.train_epoch(ms, opts, X, y, 33, perm=perms[0], return_batch_losses=True)
        runs.append([batch.cpu()] + [p.detach().cpu() for m in ms for p in trained(m)]
                    + [o.state[p][k].cpu() for m, o in zip(ms, opts) for p in trained(m) for k in ("exp_avg", "exp_avg_sq")])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_generator_draws_the_permutations_a_shuffling_loader_would():
    models = make_models(2, 50, seed=74)
    X, y = draw_clear(models, 37, seed=75)
    g = torch.Generator().manual_seed(5)
    perm = torch.stack([torch.randperm(37, generator=g) for _ in range(2)])
    a, oa = to_gpu(models)
    b, ob = to_gpu(models)
    la = sl.train_epoch(a, oa, X, y, 16, generator=torch.Generator().manual_seed(5))
    lb = sl.train_epoch(b, ob, X, y, 16, perm=perm)
    assert la == lb and all(torch.equal(p, q) for m, k in zip(a, b) for p, q in zip(trained(m), trained(k)))


# ---- state hand-over -----------------------------------------------------------------------------------------------

def test_torch_continues_the_run_from_the_kernels_state():
    n, bs, hidden = 37, 16, 50
    models = make_models(1, hidden, seed=81)
    X, y = draw_clear(models, n + 8, seed=82)
    Xe, ye, Xn, yn = X[:n], y[:n], X[n:], y[n:]
    perms = perms_for(1, n, seed=83)
    r64, o64, _, _ = reference_epochs(models, None, 0.0, Xe, ye, perms, bs, "l1", torch.float64)
    o64[0].zero_grad()
    nn.L1Loss()(r64[0](Xn.double()), yn.double()).backward()
    o64[0].step()
    ms, opts = to_gpu(models)
    sl.train_epoch(ms[0], opts[0], Xe, ye, bs, perm=perms[0])
    sd, sd64 = opts[0].state_dict(), None
    # what torch's own run leaves: state for parameters 0, 1 and 4 (fc_int's 2 and 3 never saw a gradient)
    fresh = copy.deepcopy(models[0])
    o = torch.optim.AdamW(fresh.parameters(), lr=1e-3)
    nn.L1Loss()(fresh(Xn), yn).backward()
    o.step()
    sd64 = o.state_dict()
    assert list(sd["state"].keys()) == list(sd64["state"].keys()) == [0, 1, 4]
    for k in sd["state"]:
        assert list(sd["state"][k].keys()) == list(sd64["state"][k].keys()) == ["step", "exp_avg", "exp_avg_sq"]
        for name in ("step", "exp_avg", "exp_avg_sq"):
            a, b = sd["state"][k][name], sd64["state"][k][name]
            assert a.shape == b.shape and a.dtype == b.dtype and (name != "step" or a.device == b.device)
        assert float(sd["state"][k]["step"]) == 3.0 and sd["state"][k]["exp_avg"].is_cuda
    assert sd["param_groups"] == sd64["param_groups"]
    assert ms[0].fc_int.weight.grad is None and torch.equal(ms[0].fc_int.weight.cpu(), models[0].fc_int.weight)
    opts[0].zero_grad()
    nn.L1Loss()(ms[0](Xn.to(DEV)), yn.to(DEV)).backward()
    opts[0].step()
    check_against(ms, opts, r64, o64, BAR, "epoch + torch step")
    assert float(opts[0].state[ms[0].fc_out.weight]["step"]) == 4.0


# ---- evaluate ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["l1", "mse"])
def test_evaluate_matches_fp64_and_changes_nothing(loss):
    n, bs = 300, 64
    models = make_models(3, 50, seed=91)
    X, y = draw_clear(models, n, seed=92)
    ms, _ = to_gpu(models)
    before = [p.detach().clone() for m in ms for p in m.parameters()]
    avg, batch = sl.evaluate(ms, X, y, bs, loss, return_batch_losses=True)
    assert all(torch.equal(a, b) for a, b in zip(before, [p for m in ms for p in m.parameters()]))
    want = torch.tensor([[float(LOSS[loss]()(forward64(copy.deepcopy(m).double(), X[s:s + bs].double())[2], y[s:s + bs].double()))
                          for s in range(0, n, bs)] for m in models], dtype=torch.float64)
    assert batch.shape == (3, 5) and rel(batch, want) <= BAR
    assert rel(torch.tensor(avg), want.mean(dim=1)) <= BAR
    one = sl.evaluate(ms[1], X, y, bs, LOSS[loss]())
    assert isinstance(one, float) and one == avg[1]


# ---- train_loop ----------------------------------------------------------------------------------------------------

def loaders(X, y, Xv, yv, bs, seed):
    torch.manual_seed(seed)
    return (DataLoader(TensorDataset(X, y), batch_size=bs, shuffle=True),
            DataLoader(TensorDataset(Xv, yv), batch_size=bs, shuffle=False))


def test_train_loop_on_the_gpu_follows_the_fp64_restatement():
    n, nv, bs, epochs = 37, 21, 16, 2
    models = make_models(1, 50, seed=101)
    X, y = draw_clear(models, n + nv, seed=102)
    Xt, yt, Xv, yv = X[:n], y[:n], X[n:], y[n:]
    # the reference's loop (SL/Functions.py:564-630) in fp64 on the CPU, shuffled by the same seed
    m64 = copy.deepcopy(models[0]).double()
    o64 = torch.optim.AdamW(m64.parameters(), lr=1e-3)
    tl, vl = loaders(Xt.double(), yt.double(), Xv.double(), yv.double(), bs, seed=7)
    _, t64, v64, _ = sl.train_loop(m64, tl, vl, nn.L1Loss(), o64, epochs, torch.device("cpu"))
    gm = copy.deepcopy(models[0]).to(DEV)
    og = torch.optim.AdamW(gm.parameters(), lr=1e-3)
    tl, vl = loaders(Xt, yt, Xv, yv, bs, seed=7)
    assert sl.dispatch_reason(gm, tl, vl, nn.L1Loss(), og) is None
    out, tg, vg, secs = sl.train_loop(gm, tl, vl, nn.L1Loss(), og, epochs, torch.device(DEV))
    assert out is gm and len(tg) == len(vg) == epochs and secs > 0
    # torch's own fp32 run of the same loop sets the bar, as for the short runs
    m32 = copy.deepcopy(models[0])
    tl, vl = loaders(Xt, yt, Xv, yv, bs, seed=7)
    _, t32, v32, _ = sl.train_loop(m32, tl, vl, nn.L1Loss(), torch.optim.AdamW(m32.parameters(), lr=1e-3), epochs,
                                   torch.device("cpu"))
    d32 = max(rel(p, q) for p, q in zip(trained(m32), trained(m64)))
    l32 = max(rel(torch.tensor(t32), torch.tensor(t64)), rel(torch.tensor(v32), torch.tensor(v64)))
    dk = max(rel(p, q) for p, q in zip(trained(gm), trained(m64)))
    lk = max(rel(torch.tensor(tg), torch.tensor(t64)), rel(torch.tensor(vg), torch.tensor(v64)))
    print(f"train {tg} {t64} validation {vg} {v64}; vs fp64: torch fp32 losses {l32:.2e} parameters {d32:.2e}, "
          f"kernel losses {lk:.2e} parameters {dk:.2e}")
    assert lk <= max(4 * l32, BAR) and dk <= max(4 * d32, BAR)
