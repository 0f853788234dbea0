"""Training a bank on the press, on the CPU: the torch restatement of tests/press_train_ref.py is
pinned (central differences, the truncation's two ends, six deliberate mistakes), the inputs the GPU tests share are
shown to drive every ReLU of the loss on both sides, and the three new entry points check their arguments before any
device call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import press_torch as pt
import press_train_ref as tr

T64 = lambda a: torch.tensor(np.asarray(a, np.float64))
N = fca._native


def _loss_of(c, m, x0, K=0, cdt=torch.float64, params=None):
    """Model m's (cost (B,), x, u) of case c from x0 (a tensor), through the restated loop."""
    w = params if params is not None else [T64(k) for k in c["ws"][m]]
    x, u = tr.closed_loop(x0, T64(c["refs"][m]), *w, c["smooth"], K, cdt, c["substeps"],
                          None if c["tables"] is None else c["tables"][m])
    return tr.cost(x, u, T64(c["refs"][m]), c["rows"][m], u_prev=None if c["u_prev"] is None else T64(c["u_prev"][m])), x, u


@pytest.mark.parametrize("smooth", [False, True])
def test_loss_autograd_matches_central_differences(smooth):
    """d cost[b] / d x0[b,1] (the initial speed) by autograd against (cost(x0 + h) - cost(x0 - h)) / 2h, h = 1e-6:
    within 1e-5 of the column's largest gradient for at least 95 % of the trajectories (one that crosses a kink of the
    press, of the controller or of the loss inside +-h is the remainder). (The valve column is no subject for this h: the
    difference quotient's own h^2 error reaches 8e-5 there on the deforming half of the batch and is gone at h = 1e-7.)"""
    c = tr.case(2, 64, 12, smooth=smooth, with_u_prev=True)
    for m in range(2):
        x0 = c["x0s"][m]
        a = T64(x0).requires_grad_(True)
        _loss_of(c, m, a)[0].sum().backward()
        g = a.grad.numpy()
        assert np.all(np.isfinite(g))
        for k in (1,):
            h = 1e-6
            xp, xm = x0.copy(), x0.copy()
            xp[:, k] += h
            xm[:, k] -= h
            with torch.no_grad():
                fd = ((_loss_of(c, m, T64(xp))[0] - _loss_of(c, m, T64(xm))[0]) / (2 * h)).numpy()
            rel = np.abs(fd - g[:, k]) / np.abs(g[:, k]).max()
            assert np.mean(rel <= 1e-5) >= 0.95, (m, k, np.mean(rel <= 1e-5), np.median(rel))


def _grads(c, m, K):
    a = T64(c["x0s"][m]).requires_grad_(True)
    P_ = [T64(k).requires_grad_(True) for k in c["ws"][m]]
    cost, x, u = _loss_of(c, m, a, K, params=P_)
    cost.mean().backward()
    return {"g_x0": a.grad.numpy(), "g_w_inp": P_[0].grad.numpy(), "g_b_inp": P_[1].grad.numpy(),
            "g_w_out": P_[2].grad.numpy().reshape(-1)}, x.detach().numpy(), u.detach().numpy(), cost.detach().numpy()


def test_truncation_beyond_the_run_is_no_truncation():
    c = tr.case(1, 60, 12, with_u_prev=True)
    full, _, _, cost0 = _grads(c, 0, 0)
    for K in (12, 40):
        got, _, _, cost = _grads(c, 0, K)
        assert np.array_equal(cost, cost0)
        assert all(np.array_equal(got[k], full[k]) for k in full), K
    cut = _grads(c, 0, 5)[0]
    assert max(pt.figures(cut, full).values()) > 1e-3            # and K < T is another gradient


def test_truncation_at_every_step_is_the_sum_of_one_step_gradients():
    """K = 1: every state is a constant, so the gradient is that of the T one-step problems side by side — the
    controller at the stored x_t, one press step from it, the loss's terms on (x_{t+1}, u_t, u_{t-1})."""
    c = tr.case(1, 60, 12, with_u_prev=True)
    got, x, u, _ = _grads(c, 0, 1)
    P_ = [T64(k).requires_grad_(True) for k in c["ws"][0]]
    a = T64(c["x0s"][0]).requires_grad_(True)
    ref = T64(c["refs"][0])
    starts = [a] + [T64(x[:, t]) for t in range(1, 12)]
    us = [pt.controller(s, ref[:, t], *P_, torch.float64)[0] for t, s in enumerate(starts)]
    nxt = [pt.step(s, v, True) for s, v in zip(starts, us)]
    cost = tr.cost(torch.stack([a] + nxt, 1), torch.stack(us, 1), ref, c["rows"][0], u_prev=T64(c["u_prev"][0]))
    cost.mean().backward()
    want = {"g_x0": a.grad.numpy(), "g_w_inp": P_[0].grad.numpy(), "g_b_inp": P_[1].grad.numpy(),
            "g_w_out": P_[2].grad.numpy().reshape(-1)}
    f = pt.figures(got, want)
    assert all(v <= 1e-12 for v in f.values()), f


@pytest.mark.parametrize("K", [0, 1, 5])
def test_stepwise_oracle_equals_autograd_of_the_detached_loop(K):
    """The segment-wise stepwise adjoint against end-to-end autograd of the loop with detach() at the truncation steps,
    controller in float64 on both sides, to 1e-9 of each tensor's maximum."""
    c = tr.case(2, 60, 12, with_u_prev=True)
    for m in range(2):
        want, x, u, cost = _grads(c, m, K)
        got = tr.model_stepwise(x, u, c["refs"][m], c["ws"][m], c["rows"][m], True, K, c["u_prev"][m], f64=True)
        assert np.allclose(got["cost"], cost, rtol=1e-13, atol=0)
        f = pt.figures(got, want)
        assert all(v <= 1e-9 for v in f.values()), (K, m, f)


@functools.lru_cache(maxsize=None)
def _mutant_case():
    """M = 2, B = 90, T = 12, K = 5, u_prev given, on the restatement's own record (float32 controller chain)."""
    c = tr.case(2, 90, 12, with_u_prev=True)
    us = []
    with torch.no_grad():
        for m in range(2):
            us.append(tr.closed_loop(T64(c["x0s"][m]), T64(c["refs"][m]), *(T64(k) for k in c["ws"][m]), True)[1].numpy())
    run = lambda mutant: tr.bank_stepwise(c["xs"], us, c["refs"], c["ws"], c["rows"], True, 5, c["u_prev"], mutant=mutant)
    return run, run(None)


@pytest.mark.parametrize("mutant", tr.MUTANTS)
def test_the_comparison_refuses_every_mutant(mutant):
    """Each deliberate mistake moves some gradient by at least 1e-3 of its tensor's maximum, and the comparison the GPU
    tests use turns it down."""
    run, good = _mutant_case()
    assert not tr.bank_refused(good, good)
    bad = run(mutant)
    f = tr.bank_figures(bad, good)
    assert max(f.values()) >= 1e-3, f
    assert tr.bank_refused(bad, good)


@pytest.mark.parametrize("press", [None, "model"])
@pytest.mark.parametrize("smooth", [False, True])
def test_inputs_drive_every_relu_of_the_loss(smooth, press):
    """The GPU tests' main case (M = 3, B = 300, T = 12): each of the four ReLU terms of every model is active on at
    least 5 % and inactive on at least 5 % of (b,t), and no scaled pressure lies within 1e-9 of a bound."""
    c = tr.case(3, 300, 12, smooth=smooth, press=press)
    shares, gap = tr.shares(c["xs"], c["rows"])
    for s in shares:
        assert all(0.05 <= v <= 0.95 for v in s.values()), shares
    assert gap > 1e-9, gap
    assert len({r[1:] for r in c["rows"]}) == 3                  # three models, three sets of bounds


# ------------------------------------------------------------------------------------------------ the entry points

def _bank_args(**kw):
    a = N.FcrClosedLoopBankGrad()
    a.n_models, a.B, a.T, a.ts, a.substeps, a.ctrl_hidden = 2, 4, 3, 1e-3, 4, 50
    a.in_scale[0] = a.in_scale[1] = a.ref_scale = a.out_scale = 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _loss_args(rows=((0.1, 0.0, 1.0, 0.0, 1.0, 1.0),), **kw):
    host = (ctypes.c_double * (6 * len(rows)))(*[v for r in rows for v in r])
    l = N.FcrPressLoss()
    l.terms_host = ctypes.cast(host, ctypes.POINTER(ctypes.c_double))
    l.terms_stride = 6 if len(rows) > 1 else 0
    l.p_scale[0] = l.p_scale[1] = 1.0
    for k, v in kw.items():
        if k == "p_scale":
            l.p_scale[0], l.p_scale[1] = v
        else:
            setattr(l, k, v)
    l._keep = host
    return l


COMMON = [
    (dict(n_models=-1), -1, "n_models="), (dict(n_models=70000), -4, "n_models="), (dict(B=-1), -1, "B="),
    (dict(T=-1), -1, "T="), (dict(ts=0.0), -1, "ts="), (dict(substeps=0), -1, "substeps="), (dict(smooth=2), -1, "smooth="),
    (dict(ctrl_hidden=0), -4, "ctrl_hidden=0"), (dict(ctrl_hidden=257), -4, "ctrl_hidden=257"),
    (dict(ref_scale=0.0), -1, "scale"), (dict(stride_traj=28), -1, "stride_traj"), (dict(stride_traj=27), -1, "stride_traj"),
    (dict(stride_model=28), -1, "stride_model"), (dict(stride_model=-28), -1, "stride"), (dict(ref_stride=5), -1, "ref_stride"),
    (dict(ref_stride=-12), -1, "ref_stride"), (dict(truncate=-1), -1, "truncate="), (dict(), -1, "NULL"),
]


@pytest.mark.parametrize("kw,code,msg", COMMON)
def test_bank_vjp_rejects_bad_arguments_before_any_device_call(kw, code, msg):
    lib = N.load()
    assert lib.fcr_closed_loop_bank_vjp(ctypes.byref(_bank_args(**kw)), None, None, None, 0, None) == code
    assert msg in lib.fcr_last_error().decode()
    assert lib.fcr_closed_loop_bank_vjp(None, None, None, None, 0, None) == -1 and "NULL" in lib.fcr_last_error().decode()


@pytest.mark.parametrize("kw,code,msg", COMMON)
def test_bank_loss_vjp_rejects_bad_arguments_before_any_device_call(kw, code, msg):
    lib = N.load()
    l = _loss_args()
    assert lib.fcr_closed_loop_bank_loss_vjp(ctypes.byref(_bank_args(**kw)), ctypes.byref(l), None, 0, None) == code
    assert msg in lib.fcr_last_error().decode()


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("rows,kw,msg", [
    (((0.1, 0.0, 1.0, 0.0, 1.0, 1.0), (NAN, 0.0, 1.0, 0.0, 1.0, 1.0)), {}, "row 1 holds a NaN"),
    (((0.1, 0.0, NAN, 0.0, 1.0, 1.0),), {}, "NaN"), (((INF, 0.0, 1.0, 0.0, 1.0, 1.0),), {}, "alpha="),
    (((0.1, 2.0, 1.0, 0.0, 1.0, 1.0),), {}, "lower bound"), (((0.1, 0.0, 1.0, 1.5, 1.0, 1.0),), {}, "lower bound"),
    (((0.1, 0.0, 1.0, 0.0, 1.0, -1.0),), {}, "weight="), (((0.1, 0.0, 1.0, 0.0, 1.0, INF),), {}, "weight="),
    (None, dict(p_scale=(0.0, 1.0)), "p_scale"), (None, dict(p_scale=(1.0, NAN)), "p_scale"),
    (None, dict(terms_stride=3), "terms_stride"), (None, dict(u_prev_stride=2), "u_prev_stride"),
    (None, dict(u_prev_stride=4), "without u_prev"), (None, dict(terms_host=None), "terms_host"),
])
def test_bank_loss_vjp_checks_the_loss_before_any_device_call(rows, kw, msg):
    lib = N.load()
    l = _loss_args(**kw) if rows is None else _loss_args(rows, **kw)
    assert lib.fcr_closed_loop_bank_loss_vjp(ctypes.byref(_bank_args()), ctypes.byref(l), None, 0, None) == -1
    assert msg in lib.fcr_last_error().decode()
    assert lib.fcr_closed_loop_bank_loss_vjp(ctypes.byref(_bank_args()), None, None, 0, None) == -1
    assert "loss is NULL" in lib.fcr_last_error().decode()


def test_infinite_bounds_and_a_zero_weight_are_accepted():
    """-inf / +inf switch a side off and w = 0 the whole term: the rows pass, the call then stops at its NULL pointers."""
    lib = N.load()
    l = _loss_args(((0.0, -INF, INF, -INF, 0.5, 0.0),))
    assert lib.fcr_closed_loop_bank_loss_vjp(ctypes.byref(_bank_args()), ctypes.byref(l), None, 0, None) == -1
    assert "NULL" in lib.fcr_last_error().decode() and "terms" not in lib.fcr_last_error().decode()


def test_workspace_query_and_empty_calls():
    lib = N.load()
    size, one = ctypes.c_size_t(7), ctypes.c_size_t(0)
    assert lib.fcr_closed_loop_bank_vjp_workspace_size(3, 300, 40, 65, ctypes.byref(size)) == 0
    assert lib.fcr_closed_loop_vjp_workspace_size(300, 40, 65, ctypes.byref(one)) == 0
    assert 3 * 47 * 65 * 5 * 8 <= size.value <= 3 * one.value + 2 * 256     # M times the single model's, and the cost's sums
    assert lib.fcr_closed_loop_bank_vjp_workspace_size(3, 300, 40, 257, ctypes.byref(size)) == -4 and size.value == 0
    assert lib.fcr_closed_loop_bank_vjp_workspace_size(3, 300, 40, 0, ctypes.byref(size)) == -4
    assert lib.fcr_closed_loop_bank_vjp_workspace_size(-1, 300, 40, 50, ctypes.byref(size)) == -1
    assert lib.fcr_closed_loop_bank_vjp_workspace_size(3, -1, 40, 50, ctypes.byref(size)) == -1
    assert lib.fcr_closed_loop_bank_vjp_workspace_size(3, 300, 40, 50, None) == -1
    for kw in (dict(n_models=0), dict(B=0)):
        assert lib.fcr_closed_loop_bank_vjp_workspace_size(kw.get("n_models", 3), kw.get("B", 300), 40, 50, ctypes.byref(size)) == 0
        assert size.value == 0
        assert lib.fcr_closed_loop_bank_vjp(ctypes.byref(_bank_args(**kw)), None, None, None, 0, None) == 0
        assert lib.fcr_closed_loop_bank_loss_vjp(ctypes.byref(_bank_args(**kw)), ctypes.byref(_loss_args()), None, 0, None) == 0


def test_new_symbols_are_exported_declared_and_typed():
    lib = N.load()
    header = open(f"{pt.GOLDEN}/../../include/fcr.h").read()
    for name in ("fcr_closed_loop_bank_vjp_workspace_size", "fcr_closed_loop_bank_vjp", "fcr_closed_loop_bank_loss_vjp"):
        assert name in N.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
        assert getattr(lib, name).argtypes is not None
    assert N.ABI_VERSION == 8 and lib.fcr_abi_version() == 8
    for name in ("PressLoss", "train_on_press", "press_loss"):
        assert name in fca.__all__ and hasattr(fca, name)


def _bank(M=2, hidden=50):
    bank = fca.ControllerBank(M, hidden)
    return fca.ClosedLoopBank(bank, pt.SCALERS)


def test_differentiable_bank_run_refuses_noise_recovery_not_storing_and_cpu():
    cl = _bank()
    x0, ref = torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    noise = torch.zeros(2, 3, 5, dtype=torch.float64)
    for kw in (dict(process_noise=noise), dict(meas_noise=noise), dict(feasibility=fca.FeasibilityRecovery()),
               dict(store=False)):
        with pytest.raises(ValueError, match="differentiable=True"):
            cl.run(x0, ref, differentiable=True, **kw)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        cl.run(x0, ref, differentiable=True)


def test_press_loss_checks_its_arguments():
    cl = _bank(2)
    with pytest.raises(TypeError, match="ClosedLoop"):
        fca.PressLoss(object(), tr.P_SCALE)
    for bad in ((1.0,), (0.0, 1.0), (1.0, float("inf")), "ab"):
        with pytest.raises(ValueError, match="p_scale"):
            fca.PressLoss(cl, bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="truncate"):
            fca.PressLoss(cl, tr.P_SCALE, truncate=bad)
    with pytest.raises(ValueError, match="3 LossTerms for a bank of 2"):
        fca.PressLoss(cl, tr.P_SCALE, terms=[fca.LossTerms()] * 3)
    with pytest.raises(TypeError):
        fca.PressLoss(cl, tr.P_SCALE, terms=[(0.0, 1.0)] * 2)
    pl = fca.PressLoss(cl, tr.P_SCALE, terms=[fca.LossTerms(alpha=3.0), fca.LossTerms(p1=(0.1, 0.2))], alpha=0.5, truncate=4)
    assert pl.rows() == [(3.0, 0.0, N.P1_MAX, 0.0, N.P2_MAX, 1.0), (0.5, 0.1, 0.2, 0.0, N.P2_MAX, 1.0)] and pl.n_models == 2
    single = fca.PressLoss(fca.ClosedLoop(fca.FNNModel(3, 50, 1, 1), pt.SCALERS), tr.P_SCALE)
    assert single.n_models == 1 and single.rows() == [(0.1, 0.0, N.P1_MAX, 0.0, N.P2_MAX, 1.0)]
    x0, ref = torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        pl.forward(x0, ref)
    with pytest.raises(ValueError, match="another loop"):
        fca.train_on_press([], _bank(2), pl, None)
