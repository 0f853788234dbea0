"""Gradients with respect to the 28 press parameters on the CPU: the restatement with the press as a
tensor (tests/press_param_torch.py) is pinned to tests/press_torch.py; its stepwise oracle to end-to-end autograd and to
central differences; the comparison of the GPU tests refuses seven deliberate mistakes; the inputs drive both sides of
every branch; the four new entry points check their arguments before any device call; and the fit's yardstick
(tests/golden/press_fit_cpu.json) is reproduced."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import press_param_torch as pp
import press_torch as pt

N = fca._native
T64 = lambda a: torch.tensor(np.asarray(a, np.float64))
FAKE = 4096                                 # a non-NULL, aligned address no refused call ever reads
NEW = ("fcr_plant_rk4_vjp_press", "fcr_closed_loop_vjp_press", "fcr_press_grad_sum_workspace_size", "fcr_press_grad_sum")


@pytest.mark.parametrize("smooth", [False, True])
def test_restatement_is_press_torchs(smooth):
    """rhs, step and a 12-step trajectory under three presses, and the edge rows under the oracle's: within 1e-15 of each
    value's magnitude (the same operations in the same order: the difference found is 0)."""
    x0, U = pt.open_batch(48, 12)
    tab = pt.three_rows_table(48)
    xe, ue = pt.edge_rows()
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())
    assert rel(pp.rhs(T64(x0), T64(U[:, 0]), smooth, T64(tab)), pt.rhs(T64(x0), T64(U[:, 0]), smooth, tab)) <= 1e-15
    assert rel(pp.step(T64(x0), T64(U[:, 0]), smooth, T64(tab)), pt.step(T64(x0), T64(U[:, 0]), smooth, table=tab)) <= 1e-15
    assert rel(pp.trajectory(T64(x0), T64(U), smooth, T64(tab)), pt.trajectory(T64(x0), T64(U), smooth, table=tab)) <= 1e-15
    row = np.tile(pt.oracle_row(), (8, 1))
    assert rel(pp.step(T64(xe), T64(ue[:, 0]), smooth, T64(row)), pt.step(T64(xe), T64(ue[:, 0]), smooth, table=row)) <= 1e-15
    for mutant in pp.MUTANTS:                # a mutant changes gradients only
        assert torch.equal(pp.step(T64(x0), T64(U[:, 0]), smooth, T64(tab), mutant=mutant),
                           pp.step(T64(x0), T64(U[:, 0]), smooth, T64(tab)))


@pytest.mark.parametrize("smooth", [False, True])
def test_stepwise_oracle_equals_end_to_end_autograd(smooth):
    """With the table as a leaf, S = T = 12, to 1e-9 per parameter column (and per tensor for the rest): open loop, and
    closed loop with a float64 controller on both sides."""
    B, S = 48, 12
    x0, U = pt.open_batch(B, S)
    tab = pt.three_rows_table(B)
    g_x, g_u = pt.cotangents(B, S)
    a, b, row = T64(x0).requires_grad_(True), T64(U).requires_grad_(True), T64(tab).requires_grad_(True)
    X = pp.trajectory(a, b, smooth, row)
    (X * T64(g_x)).sum().backward()
    step = pp.stepwise_param_adjoint(X.detach().numpy(), U, g_x, smooth, tab)
    f = pp.figures(step, {"g_x0": a.grad.numpy(), "g_u": b.grad.numpy(), "g_press": row.grad.numpy()})
    assert all(v <= 1e-9 for v in f.values()), f
    assert np.all(np.abs(row.grad.numpy()).max(0) > 0)    # every one of the 28 columns is driven

    x0, ref = pt.loop_batch(B, S)
    w = pt.ctrl_weights(50, 2.0)
    a, row = T64(x0).requires_grad_(True), T64(tab).requires_grad_(True)
    P_ = [T64(k).requires_grad_(True) for k in w]
    X, Uu = pp.closed_loop(a, T64(ref), *P_, smooth, row)
    ((X * T64(g_x)).sum() + (Uu * T64(g_u)).sum()).backward()
    step = pp.stepwise_param_adjoint(X.detach().numpy(), Uu.detach().numpy(), g_x, smooth, tab, g_u, w, ref, f64=True)
    want = {"g_x0": a.grad.numpy(), "g_w_inp": P_[0].grad.numpy(), "g_b_inp": P_[1].grad.numpy(),
            "g_w_out": P_[2].grad.numpy().reshape(-1), "g_press": row.grad.numpy()}
    f = pp.figures(step, want)
    assert all(v <= 1e-9 for v in f.values()), f


KL_STEP = 1e-3


@pytest.mark.parametrize("smooth", [False, True])
def test_autograd_matches_central_differences(smooth):
    """open_batch(48, 12) under three_rows_table, L_b = sum(g_x[b] * x[b]): autograd's dL_b/dtheta against
    (L_b(theta + h) - L_b(theta - h)) / 2h, h = 1e-6 |theta|, within 1e-5 of the column's maximum over the batch for at
    least 95 % of the trajectories, in every column but KL_1 and KL_2.

    KL_1 and KL_2: g * theta is ~1e-4 against 0.01 .. 24 in the other columns, so at h = 1e-6 |theta| the quotient is
    rounding-limited (measured shares: KL_1 98 % / 96 %, KL_2 71 % / 69 % for forging_model / template_model). The step
    chosen for these two is h = 1e-3 |theta| (KL_STEP): both models give 100 % at 1e-4, 1e-3 and 1e-2, and 98 % at 1e-1,
    where the truncation error shows; 1e-3 is the middle of the range that works. They meet the same 95 %."""
    B, S = 48, 12
    x0, U = pt.open_batch(B, S)
    tab = pt.three_rows_table(B)
    g_x, _ = pt.cotangents(B, S)
    loss = lambda t: (pp.trajectory(T64(x0), T64(U), smooth, t) * T64(g_x)).sum((1, 2))
    row = T64(tab).requires_grad_(True)
    loss(row).sum().backward()
    g = row.grad.numpy()
    assert np.all(np.isfinite(g))
    shares = {}
    for i, name in enumerate(pt.NAMES):
        h = (KL_STEP if name in ("KL_1", "KL_2") else 1e-6) * np.abs(tab[:, i])
        tp, tm = tab.copy(), tab.copy()
        tp[:, i] += h
        tm[:, i] -= h
        with torch.no_grad():
            fd = ((loss(T64(tp)) - loss(T64(tm))).numpy()) / (2 * h)
        shares[name] = float(np.mean(np.abs(fd - g[:, i]) <= 1e-5 * np.abs(g[:, i]).max()))
    print("shares:", shares)
    assert all(s >= 0.95 for s in shares.values()), shares


@functools.lru_cache(maxsize=None)
def _mutant_case():
    """The open loop of the GPU tests' first 48 trajectories under three presses, S = 12, smooth."""
    B, S = 48, 12
    x0, U = pt.open_batch(B, S)
    tab = pt.three_rows_table(B)
    g_x, _ = pt.cotangents(B, S)
    with torch.no_grad():
        x = pp.trajectory(T64(x0), T64(U), True, T64(tab)).numpy()
    run = lambda mutant: pp.stepwise_param_adjoint(x, U, g_x, True, tab, mutant=mutant)
    return run, run(None)


@pytest.mark.parametrize("mutant", pp.MUTANTS)
def test_the_comparison_refuses_every_mutant(mutant):
    """Each deliberate mistake moves some parameter column by at least 1e-3 of its maximum and leaves the state
    gradients alone; the comparison the GPU tests use turns it down, per trajectory and summed for a shared row."""
    run, good = _mutant_case()
    assert not pp.refused(good, good) and not pp.refused(pp.summed(good), pp.summed(good))
    bad = run(mutant)
    f = pp.figures(bad, good)
    assert f["g_press"] >= 1e-3 and f["g_x0"] == 0 and f["g_u"] == 0, f
    assert pp.refused(bad, good)
    assert pp.refused(pp.summed(bad), pp.summed(good))


def test_a_zero_column_must_stay_zero():
    _, good = _mutant_case()
    want = {"g_press": good["g_press"].copy()}
    want["g_press"][:, pp.IX["M0"]] = 0.0
    got = {"g_press": want["g_press"].copy()}
    assert not pp.refused(got, want)
    got["g_press"][3, pp.IX["M0"]] = 1e-30
    assert pp.refused(got, want)


@pytest.mark.parametrize("smooth", [False, True])
def test_inputs_drive_every_branch(smooth):
    """At least 5 % of the (trajectory, step) pairs on either side of y > 0 && yd > 0, of z >= 0 and of the friction
    knee: open_batch(300, 12) under three_rows_table, the GPU tests' open loop."""
    B, S = 300, 12
    x0, U = pt.open_batch(B, S)
    with torch.no_grad():
        x = pp.trajectory(T64(x0), T64(U), smooth, T64(pt.three_rows_table(B))).numpy()
    y, yd, z = x[:, :-1, 0], x[:, :-1, 1], x[:, :-1, 4]
    shares = {"fd": ((y > 0) & (yd > 0)).mean(), "z>=0": (z >= 0).mean(), "knee": (np.abs(yd) <= 0.5).mean()}
    assert all(0.05 <= s <= 0.95 for s in shares.values()), shares


# ------------------------------------------------------------------------------------------------ the entry points

def test_the_new_symbols_are_declared_and_exported():
    lib = N.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcr.h")).read()
    for name in NEW:
        assert name in N.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.fcr_abi_version() == 8


def call_plant(B=4, S=3, ts=1e-3, substeps=4, smooth=0, x=FAKE, u=FAKE, g_x=FAKE, press=FAKE, stride=28, g_x0=FAKE,
               g_u=FAKE, g_press=FAKE):
    lib = N.load()
    rc = lib.fcr_plant_rk4_vjp_press(B, S, ts, substeps, smooth, x, u, g_x, press, stride, g_x0, g_u, g_press, None)
    return rc, lib.fcr_last_error().decode()


PLANT_FAULTS = [
    (dict(B=-1), "B=-1"), (dict(S=-2), "S=-2"), (dict(ts=0.0), "ts=0"), (dict(substeps=0), "substeps=0"),
    (dict(smooth=2), "smooth=2"), (dict(stride=-28), "stride is negative"), (dict(stride=27), "stride_traj=27"),
    (dict(press=FAKE + 4), "parameter table must be 8-byte aligned"), (dict(press=None), "parameter table"),
    (dict(press=None, stride=0), "the parameter table is NULL"), (dict(x=None), "required pointer is NULL"),
    (dict(u=None), "required pointer is NULL"), (dict(g_x=None), "required pointer is NULL"),
    (dict(g_x0=None), "required pointer is NULL"), (dict(g_u=None), "required pointer is NULL"),
    (dict(g_press=None), "required pointer is NULL"), (dict(g_press=FAKE + 4), "8-byte aligned"),
    (dict(x=FAKE + 4), "8-byte aligned"),
]


@pytest.mark.parametrize("kw,word", PLANT_FAULTS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _) in enumerate(PLANT_FAULTS)])
def test_plant_vjp_press_refuses_a_fault_before_any_device_call(kw, word):
    rc, msg = call_plant(**kw)
    assert rc == -1 and msg.startswith("fcr_plant_rk4_vjp_press:") and word in msg, (rc, msg)


def test_plant_vjp_press_empty_batch_is_a_no_op():
    assert call_plant(B=0, x=None, u=None, g_x=None, press=None, stride=0, g_x0=None, g_u=None, g_press=None)[0] == 0


def loop_struct(**kw):
    """A fcr_closed_loop_grad that passes every check (all its pointers FAKE, a table of stride 28), then ``kw``."""
    a = N.FcrClosedLoopGrad()
    a.B, a.T, a.ts, a.substeps, a.smooth, a.ctrl_hidden, a.stride_traj = 4, 3, 1e-3, 4, 1, 50, 28
    a.in_scale[0] = a.in_scale[1] = a.ref_scale = a.out_scale = 1.0
    for name, ctype in N.FcrClosedLoopGrad._fields_:
        if ctype is ctypes.c_void_p:
            setattr(a, name, FAKE)
    for k, v in kw.items():
        if k == "in_scale0":
            a.in_scale[0] = v
        else:
            setattr(a, k, v)
    return a


def call_loop(kw, g_press=FAKE, ws=FAKE, ws_bytes=1 << 30, null=False):
    lib = N.load()
    rc = lib.fcr_closed_loop_vjp_press(None if null else ctypes.byref(loop_struct(**kw)), g_press, ws, ws_bytes, None)
    return rc, lib.fcr_last_error().decode()


LOOP_FAULTS = [
    (dict(B=-1), -1, "B=-1"), (dict(T=-2), -1, "T=-2"), (dict(substeps=0), -1, "substeps=0"), (dict(ts=0.0), -1, "ts=0"),
    (dict(smooth=2), -1, "smooth=2"), (dict(ctrl_hidden=0), -4, "ctrl_hidden=0"), (dict(ctrl_hidden=257), -4, "ctrl_hidden=257"),
    (dict(ref_scale=0.0), -1, "scales must be positive"), (dict(in_scale0=0.0), -1, "scales must be positive"),
    (dict(out_scale=float("nan")), -1, "scales must be positive"), (dict(stride_traj=-28), -1, "stride is negative"),
    (dict(stride_traj=27), -1, "stride_traj=27"), (dict(press=FAKE + 4), -1, "parameter table must be 8-byte aligned"),
    (dict(press=None), -1, "parameter table"), (dict(press=None, stride_traj=0), -1, "the parameter table is NULL"),
    (dict(g_w_inp=None), -1, "parameter gradient is NULL"), (dict(g_b_inp=FAKE + 4), -1, "8-byte aligned"),
    (dict(x=None), -1, "required pointer is NULL"), (dict(g_x=None), -1, "required pointer is NULL"),
    (dict(g_x0=None), -1, "required pointer is NULL"), (dict(ctrl_w_out=None), -1, "required pointer is NULL"),
    (dict(ref=None), -1, "required pointer is NULL"), (dict(u=None), -1, "required pointer is NULL"),
    (dict(g_u=None), -1, "required pointer is NULL"), (dict(dv=None), -1, "required pointer is NULL"),
    (dict(dv=FAKE + 4), -1, "8-byte aligned"),
]


@pytest.mark.parametrize("kw,code,word", LOOP_FAULTS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _, _) in enumerate(LOOP_FAULTS)])
def test_loop_vjp_press_refuses_a_fault_before_any_device_call(kw, code, word):
    rc, msg = call_loop(kw)
    assert rc == code and msg.startswith("fcr_closed_loop_vjp_press:") and word in msg, (rc, msg)


def test_loop_vjp_press_its_own_arguments():
    for kw, code, word in ((dict(g_press=None), -1, "required pointer is NULL"), (dict(g_press=FAKE + 4), -1, "8-byte aligned"),
                           (dict(ws=None), -1, "workspace is NULL"), (dict(ws_bytes=8), -2, "bytes"),
                           (dict(ws=FAKE + 4), -1, "workspace must be 8-byte aligned"), (dict(null=True), -1, "args is NULL")):
        rc, msg = call_loop({}, **kw)
        assert rc == code and msg.startswith("fcr_closed_loop_vjp_press:") and word in msg, (kw, rc, msg)
    empty = dict(B=0, press=None, stride_traj=0, g_w_inp=None, g_b_inp=None, g_w_out=None)   # and nothing to zero
    assert call_loop(empty, g_press=None, ws=None, ws_bytes=0)[0] == 0


def test_press_grad_sum_checks_its_arguments_before_any_device_call():
    lib = N.load()
    size = ctypes.c_size_t(7)
    assert lib.fcr_press_grad_sum_workspace_size(300, ctypes.byref(size)) == 0 and size.value >= 2 * 28 * 8
    assert lib.fcr_press_grad_sum_workspace_size(0, ctypes.byref(size)) == 0 and size.value == 0
    assert lib.fcr_press_grad_sum_workspace_size(-1, ctypes.byref(size)) == -1 and size.value == 0
    assert "fcr_press_grad_sum_workspace_size: B=-1" in lib.fcr_last_error().decode()
    assert lib.fcr_press_grad_sum_workspace_size(300, None) == -1 and "bytes is NULL" in lib.fcr_last_error().decode()
    big = 1 << 20
    for args, code, word in (((-1, FAKE, FAKE, FAKE, big), -1, "B=-1"), ((300, None, FAKE, FAKE, big), -1, "g_press is NULL"),
                             ((300, FAKE, None, FAKE, big), -1, "g_row is NULL"), ((300, FAKE + 4, FAKE, FAKE, big), -1, "8-byte aligned"),
                             ((300, FAKE, FAKE + 4, FAKE, big), -1, "8-byte aligned"), ((300, FAKE, FAKE, None, big), -1, "workspace is NULL"),
                             ((300, FAKE, FAKE, FAKE, 2 * 28 * 8 - 1), -2, "bytes"),
                             ((300, FAKE, FAKE, FAKE + 4, big), -1, "workspace must be 8-byte aligned")):
        rc = lib.fcr_press_grad_sum(*args, None)
        msg = lib.fcr_last_error().decode()
        assert rc == code and msg.startswith("fcr_press_grad_sum:") and word in msg, (args, rc, msg)
    assert lib.fcr_press_grad_sum(0, None, None, None, 0, None) == 0          # empty, nothing to zero


# ------------------------------------------------------------------------------------------------ the Python layer

def test_fit_press_refuses_unknown_fields_and_the_cpu():
    x_obs, u = torch.zeros(2, 4, 5, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="fields"):
        fca.fit_press(x_obs, u, ["CD", "VISCOSITY"])
    with pytest.raises(ValueError, match="fields"):
        fca.fit_press(x_obs, u, [])
    with pytest.raises(RuntimeError, match="ROCm device only"):
        fca.fit_press(x_obs, u, ["CD"])
    assert fca.plant.fit_press is fca.fit_press


def test_a_press_tensor_asking_for_its_gradient_needs_the_device():
    x0, u = torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    row = torch.tensor(fca.PressParams().as_row(), requires_grad=True)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        fca.forging_rk4(x0, u, params=row)
    assert "No gradient reaches ``params``" not in fca.forging_rk4.__doc__
    assert "or ``plant_params``" not in fca.ClosedLoop.run.__doc__


def test_the_fits_yardstick_is_reproduced():
    """L-BFGS on the CPU restatement, B = 16, S = 12, smooth, CD / M0 / KB from 0.85 / 0.9 / 1.1: the recorded per-field
    errors and loss / loss0 (tests/golden/press_fit_cpu.json, tests/golden/make_press_fit_cpu.py) within a factor 3."""
    rec = json.load(open(os.path.join(pt.GOLDEN, pp.FIT_GOLDEN)))
    assert (rec["B"], rec["S"], rec["smooth"], tuple(rec["fields"]), tuple(rec["true"])) == (16, 12, True, pp.FIT_FIELDS, pp.FIT_TRUE)
    x_obs, U = pp.fit_inputs(rec["B"], rec["S"], rec["smooth"])
    r = pp.fit_cpu(x_obs, U)
    errors, ratio = pp.fit_errors(r["multipliers"]), r["loss"] / r["loss0"]
    print("errors:", errors, "recorded:", rec["errors"], "loss/loss0:", ratio, "recorded:", rec["loss_ratio"])
    for name, e, e0 in zip(pp.FIT_FIELDS, errors, rec["errors"]):
        assert e0 / 3 <= e <= 3 * e0, (name, e, e0)
    assert rec["loss_ratio"] / 3 <= ratio <= 3 * rec["loss_ratio"], (ratio, rec["loss_ratio"])
    assert abs(r["loss0"] / rec["loss0"] - 1) <= 1e-9
