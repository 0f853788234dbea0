"""CPU: the feasibility projection's fixture and restatement (tests/feasibility_np.py), and the host side of its
entry points (argument checks of the C ABI and of the Python wrappers; no kernel runs here)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
from conftest import GOLDEN
from feasibility_np import violation
from tests.golden.make_feasibility_cases import classes

U_LO, U_HI = -0.2, 0.2


@pytest.fixture(scope="module")
def cases():
    return dict(np.load(os.path.join(GOLDEN, "feasibility_cases.npz")))


def test_fixture_holds_every_class(cases):
    n = cases["x"].shape[0]
    assert n % 64 and 200 <= n <= 1000
    counts = {k: int(m.sum()) for k, m in classes(cases["u_nn"], cases["u"], cases["flag"]).items()}
    print(counts)
    assert set(counts) == {"flag0_inside", "flag0_outside", "flag1_up", "flag1_down", "flag2"}
    assert all(c >= 20 for c in counts.values()), counts
    assert sum(counts.values()) == n
    # no flag of the fixture hangs on rounding: kernel and restatement may differ only where |v(u_nn)| <= 1e-9
    assert not np.isnan(cases["v_nn"]).any() and np.abs(cases["v_nn"]).min() > 1e-9
    assert np.array_equal(cases["v_nn"], violation(cases["x"], cases["u_nn"]))


def test_restatement_properties_on_the_fixture(cases):
    x, u_nn, u, flag = cases["x"], cases["u_nn"], cases["u"], cases["flag"]
    f0, f1, f2 = flag == 0, flag == 1, flag == 2
    assert np.array_equal(u[f0], u_nn[f0]) and np.all(cases["v_nn"][f0] <= 0)
    assert np.all(cases["v_nn"][~f0] > 0)
    # flag 1: u is feasible and a step of 1e-9 towards u_nn (above the final bracket 0.2 / 2^30 = 1.9e-10) is not
    assert np.all(violation(x[f1], u[f1]) <= 0)
    assert np.all(violation(x[f1], u[f1] + np.sign(u_nn[f1] - u[f1]) * 1e-9) > 0)
    assert np.all(np.abs(u[f1] - u_nn[f1]) > 0)
    assert np.array_equal(u[f2], np.clip(u_nn[f2], U_LO, U_HI))
    assert np.array_equal(cases["v"], violation(x, u))


def feas_struct(**kw):
    f = fca.FeasibilityRecovery().struct()
    for k, v in kw.items():
        setattr(f, k, v)
    return f


BAD = [(dict(p1_lo=32e6), "p1 bounds"), (dict(p2_lo=1.0, p2_hi=1.0), "p2 bounds"), (dict(u_lo=0.2), "u_lo"),
       (dict(u_hi=float("nan")), "u_lo"), (dict(expand=0), "expand"), (dict(expand=21), "expand"),
       (dict(bisect=0), "bisect"), (dict(bisect=61), "bisect"), (dict(substeps=0), "substeps"), (dict(ts=0.0), "ts=")]


@pytest.mark.parametrize("kw,word", BAD)
def test_project_abi_rejects_bad_parameters(kw, word):
    lib = fca._native.load()
    f = feas_struct(**kw)
    assert lib.fcr_feasibility_project(ctypes.byref(f), 4, 64, 64, 64, 64, None, None) == -1
    msg = lib.fcr_last_error().decode()
    assert msg.startswith("fcr_feasibility_project") and word in msg, msg


def test_project_abi_rejects_bad_buffers():
    lib = fca._native.load()
    f = feas_struct()
    assert lib.fcr_feasibility_project(None, 4, 64, 64, 64, 64, None, None) == -1
    assert "NULL" in lib.fcr_last_error().decode()
    assert lib.fcr_feasibility_project(ctypes.byref(f), -1, 64, 64, 64, 64, None, None) == -1
    assert "B=-1" in lib.fcr_last_error().decode()
    for args in ((None, 64, 64, 64), (64, None, 64, 64), (64, 64, None, 64), (64, 64, 64, None)):   # v alone may be NULL
        assert lib.fcr_feasibility_project(ctypes.byref(f), 4, *args, None, None) == -1
        assert "NULL" in lib.fcr_last_error().decode()
    assert lib.fcr_feasibility_project(ctypes.byref(f), 4, 64, 64, 64, 64, 12, None) == -1
    assert "aligned" in lib.fcr_last_error().decode()
    assert lib.fcr_feasibility_project(ctypes.byref(f), 0, None, None, None, None, None, None) == 0   # empty: no launch


def loop_struct():
    a = fca._native.FcrClosedLoop()
    a.B, a.T, a.ts, a.substeps, a.ctrl_hidden = 4, 3, 1e-3, 4, 50
    a.in_scale[0] = a.in_scale[1] = a.ref_scale = a.out_scale = 1.0
    a.x0 = a.ref = a.x = a.u = a.ctrl_w_inp = a.ctrl_b_inp = a.ctrl_w_out = 64
    return a


def test_closed_loop_zeroed_struct_still_means_no_recovery():
    a = fca._native.FcrClosedLoop()
    assert not a.feasibility and a.u_nn is None and a.feas_flag is None
    assert fca._native.ABI_VERSION == 8 and "fcr_feasibility_project" in fca._native.EXPORTS


@pytest.mark.parametrize("kw,word", BAD)
def test_closed_loop_abi_rejects_bad_recovery_parameters(kw, word):
    lib = fca._native.load()
    a, f = loop_struct(), feas_struct(**kw)
    a.feasibility = ctypes.pointer(f)
    a.u_nn = a.feas_flag = 64
    assert lib.fcr_closed_loop_run(ctypes.byref(a), None) == -1
    msg = lib.fcr_last_error().decode()
    assert msg.startswith("fcr_closed_loop_run") and word in msg, msg


def test_closed_loop_abi_needs_the_recovery_outputs():
    lib = fca._native.load()
    a, f = loop_struct(), feas_struct()
    a.feasibility = ctypes.pointer(f)
    for u_nn, flag in ((None, 64), (64, None)):
        a.u_nn, a.feas_flag = u_nn, flag
        assert lib.fcr_closed_loop_run(ctypes.byref(a), None) == -1
        msg = lib.fcr_last_error().decode()
        assert "NULL" in msg and "feasibility" in msg, msg
    a.u_nn, a.feas_flag = 12, 64
    assert lib.fcr_closed_loop_run(ctypes.byref(a), None) == -1 and "aligned" in lib.fcr_last_error().decode()


def test_python_entry_points_refuse_cpu_tensors():
    fr = fca.FeasibilityRecovery()
    assert fca.closed_loop.FeasibilityRecovery is fr.__class__
    with pytest.raises(RuntimeError, match="ROCm device only"):
        fr.project(torch.zeros(3, 5, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    cl = fca.ClosedLoop(fca.FNNModel(3, 50, 1, 1), {"input": np.ones(3), "y_dot": 1.0, "output": 1.0})
    with pytest.raises(RuntimeError, match="ROCm device only"):
        cl.run(torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64), feasibility=fr)
    f = fca.FeasibilityRecovery(p1=(1e6, 30e6), u_bounds=(-0.1, 0.3), ts=2e-3, substeps=2, expand=8, bisect=20).struct()
    assert (f.p1_lo, f.p1_hi, f.p2_lo, f.p2_hi, f.u_lo, f.u_hi) == (1e6, 30e6, 0.0, 32e6, -0.1, 0.3)
    assert (f.ts, f.substeps, f.expand, f.bisect) == (2e-3, 2, 8, 20)
