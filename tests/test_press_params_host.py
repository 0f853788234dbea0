"""CPU: the press as data — PressParams against the oracle's constants and fcr_press_nominal, the oracle's patch helper,
the sampler, every refusal of the three *_press entry points (each returned before any launch), and the sensitivity
table that gives tests/test_gpu_press_params.py its teeth."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import oracle.plant_np as plant_np
import press_np
from conftest import ROOT
from oracle.closed_loop_np import closed_loop
from test_closed_loop import SCALERS, ctrl_weights
from test_gpu_feasibility import press_case

N = fca._native
P = fca.PressParams
SCALE_ARGS = (SCALERS["input"][:2], SCALERS["y_dot"], SCALERS["output"])
FAKE = 4096                                # a non-NULL, aligned address no refused call ever reads


def nominal_struct():
    s = N.FcrPress()
    N.load().fcr_press_nominal(ctypes.byref(s))
    return s


def small_loop():
    x0, ref = press_case()
    return x0[:50], ref[:50, :40]


def test_defaults_are_the_oracles_constants_and_the_librarys():
    assert P.NAMES == press_np.NAMES and len(P.NAMES) == 28
    s = nominal_struct()
    assert [n for n, _ in N.FcrPress._fields_] == [n.lower() for n in P.NAMES]
    for n in P.NAMES:
        assert getattr(P(), n) == float(getattr(plant_np, n)) == getattr(s, n.lower()), n
    assert np.array_equal(P().as_row(), press_np.oracle_row())
    assert ctypes.sizeof(N.FcrPress) == 28 * 8


def test_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "fcr.h")).read()
    body = re.search(r"typedef struct fcr_press \{(.*?)\} fcr_press;", text, re.S).group(1)
    names = [w.strip() for w in body.replace("double", "").replace(";", "").split(",")]
    assert names == [n for n, _ in N.FcrPress._fields_]
    assert N.ABI_VERSION == 8
    for name in ("fcr_press_nominal", "fcr_plant_rk4_press", "fcr_feasibility_project_press", "fcr_closed_loop_run_bank_press"):
        assert name in N.EXPORTS and hasattr(N.load(), name)


def test_replace_row_table_and_validate():
    p = P().replace(PS=30e6, T_DEF=800.0)
    assert p.PS == 30e6 and p.T_DEF == 800.0 and p.KB == P().KB and P().PS == 32e6
    with pytest.raises(Exception):
        p.PS = 1.0                                                           # frozen
    row = p.as_row()
    assert row.dtype == np.float64 and row.shape == (28,) and row[P.NAMES.index("PS")] == 30e6
    tab = p.table(7)
    assert tab.shape == (7, 28) and tab.dtype == torch.float64 and np.array_equal(tab.numpy(), np.tile(row, (7, 1)))
    assert P.validate(tab) and P.validate(tab.reshape(1, 7, 28))
    for name in P.POSITIVE:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            t = tab.clone()
            t[3, P.NAMES.index(name)] = bad
            assert not P.validate(t), (name, bad)
    t = tab.clone()
    t[0, P.NAMES.index("M1")] = float("nan")
    assert not P.validate(t)
    t = tab.clone()
    t[0, P.NAMES.index("M1")] = -5.0                                         # a sign the equations do not care about
    assert P.validate(t)
    with pytest.raises(ValueError):
        P.validate(torch.zeros(3, 27))
    with pytest.raises(ValueError):
        fca.FeasibilityRecovery(model_params=np.zeros(27))
    assert fca.FeasibilityRecovery(model_params=row).model_params == p


def test_patched_nominal_is_the_unpatched_oracle():
    x0, ref = small_loop()
    base = closed_loop(x0, ref, *ctrl_weights(), *SCALE_ARGS, smooth=False)
    with press_np.patched(press_np.oracle_row()):
        same = closed_loop(x0, ref, *ctrl_weights(), *SCALE_ARGS, smooth=False)
    assert all(np.array_equal(a, b) for a, b in zip(base, same))
    moved = press_np.oracle_row()
    moved[P.NAMES.index("D1")] *= 1.1
    with press_np.patched(moved):
        assert plant_np.A1 == np.pi * 0.66 ** 2 / 4 or abs(plant_np.A1 - np.pi * 0.66 ** 2 / 4) < 1e-15
        with press_np.patched(press_np.oracle_row()):                        # patches nest
            assert plant_np.D1 == 0.6 and plant_np.A1 == np.pi * 0.6 ** 2 / 4
        assert plant_np.D1 == moved[P.NAMES.index("D1")]
    assert plant_np.D1 == 0.6 and plant_np.A1 == np.pi * 0.6 ** 2 / 4
    # a table of two sets is the two runs, row by row
    table = np.tile(press_np.oracle_row(), (50, 1))
    table[1::2] = moved
    x, u = press_np.closed_loop_press(table, x0, ref, *ctrl_weights(), *SCALE_ARGS, smooth=False)
    assert np.array_equal(x[0::2], base[0][0::2]) and not np.array_equal(x[1::2], base[0][1::2])


def test_sample_is_deterministic_and_moves_only_the_named_fields():
    rel = {"PS": 0.1, "KB": 0.2, "T_DEF": 0.05}
    a = P().sample(40, rel, rng=np.random.RandomState(3))
    b = P().sample(40, dict(reversed(list(rel.items()))), rng=np.random.RandomState(3))   # the order of `rel` is nothing
    assert a.shape == (40, 28) and a.dtype == torch.float64 and torch.equal(a, b)
    a = a.numpy()
    nom = P().as_row()
    for i, n in enumerate(P.NAMES):
        if n in rel:
            assert np.all(np.abs(a[:, i] / nom[i] - 1) <= rel[n]) and np.ptp(a[:, i]) > 0, n
        else:
            assert np.all(a[:, i] == nom[i]), n
    # the documented draw order: the named fields in the order of NAMES, one call of n draws each
    rng = np.random.RandomState(3)
    for n in ("KB", "PS", "T_DEF"):
        i = P.NAMES.index(n)
        assert np.array_equal(a[:, i], nom[i] * (1.0 + rel[n] * rng.uniform(-1.0, 1.0, 40))), n
    g = P().replace(PS=30e6).sample(1000, {"PS": 0.01}, dist="normal", rng=np.random.RandomState(5)).numpy()
    ps = g[:, P.NAMES.index("PS")]
    assert abs(ps.mean() / 30e6 - 1) < 2e-3 and 0.008 < ps.std() / 30e6 < 0.012
    assert np.array_equal(ps, 30e6 * (1.0 + 0.01 * np.random.RandomState(5).standard_normal(1000)))
    with pytest.raises(ValueError, match="unknown"):
        P().sample(3, {"ps": 0.1})
    with pytest.raises(ValueError, match="dist"):
        P().sample(3, {"PS": 0.1}, dist="cauchy")
    assert torch.equal(P().sample(5, {"PS": 0.1}), P().sample(5, {"PS": 0.1}))          # the default generator is seeded


# ---------------------------------------------------------------------------------------------
# refusals, each before any launch (no GPU here: a launch would fail differently)
# ---------------------------------------------------------------------------------------------
def refused(rc, *words):
    msg = N.load().fcr_last_error().decode()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def bank_args(B=4, T=3, M=2):
    a = N.FcrClosedLoopBank()
    a.B, a.T, a.ts, a.substeps, a.ctrl_hidden, a.n_models = B, T, 1e-3, 4, 50, M
    a.in_scale[0] = a.in_scale[1] = a.ref_scale = a.out_scale = 1.0
    a.p1_hi = a.p2_hi = 32e6
    return a


TABLE_CASES = [((None, 0, 28), ("NULL",)), ((FAKE, -28, 28), ("negative",)), ((FAKE, 0, -28), ("negative",)),
               ((FAKE, 0, 27), ("stride_traj", "multiple of 28")), ((FAKE, 0, 8), ("stride_traj",)),
               ((FAKE, 100, 28), ("stride_model", "multiple of 28")), ((FAKE, 84, 28), ("stride_model", "B * stride_traj")),
               ((FAKE + 4, 112, 28), ("aligned",))]


@pytest.mark.parametrize("table,words", TABLE_CASES)
def test_bank_refuses_a_bad_table(table, words):
    lib = N.load()
    a = bank_args()
    refused(lib.fcr_closed_loop_run_bank_press(ctypes.byref(a), table[0], table[1], table[2], None, None), *words)


def test_bank_accepts_every_documented_layout_up_to_the_next_check():
    """(28,), (B,28), (M,B,28) and a per-model shared row pass the table's checks: the call is then refused for its NULL
    buffers, as fcr_closed_loop_run_bank is."""
    lib = N.load()
    a = bank_args()
    for sm, st in ((0, 0), (0, 28), (4 * 28, 28), (28, 0), (8 * 28, 56)):
        refused(lib.fcr_closed_loop_run_bank_press(ctypes.byref(a), FAKE, sm, st, None, None), "required pointer is NULL")
    assert lib.fcr_closed_loop_run_bank_press(None, FAKE, 0, 0, None, None) == -1
    empty = bank_args(B=0)
    assert lib.fcr_closed_loop_run_bank_press(ctypes.byref(empty), FAKE, 0, 0, None, None) == 0      # B = 0: a no-op
    assert lib.fcr_closed_loop_run_bank_press(ctypes.byref(empty), None, 0, 28, None, None) == 0     # an empty table too
    refused(lib.fcr_closed_loop_run_bank_press(ctypes.byref(empty), None, 0, 27, None, None), "stride_traj")


@pytest.mark.parametrize("stride,table,words", [(28, None, ("NULL",)), (-28, FAKE, ("negative",)), (29, FAKE, ("multiple of 28",)),
                                                (28, FAKE + 2, ("aligned",))])
def test_plant_refuses_a_bad_table(stride, table, words):
    refused(N.load().fcr_plant_rk4_press(4, 3, 1e-3, 4, 0, None, None, None, table, stride, None), *words)


def test_plant_checks_its_other_arguments_as_fcr_plant_rk4_does():
    lib = N.load()
    for args, word in (((-1, 3, 1e-3, 4, 0), "B="), ((4, 3, 0.0, 4, 0), "ts="), ((4, 3, 1e-3, 0, 0), "substeps="),
                       ((4, 3, 1e-3, 4, 2), "smooth="), ((4, 3, 1e-3, 4, 0), "required pointer is NULL")):
        refused(lib.fcr_plant_rk4_press(*args, None, None, None, FAKE, 28, None), word)
    assert lib.fcr_plant_rk4_press(0, 5, 1e-3, 4, 0, None, None, None, FAKE, 0, None) == 0
    assert lib.fcr_plant_rk4_press(0, 5, 1e-3, 4, 0, None, None, None, None, 28, None) == 0         # an empty (0,28) table


@pytest.mark.parametrize("field", [n.lower() for n in P.POSITIVE])
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")], ids=["zero", "negative", "nan", "inf"])
def test_a_bad_model_field_is_refused(field, bad):
    lib = N.load()
    model = nominal_struct()
    setattr(model, field, bad)
    a = bank_args()
    refused(lib.fcr_closed_loop_run_bank_press(ctypes.byref(a), FAKE, 0, 28, ctypes.byref(model), None), "model field", field)
    f = fca.FeasibilityRecovery().struct()
    refused(lib.fcr_feasibility_project_press(ctypes.byref(f), ctypes.byref(model), 4, None, None, None, None, None, None),
            "model field", field)


def test_project_press_checks_like_project():
    lib = N.load()
    f = fca.FeasibilityRecovery().struct()
    model = nominal_struct()
    refused(lib.fcr_feasibility_project_press(ctypes.byref(f), ctypes.byref(model), 4, None, None, None, None, None, None),
            "required pointer is NULL")
    refused(lib.fcr_feasibility_project_press(ctypes.byref(f), None, 4, None, None, None, None, None, None),
            "required pointer is NULL")                                       # NULL model: the nominal one
    model.m2 = float("nan")                                                   # any field must be finite
    refused(lib.fcr_feasibility_project_press(ctypes.byref(f), ctypes.byref(model), 4, None, None, None, None, None, None),
            "m2", "finite")
    assert lib.fcr_feasibility_project_press(ctypes.byref(f), None, 0, None, None, None, None, None, None) == 0
    refused(lib.fcr_feasibility_project_press(None, None, 4, None, None, None, None, None, None), "NULL")


def test_python_refuses_cpu_tensors_and_bad_shapes():
    x0, u = torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        fca.forging_rk4(x0, u, params=P())
    cl = fca.ClosedLoop(fca.FNNModel(3, 50, 1, 1), SCALERS)
    with pytest.raises(ValueError, match="plant_params"):
        cl.run(x0, u, plant_params=np.zeros((3, 28)))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        cl.run(x0, u, plant_params=P())


# ---------------------------------------------------------------------------------------------
# the sensitivity table
# ---------------------------------------------------------------------------------------------
def test_every_field_moves_the_oracle_at_its_factor():
    """The sensitivity table: FACTORS (tests/press_np.py) is the asserted part — every field's factor, and which four are
    raised; the figures below are the measurements behind it. The plain non-smooth loop of press_case() (B = 50, T = 40)
    under one field scaled at a time, as the largest |x - x_nominal| over the largest |x_nominal| of a state — the
    normalisation of this family's 1e-5 bars, NOT a state's max - min range, so the figures differ from a table made with
    the range (PT x1.1 is 1.5e-3 here; normalised by the range it was measured at 5.4e-4, hence its x2: it passes under either). Measured at x1.1: D2 0.36, D1 0.32, T_DEF 0.13, M1 0.13,
    CD 0.13, D 0.13, B0 0.12, PS 0.093, H0 0.090, M4 0.087, K = M0 = W0 0.066, RHO 0.060, KB 0.057, MU 0.052,
    M_MASS 0.048, T1 0.041, V2_0 0.036, V1_0 0.035, G 0.024, M2 0.019, M3 0.010, FT 1.8e-3, PT 1.5e-3; below 1e-3 at
    x1.1 and therefore raised: B_DAMP (x3), KL_1 (x5), KL_2 (x16); PT is raised to x2 for margin. Every set keeps the
    oracle finite and away from the friction law's sign flip at y_dot = -0.5."""
    assert set(press_np.FACTORS) == set(P.NAMES)
    assert {n for n, f in press_np.FACTORS.items() if f != 1.1} == {"B_DAMP", "KL_1", "KL_2", "PT"}
    x0, ref = small_loop()
    xn, _ = closed_loop(x0, ref, *ctrl_weights(), *SCALE_ARGS, smooth=False)
    scale = np.abs(xn).reshape(-1, 5).max(0)
    rows = press_np.one_field_rows()
    assert np.array_equal(rows[0], press_np.oracle_row())
    for i, n in enumerate(P.NAMES):
        assert np.flatnonzero(rows[i + 1] != rows[0]).tolist() == [i]
        with press_np.patched(rows[i + 1]):
            x, _ = closed_loop(x0, ref, *ctrl_weights(), *SCALE_ARGS, smooth=False)
        moved = (np.abs(x - xn).reshape(-1, 5) / scale).max()
        print(f"{n} x{press_np.FACTORS[n]}: moved {moved:.3g}")
        assert np.isfinite(x).all() and x[:, :, 1].min() > -0.5, n
        assert moved >= press_np.MOVE_MIN, (n, moved)
