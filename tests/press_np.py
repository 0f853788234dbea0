"""The fp64 oracle under other press parameters (TEST INFRASTRUCTURE ONLY).

``oracle/plant_np.py`` reads its constants as module globals at call time, so a row of 28 parameters is applied by
patching them — the 28 and the three the module derives from them (``A1``, ``A2``, ``A_SPREAD``, each with the module's
own expression) — for the length of a ``with`` block. Patches nest: the recovering loop's ``project`` callback re-patches
the MODEL's set around the projection while the loop's plant step runs under the PLANT's set. A per-trajectory table is
checked by grouping its rows into sets and calling the oracle once per set (:func:`by_set`).
"""
from __future__ import annotations

import contextlib
from unittest import mock

import numpy as np

import oracle.plant_np as plant_np
from feasibility_np import project
from oracle.closed_loop_np import closed_loop

NAMES = ("M_MASS", "B_DAMP", "FT", "D1", "D2", "G", "KB", "V1_0", "V2_0", "KL_1", "KL_2", "CD", "RHO", "D", "PS", "PT",
         "MU", "K", "W0", "H0", "B0", "T_DEF", "T1", "M0", "M1", "M2", "M3", "M4")


_ORACLE_ROW = np.array([float(getattr(plant_np, n)) for n in NAMES])   # read at import: no patch is active


def oracle_row() -> np.ndarray:
    """The oracle's own (unpatched) constants as a row."""
    return _ORACLE_ROW.copy()


def patched(row):
    """Context manager: ``oracle.plant_np`` computes with the press of ``row`` (28 values in the order of NAMES)."""
    row = np.asarray(row, np.float64)
    assert row.shape == (len(NAMES),), row.shape
    v = dict(zip(NAMES, (float(a) for a in row)))
    v["A1"] = np.pi * v["D1"] ** 2 / 4
    v["A2"] = np.pi * v["D2"] ** 2 / 4
    v["A_SPREAD"] = 0.14 + 0.36 * (v["B0"] / v["W0"]) - 0.054 * (v["B0"] / v["W0"]) ** 2
    return mock.patch.multiple(plant_np, **v)


def by_set(table):
    """[(row, indices)] of the distinct rows of ``table (B,28)``, in order of first appearance."""
    table = np.asarray(table, np.float64)
    rows, inverse = np.unique(table, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = sorted(range(len(rows)), key=lambda k: np.flatnonzero(inverse == k)[0])
    return [(rows[k], np.flatnonzero(inverse == k)) for k in order]


def trajectory(table, x0, U, ts=1e-3, substeps=4, smooth=False):
    """``oracle.plant_np.trajectory`` where trajectory b integrates the press of ``table[b]``."""
    out = np.empty((x0.shape[0], U.shape[1] + 1, 5))
    for row, idx in by_set(table):
        with patched(row):
            out[idx] = plant_np.trajectory(x0[idx], U[idx], ts, substeps, smooth)
    return out


def closed_loop_press(table, x0, ref, W_inp, b_inp, W_out, in_scale, ref_scale, out_scale, ts=1e-3, substeps=4, smooth=True,
                      process_noise=None, meas_noise=None, feas=None, model_row=None):
    """The batched loop where trajectory b's press is ``table[b]``; with ``feas`` (a dict of feasibility_np.project's
    parameters, possibly empty) every step projects the command with the MODEL ``model_row`` (default: the oracle's own
    constants) — the nested patch. Returns ``closed_loop``'s tuple: (x, u) or (x, u, u_nn, flag)."""
    model_row = oracle_row() if model_row is None else np.asarray(model_row, np.float64)
    B, T = ref.shape
    sel = lambda a, idx: None if a is None else a[idx]
    outs = None
    for row, idx in by_set(table):
        proj = None
        if feas is not None:
            def proj(m, x, u_nn):
                with patched(model_row):                      # inside the plant's patch: the model's own press
                    return project(m, u_nn, **feas)[:2]
        with contextlib.ExitStack() as stack:
            stack.enter_context(patched(row))
            with np.errstate(all="ignore"):
                r = closed_loop(x0[idx], ref[idx], W_inp, b_inp, W_out, in_scale, ref_scale, out_scale, ts, substeps, smooth,
                                sel(process_noise, idx), sel(meas_noise, idx), project=proj)
        if outs is None:
            outs = [np.empty((B,) + a.shape[1:], a.dtype) for a in r]
        for dst, a in zip(outs, r):
            dst[idx] = a
    return tuple(outs)


# The factor by which each field is scaled where a test moves one field at a time: x1.1, except the four fields whose
# x1.1 moves the plain non-smooth loop of press_case() (B = 50, T = 40) by less than 1e-3 of every state's largest
# magnitude. tests/test_press_params_host.py asserts that every factor here moves that loop by at least 1e-3.
FACTORS = {n: 1.1 for n in NAMES}
FACTORS.update(B_DAMP=3.0, KL_1=5.0, KL_2=16.0, PT=2.0)
MOVE_MIN = 1e-3


def one_field_rows():
    """(29, 28): the oracle's own row, then one row per field with that field times its factor."""
    rows = np.tile(oracle_row(), (len(NAMES) + 1, 1))
    for i, n in enumerate(NAMES):
        rows[i + 1, i] *= FACTORS[n]
    return rows
