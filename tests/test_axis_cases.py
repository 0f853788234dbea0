"""CPU: the axis cases (tests/axis_cases.py) would show a defect on the axis each varies.

For every case: the two fp64 restatements agree to 1e-10 (make_golden.py's bar); the in-loss controller's units are
neither all dead nor all alive; no trajectory lies within an fp32 rounding of a kink; and three mutants of the fp64
oracle — alpha compiled in as 20, the last controller unit ignored, the noise dropped — each move the loss or a gradient
by at least 1e-3, a hundred times the 1e-5 the kernels are held to on the same cases (tests/test_gpu_axes.py). The
comparison that test applies to the GPU's outputs (axis_cases.failures) is fed each mutant's outputs here and must
refuse them.
"""
import numpy as np
import pytest
import torch

import axis_cases as A
from oracle import rollout_torch as T
from test_gpu_parity import TOL
from test_gpu_precision import TOL_FEATS, TOL_GRADS, TOL_LOSS

MOVED = 1e-3                     # test_kink_cases.MOVED
ACTIVE = (0.25, 0.75)            # share of (in-loss evaluation, unit) pairs with z > 0
EVERY = [(n, None) for n in A.CASES] + [(n, m) for n, b in A.BANKS.items() for m in range(b["M"])]
IDS = [n if m is None else f"{n}-model{m}" for n, m in EVERY]


def get(name, m):
    return A.build(name) if m is None else A.build_bank(name)["models"][m]


@pytest.mark.parametrize("name,m", EVERY, ids=IDS)
def test_case_conditions(name, m):
    c = get(name, m)
    nz = None if c["noise"] is None else c["noise"].astype(np.float64)
    t64 = T.loss_and_grads(c["params"], c["X"], c["u0"], c["states"], c["N"], c["alpha"], nz, dtype=torch.float64)
    worst = max(A.relerr(t64[k], c["ref"][k]) for k in A.FEATS + A.GRADS)
    share = float((c["z"] > 0).mean()) if c["z"].size else None
    print(f"{c['name']}: fp64 restatements {worst:.2e}, z > 0 in {share}, kink margin {c['margin']:.2e} "
          f"({c['passed_over']} replaced), per-unit fp32 restatement "
          + " ".join(f"{k}={v:.2e}" for k, v in c["unit32"].items()) + f", bound {c['unit_bound']:.3g}")
    assert worst <= 1e-10, worst
    assert abs(float(t64["loss_scalar"]) - c["ref"]["loss_scalar"]) <= 1e-10 * abs(c["ref"]["loss_scalar"])
    assert c["margin"] > A.BAND, c["margin"]
    assert len(c["X"]) == spec_of(name)["B"] and c["passed_over"] <= A.spare(len(c["X"]))
    assert c["params"]["W_inp"].shape == (c["w"], 3) and c["ref"]["g_W_out"].shape == (1, c["w"])
    for k in ("X", "u0", "states", "noise"):
        assert c[k] is None or c[k].dtype == np.float32, k
    for k in A.CTRL:
        assert np.array_equal(c["params"][k], c["params"][k].astype(np.float32)), k
    if c["N"] > 1:
        assert c["z"].shape == (c["N"] - 1, len(c["X"]), c["w"])
        live = np.delete(c["z"], c["dead"], axis=2) if c["dead"] is not None else c["z"]
        assert ACTIVE[0] <= float((live > 0).mean()) <= ACTIVE[1], share
    else:
        assert all(not np.any(c["ref"][k]) for k in A.UNIT_GRADS)      # no in-loss call: zero controller gradients
    if c["dead"] is not None:
        assert c["z"][:, :, c["dead"]].max() <= -1e-4
        assert all(A.per_unit(c["ref"][k], c["ref"][k]) == 0.0 for k in A.UNIT_GRADS)
        assert not np.any(c["ref"]["g_W_inp"][c["dead"]]) and c["ref"]["g_W_out"][0, c["dead"]] == 0.0
    if c["alpha"] == 0.0:
        assert not np.any(c["ref"]["command"])


def test_tables_hold_what_they_promise():
    """The shapes stay tiny, every kernel family is reached on every axis, and the drop-in's default is what runs."""
    import forging_control_amd as fca
    assert fca.MPCLoss(prediction_horizon=3).alpha == A.ALPHA_DEFAULT
    for name, s in A.CASES.items():
        assert s["B"] <= 140 and s["N"] <= 12 and s["H"] <= 128 and 1 <= s["w"] <= 52, name
        assert ("wide" in s["families"]) == (s["H"] > 52) == (s["families"] == ("wide",)), name
    fams = lambda kind: {f for s in A.CASES.values() if s["kind"] == kind for f in s["families"]}
    assert fams("width") == {"pipe", "onewg", "small", "fused", A.F16, "wide"}
    assert fams("alpha") == {"pipe", "onewg", "fused", A.F16, "wide"} and fams("noise") == {"wide"}
    assert {s["w"] for s in A.CASES.values() if s["kind"] == "width" and s["H"] == 50} == {1, 3, 4, 5, 49, 51, 52}
    assert [s["kind"] for s in A.CASES.values()].count("crossed") == 3
    assert sum(s["dead"] is not None for s in A.CASES.values()) == 1


# ---------------------------------------------------------------------------------------------
# mutants: the fp64 oracle with one axis compiled in
# ---------------------------------------------------------------------------------------------
def _alpha_20(c):
    return A.oracle(c["params"], c["X"], c["u0"], c["states"], c["N"], A.ALPHA, c["noise"])[0]


def _no_noise(c):
    return A.oracle(c["params"], c["X"], c["u0"], c["states"], c["N"], c["alpha"], None)[0]


def _last_unit_ignored(c):
    """The rollout with unit w - 1 sliced off the controller inside the loss; its gradients zero-padded to the caller's
    shapes. u0 is data (the caller's controller computed it), so the defect acts inside the loss only."""
    p = dict(c["params"])
    p["W_inp"], p["b_inp"], p["W_out"] = p["W_inp"][:-1], p["b_inp"][:-1], p["W_out"][:, :-1]
    o = A.oracle(p, c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"])[0]
    o["g_W_inp"] = np.concatenate([o["g_W_inp"], np.zeros((1, 3))], axis=0)
    o["g_b_inp"] = np.concatenate([o["g_b_inp"], np.zeros(1)])
    o["g_W_out"] = np.concatenate([o["g_W_out"], np.zeros((1, 1))], axis=1)
    return o


MUTANTS = {"alpha:=20": _alpha_20, "last unit ignored": _last_unit_ignored, "noise dropped": _no_noise}


def spec_of(name):
    return A.CASES[name] if name in A.CASES else {**A.BANKS[name], "kind": "width", "noise": False, "dead": None}


def applies(mutant, s):
    """Whether ``mutant`` applies to a case with spec ``s``."""
    if mutant == "alpha:=20":
        return s["kind"] in ("alpha", "crossed")
    if mutant == "noise dropped":
        return s["noise"]
    # the last unit: the cases that vary the width, where there is a unit to lose and it is not the dead one
    return s["kind"] in ("width", "crossed") and s["w"] > 1 and s["dead"] != s["w"] - 1


APPLIED = [(n, m, k) for n, m in EVERY for k in MUTANTS if applies(k, spec_of(n))]


def test_every_case_has_a_mutant_but_n1():
    none = [i for (n, m), i in zip(EVERY, IDS) if not any(applies(k, spec_of(n)) for k in MUTANTS)]
    assert none == ["h50_w1_b20_n3", "h64_w1_b24_n3", "h50_w7_b20_n1"] + [f"h50_bank3_w1-model{m}" for m in range(3)]


def test_single_unit_controllers_are_felt():
    """Width 1 has no last unit to lose beside another: there the mutant is the controller ignored altogether (the
    in-loss command 0), which must move the loss or a gradient by MOVED as well."""
    for c in (get(n, m) for n, m in EVERY):
        if c["w"] != 1:
            continue
        p = {**c["params"], "W_out": np.zeros((1, 1))}
        o = A.oracle(p, c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"])[0]
        moved = max(A.errors(c, o)[0].values())
        print(c["name"], f"controller ignored: {moved:.3g}")
        assert moved >= MOVED, (c["name"], moved)
        assert A.failures(c, o, TOL) and A.failures(c, o, TOL, (TOL_LOSS, TOL_FEATS, TOL_GRADS))


@pytest.mark.parametrize("name,m,mutant", APPLIED,
                         ids=[f"{n if m is None else f'{n}-model{m}'}-{k.replace(' ', '_')}" for n, m, k in APPLIED])
def test_mutant_moves_the_outputs_and_is_refused(name, m, mutant):
    c = get(name, m)
    o = MUTANTS[mutant](c)
    wide, unit = A.errors(c, o)
    moved = max(wide[k] for k in ("loss_scalar",) + A.GRADS)
    print(f"{c['name']} {mutant}: moved {moved:.3g}, per-unit {max(unit.values()):.3g}")
    assert moved >= MOVED, (c["name"], mutant, moved)
    # the comparison of tests/test_gpu_axes.py, given the mutant's outputs where the GPU's would go, refuses them
    as32 = {k: np.asarray(v, np.float32) if isinstance(v, np.ndarray) else np.float32(v) for k, v in o.items()}
    bad = A.failures(c, as32, TOL)
    assert bad, (c["name"], mutant)
    print("   refused for", sorted(bad))
    if A.F16 in c["families"]:                                   # ... and at the f16 mode's wider bars
        assert A.failures(c, as32, TOL, (TOL_LOSS, TOL_FEATS, TOL_GRADS)), (c["name"], mutant)
    # and it accepts the oracle's own outputs rounded to float32
    own = {k: np.asarray(v, np.float32) if isinstance(v, np.ndarray) else np.float32(v) for k, v in c["ref"].items()}
    assert A.failures(c, own, TOL) == {}
    assert A.failures(c, own, TOL, (TOL_LOSS, TOL_FEATS, TOL_GRADS)) == {}
