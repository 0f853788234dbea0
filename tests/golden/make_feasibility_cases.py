"""Write tests/golden/feasibility_cases.npz: states and commands with the projection's expected result.

The expected values come from the NumPy restatement (tests/feasibility_np.py on oracle/plant_np.py), not from the
kernel. Two sources:

* the closed loop of tests/test_closed_loop.py::test_gpu_closed_loop_matches_oracle (B = 300, T = 120, seed 4,
  smooth=False) run with recovery: every (state, u_nn) the search corrected, and as many feasible ones drawn from
  the same run (the first n_loop cases; ref_loop holds the speed reference each of them was met under);
* a seeded scan (default_rng(7), 4 000 draws: y in [0, 0.03], y_dot in +-0.5, p1, p2 in [-2e6, 34e6], z in +-0.1,
  u_nn in +-0.25), from which the first PER_CLASS cases of each class are kept: flag 0 with u_nn inside / outside
  u_bounds, flag 1 corrected upward / downward, flag 2.

Run from the repository root: python tests/golden/make_feasibility_cases.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from feasibility_np import closed_loop_recover, project, violation  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "feasibility_cases.npz")
PER_CLASS = 40
SCALERS = {"input": np.array([0.9113443, 0.3758976, 0.9113443]), "y_dot": 0.9113443, "output": 0.3}   # test_closed_loop.py


def classes(u_nn, u, flag, u_bounds=(-0.2, 0.2)):
    inside = (u_nn >= u_bounds[0]) & (u_nn <= u_bounds[1])
    return {"flag0_inside": (flag == 0) & inside, "flag0_outside": (flag == 0) & ~inside,
            "flag1_up": (flag == 1) & (u > u_nn), "flag1_down": (flag == 1) & (u < u_nn), "flag2": flag == 2}


def loop_cases():
    import importlib
    fca = importlib.import_module("forging-control_amd")
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_ref.npz"))
    B, T = 300, 120
    rng = np.random.default_rng(4)
    x0 = np.zeros((B, 5))
    x0[:, 2] = rng.uniform(1e6, 4e6, B)
    x0[:, 3] = rng.uniform(1e6, 4e6, B)
    ref = fca.closed_loop.reference_speeds(B, T, 1e-3, 1, 100)
    xs, us, un, fl = closed_loop_recover(x0, ref, w["W_inp"], w["b_inp"], w["W_out"], SCALERS["input"][:2],
                                         SCALERS["y_dot"], SCALERS["output"], smooth=False)
    assert not (fl == 2).any()
    b1, t1 = np.nonzero(fl == 1)
    b0, t0 = np.nonzero(fl == 0)
    pick = np.sort(np.random.default_rng(11).choice(b0.size, b1.size, replace=False))
    b, t = np.concatenate([b1, b0[pick]]), np.concatenate([t1, t0[pick]])
    p = xs[:, 1:, 2:4]
    print(f"loop: {b1.size} corrected steps in {np.unique(b1).size} trajectories, first at step {t1.min()}, "
          f"largest |du| {np.abs(us - un).max():.3g}, p range [{p.min():.3g}, {p.max():.3g}]")
    return xs[b, t], un[b, t], ref[b, t]


def scan_cases():
    rng = np.random.default_rng(7)
    n = 4000
    x = np.stack([rng.uniform(0, 0.03, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-2e6, 34e6, n),
                  rng.uniform(-2e6, 34e6, n), rng.uniform(-0.1, 0.1, n)], axis=1)
    u_nn = rng.uniform(-0.25, 0.25, n)
    u, flag, v = project(x, u_nn)
    cls = classes(u_nn, u, flag)
    print("scan:", {k: int(m.sum()) for k, m in cls.items()}, "NaN:", int(np.isnan(v).sum()))
    keep = np.sort(np.concatenate([np.flatnonzero(m)[:PER_CLASS] for m in cls.values()]))
    return x[keep], u_nn[keep]


if __name__ == "__main__":
    xl, ul, refl = loop_cases()
    xsc, usc = scan_cases()
    x, u_nn = np.concatenate([xl, xsc]), np.concatenate([ul, usc])
    u, flag, v = project(x, u_nn)
    v_nn = violation(x, u_nn)
    assert x.shape[0] % 64, x.shape
    assert not np.isnan(v_nn).any() and np.abs(v_nn).min() > 1e-9, np.abs(v_nn).min()   # no flag hangs on rounding
    np.savez_compressed(OUT, x=x, u_nn=u_nn, u=u, flag=flag, v=v, v_nn=v_nn, n_loop=np.int64(xl.shape[0]), ref_loop=refl)
    print(OUT, x.shape, {k: int(m.sum()) for k, m in classes(u_nn, u, flag).items()}, "min |v(u_nn)|",
          np.abs(v_nn).min())
