"""Timing of the batched harness loop (NeuralNetwork.loop, Functions.py:1014-1289) — one JSON line.

* ``ClosedLoop.run`` at B = 65 536 trajectories x T = 300 steps (UL/Main.py:79 T_TRAJ), as scripts/bench_closed_loop.py
  sets it up: clean, with process noise ``w``, and with ``w`` and measurement noise ``v`` (Gaussian, the reference's
  standard deviations, drawn on the device: the timing does not depend on the stream's order).
* ``simulate_rollout`` (one launch, fcr_lstm_rollout) at B = 4 096, T = 300 with the reference's surrogate weights,
  against the composition it replaces on the same inputs: T launches of ``simulate_step`` with the window shuffled in
  torch between them (``inference._rollout_by_steps``); the two results are compared as well.

Each figure is the median of ``--repeats`` timed calls after one warm-up call; the single timings are kept beside it.
``--recovery`` times the loop with feasibility recovery instead (:func:`recovery`), one JSON line as well.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import forging_control_amd as fca  # noqa: E402

SCALERS = {"input": np.array([0.9113443, 0.3758976, 0.9113443]), "y_dot": 0.9113443, "output": 0.3}
PROCESS_STD = [0.5, 2.0, 5e7, 5e7, 2.0]      # UL/Main.py:88-112
MEAS_STD = [1e-4, 1e-2, 1e4, 1e4, 1e-3]
DEV = "cuda:0"


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"ms": float(np.median(out)), "each_ms": [round(v, 4) for v in out]}


def recovery(a):
    """--recovery: ``ClosedLoop.run`` with and without ``feasibility=FeasibilityRecovery()`` and ``project`` alone.

    * ``feasible``: B x T with every trajectory's working-stroke reference held (no step is flagged; the line reports
      the count): the price of the 32-right-hand-side check beside the plant step's 16.
    * ``corrections``: the inputs of tests/test_closed_loop.py::test_gpu_closed_loop_matches_oracle (300 trajectories,
      120 steps, smooth=False) tiled to B: waves with an infeasible lane run the search.
    * ``clean`` / ``w_v``: the same B x T without recovery, as the default mode times them.
    * ``project``: the fixture tests/golden/feasibility_cases.npz tiled to B."""
    B, T = a.batch, a.steps
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_ref.npz"))
    ctrl = fca.FNNModel(3, 50, 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(w["W_inp"]))
        ctrl.fc_inp.bias.copy_(torch.tensor(w["b_inp"]))
        ctrl.fc_out.weight.copy_(torch.tensor(w["W_out"]))
    fr = fca.FeasibilityRecovery()
    dev = lambda v: torch.tensor(v, device=DEV)
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 5))
    x0[:, 2:4] = rng.uniform(1e6, 4e6, (B, 2))
    ref = fca.closed_loop.reference_speeds(64, T, 1e-3, 1, 100)[rng.integers(0, 64, B)]
    cl = fca.ClosedLoop(ctrl, SCALERS)
    x0_d, ref_d, held_d = dev(x0), dev(ref), dev(np.repeat(ref[:, :1], T, axis=1))
    g = torch.Generator(device=DEV).manual_seed(0)
    draw = lambda std: torch.randn(B, T, 5, dtype=torch.float64, device=DEV, generator=g) * torch.tensor(std, device=DEV)
    wn, vn = draw(PROCESS_STD), draw(MEAS_STD)
    out = {"B": B, "T": T, "clean": timed(lambda: cl.run(x0_d, ref_d), a.repeats),
           "w_v": timed(lambda: cl.run(x0_d, ref_d, process_noise=wn, meas_noise=vn), a.repeats)}
    del wn, vn
    out["feasible_clean"] = timed(lambda: cl.run(x0_d, held_d), a.repeats)
    out["feasible"] = timed(lambda: cl.run(x0_d, held_d, feasibility=fr), a.repeats)
    flag = cl.run(x0_d, held_d, feasibility=fr)[2]["flag"]
    out["feasible"]["flagged_steps"] = int((flag != 0).sum())
    out["feasible"]["over_clean"] = out["feasible"]["ms"] / out["feasible_clean"]["ms"]
    del flag

    r4 = np.random.default_rng(4)                      # test_gpu_closed_loop_matches_oracle's inputs
    xs = np.zeros((300, 5))
    xs[:, 2] = r4.uniform(1e6, 4e6, 300)
    xs[:, 3] = r4.uniform(1e6, 4e6, 300)
    tile = np.arange(B) % 300
    xc_d, rc_d = dev(xs[tile]), dev(fca.closed_loop.reference_speeds(300, 120, 1e-3, 1, 100)[tile])
    cn = fca.ClosedLoop(ctrl, SCALERS, smooth=False)
    cor = {"B": B, "T": 120, "plain": timed(lambda: cn.run(xc_d, rc_d), a.repeats),
           "recovery": timed(lambda: cn.run(xc_d, rc_d, feasibility=fr), a.repeats)}
    flag = cn.run(xc_d, rc_d, feasibility=fr)[2]["flag"]
    cor["flagged_steps"] = [int((flag == k).sum()) for k in (1, 2)]
    cor["over_plain"] = cor["recovery"]["ms"] / cor["plain"]["ms"]
    out["corrections"] = cor

    c = np.load(os.path.join(ROOT, "tests", "golden", "feasibility_cases.npz"))
    tile = np.arange(B) % c["x"].shape[0]
    xp_d, up_d = dev(c["x"][tile]), dev(c["u_nn"][tile])
    out["project"] = {"B": B, "flags_0_1_2": [int((c["flag"][tile] == k).sum()) for k in range(3)],
                      **timed(lambda: fr.project(xp_d, up_d), a.repeats)}
    print(json.dumps({"metric": "harness loop, feasibility recovery", "device": torch.cuda.get_device_name(0), **out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rollout-batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--recovery", action="store_true", help="time the loop with feasibility recovery instead")
    a = ap.parse_args()
    if a.recovery:
        return recovery(a)
    B, T = a.batch, a.steps
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_ref.npz"))
    ctrl = fca.FNNModel(3, 50, 1, 1).to(DEV)
    sim = fca.LSTMModel(5, 50, 4, 3)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(w["W_inp"]))
        ctrl.fc_inp.bias.copy_(torch.tensor(w["b_inp"]))
        ctrl.fc_out.weight.copy_(torch.tensor(w["W_out"]))
        for k in range(3):
            getattr(sim.lstm, f"weight_ih_l{k}").copy_(torch.as_tensor(w[f"Wih{k}"]))
            getattr(sim.lstm, f"weight_hh_l{k}").copy_(torch.as_tensor(w[f"Whh{k}"]))
        sim.fc.weight.copy_(torch.as_tensor(w["fcW"]))
        sim.fc.bias.copy_(torch.as_tensor(w["fcb"]))
    sim = sim.to(DEV)
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 5))
    x0[:, 2:4] = rng.uniform(1e6, 4e6, (B, 2))
    ref = fca.closed_loop.reference_speeds(64, T, 1e-3, 1, 100)[rng.integers(0, 64, B)]
    cl = fca.ClosedLoop(ctrl, SCALERS)
    x0_d, ref_d = torch.tensor(x0, device=DEV), torch.tensor(ref, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    draw = lambda std: torch.randn(B, T, 5, dtype=torch.float64, device=DEV, generator=g) * torch.tensor(std, device=DEV)
    wn, vn = draw(PROCESS_STD), draw(MEAS_STD)
    run = {"clean": timed(lambda: cl.run(x0_d, ref_d), a.repeats),
           "w": timed(lambda: cl.run(x0_d, ref_d, process_noise=wn), a.repeats),
           "w_v": timed(lambda: cl.run(x0_d, ref_d, process_noise=wn, meas_noise=vn), a.repeats)}
    del wn, vn

    Br = a.rollout_batch
    row = np.empty((Br, 5))
    row[:, [0, 3]] = rng.uniform(-0.5, 0.5, (Br, 2))
    row[:, 1:3] = rng.uniform(0.05, 0.9, (Br, 2))
    row[:, 4] = rng.uniform(-1, 1, Br)
    window0 = torch.tensor(np.repeat(row[:, None, :], 10, axis=1), dtype=torch.float32, device=DEV)
    cmd = torch.tensor(np.repeat(rng.uniform(-1, 1, (Br, (T + 3) // 4)), 4, axis=1)[:, :T], dtype=torch.float32, device=DEV)
    one = timed(lambda: fca.simulate_rollout(sim, window0, cmd), a.repeats)
    ones = torch.ones(4, device=DEV)
    steps = timed(lambda: fca.inference._rollout_by_steps(sim, window0, cmd, ones, None), max(1, a.repeats // 2))
    xa = fca.simulate_rollout(sim, window0, cmd)
    xb = fca.inference._rollout_by_steps(sim, window0, cmd, ones, None)
    line = {"metric": "harness loop", "device": torch.cuda.get_device_name(0),
            "closed_loop_run": {"B": B, "T": T, **run,
                                "trajectory_steps_per_s": {k: B * T / (v["ms"] * 1e-3) for k, v in run.items()}},
            "simulate_rollout": {"B": Br, "T": T, "one_launch": one, "simulate_step_composition": steps,
                                 "speedup": steps["ms"] / one["ms"],
                                 "max_abs_difference": float((xa - xb).abs().max())}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
