"""Timing of the bank closed loop with the press as data (ClosedLoopBank.run(plant_params=...),
fcr_closed_loop_run_bank_press) against the same call without parameters — one JSON line per cell.

(M, B, T) = (1, 65 536, 300) and (10, 4 096, 300), the ten shipped seeds cycled to M, one shared set of trajectories
(scripts/bench_loop_bank.py's press and references), ``store=False`` so the figure is the loop and not its stores.
Plain (smooth plant) and recovering (non-smooth plant, nominal model). Arms, alternating call by call in this one
process, each figure the median of ``--repeats`` wall-clock timings after one warm-up call of each arm:

* ``nominal``  no parameters: the kernels compiled with the reference's press;
* ``shared``   one (28,) row for every trajectory, read through zero strides;
* ``table``    a (B,28) table, every row another press (all 28 fields within +-5 %), shared by the models.

With FCR_LIB + FCR_DEV=1 naming another build of the library (the parent commit's) ``--nominal-only`` times the first
arm alone, for the comparison of the unchanged path against its own earlier self.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import forging_control_amd as fca  # noqa: E402
from bench_loop_bank import DEV, SCALERS, alternate, bank_of, press  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--cells", type=int, nargs="*", default=[1, 65536, 10, 4096], help="M B pairs")
    ap.add_argument("--nominal-only", action="store_true")
    a = ap.parse_args()
    T = a.steps
    name = torch.cuda.get_device_name(0)
    fr = fca.FeasibilityRecovery()
    for M, B in zip(a.cells[0::2], a.cells[1::2]):
        x0, ref = press(B, T)
        bank = bank_of(M)
        row = fca.PressParams().table(1, DEV)[0]
        table = fca.PressParams().sample(B, {n: 0.05 for n in fca.PressParams.NAMES}, rng=np.random.RandomState(1), device=DEV)
        for recover in (False, True):
            smooth, feas = not recover, fr if recover else None
            clb = fca.ClosedLoopBank(bank, SCALERS, smooth=smooth)
            arms = {"nominal": lambda: clb.run(x0, ref, feasibility=feas, store=False)}
            if not a.nominal_only:
                arms["shared"] = lambda: clb.run(x0, ref, feasibility=feas, store=False, plant_params=row)
                arms["table"] = lambda: clb.run(x0, ref, feasibility=feas, store=False, plant_params=table)
            r = alternate(arms, a.repeats)
            line = {"metric": "closed loop, bank of controllers: press as data", "device": name, "M": M, "B": B, "T": T,
                    "recovery": recover, "library": os.path.basename(fca._native.LIB_PATH), **r}
            if not a.nominal_only:
                line["shared_over_nominal"] = r["shared"]["ms"] / r["nominal"]["ms"]
                line["table_over_nominal"] = r["table"]["ms"] / r["nominal"]["ms"]
                res = clb.run(x0, ref, feasibility=feas, store=False, plant_params=table)
                line["viol_frac_table"] = res["metrics"]["viol_frac"].tolist()[:3]
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
