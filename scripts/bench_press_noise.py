"""Timing of a training step on the press under noise — one JSON line, also written to --out
(default profiles/press_noise_bench.log).

§7.16's four settings: M in {1, 10} controllers of the reference's width on B = 65 536 // M trajectories each, T in
{50, 300} steps, the smooth model, the reference's press. Per setting, a ``PressLoss`` training step (forward launch,
fused reverse launch, parameter kernels, autograd: ``loss.sum().backward()``)

* ``clean``: without noise (the kernels of §7.16);
* ``w``: under process noise alone (the existing noisy forward; the noisy reverse kernel, the record being the state);
* ``wv``: under process and measurement noise (the forward that also stores x_state; the reverse reads it);

and beside them the forward and the fused reverse launch of each variant alone. The noise is pre-drawn once per setting
(``device_noise``, shared by the models) and not timed. All in one process; each figure is the median of ``--repeats``
timed calls after one warm-up of every variant, the variants timed in turns, one call each per round.

``--clean-only``: the noise-free variants alone — what a library from before §7.18 can run (FCR_DEV=1 FCR_LIB=<that
build>), for the same-session comparison of the noise-free step across two builds.
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
from forging_control_amd.closed_loop import bank_loss_vjp, device_noise  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_press_train import DEV, P_SCALE, SCALERS, inputs, timed_in_turns  # noqa: E402

PROCESS_STD = [0.5, 2.0, 5e7, 5e7, 2.0]     # the harness's (UL/Main.py:88-112)
MEAS_STD = [1e-4, 1e-2, 1e4, 1e4, 1e-3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=65536, help="trajectories over all models: B = total // M per model")
    ap.add_argument("--models", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--steps", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--clean-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "press_noise_bench.log"))
    a = ap.parse_args()
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_ref.npz"))
    out = {"bench": "press_noise", "total": a.total, "repeats": a.repeats, "clean_only": a.clean_only,
           "library": os.path.relpath(fca._native.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0)}
    for M in a.models:
        B = a.total // M
        models = []
        for m in range(M):                                    # the reference's controller, W_out scaled per model
            ctrl = fca.FNNModel(3, 50, 1, 1).to(DEV)
            with torch.no_grad():
                ctrl.fc_inp.weight.copy_(torch.tensor(w["W_inp"]))
                ctrl.fc_inp.bias.copy_(torch.tensor(w["b_inp"]))
                ctrl.fc_out.weight.copy_(torch.tensor(w["W_out"]) * (1.0 + 0.05 * m))
            models.append(ctrl)
        bank = fca.ControllerBank.from_models(models).to(DEV)
        loop = fca.ClosedLoopBank(bank, SCALERS, smooth=True)
        terms = [fca.LossTerms(p1=(0.05 + 0.01 * m, 0.2), p2=(0.05, 0.1 + 0.01 * m), alpha=10.0 + m) for m in range(M)]
        rows = [t.as_row(0.1) for t in terms]
        pl = fca.PressLoss(loop, P_SCALE, terms=terms)
        for T in a.steps:
            x0, ref = inputs(B, T)
            wn, vn = device_noise(B, T, PROCESS_STD, MEAS_STD, DEV, torch.Generator(DEV).manual_seed(5))
            variants = {"clean": {}} if a.clean_only else {
                "clean": {}, "w": dict(process_noise=wn), "wv": dict(process_noise=wn, meas_noise=vn)}
            fns, kept = {}, []
            for name, kw in variants.items():
                noisy = bool(kw)
                if noisy:
                    with torch.no_grad():
                        r = loop.run_differentiable(x0, ref, kw.get("process_noise"), kw.get("meas_noise"))
                    state = r["x_state"] if "meas_noise" in kw else None
                    fns[f"{name}_fwd"] = (lambda kw=kw: loop._launch(x0, ref, kw.get("process_noise"), kw.get("meas_noise"),
                                                                     None, True, None, None, with_state=True))
                    fns[f"{name}_bwd"] = (lambda r=r, kw=kw, state=state: bank_loss_vjp(
                        loop, r["x"], r["u"], ref, rows, P_SCALE, want_x0=False, process_noise=kw.get("process_noise"),
                        x_state=state))
                else:
                    r = loop.run(x0, ref)
                    fns["clean_fwd"] = lambda: loop.run(x0, ref)
                    fns["clean_bwd"] = lambda r=r: bank_loss_vjp(loop, r["x"], r["u"], ref, rows, P_SCALE, want_x0=False)
                kept.append(r)

                def step(kw=kw):
                    bank.zero_grad(set_to_none=True)
                    pl.forward(x0, ref, **kw)[0].sum().backward()

                fns[f"{name}_step"] = step
            t = timed_in_turns(fns, a.repeats)
            for name in variants:
                if name != "clean":
                    t[f"{name}_step_over_clean"] = round(t[f"{name}_step"]["ms"] / t["clean_step"]["ms"], 4)
            out[f"M{M}_B{B}_T{T}"] = t
            del kept, fns, wn, vn
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
