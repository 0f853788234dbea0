"""Timing of a training step on the press — one JSON line, also written to --out
(default profiles/press_train_bench.log).

For M in {1, 10} controllers of the reference's width on B = 65 536 // M trajectories each, T in {50, 300} steps, the
smooth model, the reference's press, each model with its own alpha and pressure bounds:

* ``fwd``: the forward launch (``ClosedLoopBank.run``), as every path below makes it;
* ``fused_bwd``: ``fcr_closed_loop_bank_loss_vjp`` on the stored record — the reverse launch with the loss's cotangents
  formed in registers, the cost's sum, the parameter kernels; ``fused_step`` = ``fwd`` + ``fused_bwd`` in one window,
  ``press_loss_step`` the same through ``PressLoss`` and autograd (``loss.sum().backward()``);
* ``general_bwd``: ``fcr_closed_loop_bank_vjp`` on the same record with the loss's cotangents given as tensors
  (``g_x``, ``g_u`` computed beforehand, not timed): the reverse launch reads 24 B per record element where the fused
  one reads 8 B; ``general_over_fused`` is their ratio;
* ``loop_step``: what the library could do for this loss before the bank's adjoint — M calls of
  ``ClosedLoop.run(differentiable=True)``, the loss written in torch on each record, ``backward()``;
  ``loop_over_fused`` = ``loop_step`` / ``press_loss_step``.

All in one process. Each figure is the median of ``--repeats`` timed calls (device events around work that ends in a
synchronise) after one warm-up call of every variant; the variants of one setting are timed in turns, one call each per
round, so a drift of the machine falls on all of them alike. The single timings are kept beside the medians. The
fused and the torch-written loss are compared before anything is timed (``loss_rel_diff``).
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
from forging_control_amd.closed_loop import bank_loss_vjp, bank_vjp  # noqa: E402

SCALERS = {"input": np.array([0.9113443, 0.3758976, 0.9113443]), "y_dot": 0.9113443, "output": 0.3}
P_SCALE = (32e6 / fca._native.P1_MAX, 32e6 / fca._native.P2_MAX)
DEV = "cuda:0"


def timed_in_turns(fns, repeats):
    """{name: {"ms": median, "each_ms": [...]}} of the callables, one warm-up each, then ``repeats`` rounds."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    each = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            each[k].append(e0.elapsed_time(e1))
    return {k: {"ms": float(np.median(v)), "each_ms": [round(t, 4) for t in v]} for k, v in each.items()}


def inputs(B, T):
    """scripts/bench_press_grad.py's batch: a press at rest, pressures around the traces' starting values, the harness's
    references."""
    rng = np.random.default_rng(4)
    x0 = np.zeros((B, 5))
    x0[:, 2] = rng.uniform(1e6, 4e6, B)
    x0[:, 3] = rng.uniform(1e6, 4e6, B)
    ref = np.tile(fca.closed_loop.reference_speeds(256, T, 1e-3, 1, 100), (B // 256 + 1, 1))[:B]
    return torch.tensor(x0, device=DEV), torch.tensor(ref, device=DEV)


def torch_cost(x, u, ref, row):
    """The loss of DESIGN.md §7.16 on one model's record, in torch: cost (B,)."""
    alpha, lo1, hi1, lo2, hi2, w = row
    e = (x[:, 1:, 1] - ref) / SCALERS["y_dot"]
    d = torch.cat([torch.zeros_like(u[:, :1]), u[:, 1:] - u[:, :-1]], 1) / SCALERS["output"]
    P1, P2 = x[:, 1:, 2] / P_SCALE[0], x[:, 1:, 3] / P_SCALE[1]
    c = w * (torch.relu(lo1 - P1) + torch.relu(P1 - hi1) + torch.relu(lo2 - P2) + torch.relu(P2 - hi2))
    return (e * e + alpha * d * d + c).mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=65536, help="trajectories over all models: B = total // M per model")
    ap.add_argument("--models", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--steps", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "press_train_bench.log"))
    a = ap.parse_args()
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_ref.npz"))
    out = {"bench": "press_train", "total": a.total, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
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
        singles = [fca.ClosedLoop(c, SCALERS, smooth=True) for c in models]
        terms = [fca.LossTerms(p1=(0.05 + 0.01 * m, 0.2), p2=(0.05, 0.1 + 0.01 * m), alpha=10.0 + m) for m in range(M)]
        rows = [t.as_row(0.1) for t in terms]
        pl = fca.PressLoss(loop, P_SCALE, terms=terms)
        for T in a.steps:
            x0, ref = inputs(B, T)
            r = loop.run(x0, ref)
            x, u = r["x"], r["u"]
            xs, us = x.clone().requires_grad_(True), u.clone().requires_grad_(True)
            loss_t = torch.stack([torch_cost(xs[m], us[m], ref, rows[m]).mean() for m in range(M)])
            g_x, g_u = torch.autograd.grad(loss_t.sum(), (xs, us))
            fused = bank_loss_vjp(loop, x, u, ref, rows, P_SCALE, want_x0=False)
            rel = float((fused["loss"] - loss_t.detach()).abs().max() / loss_t.detach().abs().max())
            del xs, us, loss_t

            def press_loss_step():
                bank.zero_grad(set_to_none=True)
                pl.forward(x0, ref)[0].sum().backward()

            def loop_step():
                for m, (single, ctrl) in enumerate(zip(singles, models)):
                    ctrl.zero_grad(set_to_none=True)
                    xm, um = single.run(x0, ref, differentiable=True)
                    torch_cost(xm, um, ref, rows[m]).mean().backward()

            def fused_step():
                rr = loop.run(x0, ref)
                bank_loss_vjp(loop, rr["x"], rr["u"], ref, rows, P_SCALE, want_x0=False)

            t = timed_in_turns({
                "fwd": lambda: loop.run(x0, ref),
                "fused_bwd": lambda: bank_loss_vjp(loop, x, u, ref, rows, P_SCALE, want_x0=False),
                "general_bwd": lambda: bank_vjp(loop, x, u, ref, g_x, g_u, want_x0=False),
                "fused_step": fused_step, "press_loss_step": press_loss_step, "loop_step": loop_step}, a.repeats)
            t["general_over_fused"] = round(t["general_bwd"]["ms"] / t["fused_bwd"]["ms"], 3)
            t["loop_over_fused"] = round(t["loop_step"]["ms"] / t["press_loss_step"]["ms"], 3)
            t["loss_rel_diff"] = rel
            out[f"M{M}_B{B}_T{T}"] = t
            del x, u, g_x, g_u, r, fused
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
