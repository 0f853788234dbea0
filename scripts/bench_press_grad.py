"""Timing of the differentiable press — one JSON line.

At B = 65 536 trajectories and T = 50 and 300 steps, for the open-loop rollout (``forging_rk4`` / ``fcr_plant_rk4_vjp``)
and the closed loop (``ClosedLoop.run`` / ``fcr_closed_loop_vjp`` with its parameter-gradient kernels), smooth model,
the reference's press and controller:

* ``fwd_ms``: the forward launch, as a call without gradients makes it;
* ``bwd_ms``: the backward alone, on the stored run; ``bwd_over_fwd`` is the multiple of the same build's forward.

Each figure is the median of ``--repeats`` timed calls after one warm-up call; the single timings are kept beside it.
``--forward-only`` skips the backward: with ``FCR_LIB`` naming a library built from the parent commit (and ``FCR_DEV=1``)
it gives the parent's forward launches in the same session, the spread the new build's forward is to be inside of.

``--press-grad`` times the backward with the gradients of the 28 press parameters instead: for the
closed loop (``loop_vjp``) and the open loop (``forging_rk4``'s autograd), under the reference's press given as data,

* ``*_bwd_table``: the plain backward through a ``(B,28)`` table, no parameter gradient (the kernels of §7.13);
* ``*_bwd_press_table``: the same with ``g_press (B,28)``; ``*_bwd_press_row``: one shared ``(28,)`` row, the fixed-order
  sum over the trajectories included;
* ``*_press_table_over_table`` / ``*_press_row_over_table``: their multiples of the plain table backward.
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


def inputs(B, T):
    """tests/test_closed_loop.py's batch: a press at rest with pressures around the traces' starting values, the
    harness's references; the open loop replays the closed loop's commands."""
    rng = np.random.default_rng(4)
    x0 = np.zeros((B, 5))
    x0[:, 2] = rng.uniform(1e6, 4e6, B)
    x0[:, 3] = rng.uniform(1e6, 4e6, B)
    ref = np.tile(fca.closed_loop.reference_speeds(256, T, 1e-3, 1, 100), (B // 256 + 1, 1))[:B]
    return torch.tensor(x0, device=DEV), torch.tensor(ref, device=DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--press-grad", action="store_true")
    a = ap.parse_args()
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_ref.npz"))
    ctrl = fca.FNNModel(3, 50, 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.tensor(w["W_inp"]))
        ctrl.fc_inp.bias.copy_(torch.tensor(w["b_inp"]))
        ctrl.fc_out.weight.copy_(torch.tensor(w["W_out"]))
    loop = fca.ClosedLoop(ctrl, SCALERS, smooth=True)
    out = {"bench": "press_param_grad" if a.press_grad else "press_grad", "B": a.batch, "repeats": a.repeats, "lib": fca._native.LIB_PATH,
           "device": torch.cuda.get_device_name(0)}
    for T in a.steps if a.press_grad else ():
        x0, ref = inputs(a.batch, T)
        table = fca.PressParams().table(a.batch, DEV)
        row = table[0].clone()
        x, u = loop.run(x0, ref, plant_params=table)
        g_x = torch.randn_like(x) / x.abs().amax((0, 1)).clamp_min(1e-30)
        g_u = torch.randn_like(u)
        vjp = lambda press, grad: fca.closed_loop.loop_vjp(loop, x, u, ref, g_x, g_u, plant_params=press, press_grad=grad)
        r = {"closed_bwd_table": timed(lambda: vjp(table, False), a.repeats),
             "closed_bwd_press_table": timed(lambda: vjp(table, True), a.repeats),
             "closed_bwd_press_row": timed(lambda: vjp(row, True), a.repeats)}
        xa = x0.clone().requires_grad_(True)
        leaf_t, leaf_r = table.clone().requires_grad_(True), row.clone().requires_grad_(True)
        X0 = fca.forging_rk4(xa, u, smooth=True, params=table)
        Xt = fca.forging_rk4(xa, u, smooth=True, params=leaf_t)
        Xr = fca.forging_rk4(xa, u, smooth=True, params=leaf_r)
        r["open_bwd_table"] = timed(lambda: torch.autograd.grad(X0, xa, g_x, retain_graph=True), a.repeats)
        r["open_bwd_press_table"] = timed(lambda: torch.autograd.grad(Xt, (xa, leaf_t), g_x, retain_graph=True), a.repeats)
        r["open_bwd_press_row"] = timed(lambda: torch.autograd.grad(Xr, (xa, leaf_r), g_x, retain_graph=True), a.repeats)
        for k in ("closed", "open"):
            for form in ("table", "row"):
                r[f"{k}_press_{form}_over_table"] = round(r[f"{k}_bwd_press_{form}"]["ms"] / r[f"{k}_bwd_table"]["ms"], 3)
        out[f"T{T}"] = r
        del x, u, g_x, g_u, X0, Xt, Xr, xa, leaf_t, leaf_r, table, row
        torch.cuda.empty_cache()
    for T in () if a.press_grad else a.steps:
        x0, ref = inputs(a.batch, T)
        x, u = loop.run(x0, ref)
        r = {"closed_fwd": timed(lambda: loop.run(x0, ref), a.repeats),
             "open_fwd": timed(lambda: fca.forging_rk4(x0, u, smooth=True), a.repeats)}
        if not a.forward_only:
            g_x = torch.randn_like(x) / x.abs().amax((0, 1)).clamp_min(1e-30)
            g_u = torch.randn_like(u)
            r["closed_bwd"] = timed(lambda: fca.closed_loop.loop_vjp(loop, x, u, ref, g_x, g_u), a.repeats)
            xa = x0.clone().requires_grad_(True)
            X = fca.forging_rk4(xa, u, smooth=True)
            r["open_bwd"] = timed(lambda: torch.autograd.grad(X, xa, g_x, retain_graph=True), a.repeats)
            for k in ("closed", "open"):
                r[f"{k}_bwd_over_fwd"] = round(r[f"{k}_bwd"]["ms"] / r[f"{k}_fwd"]["ms"], 3)
            del g_x, g_u, X, xa
        out[f"T{T}"] = r
        del x, u
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
