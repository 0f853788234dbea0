"""Timing of the MPC baseline on the press — one JSON line.

* ``solve``: ``PressMPC.solve`` (``fcr_mpc_solve``) at ``--batch`` problems (default 65 536), N = 10, K = 3, smooth model,
  the reference's press, warm-ish problems around the reference's trace;
* ``loop``: ``PressMPC.run`` (``fcr_mpc_closed_loop``) at the same batch over ``--steps`` steps (default 300), with the
  per-step time and, when fewer steps were run, nothing extrapolated;
* ``torch``: the same algorithm as a user can write it today — ``forging_rk4`` differentiable, one backward pass per
  residual row for J, batched ``torch.linalg.cholesky`` — at ``--torch-batch`` problems;
* ``step_equivalents_per_s``: sampling steps of the press per second the solve kernel sustains, counting a step's adjoint
  under one cotangent as 2.5 steps (12 recomputed + 12 stage + 16 adjoint right-hand sides against a step's 16), to set
  beside the plant kernel's rate. A linearisation costs N (1 + 5 x 2.5) of them, a trial rollout N; the
  count uses the trace's accept flags (a rejected iteration reuses the linearisation).

Each figure is the median of ``--repeats`` timed calls after one warm-up call.
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

DEV = "cuda:0"
R_U = 0.02


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
    return {"ms": float(np.median(out)), "each_ms": [round(v, 3) for v in out]}


def inputs(B, T):
    d = np.load(os.path.join(ROOT, "tests", "golden", "plant_trace.npz"))["mpc"]
    rng = np.random.default_rng(0)
    rows = d[rng.integers(1, len(d), B)]
    x0 = rows[:, 2:7] * (1 + 0.02 * rng.standard_normal((B, 5)))
    ref = np.repeat(rows[:, 1:2] + 0.05 * rng.standard_normal((B, 1)), T, 1)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)
    return t(x0), t(ref), t(rows[:, 7])


def torch_solve(x0, ref, u_prev, N, K, lam0=1e-3):
    """The algorithm of csrc/fcr_mpc.h in torch on the device, without bounds: J row by row through forging_rk4's adjoint."""
    B = x0.shape[0]
    sru = R_U ** 0.5

    def residuals(U):
        x = fca.forging_rk4(x0, U, smooth=True)
        return torch.cat([x[:, 1:, 1] - ref, sru * (U - torch.cat([u_prev[:, None], U[:, :-1]], 1))], 1)

    U = u_prev[:, None].expand(B, N).contiguous()
    lam = torch.full((B,), lam0, dtype=torch.float64, device=DEV)
    for _ in range(K):
        Ug = U.detach().clone().requires_grad_(True)
        r = residuals(Ug)
        J = torch.stack([torch.autograd.grad(r[:, i].sum(), Ug, retain_graph=True)[0] for i in range(r.shape[1])], 1)
        r = r.detach()
        H = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])[:, :, 0]
        M = H + torch.diag_embed(lam[:, None] * torch.diagonal(H, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(M)
        Un = U + torch.cholesky_solve(-g[:, :, None], L)[:, :, 0]
        with torch.no_grad():
            accept = ((residuals(Un) ** 2).sum(1) < (r * r).sum(1)) & (info == 0)
        U = torch.where(accept[:, None], Un, U)
        lam = torch.where(accept, (lam * 0.3).clamp(min=1e-12), (lam * 10).clamp(max=1e12))
    return U


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--torch-batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    N, K = a.horizon, a.iters
    mpc = fca.PressMPC(n_horizon=N, iters=K)
    x0, ref, up = inputs(a.batch, max(a.steps, N))
    res = {"gpu": torch.cuda.get_device_name(0), "B": a.batch, "N": N, "K": K}
    res["solve"] = timed(lambda: mpc.solve(x0, ref[:, :N], up), a.repeats)
    tr = mpc.solve(x0, ref[:, :N], up, trace=True)
    acc = tr["trace"][:, :, 3] != 0
    fresh = torch.cat([torch.ones_like(acc[:, :1]), acc[:, :-1]], 1).double().mean(0).sum().item()   # linearisations per lane
    steps = a.batch * N * (fresh * 13.5 + K)
    print("solve:", res["solve"], file=sys.stderr, flush=True)
    res["solve"].update(linearisations_per_lane=round(fresh, 3), accepted_mean=round(acc.double().sum(1).mean().item(), 3),
                        step_equivalents_per_s=steps / (res["solve"]["ms"] * 1e-3))
    if a.steps > 0:
        res["loop"] = timed(lambda: mpc.run(x0, ref[:, :a.steps], u_init=up), max(1, a.repeats - 2))
        res["loop"].update(T=a.steps, ms_per_step=res["loop"]["ms"] / a.steps)
        print("loop:", res["loop"], file=sys.stderr, flush=True)
    if a.torch_batch > 0:
        xb, rb, ub = x0[:a.torch_batch], ref[:a.torch_batch, :N], up[:a.torch_batch]
        res["torch"] = timed(lambda: torch_solve(xb, rb, ub, N, K), a.repeats)
        res["torch"].update(B=xb.shape[0], per_problem_over_kernel=(res["torch"]["ms"] / xb.shape[0])
                            / (res["solve"]["ms"] / a.batch))
        Ut, Uk = torch_solve(xb[:256], rb[:256], ub[:256], N, K), mpc.solve(xb[:256], rb[:256], ub[:256])["U"]
        res["torch"]["max_abs_dU_vs_kernel"] = float((Ut - Uk).abs().max())
    print(json.dumps(res))
