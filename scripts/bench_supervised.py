"""One epoch of the supervised baseline (Supervised Learning/Main.py:143-159): the epoch kernel against the eager loop.

Workload, the reference's shape: n = 16 800 samples (80 trajectories x 300 steps x 0.7 train split), batch 256
(66 steps, the last of 160), FNNModel 3 -> 50 -> 1, nn.L1Loss, AdamW(lr = 1e-3); seeded synthetic samples.
  kernel     fcr_supervised_epoch for M = 1, 10 and 256 models: device time of the launch (events around a burst of
             launches) and host wall time of supervised.train_epoch (permutations, stacking, the launch, copying
             parameters and optimizer state back, one read of the losses);
  eager      the M = 1 epoch as the parent commit runs it: FNNModel.forward on HIP + torch L1Loss + AdamW + .item()
             per step, (a) through the reference's shuffling DataLoader over CPU tensors, (b) over batches already on
             the device (no loader at all: the best an eager loop can do);
  crossover  M = 1, n = 262 144: kernel epoch against eager loop (b) as the batch grows, for EPOCH_KERNEL_MAX_BATCH.
Medians of REPS timed windows after a warm-up of every shape; one JSON line per row.
    python scripts/bench_supervised.py [--reps 7] [--no-crossover]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import forging_control_amd as fca  # noqa: E402
from forging_control_amd import supervised as sl  # noqa: E402

DEV = "cuda:0"


def samples(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), torch.rand(n, 1, generator=g) * 1.6 - 0.8


def models(M, hidden=50, seed=1):
    torch.manual_seed(seed)
    ms = [fca.FNNModel(3, hidden, 1, 1).to(DEV) for _ in range(M)]
    return ms, [torch.optim.AdamW(m.parameters(), lr=1e-3) for m in ms]


def wall(fn, reps):
    """Median and spread of the host wall time of fn(), each run ending in a device synchronise."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def kernel_ms(M, X, y, bs, reps, burst):
    """Device time of one training launch: events around `burst` back-to-back launches on ready buffers."""
    ms, _ = models(M)
    dev, hidden, wi, bi, wo = sl._stack(ms)
    n = X.shape[0]
    perm = torch.stack([torch.randperm(n) for _ in range(M)]).to(DEV, torch.int32)
    moments = [torch.zeros_like(t) for t in (wi, bi, wo, wi, bi, wo)]
    step = torch.zeros(M, device=DEV)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    run = lambda: sl._launch(dev, hidden, wi, bi, wo, X, y, bs, fca._native.LOSS_L1, perm, hyper, moments, step)
    run()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(burst):
            run()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / burst)
    return statistics.median(out), min(out), max(out)


def eager_device_epoch(model, opt, Xd, yd, bs, loss_function):
    """The eager loop over batches that are already on the device, in a fresh shuffled order."""
    order = torch.randperm(Xd.shape[0]).to(DEV)
    Xs, ys = Xd[order], yd[order]
    total = 0
    for s in range(0, Xd.shape[0], bs):
        opt.zero_grad()
        loss = loss_function(model(Xs[s:s + bs]), ys[s:s + bs])
        loss.backward()
        opt.step()
        total += loss.item()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-crossover", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_supervised.py needs the GPU: there is no CPU path to time")
    n, bs = 16800, 256
    X, y = samples(n)
    Xd, yd = X.to(DEV), y.to(DEV)
    cfg = {"n": n, "batch": bs, "hidden": 50, "loss": "L1", "optimizer": "AdamW(lr=1e-3)", "steps": (n + bs - 1) // bs}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "config": cfg, "reps": a.reps}))
    rows = {}
    for M in (1, 10, 256):
        k = kernel_ms(M, Xd, yd[:, 0].contiguous(), bs, a.reps, burst=20)
        ms, opts = models(M)
        sl.train_epoch(ms, opts, Xd, yd, bs)                       # warm-up
        w = wall(lambda: sl.train_epoch(ms, opts, Xd, yd, bs), a.reps)
        rows[M] = (k, w)
        print(json.dumps({"row": "kernel", "M": M, "launch_ms": round(k[0], 4), "launch_ms_min_max": [round(k[1], 4), round(k[2], 4)],
                          "train_epoch_wall_ms": round(w[0], 3), "train_epoch_wall_ms_min_max": [round(w[1], 3), round(w[2], 3)]}))
    (m,), (o,) = models(1)
    loader = DataLoader(TensorDataset(X, y), batch_size=bs, shuffle=True)
    sl._train_model_eager(loader, m, nn.L1Loss(), o, torch.device(DEV))           # warm-up
    ea = wall(lambda: sl._train_model_eager(loader, m, nn.L1Loss(), o, torch.device(DEV)), a.reps)
    eager_device_epoch(m, o, Xd, yd, bs, nn.L1Loss())
    eb = wall(lambda: eager_device_epoch(m, o, Xd, yd, bs, nn.L1Loss()), a.reps)
    print(json.dumps({"row": "eager", "M": 1, "dataloader_epoch_ms": round(ea[0], 2), "dataloader_min_max": [round(ea[1], 2), round(ea[2], 2)],
                      "device_batches_epoch_ms": round(eb[0], 2), "device_batches_min_max": [round(eb[1], 2), round(eb[2], 2)]}))
    k1, w1 = rows[1]
    print(json.dumps({"row": "ratio", "M": 1,
                      "eager_dataloader_over_train_epoch_wall": round(ea[0] / w1[0], 1),
                      "eager_device_batches_over_train_epoch_wall": round(eb[0] / w1[0], 1),
                      "eager_device_batches_over_launch": round(eb[0] / k1[0], 1),
                      "M10_over_M1_launch": round(rows[10][0][0] / k1[0], 3), "M256_over_M1_launch": round(rows[256][0][0] / k1[0], 3),
                      "M10_over_M1_wall": round(rows[10][1][0] / w1[0], 3), "M256_over_M1_wall": round(rows[256][1][0] / w1[0], 3)}))
    if a.no_crossover:
        return
    n2 = 262144
    X2, y2 = samples(n2, seed=2)
    X2d, y2d = X2.to(DEV), y2.to(DEV)
    for b in (1024, 4096, 8192, 16384, 65536, 262144):
        (m,), (o,) = models(1)
        sl.train_epoch(m, o, X2d, y2d, b)
        kw = wall(lambda: sl.train_epoch(m, o, X2d, y2d, b), max(5, a.reps - 2))
        eager_device_epoch(m, o, X2d, y2d, b, nn.L1Loss())
        ew = wall(lambda: eager_device_epoch(m, o, X2d, y2d, b, nn.L1Loss()), max(5, a.reps - 2))
        print(json.dumps({"row": "crossover", "M": 1, "n": n2, "batch": b, "steps": n2 // b, "train_epoch_wall_ms": round(kw[0], 3),
                          "eager_device_batches_epoch_ms": round(ew[0], 3), "eager_over_kernel": round(ew[0] / kw[0], 2)}))


if __name__ == "__main__":
    main()
