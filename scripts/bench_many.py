"""M controllers side by side against a loop of M single-model steps, one JSON line per M.

The reference trains ten seeds of the controller, each at B = 15 (UL/Main.py:84, 297). Timed per optimizer step, at
H = 50, N = 10, B = 15:
  many        NeuralNetwork.train_models' body — bank(X), MPCLoss.forward_many, losses.sum().backward(), AdamW over the
              bank — eager, and replayed from one HIP graph (captured_models_step);
  loop        the best the library offered before: M single-model steps through train_model's body (the layer-pipelined
              kernels), eager, and each replayed from its own HIP graph (captured_step).
The arms alternate step by step in one process; each step is timed on its own (synchronised) and the medians of
--steps steps after warm-up are reported. The default run starts --procs fresh processes one after the other and
prints, per M, each process's medians and the median and spread (max - min) over the processes.
    python scripts/bench_many.py [--M 1 2 3 5 10 20 64] [--steps 25] [--procs 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("many_eager", "many_graphed", "loop_eager", "loop_graphed")


def child(Ms, steps, warmup):
    import numpy as np
    import torch

    import bench
    import forging_control_amd as fca
    from forging_control_amd.many import ControllerBank

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    seeds = np.load(os.path.join(ROOT, "tests", "golden", "ul_seed_controllers.npz"))
    B, N = 15, 10

    def controllers(M):
        sim, _ = bench.load_weights(dev, 50)
        out = []
        for m in range(M):
            c = fca.FNNModel(3, 50, 1, 1).to(dev)
            with torch.no_grad():
                c.fc_inp.weight.copy_(torch.as_tensor(seeds["W_inp"][m % 10]))
                c.fc_inp.bias.copy_(torch.as_tensor(seeds["b_inp"][m % 10]))
                c.fc_out.weight.copy_(torch.as_tensor(seeds["W_out"][m % 10]))
            out.append(c)
        return sim, out

    def one(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1000.0 * (time.perf_counter() - t0)

    for M in Ms:
        batches = [bench.synth_batch(B, dev, 7 + m) for m in range(M)]
        X, S = torch.stack([b[0] for b in batches]), torch.stack([b[1] for b in batches])
        fns = {}
        for graphed in (False, True):
            sim, ctrls = controllers(M)
            bank = ControllerBank.from_models(ctrls)
            loss_many = fca.MPCLoss(prediction_horizon=N, alpha=bench.ALPHA, many_min_models=1)
            opt = torch.optim.AdamW(bank.parameters(), lr=1e-4, capturable=True)
            if graphed:
                step = fca.NeuralNetwork.captured_models_step(sim, bank, loss_many, opt, dev)
                fns["many_graphed"] = lambda step=step: step(X, S)
            else:
                def many_eager(bank=bank, opt=opt, loss_many=loss_many, sim=sim):
                    opt.zero_grad()
                    losses, _ = loss_many.forward_many(sim, bank, X, bank(X), S, dev)
                    losses.sum().backward()
                    opt.step()
                fns["many_eager"] = many_eager
            sim, ctrls = controllers(M)
            loss_one = fca.MPCLoss(prediction_horizon=N, alpha=bench.ALPHA)
            opts = [torch.optim.AdamW(c.parameters(), lr=1e-4, capturable=True) for c in ctrls]
            if graphed:
                steps_m = [fca.NeuralNetwork.captured_step(sim, c, loss_one, o, dev) for c, o in zip(ctrls, opts)]

                def loop_graphed(steps_m=steps_m):
                    for m, st in enumerate(steps_m):
                        st(X[m], S[m])
                fns["loop_graphed"] = loop_graphed
            else:
                def loop_eager(ctrls=ctrls, opts=opts, loss_one=loss_one, sim=sim):
                    for m, (c, o) in enumerate(zip(ctrls, opts)):
                        o.zero_grad()
                        loss, _ = loss_one(sim, c, X[m], c(X[m]), S[m], dev)
                        loss.backward()
                        o.step()
                fns["loop_eager"] = loop_eager
        for _ in range(warmup):
            for a in ARMS:
                fns[a]()
        times = {a: [] for a in ARMS}
        for _ in range(steps):      # the arms alternate step by step
            for a in ARMS:
                times[a].append(one(fns[a]))
        families = (loss_one.last_call.forward, loss_many.last_call.route)
        print(json.dumps({"M": M, "B": B, "N": N, "H": 50, "steps": steps, "loop_family": families[0],
                          "many_route": families[1],
                          "median_ms": {a: statistics.median(times[a]) for a in ARMS}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="*", default=[1, 2, 3, 5, 10, 20, 64])
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.M, args.steps, args.warmup)
    runs = []
    for p in range(args.procs):   # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup",
                            str(args.warmup), "--M"] + [str(m) for m in args.M], capture_output=True, text=True, timeout=900)
        if r.returncode:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"process {p} failed with exit status {r.returncode}")
        rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        for row in rows:
            print(json.dumps({"process": p, **row}), flush=True)
        runs.append({row["M"]: row["median_ms"] for row in rows})
    for M in args.M:
        med = {a: statistics.median(r[M][a] for r in runs) for a in ARMS}
        spread = {a: max(r[M][a] for r in runs) - min(r[M][a] for r in runs) for a in ARMS}
        print(json.dumps({"summary": True, "M": M, "median_ms": med, "spread_ms": spread,
                          "loop_over_many_eager": med["loop_eager"] / med["many_eager"],
                          "loop_over_many_graphed": med["loop_graphed"] / med["many_graphed"],
                          "many_wins_graphed": med["loop_graphed"] - med["many_graphed"] > spread["loop_graphed"]}), flush=True)


if __name__ == "__main__":
    main()
