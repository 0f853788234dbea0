"""Record the CPU yardstick of the press fit (tests/golden/press_fit_cpu.json):
    python tests/golden/make_press_fit_cpu.py
L-BFGS on the log-multipliers of CD, M0 and KB, on the fp64 torch restatement (tests/press_param_torch.py: fit_inputs,
fit_cpu), B = 16 trajectories of S = 12 steps, smooth model, true multipliers 0.85 / 0.9 / 1.1. The file keeps the
per-field errors |multiplier / true - 1| and loss / loss0; tests/test_press_param_grad_host.py reproduces them within a
factor 3, and tests/test_gpu_press_param_grad.py holds plant.fit_press on the GPU against them."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import press_param_torch as pp  # noqa: E402

if __name__ == "__main__":
    x_obs, U = pp.fit_inputs()
    r = pp.fit_cpu(x_obs, U)
    out = {"B": 16, "S": 12, "smooth": True, "fields": list(pp.FIT_FIELDS), "true": list(pp.FIT_TRUE),
           "multipliers": r["multipliers"], "errors": pp.fit_errors(r["multipliers"]), "loss0": r["loss0"],
           "loss": r["loss"], "loss_ratio": r["loss"] / r["loss0"], "evals": r["evals"]}
    with open(os.path.join(HERE, pp.FIT_GOLDEN), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
