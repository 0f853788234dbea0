"""Generator of tests/golden/ul_seed_controllers.npz: the ten seeds of the unsupervised controller the reference ships
(``Unsupervised Learning/results/NN_controller_N_10_{0..9}.pt``, state_dicts of FNNModel(3, 50, 1, 1)) as plain float32
arrays stacked over the seed — W_inp (10,50,3), b_inp (10,50), W_out (10,1,50); fc_int, which a width_dim = 1
controller never evaluates, is left out.
    python tests/golden/make_ul_seed_controllers.py REFERENCE_ROOT
Only this script reads the reference; the tests read the .npz."""
import os
import sys

import numpy as np
import torch

KEYS = {"W_inp": "fc_inp.weight", "b_inp": "fc_inp.bias", "W_out": "fc_out.weight"}


def main(ref_root):
    results = os.path.join(ref_root, "Unsupervised Learning", "results")
    sds = [torch.load(os.path.join(results, f"NN_controller_N_10_{i}.pt"), map_location="cpu", weights_only=True)
           for i in range(10)]
    out = {k: np.stack([sd[name].numpy().astype(np.float32) for sd in sds]) for k, name in KEYS.items()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ul_seed_controllers.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
