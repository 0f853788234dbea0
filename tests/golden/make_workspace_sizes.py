"""Workspace sizes the library's host-side size queries return, as a fixture: a refactor of the host code must leave
every workspace layout's total byte-identical (the offsets inside it are sums of the same slabs in the same order).

    python tests/golden/make_workspace_sizes.py        # rewrites tests/golden/workspace_sizes.json

The queries run on the host (no GPU). The H > 52 rollout sizes are taken at explicit keep budgets only: the default
budget asks the device for its free memory. tests/test_workspace_sizes.py compares measure() with the file."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "workspace_sizes.json")

ROLLOUT = [(15, 10, 50), (1, 5, 50), (1000, 3, 50), (8208, 2, 50), (48, 4, 40), (33, 3, 7), (513, 2, 50), (129, 2, 64),
           (300, 2, 264), (110, 1, 256)]
KEEP_BUDGETS = (0, 1 << 40)
LSTM = [(256, 50), (1, 50), (33, 7), (100, 64), (110, 256), (300, 264)]
CELL_HOOK = [(300, 64, 0), (129, 200, 1), (300, 256, 1)]


def measure() -> dict:
    """{case name: bytes (or kept windows)} from the built library."""
    import forging_control_amd as fca
    n = fca._native
    lib = n.load()
    out = {}
    for B, N, H in ROLLOUT:
        for precision in ((0, 1) if H == 50 else (0,)):
            d = fca.rollout.make_dims(B, N, H, 3, 50, 20.0, precision=precision)
            tag = f"rollout B={B} N={N} H={H}" + (" f16" if precision else "")
            if H <= 52:
                out[f"{tag} fwd"] = n.workspace_bytes(d, False)
                out[f"{tag} bwd"] = n.workspace_bytes(d, True)
                continue
            for budget in KEEP_BUDGETS:
                o = n.make_options(wide_keep_budget=budget)
                out[f"{tag} keep={budget} fwd"] = n.workspace_bytes(d, False, o)
                out[f"{tag} keep={budget} bwd"] = nbytes = n.workspace_bytes(d, True, o)
                out[f"{tag} keep={budget} kept"] = n.kept_windows(d, nbytes)
    for B, H in LSTM:
        d = fca.rollout.make_dims(B, 1, H, 3, 1, 0.0)
        for wb in (0, 1):
            nbytes = ctypes.c_size_t(0)
            n.check(lib.fcr_lstm_workspace_size(ctypes.byref(d), wb, ctypes.byref(nbytes)), "fcr_lstm_workspace_size")
            out[f"lstm B={B} H={H} {'bwd' if wb else 'fwd'}"] = int(nbytes.value)
    for B, H, layer0 in CELL_HOOK:
        nbytes = ctypes.c_size_t(0)
        n.check(lib.fcr_wide_bwd_cell_workspace(B, H, layer0, ctypes.byref(nbytes)), "fcr_wide_bwd_cell_workspace")
        out[f"cell hook B={B} H={H} layer0={layer0}"] = int(nbytes.value)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    with open(PATH, "w") as f:
        json.dump(measure(), f, indent=1)
        f.write("\n")
    print("wrote", PATH)
