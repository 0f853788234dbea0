"""GPU: the fused H <= 52 backward (csrc/fcr_bwd.h) forms only the dx tiles in the last cell of a phase (DX_ONLY): the
FIRST cell at t = 0, or the truncated-last cell at t_lo >= 1, whose dh_prev and dc nothing consumes.

The fused kernels are forced (small_batch_limit = 0) on a workspace the test owns (tests/test_gpu_record_contract.py's
way): once pre-filled with byte 0xFF (a NaN as f16 and as fp32) and once with zeros. A value the skipped tiles no
longer form, read anywhere, would make the gradients non-finite, differ between the two fills, or leave the fp64 oracle
(oracle/rollout_torch.py, the parity tests' 1e-5). The small-batch backward, which runs every cell in full, is held to
the same oracle beside it (the reach tests put the two families within 2e-6 of each other, not bit-equal).

B = 16, 17, 130: one full group, a ragged second one, and a second workgroup (eight groups each) with a ragged last
group. N = 1: every phase is its truncated-last cell alone; N = 2, 3: truncated-last cells behind one and two generic
ones; N = 10 ends on the first full window (FIRST cells); N = 12 has full windows past j = 9. H = 16, 32, 50: one case
per slot tier (HS = 4, 8, 13: the shared tile holds 4, 4 and 1 dx slots in layers >= 1)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
from conftest import load_case, relerr
from oracle import rollout_torch as T
from test_gpu_parity import DEV, GRADS, TOL, _synth, _u0

pytestmark = pytest.mark.gpu
native = fca._native
BIG = 1 << 30
FILLS = (0xFF, 0x00)
ALPHA = 20.0


@functools.lru_cache(maxsize=None)
def _case(H, B, N):
    """Parameters, inputs and the fp64 oracle's gradients of one shape: computed once, shared, never changed."""
    from tests.golden.make_golden import synth_params
    params = load_case("ref_b15_n10")[1] if H == 50 else synth_params(H, 6100 + H)
    X, S, _ = _synth(B, N, 6200 + H + 13 * B + N)
    u0 = _u0(params, X)
    return params, X, u0, S, T.loss_and_grads(params, X, u0, S, N, ALPHA, dtype=torch.float64)


class _Call:
    """fcr_forward / fcr_backward on one caller-owned workspace."""

    def __init__(self, H, B, N):
        self.lib = native.load()
        params, X, u0, S, self.oracle = _case(H, B, N)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)), device=DEV)
        self.B, self.N = B, N
        self.X, self.u0, self.S = d(X), d(u0).reshape(B, 1), d(S)
        self.keep = {k: d(params[k]) for k in ("W_inp", "b_inp", "W_out", "fcW", "fcb")}
        self.keep.update({f"Wih{k}": d(params["Wih"][k]) for k in range(3)})
        self.keep.update({f"Whh{k}": d(params["Whh"][k]) for k in range(3)})
        self.hidden = params["W_inp"].shape[0]
        self.dims = fca.rollout.make_dims(B, N, H, 3, self.hidden, ALPHA, precision=native.PRECISION_FP32)
        w = native.FcrWeights()
        w.ctrl_w_inp, w.ctrl_b_inp, w.ctrl_w_out = (self.keep[k].data_ptr() for k in ("W_inp", "b_inp", "W_out"))
        for k in range(3):
            w.w_ih[k] = self.keep[f"Wih{k}"].data_ptr()
            w.w_hh[k] = self.keep[f"Whh{k}"].data_ptr()
        w.fc_w, w.fc_b = self.keep["fcW"].data_ptr(), self.keep["fcb"].data_ptr()
        self.w = w
        nbytes = max(native.workspace_bytes(self.dims, True, native.make_options(lim)) for lim in (0, BIG))
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.out = {k: torch.empty(s, **f32) for k, s in dict(loss=(), cost=B, command=B, error=B, pred=B * N,
                                                              xhat=(B, N, 4)).items()}
        self.dl = torch.ones(1, **f32)

    def run(self, fill, small_limit):
        """Forward and backward of one family on the workspace pre-filled with ``fill``."""
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        B, o = self.B, self.out
        self.ws.fill_(fill)
        opts = native.make_options(small_limit)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        native.check(self.lib.fcr_forward(ctypes.byref(self.dims), ctypes.byref(opts), ctypes.byref(self.w), p(self.X),
                                          p(self.u0), p(self.S), None, p(o["loss"]), p(o["cost"]), p(o["command"]),
                                          p(o["error"]), p(o["pred"]), p(o["xhat"]), 1, p(self.ws), self.ws.numel(), st),
                     "fcr_forward")
        fwd = native.KERNEL_FAMILIES[opts.kernels]
        f32 = dict(dtype=torch.float32, device=DEV)
        g = {"g_u0": torch.empty(B, 1, **f32), "g_W_inp": torch.empty(self.hidden, 3, **f32),
             "g_b_inp": torch.empty(self.hidden, **f32), "g_W_out": torch.empty(1, self.hidden, **f32)}
        opts = native.make_options(small_limit)
        native.check(self.lib.fcr_backward(ctypes.byref(self.dims), ctypes.byref(opts), p(self.X), p(self.S),
                                           p(o["pred"]), p(self.dl), p(g["g_u0"]), p(g["g_W_inp"]),
                                           p(g["g_b_inp"]), p(g["g_W_out"]), p(self.ws), self.ws.numel(), st),
                     "fcr_backward")
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in g.items()}
        out["g_u0"] = out["g_u0"].reshape(-1)
        return (fwd, native.KERNEL_FAMILIES[opts.kernels]), out


CASES = [(50, B, N) for B in (16, 17, 130) for N in (1, 2, 3, 10, 12)] + [(16, 17, 3), (16, 17, 10), (32, 17, 3), (32, 17, 10)]


@pytest.mark.parametrize("H,B,N", CASES, ids=[f"H{h}-B{b}-N{n}" for h, b, n in CASES])
def test_last_cells_form_only_dx(H, B, N):
    call = _Call(H, B, N)
    got = {}
    for fill in FILLS:
        fam, got[fill] = call.run(fill, 0)
        assert fam == ("fused", "fused"), fam
    small = got[FILLS[1]]   # H = 16: the small-batch family starts at the HS = 8 tier, so there is no second family
    if H >= 32:
        fam, small = call.run(0x00, BIG)
        assert fam == ("small", "small"), fam
    for k, _ in GRADS:
        a, z = got[FILLS[0]][k], got[FILLS[1]][k]
        assert np.isfinite(a).all() and np.isfinite(z).all(), (k, "non-finite")
        ea, ez, es = relerr(a, call.oracle[k]), relerr(z, call.oracle[k]), relerr(small[k], call.oracle[k])
        print(f"last cell H{H} B{B} N{N} {k}: fused relerr 0xFF fill {ea:.3e}, zero fill {ez:.3e}; small-batch {es:.3e}; "
              f"fused vs small-batch {relerr(a, small[k]):.3e}")
        assert ea <= TOL and ez <= TOL and es <= TOL, (k, ea, ez, es)
        assert np.array_equal(a, z), (k, "differs between the 0xFF and the zero fill")
