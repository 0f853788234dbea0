"""The forward-record contract of the H <= 52 rollout (csrc/fcr_rollout.hip at small_limit_of): a fused forward with
with_backward = 1 writes, in window j, the h and c records of t >= t_lo(j) - 1 only (t_lo = max(0, 9 - j)); the records
before them stay holes of the workspace, and every backward family — fused, one-workgroup small-batch, layer-pipelined
— reads written records only.

The C ABI is driven with a workspace the test owns (MPCLoss allocates its own inside the call). Each case runs the
forward and every backward family the shape reaches twice: on a workspace pre-filled with byte 0xFF (a NaN as f16 and
as fp32) and on one pre-filled with zeros. A backward that reads a hole gives a non-finite gradient, a gradient off
the fp64 oracle (oracle/rollout_np.py), or one that differs between the two fills; where the cell that read it is one no
gradient reaches (the small-batch and pipelined backwards run those too), what it wrote into the workspace differs
between the two fills.

Shapes: B = 24 is two 16-trajectory groups, the second ragged. N = 1 and 3 are the deepest truncations (N = 1: every
phase is one cell), N = 10 ends on the first full window, N = 12 has full windows after the truncated ones. The
tolerances are the parity tests': 1e-5 (tests/test_gpu_parity.py) in the fp32-accurate mode, the f16 mode's stated
gradient tolerance (tests/test_gpu_precision.py) in the f16 mode.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
from conftest import load_case, relerr
from oracle import rollout_np as R
from test_gpu_parity import DEV, GRADS, TOL, _synth, _u0
from test_gpu_precision import TOL_GRADS

pytestmark = pytest.mark.gpu
native = fca._native
BIG = 1 << 30
B = 24
FILLS = (0xFF, 0x00)


@functools.lru_cache(maxsize=None)
def _case(H, N):
    """Parameters, inputs and the fp64 oracle's gradients of one shape: computed once, shared, never changed."""
    from tests.golden.make_golden import synth_params
    params = load_case("ref_b15_n10")[1] if H == 50 else synth_params(H, 2100 + H)
    X, S, _ = _synth(B, N, 2200 + H + N)
    u0 = _u0(params, X)
    _, _, tape = R.rollout_forward(params, X, u0, S, N, 20.0)
    return params, X, u0, S, R.rollout_backward(params, tape)


class _Call:
    """fcr_forward / fcr_backward on one caller-owned workspace."""

    def __init__(self, H, N, precision):
        self.lib = native.load()
        params, X, u0, S, self.oracle = _case(H, N)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)), device=DEV)
        self.N = N
        self.X, self.u0, self.S = d(X), d(u0).reshape(B, 1), d(S)
        self.keep = {k: d(params[k]) for k in ("W_inp", "b_inp", "W_out", "fcW", "fcb")}
        self.keep.update({f"Wih{k}": d(params["Wih"][k]) for k in range(3)})
        self.keep.update({f"Whh{k}": d(params["Whh"][k]) for k in range(3)})
        self.hidden = params["W_inp"].shape[0]
        self.dims = fca.rollout.make_dims(B, N, H, 3, self.hidden, 20.0, precision=precision)
        w = native.FcrWeights()
        w.ctrl_w_inp, w.ctrl_b_inp, w.ctrl_w_out = (self.keep[k].data_ptr() for k in ("W_inp", "b_inp", "W_out"))
        for k in range(3):
            w.w_ih[k] = self.keep[f"Wih{k}"].data_ptr()
            w.w_hh[k] = self.keep[f"Whh{k}"].data_ptr()
        w.fc_w, w.fc_b = self.keep["fcW"].data_ptr(), self.keep["fcb"].data_ptr()
        self.w = w
        # one workspace layout for every family (csrc/fcr_rollout.hip): the largest size any option asks for
        nbytes = max(native.workspace_bytes(self.dims, True, native.make_options(lim)) for lim in (0, BIG))
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.out = {k: torch.empty(s, **f32) for k, s in dict(loss=(), cost=B, command=B, error=B, pred=B * N,
                                                              xhat=(B, N, 4)).items()}
        self.dl = torch.ones(1, **f32)

    def forward(self, fill, small_limit):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        self.ws.fill_(fill)
        opts = native.make_options(small_limit)
        o = self.out
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        native.check(self.lib.fcr_forward(ctypes.byref(self.dims), ctypes.byref(opts), ctypes.byref(self.w), p(self.X),
                                          p(self.u0), p(self.S), None, p(o["loss"]), p(o["cost"]), p(o["command"]),
                                          p(o["error"]), p(o["pred"]), p(o["xhat"]), 1, p(self.ws), self.ws.numel(), st),
                     "fcr_forward")
        torch.cuda.synchronize()
        self.after_forward = self.ws.clone()   # every backward starts from the workspace as the forward left it
        return native.KERNEL_FAMILIES[opts.kernels]

    def backward(self, small_limit):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        self.ws.copy_(self.after_forward)
        opts = native.make_options(small_limit)
        f32 = dict(dtype=torch.float32, device=DEV)
        g = {"g_u0": torch.empty(B, 1, **f32), "g_W_inp": torch.empty(self.hidden, 3, **f32),
             "g_b_inp": torch.empty(self.hidden, **f32), "g_W_out": torch.empty(1, self.hidden, **f32)}
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        native.check(self.lib.fcr_backward(ctypes.byref(self.dims), ctypes.byref(opts), p(self.X), p(self.S),
                                           p(self.out["pred"]), p(self.dl), p(g["g_u0"]), p(g["g_W_inp"]),
                                           p(g["g_b_inp"]), p(g["g_W_out"]), p(self.ws), self.ws.numel(), st),
                     "fcr_backward")
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in g.items()}
        out["g_u0"] = out["g_u0"].reshape(-1)
        out["workspace"] = self.ws.cpu().numpy()   # as the forward and this backward left it
        return native.KERNEL_FAMILIES[opts.kernels], out


def _with_pipe_limit(lim, fn):
    prev = native.set_small_pipe_limit(lim)
    try:
        return fn()
    finally:
        native.set_small_pipe_limit(prev)


# backward families: (name, small_batch_limit, small_pipe_limit, family the call must report)
FUSED = ("fused", 0, 512, "fused")
SMALL = ("small", BIG, 0, "small")
PIPE = ("pipelined", BIG, 512, "small")


def _check(call, got, tol, tag, workspace=True):
    """got: {fill: {backward name: gradients and the workspace}}"""
    for name in got[FILLS[0]]:
        for k, _ in GRADS:
            a, z = got[FILLS[0]][name][k], got[FILLS[1]][name][k]
            assert np.isfinite(a).all() and np.isfinite(z).all(), (tag, name, k, "non-finite")
            ea, ez = relerr(a, call.oracle[k]), relerr(z, call.oracle[k])
            print(f"{tag} {name} {k}: relerr 0xFF fill {ea:.3e}, zero fill {ez:.3e}")
            assert ea <= tol and ez <= tol, (tag, name, k, ea, ez)
            assert np.array_equal(a, z), (tag, name, k, "differs between the 0xFF and the zero fill")
        if not workspace:
            continue
        # Nothing either pass WROTE depends on the fill: the two workspaces differ only in bytes no kernel touched,
        # which still hold their fills. The small-batch and pipelined backwards also run the cells no gradient
        # reaches, whose results leave the gradients alone but land in the workspace (the d hand-off records, the
        # window-row gradients): recomputed from a hole they would differ here.
        a, z = got[FILLS[0]][name]["workspace"], got[FILLS[1]][name]["workspace"]
        d = a != z
        stale = int(np.count_nonzero(d & ((a != FILLS[0]) | (z != FILLS[1]))))
        print(f"{tag} {name}: {int(d.sum())} of {a.size} workspace bytes never written, {stale} written from a hole")
        assert stale == 0, (tag, name, stale, "workspace bytes written from an unwritten record")


FWD_CASES = ([(H, N, "fp32", (FUSED, SMALL, PIPE)) for H in (50, 32) for N in (1, 3, 10, 12)]
             + [(12, 3, "fp32", (FUSED,))] + [(50, N, "f16", (FUSED,)) for N in (3, 10)])


@pytest.mark.parametrize("H,N,precision,backwards", FWD_CASES, ids=[f"H{c[0]}-N{c[1]}-{c[2]}" for c in FWD_CASES])
def test_every_backward_reads_only_what_the_fused_forward_wrote(H, N, precision, backwards):
    call = _Call(H, N, fca.rollout.PRECISIONS[precision])
    got = {}
    for fill in FILLS:
        assert call.forward(fill, 0) == "fused"
        got[fill] = {}
        for name, small, pipe, family in backwards:
            fam, g = _with_pipe_limit(pipe, lambda: call.backward(small))
            assert fam == family, (name, fam)
            got[fill][name] = g
    _check(call, got, TOL if precision == "fp32" else TOL_GRADS, f"H{H} N{N} {precision} fused forward,")


@pytest.mark.parametrize("H", [50, 32])
@pytest.mark.parametrize("N", [1, 3, 10, 12])
def test_fused_backward_after_the_small_forward(H, N):
    """The small-batch forward writes every record; the fused backward reads its subset, whatever the holes held."""
    call = _Call(H, N, native.PRECISION_FP32)
    got = {}
    for fill in FILLS:
        assert _with_pipe_limit(0, lambda: call.forward(fill, BIG)) == "small"
        fam, g = call.backward(0)
        assert fam == "fused"
        got[fill] = {"fused": g}
    # (no workspace comparison here: the fused backward launches whole workgroups of eight waves, and the padding waves
    # recompute from slab regions only a fused forward's padding waves write; their results belong to no trajectory)
    _check(call, got, TOL, f"H{H} N{N} fp32 small forward,", workspace=False)
