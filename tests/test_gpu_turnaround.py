"""The fused H <= 52 backward's window turn-around (csrc/fcr_bwd.h): the layer-2 image refill is started
(lds_fill_begin) before the window head's loads and arithmetic and awaited (lds_fill_end) after them, and the
row-gradient sum is a fixed, unrolled run of kL terms (csrc/fcr_rowgrad.h). Nothing the kernel computes changes with
that; what can go wrong is a head that reads the region being refilled, a refill that is not awaited, a clamped row
term that is added after all, or a wrong window in the sum. Every case forces the fused family (small_batch_limit=0)
in more than one workgroup: B = 145 is workgroup 0 full (eight waves of 16 trajectories) and workgroup 1 with two
waves, the second padded (one trajectory). The forward is checked beside it: its outputs are the backward's inputs.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import forging_control_amd as fca
from conftest import load_case, relerr
from oracle import rollout_np as R
from test_gpu_parity import DEV, FEATS, GRADS, TOL, _synth, _u0, run
from test_gpu_precision import TOL_FEATS, TOL_GRADS, TOL_LOSS

pytestmark = pytest.mark.gpu
native = fca._native
FUSED = ("fused", "fused")
BIG = 1 << 30
B = 145


@functools.lru_cache(maxsize=None)
def _case(N):
    """Inputs and the fp64 oracle of one horizon: computed once, shared, never changed."""
    params = load_case("ref_b15_n10")[1]
    X, S, _ = _synth(B, N, 3100 + N)
    u0 = _u0(params, X)
    loss, f, tape = R.rollout_forward(params, X, u0, S, N, 20.0)
    return params, X, u0, S, float(loss), f, R.rollout_backward(params, tape)


@pytest.mark.parametrize("N", [1, 2, 3, 10, 12])
def test_two_workgroups_ragged(N):
    """N = 1: no row-gradient term inside the window loop, only the closing one; N = 2, 3: rows with fewer windows than
    terms (clamped terms trail); N = 10: every truncation depth; N = 12: rows whose oldest window is not window 0."""
    params, X, u0, S, loss64, f, g = _case(N)
    o = run(params, X, u0, S, N, 20.0, small_batch_limit=0)
    assert o["families"] == FUSED
    for k in FEATS + ("xhat",):
        e = relerr(o[k], f[k])
        print(f"N={N} {k}: fused vs oracle {e:.3e}")
        assert e <= TOL, (N, k, e)
    for k, _n in GRADS:
        e = relerr(o[k], g[k])
        print(f"N={N} {k}: fused vs oracle {e:.3e}")
        assert e <= TOL, (N, k, e)
    s = run(params, X, u0, S, N, 20.0, small_batch_limit=BIG)
    assert s["families"] == ("small", "small")
    for k in FEATS + ("xhat",) + tuple(k for k, _n in GRADS):
        e = relerr(o[k], s[k])
        print(f"N={N} {k}: fused vs small-batch {e:.3e}")
        assert e <= 2e-6, (N, k, e)


@pytest.mark.parametrize("name", ["h16_b33_n4", "h32_b16_n6"])
def test_tiers(name):
    """HS = 4 (H = 16) and HS = 8 (H = 32): their own image sizes, hence their own refill chunk counts."""
    c, params = load_case(name)
    o = run(params, c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"], small_batch_limit=0)
    assert o["families"] == FUSED
    for k in ("loss", "prediction", "xhat") + tuple(k for k, _n in GRADS):
        e = relerr(o[k], c[f"{k}_64"])
        print(f"{name} {k}: {e:.3e}")
        assert e <= TOL, (name, k, e)


@pytest.mark.parametrize("N", [3, 10])
def test_f16_mode(N):
    """No refill in this mode: the head's batched loads and the unrolled row sum alone."""
    params, X, u0, S, loss64, f, g = _case(N)
    o = run(params, X, u0, S, N, 20.0, small_batch_limit=0, precision="f16")
    assert o["families"] == FUSED
    assert abs(o["loss_scalar"] - loss64) <= TOL_LOSS * abs(loss64)
    for k in FEATS + ("xhat",):
        assert relerr(o[k], f[k]) <= TOL_FEATS, (N, k, relerr(o[k], f[k]))
    for k, _n in GRADS:
        assert relerr(o[k], g[k]) <= TOL_GRADS, (N, k, relerr(o[k], g[k]))


def test_noise():
    """The golden case with measurement noise on every step's xhat, which the backward's head reads."""
    c, params = load_case("refnoise_b15_n10")
    o = run(params, c["X"], c["u0"], c["states"], c["N"], c["alpha"], c["noise"], small_batch_limit=0)
    assert o["families"] == FUSED
    for k in ("loss", "prediction", "xhat") + tuple(k for k, _n in GRADS):
        e = relerr(o[k], c[f"{k}_64"])
        assert e <= TOL, (k, e)


class _Call:
    """fcr_forward + fcr_backward (fused family, fp32 mode) on one caller-owned workspace; every output as bytes."""

    def __init__(self, N):
        self.lib = native.load()
        params, X, u0, S = _case(N)[:4]
        d = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)), device=DEV)
        self.N = N
        self.X, self.u0, self.S = d(X), d(u0).reshape(B, 1), d(S)
        self.keep = {k: d(params[k]) for k in ("W_inp", "b_inp", "W_out", "fcW", "fcb")}
        self.keep.update({f"Wih{k}": d(params["Wih"][k]) for k in range(3)})
        self.keep.update({f"Whh{k}": d(params["Whh"][k]) for k in range(3)})
        self.hidden = params["W_inp"].shape[0]
        self.dims = fca.rollout.make_dims(B, N, 50, 3, self.hidden, 20.0, precision=0)
        w = native.FcrWeights()
        w.ctrl_w_inp, w.ctrl_b_inp, w.ctrl_w_out = (self.keep[k].data_ptr() for k in ("W_inp", "b_inp", "W_out"))
        for k in range(3):
            w.w_ih[k] = self.keep[f"Wih{k}"].data_ptr()
            w.w_hh[k] = self.keep[f"Whh{k}"].data_ptr()
        w.fc_w, w.fc_b = self.keep["fcW"].data_ptr(), self.keep["fcb"].data_ptr()
        self.w = w
        self.opts = native.make_options(0)
        self.ws = torch.empty(native.workspace_bytes(self.dims, True, self.opts), dtype=torch.uint8, device=DEV)
        self.dl = torch.ones(1, dtype=torch.float32, device=DEV)

    def __call__(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        f32 = dict(dtype=torch.float32, device=DEV)
        N = self.N
        o = {k: torch.empty(s, **f32) for k, s in dict(loss=(), cost=B, command=B, error=B, pred=B * N,
                                                       xhat=(B, N, 4), g_u0=(B, 1), g_W_inp=(self.hidden, 3),
                                                       g_b_inp=self.hidden, g_W_out=(1, self.hidden)).items()}
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        native.check(self.lib.fcr_forward(ctypes.byref(self.dims), ctypes.byref(self.opts), ctypes.byref(self.w),
                                          p(self.X), p(self.u0), p(self.S), None, p(o["loss"]), p(o["cost"]),
                                          p(o["command"]), p(o["error"]), p(o["pred"]), p(o["xhat"]), 1, p(self.ws),
                                          self.ws.numel(), st), "fcr_forward")
        assert native.KERNEL_FAMILIES[self.opts.kernels] == "fused"
        native.check(self.lib.fcr_backward(ctypes.byref(self.dims), ctypes.byref(self.opts), p(self.X), p(self.S),
                                           p(o["pred"]), p(self.dl), p(o["g_u0"]), p(o["g_W_inp"]), p(o["g_b_inp"]),
                                           p(o["g_W_out"]), p(self.ws), self.ws.numel(), st), "fcr_backward")
        assert native.KERNEL_FAMILIES[self.opts.kernels] == "fused"
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def test_repeats_and_workspace_fills_are_bit_equal():
    """A refill that lands late, or a head that reads the refilled region, races: it shows as a difference between
    repeats of one call, or between a workspace pre-filled with NaN bytes and one pre-filled with zeros."""
    call = _Call(10)
    call.ws.fill_(0xFF)
    first = call()
    for k, v in first.items():
        assert np.isfinite(v).all(), k
    for rep in range(1, 20):
        again = call()
        for k, v in first.items():
            assert np.array_equal(v.view(np.uint32), again[k].view(np.uint32)), (rep, k)
    call.ws.fill_(0x00)
    zero = call()
    for k, v in first.items():
        assert np.isfinite(zero[k]).all(), k
        assert np.array_equal(v.view(np.uint32), zero[k].view(np.uint32)), (k, "differs between the fills")
    g = _case(10)[6]
    for k, _n in GRADS:
        assert relerr(first[k].reshape(np.shape(g[k])), g[k]) <= TOL, (k, relerr(first[k].reshape(np.shape(g[k])), g[k]))
