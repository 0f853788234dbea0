"""The reach rule of the fused H <= 52 backward (csrc/fcr_bwd.h), pinned in fp64 torch on the CPU.

Only u0 (row 9 of window 0) and the appended rows (xhat_j, u_{j+1}) carry a gradient; in window j they sit at
positions t_lo(j) = max(0, 9 - j) .. 9, and the rows before them are the caller's `states`. An LSTM cell at step t
sends gradient only to rows s <= t and to the (frozen) weights, so cutting the graph in front of row t_lo(j) of every
window (rows [0, t_lo) under no_grad, their (h, c) carried into rows [t_lo, 10)) must leave the gradients of u0 and of
the three controller tensors what the untruncated rollout (oracle.rollout_torch) gives, and cutting one row later must
not: the bound is tight.
"""
import numpy as np
import pytest
import torch

from conftest import load_case, relerr
from oracle import rollout_np as R
from oracle import rollout_torch as TT
from tests.golden.make_golden import synth_inputs

KL = 10
GRADS = ("g_u0", "g_W_inp", "g_b_inp", "g_W_out")
B = 4
ALPHA = 20.0


def t_lo(j):
    return max(0, KL - 1 - j)


class TruncatedSim:
    """The surrogate as mpc_loss calls it, once per window j = 0, 1, ...: rows [0, t_lo(j) + extra) without a graph."""

    def __init__(self, sim, extra):
        self.sim, self.extra, self.j = sim, extra, 0

    def __call__(self, window):
        cut = min(KL, t_lo(self.j) + self.extra)
        self.j += 1
        sim = self.sim
        zeros = window.new_zeros(sim.layers, window.shape[0], sim.hidden)
        state = (zeros, zeros)
        if cut > 0:
            with torch.no_grad():
                hseq, state = sim.lstm(window[:, :cut], state)
            if cut == KL:
                return sim.fc(hseq[:, -1, :])
        hseq, _ = sim.lstm(window[:, cut:], state)
        return sim.fc(hseq[:, -1, :])


def truncated_grads(params, X, u0, S, N, extra):
    sim, ctrl = TT.build_modules(params, torch.float64, lstm_requires_grad=False)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    u0_t = t(u0).reshape(-1, 1).clone().requires_grad_(True)
    loss, _ = TT.mpc_loss(TruncatedSim(sim, extra), ctrl, t(X), u0_t, t(S), N, ALPHA)
    loss.backward()
    g = lambda p: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy()
    return {"g_u0": u0_t.grad.reshape(-1).numpy(), "g_W_inp": g(ctrl.fc_inp.weight), "g_b_inp": g(ctrl.fc_inp.bias),
            "g_W_out": g(ctrl.fc_out.weight)}


@pytest.fixture(scope="module")
def ref_params():
    return load_case("ref_b15_n10")[1]


@pytest.mark.parametrize("N", [1, 2, 3, 9, 10, 11, 12])
def test_cells_before_t_lo_carry_no_gradient(ref_params, N):
    X, S, _ = synth_inputs(B, N, 900 + N)
    u0, _ = R.fnn_forward(np.asarray(X, np.float64), ref_params["W_inp"], ref_params["b_inp"], ref_params["W_out"])
    full = TT.loss_and_grads(ref_params, X, u0, S, N, ALPHA, dtype=torch.float64)
    cut = truncated_grads(ref_params, X, u0, S, N, 0)
    for k in GRADS:
        assert relerr(cut[k], full[k]) <= 1e-12, (N, k, relerr(cut[k], full[k]))
    # one row further drops the cell that reads the first row with a gradient: the bound is tight
    over = truncated_grads(ref_params, X, u0, S, N, 1)
    assert not relerr(over["g_u0"], full["g_u0"]) <= 1e-12, (N, relerr(over["g_u0"], full["g_u0"]))
