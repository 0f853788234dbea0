"""fp64 references for the surrogate's differentiable free run (TEST INFRASTRUCTURE ONLY; not a test module).

* :func:`autograd_free_run` — the free run end to end under autograd: the window cloned, cmd[:,0] written in place into
  its last row, the shifts by torch.cat, on ``oracle.surrogate_torch.build``'s model.
* :func:`recursion` — the reverse written out as the kernels run it: per step ȳ_t = G_t + gain ⊙ P_t[0:4], one window's
  backward by autograd (weight gradients and the row gradients R_t), and R_t's rows credited to the generated rows P_s,
  to window0 or to cmd. ``mutant`` breaks it in one of four ways (MUTANTS).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import surrogate_torch as S

KEYS = ("Wih0", "Wih1", "Wih2", "Whh0", "Whh1", "Whh2", "fcW", "fcb", "window0", "cmd")
MUTANTS = ("no_gain", "late_credit", "no_expiry", "cmd0_in_window")


def params_of(w):
    """load_weights' flat dict -> the oracle's parameter dict, float64."""
    return {"Wih": [np.asarray(w[f"Wih{k}"], np.float64) for k in range(3)],
            "Whh": [np.asarray(w[f"Whh{k}"], np.float64) for k in range(3)],
            "fcW": np.asarray(w["fcW"], np.float64), "fcb": np.asarray(w["fcb"], np.float64)}


def inputs(B, T, seed):
    """window0 and cmd drawn as test_surrogate.batch draws windows (uniform, pressures in [0, 1.1]), targets and a
    normal cotangent G."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1, 1, (B, 10, 5))
    w[..., 1:3] = rng.uniform(0, 1.1, (B, 10, 2))
    return {"window0": w, "cmd": rng.uniform(-1, 1, (B, T)), "target": rng.uniform(-1, 1, (B, T, 4)),
            "G": rng.standard_normal((B, T, 4))}


def _weights(m):
    return [getattr(m.lstm, f"weight_ih_l{k}") for k in range(3)] + \
           [getattr(m.lstm, f"weight_hh_l{k}") for k in range(3)] + [m.fc.weight, m.fc.bias]


def _t(a):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float64))


def free_run(m, window0, cmd, gain, noise):
    """x̂ (B,T,4) on torch tensors, differentiable."""
    win = window0.clone()
    win[:, 9, 4] = cmd[:, 0]
    out = []
    for t in range(cmd.shape[1]):
        if t > 0:
            row = torch.cat([gain * out[-1], cmd[:, t:t + 1]], dim=1)
            win = torch.cat([win[:, 1:], row[:, None, :]], dim=1)
        y = m(win)
        out.append(y if noise is None else y + noise[:, t])
    return torch.stack(out, dim=1)


def autograd_free_run(params, window0, cmd, gain=None, noise=None, G=None, target=None):
    """{'xhat', 'loss', every key of KEYS} as float64 numpy; loss = sum(G * x̂), or MSE against target."""
    m = S.build(params)
    w0, c = _t(window0).requires_grad_(True), _t(cmd).requires_grad_(True)
    g = torch.ones(4, dtype=torch.float64) if gain is None else _t(gain)
    xhat = free_run(m, w0, c, g, _t(noise))
    loss = (xhat * _t(G)).sum() if G is not None else torch.nn.functional.mse_loss(xhat, _t(target))
    grads = torch.autograd.grad(loss, _weights(m) + [w0, c])
    out = {k: v.numpy() for k, v in zip(KEYS, grads)}
    out["xhat"], out["loss"] = xhat.detach().numpy(), float(loss.detach())
    return out


def recursion(params, window0, cmd, gain=None, noise=None, G=None, mutant=None):
    """The gradients of sum(G * x̂) by the ring recursion; keys as KEYS."""
    assert mutant is None or mutant in MUTANTS
    m = S.build(params)
    wts = _weights(m)
    w0, c, G = _t(window0), _t(cmd), _t(G)
    g = torch.ones(4, dtype=torch.float64) if gain is None else _t(gain)
    B, T = c.shape
    with torch.no_grad():
        windows, win, nz = [], w0.clone(), _t(noise)
        win[:, 9, 4] = c[:, 0]
        for t in range(T):
            if t > 0:
                win = torch.cat([win[:, 1:], torch.cat([g * xh, c[:, t:t + 1]], dim=1)[:, None, :]], dim=1)
            windows.append(win)
            xh = m(win) if nz is None else m(win) + nz[:, t]
    P = torch.zeros(B, T, 5, dtype=torch.float64)        # P[:, s]: the row generated at step s
    g_w0 = torch.zeros(B, 10, 5, dtype=torch.float64)
    g_cmd = torch.zeros(B, T, dtype=torch.float64)
    g_wts = [torch.zeros_like(p) for p in wts]
    for t in range(T - 1, -1, -1):
        ybar = G[:, t] + (P[:, t, :4] if mutant == "no_gain" else g * P[:, t, :4])
        W = windows[t].clone().requires_grad_(True)
        grads = torch.autograd.grad(m(W), [W] + wts, grad_outputs=ybar)
        for acc, gi in zip(g_wts, grads[1:]):
            acc += gi
        R = grads[0]
        if mutant == "no_expiry" and t - 11 >= 0:          # the row that left after W_{t-1} still takes row 0's gradient
            P[:, t - 11] += R[:, 0]
        for j in range(10):
            s = t - 10 + j
            if s >= 0:
                s = s + 1 if mutant == "late_credit" else s
                if s < T:
                    P[:, s] += R[:, j]
            elif j + t == 9:                                # window0's last row: its command was overwritten by cmd[0]
                g_w0[:, 9, :4] += R[:, j, :4]
                if mutant == "cmd0_in_window":
                    g_w0[:, 9, 4] += R[:, j, 4]
                else:
                    g_cmd[:, 0] += R[:, j, 4]
            else:
                g_w0[:, j + t] += R[:, j]
    g_cmd[:, 1:] = P[:, :T - 1, 4]
    return {k: v.numpy() for k, v in zip(KEYS, g_wts + [g_w0, g_cmd])}


def rel(a, b):
    """max|a - b| / max|b| (0 / 0 = 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.abs(b).max() if b.size else 0.0
    num = np.abs(a - b).max() if b.size else 0.0
    return 0.0 if num == 0.0 else num / den if den > 0 else np.inf
