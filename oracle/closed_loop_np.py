"""NumPy restatement of the batched closed loop (TEST INFRASTRUCTURE ONLY).

Per step, as NeuralNetwork.loop (Functions.py:1116-1200), with the harness's pre-drawn noise and a projection of the
command (its feasibility recovery) as options:
NN_make_step (Functions.py:1594-1604) — MaxAbs-scaled [y_dot, z, ref] in fp64 (the reference column by
scalers['y_dot']), the FNN in float32 (Linear+ReLU, Linear without bias, Hardtanh; the kernel's FMA order),
unscaled by scalers['output'] in float32 — then the plant step of oracle/plant_np.py (RK4 of
Functions.py:1743-1781). PARITY STATUS: composed of restatements pinned elsewhere (plant_np: the
reference's traces; the FNN: the rollout oracle's fixtures); the loop order follows the reference.
"""
from __future__ import annotations

import numpy as np

from .plant_np import rk4_step


def _fma32(a, b, c):
    """float32 fused multiply-add: the float32 x float32 product is exact in float64, the sum is rounded
    once to float64 and then to float32 (a double rounding that differs from fmaf only in vanishingly
    rare ties)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def controller_u(x, ref, W_inp, b_inp, W_out, in_scale, ref_scale, out_scale):
    """u = scalers['output'].inverse_transform(FNN(float32(X_new))) (Functions.py:1594-1604), the float32
    dot products accumulated in the kernel's order (one FMA chain per hidden unit, then over units) so the
    closed loop is compared free of summation-order noise."""
    f32 = np.float32
    s0 = (x[:, 1] / in_scale[0]).astype(f32)
    s1 = (x[:, 4] / in_scale[1]).astype(f32)
    s2 = (ref / ref_scale).astype(f32)
    W_inp, b_inp, W_out = W_inp.astype(f32), b_inp.astype(f32), W_out.astype(f32)
    v = np.zeros_like(s0)
    for j in range(W_inp.shape[0]):
        z = _fma32(np.full_like(s0, W_inp[j, 0]), s0, np.full_like(s0, b_inp[j]))
        z = _fma32(np.full_like(s0, W_inp[j, 1]), s1, z)
        z = _fma32(np.full_like(s0, W_inp[j, 2]), s2, z)
        v = _fma32(np.full_like(s0, W_out[0, j]), np.maximum(z, f32(0)), v)
    v = np.clip(v, f32(-1), f32(1))
    return (v * f32(out_scale)).astype(np.float64)


def closed_loop(x0, ref, W_inp, b_inp, W_out, in_scale, ref_scale, out_scale, ts=1e-3, substeps=4, smooth=True,
                process_noise=None, meas_noise=None, project=None):
    """x (B,T+1,5), u (B,T). One step: the controller reads the record m = x + meas_noise[:, t-1] (x0 at t = 0), the
    plant steps the unperturbed state x under process_noise[:, t] (rk4_step's ``w``), the new record is x[:, t+1].
    ``project(m, x, u_nn) -> (u, flag)`` stands between the controller and the press (the harness's feasibility
    recovery, tests/feasibility_np.py); with it the result is x, u, u_nn (B,T), flag (B,T)."""
    x = m = np.asarray(x0, np.float64)
    B, T = ref.shape
    xs, us, un, fl = np.empty((B, T + 1, 5)), np.empty((B, T)), np.empty((B, T)), np.zeros((B, T), np.int32)
    xs[:, 0] = x
    for t in range(T):
        u = un[:, t] = controller_u(m, ref[:, t], W_inp, b_inp, W_out, in_scale, ref_scale, out_scale)
        if project is not None:
            u, fl[:, t] = project(m, x, u)
        x = rk4_step(x, u, ts, substeps, smooth, None if process_noise is None else process_noise[:, t])
        m = x if meas_noise is None else x + meas_noise[:, t]
        us[:, t] = u
        xs[:, t + 1] = m
    return (xs, us) if project is None else (xs, us, un, fl)
