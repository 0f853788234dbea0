"""ctypes binding of the C ABI in include/fcr.h (libfcr.so, built for gfx950).

The library is the only compute path of this package: if it is missing or fails to load, every
entry point raises — there is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes
import os
import sys
import threading

import torch

_LIB_NAME = "libfcr.so"
_HERE = os.path.dirname(os.path.abspath(__file__))
_IN_TREE = os.path.join(_HERE, "lib", _LIB_NAME)
# FCR_LIB: another build of the same ABI (A/B timing, scripts/inject_stale_lo.sh's fault-injected build). A development
# switch only: it takes effect together with FCR_DEV=1 (load() refuses FCR_LIB without it and says on stderr which
# library it loaded when it is honoured); the in-tree library otherwise.
LIB_PATH = os.environ.get("FCR_LIB") or _IN_TREE

FCR_OK = 0
# 8: fcr_feasibility + fcr_feasibility_project; fcr_closed_loop gains feasibility / u_nn / feas_flag (NULL = off).
# fcr_supervised + fcr_supervised_epoch are a pure addition to it (no existing call or struct changed), so the number stays.
ABI_VERSION = 8
PRECISION_FP32, PRECISION_F16 = 0, 1
ERRORS = {-1: "FCR_EINVAL", -2: "FCR_EWORKSPACE", -3: "FCR_EHIP", -4: "FCR_EUNSUPPORTED"}

# Every symbol include/fcr.h declares (tests check the .so exports exactly these).
EXPORTS = ("fcr_workspace_size", "fcr_wide_kept_windows", "fcr_forward", "fcr_backward", "fcr_lstm_workspace_size",
           "fcr_lstm_forward", "fcr_lstm_backward", "fcr_plant_rk4", "fcr_closed_loop_run", "fcr_window_gather",
           "fcr_fnn_workspace_size", "fcr_fnn_forward", "fcr_fnn_backward", "fcr_set_small_batch_limit",
           "fcr_get_small_batch_limit", "fcr_set_small_pipe_limit", "fcr_get_small_pipe_limit", "fcr_set_small_pipe_sets",
           "fcr_get_small_pipe_sets", "fcr_set_wide_keep_budget", "fcr_get_wide_keep_budget", "fcr_last_error",
           "fcr_abi_version", "fcr_wide_bwd_cell_workspace", "fcr_wide_bwd_cell", "fcr_lstm_rollout_workspace_size",
           "fcr_lstm_rollout", "fcr_feasibility_project", "fcr_supervised_epoch", "fcr_many_workspace_size",
           "fcr_forward_many", "fcr_backward_many", "fcr_fnn_forward_many", "fcr_fnn_backward_many",
           "fcr_closed_loop_run_bank", "fcr_press_nominal", "fcr_plant_rk4_press", "fcr_feasibility_project_press",
           "fcr_closed_loop_run_bank_press", "fcr_loss_terms_default", "fcr_forward_terms", "fcr_backward_terms",
           "fcr_forward_many_terms", "fcr_backward_many_terms", "fcr_plant_rk4_vjp", "fcr_closed_loop_vjp_workspace_size",
           "fcr_closed_loop_vjp", "fcr_plant_rk4_vjp_press", "fcr_closed_loop_vjp_press",
           "fcr_press_grad_sum_workspace_size", "fcr_press_grad_sum", "fcr_closed_loop_bank_vjp_workspace_size",
           "fcr_closed_loop_bank_vjp", "fcr_closed_loop_bank_loss_vjp", "fcr_mpc_workspace_size", "fcr_mpc_solve",
           "fcr_mpc_closed_loop", "fcr_closed_loop_run_bank_press_state", "fcr_closed_loop_bank_vjp_noise",
           "fcr_closed_loop_bank_loss_vjp_noise", "fcr_lstm_rollout_backward_workspace_size", "fcr_lstm_rollout_backward")
LOSS_L1, LOSS_MSE = 0, 1
P1_MAX, P2_MAX = 2.122366, 1.036233   # the default upper pressure bounds (Functions.py:1411; csrc/fcr_common.h)


def default_terms_row(alpha):
    """fcr_loss_terms_default as a row (alpha, p1_lo, p1_hi, p2_lo, p2_hi, w_con)."""
    return (float(alpha), 0.0, P1_MAX, 0.0, P2_MAX, 1.0)
OPT_INHERIT, KEEP_AUTO = -2, -1
INT32_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1


class FcrDims(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("L", ctypes.c_int32), ("H", ctypes.c_int32),
        ("layers", ctypes.c_int32), ("in_dim", ctypes.c_int32), ("out_dim", ctypes.c_int32),
        ("ctrl_in", ctypes.c_int32), ("ctrl_hidden", ctypes.c_int32), ("alpha", ctypes.c_float),
        ("precision", ctypes.c_int32),
    ]


class FcrOptions(ctypes.Structure):
    """fcr_options (include/fcr.h): the per-call kernel options; `kernels` is written by each call."""
    _fields_ = [("small_batch_limit", ctypes.c_int32), ("kernels", ctypes.c_int32), ("wide_keep_budget", ctypes.c_int64)]


def make_options(small_batch_limit=None, wide_keep_budget=None) -> FcrOptions:
    """Per-call options: None inherits the process-wide default; wide_keep_budget "auto" = the library's policy."""
    keep = OPT_INHERIT if wide_keep_budget is None else KEEP_AUTO if wide_keep_budget == "auto" else int(wide_keep_budget)
    if wide_keep_budget is not None and not KEEP_AUTO <= keep <= INT64_MAX:
        raise ValueError(f"wide_keep_budget must be 0..2**63-1 bytes, 'auto' or None, got {wide_keep_budget!r}")
    small = OPT_INHERIT if small_batch_limit is None else int(small_batch_limit)
    # the fields are c_int32 / c_int64: a value outside them would wrap silently into INHERIT or 'never'
    if small_batch_limit is not None and not 0 <= small <= INT32_MAX:
        raise ValueError(f"small_batch_limit must be 0..2**31-1 or None, got {small_batch_limit!r}")
    return FcrOptions(small, 0, keep)


class FcrWeights(ctypes.Structure):
    _fields_ = [
        ("ctrl_w_inp", ctypes.c_void_p), ("ctrl_b_inp", ctypes.c_void_p), ("ctrl_w_out", ctypes.c_void_p),
        ("w_ih", ctypes.c_void_p * 3), ("w_hh", ctypes.c_void_p * 3),
        ("fc_w", ctypes.c_void_p), ("fc_b", ctypes.c_void_p),
    ]


class FcrLossTerms(ctypes.Structure):
    """fcr_loss_terms (include/fcr.h): the loss's alpha, pressure bounds, constraint weight and reference preview."""
    _fields_ = [
        ("alpha", ctypes.c_float), ("p1_lo", ctypes.c_float), ("p1_hi", ctypes.c_float), ("p2_lo", ctypes.c_float),
        ("p2_hi", ctypes.c_float), ("w_con", ctypes.c_float),
        ("ref", ctypes.c_void_p), ("ref_stride_b", ctypes.c_int64), ("ref_stride_j", ctypes.c_int64),
        ("table", ctypes.c_void_p), ("table_stride", ctypes.c_int64), ("ref_stride_m", ctypes.c_int64),
    ]


def make_loss_terms(row, ref=None, ref_strides=(0, 0, 0), table=None, table_stride=0) -> FcrLossTerms:
    """fcr_loss_terms from a row (alpha, p1_lo, p1_hi, p2_lo, p2_hi, w_con), a reference tensor (or None: X's column)
    with its (model, trajectory, step) element strides, and a device table of rows (or None) for the many calls."""
    t = FcrLossTerms(*[float(v) for v in row])
    if ref is not None:
        t.ref = ref.data_ptr()
        t.ref_stride_m, t.ref_stride_b, t.ref_stride_j = (int(s) for s in ref_strides)
    if table is not None:
        t.table = table.data_ptr()
        t.table_stride = int(table_stride)
    return t


class FcrWindows(ctypes.Structure):
    _fields_ = [
        ("rows", ctypes.c_int64), ("traj_len", ctypes.c_int32), ("lookback", ctypes.c_int32),
        ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32),
        ("X", ctypes.c_void_p), ("Y", ctypes.c_void_p), ("Z", ctypes.c_void_p),
    ]


class FcrFeasibility(ctypes.Structure):
    """fcr_feasibility (include/fcr.h): the parameters of the feasibility projection."""
    _fields_ = [
        ("p1_lo", ctypes.c_double), ("p1_hi", ctypes.c_double), ("p2_lo", ctypes.c_double), ("p2_hi", ctypes.c_double),
        ("u_lo", ctypes.c_double), ("u_hi", ctypes.c_double), ("ts", ctypes.c_double),
        ("substeps", ctypes.c_int32), ("expand", ctypes.c_int32), ("bisect", ctypes.c_int32),
    ]


class FcrClosedLoop(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32), ("T", ctypes.c_int32), ("ts", ctypes.c_double),
        ("substeps", ctypes.c_int32), ("smooth", ctypes.c_int32),
        ("x0", ctypes.c_void_p), ("ref", ctypes.c_void_p),
        ("ctrl_w_inp", ctypes.c_void_p), ("ctrl_b_inp", ctypes.c_void_p), ("ctrl_w_out", ctypes.c_void_p),
        ("ctrl_hidden", ctypes.c_int32), ("in_scale", ctypes.c_double * 2),
        ("ref_scale", ctypes.c_double), ("out_scale", ctypes.c_double),
        ("x", ctypes.c_void_p), ("u", ctypes.c_void_p),
        ("process_noise", ctypes.c_void_p), ("meas_noise", ctypes.c_void_p),   # (B,T,5) fp64 each, or NULL
        ("feasibility", ctypes.POINTER(FcrFeasibility)),                       # NULL = no recovery
        ("u_nn", ctypes.c_void_p), ("feas_flag", ctypes.c_void_p),             # (B,T) fp64 / int32, with feasibility
    ]


class FcrClosedLoopBank(ctypes.Structure):
    """fcr_closed_loop_bank (include/fcr.h): FcrClosedLoop's fields for M stacked controllers, then the bank's own."""
    _fields_ = FcrClosedLoop._fields_ + [
        ("n_models", ctypes.c_int32),
        ("x0_stride", ctypes.c_int64), ("ref_stride", ctypes.c_int64),         # elements between models; 0 = shared
        ("process_noise_stride", ctypes.c_int64), ("meas_noise_stride", ctypes.c_int64),
        ("p1_lo", ctypes.c_double), ("p1_hi", ctypes.c_double), ("p2_lo", ctypes.c_double), ("p2_hi", ctypes.c_double),
        ("traj_stats", ctypes.c_void_p), ("traj_counts", ctypes.c_void_p),     # (M,B,6) fp64, (M,B,3) int32
        ("x_final", ctypes.c_void_p), ("summary", ctypes.c_void_p),            # (M,B,5), (M,10) fp64
    ]


class FcrPress(ctypes.Structure):
    """fcr_press (include/fcr.h): the press and the workpiece, one row of a parameter table."""
    _fields_ = [(n, ctypes.c_double) for n in (
        "m_mass", "b_damp", "ft", "d1", "d2", "g", "kb", "v1_0", "v2_0", "kl_1", "kl_2", "cd", "rho", "d", "ps", "pt",
        "mu", "k", "w0", "h0", "b0", "t_def", "t1", "m0", "m1", "m2", "m3", "m4")]


class FcrClosedLoopGrad(ctypes.Structure):
    """fcr_closed_loop_grad (include/fcr.h): the closed loop's stored run and incoming gradients, and where its
    vector-Jacobian product goes."""
    _fields_ = [
        ("B", ctypes.c_int32), ("T", ctypes.c_int32), ("ts", ctypes.c_double),
        ("substeps", ctypes.c_int32), ("smooth", ctypes.c_int32), ("ref", ctypes.c_void_p),
        ("ctrl_w_inp", ctypes.c_void_p), ("ctrl_b_inp", ctypes.c_void_p), ("ctrl_w_out", ctypes.c_void_p),
        ("ctrl_hidden", ctypes.c_int32), ("in_scale", ctypes.c_double * 2),
        ("ref_scale", ctypes.c_double), ("out_scale", ctypes.c_double),
        ("x", ctypes.c_void_p), ("u", ctypes.c_void_p), ("g_x", ctypes.c_void_p), ("g_u", ctypes.c_void_p),
        ("press", ctypes.c_void_p), ("stride_traj", ctypes.c_int64),
        ("g_x0", ctypes.c_void_p), ("dv", ctypes.c_void_p),
        ("g_w_inp", ctypes.c_void_p), ("g_b_inp", ctypes.c_void_p), ("g_w_out", ctypes.c_void_p),   # fp64
    ]


class FcrClosedLoopBankGrad(ctypes.Structure):
    """fcr_closed_loop_bank_grad (include/fcr.h): the stored run of M stacked controllers and where its adjoint goes."""
    _fields_ = [
        ("n_models", ctypes.c_int32), ("B", ctypes.c_int32), ("T", ctypes.c_int32), ("ts", ctypes.c_double),
        ("substeps", ctypes.c_int32), ("smooth", ctypes.c_int32), ("ref", ctypes.c_void_p), ("ref_stride", ctypes.c_int64),
        ("ctrl_w_inp", ctypes.c_void_p), ("ctrl_b_inp", ctypes.c_void_p), ("ctrl_w_out", ctypes.c_void_p),
        ("ctrl_hidden", ctypes.c_int32), ("in_scale", ctypes.c_double * 2),
        ("ref_scale", ctypes.c_double), ("out_scale", ctypes.c_double),
        ("x", ctypes.c_void_p), ("u", ctypes.c_void_p),
        ("press", ctypes.c_void_p), ("stride_model", ctypes.c_int64), ("stride_traj", ctypes.c_int64),
        ("truncate", ctypes.c_int32),
        ("g_x0", ctypes.c_void_p), ("dv", ctypes.c_void_p),                                          # (M,B,5) or NULL, (M,B,T)
        ("g_w_inp", ctypes.c_void_p), ("g_b_inp", ctypes.c_void_p), ("g_w_out", ctypes.c_void_p),   # fp64, stacked
    ]


class FcrPressLoss(ctypes.Structure):
    """fcr_press_loss (include/fcr.h): the MPC loss on the press record — the terms table (device) and its host copy, the
    pressure scales, u_prev, and where cost (M,B) and loss (M) go."""
    _fields_ = [
        ("terms", ctypes.c_void_p), ("terms_stride", ctypes.c_int64), ("terms_host", ctypes.POINTER(ctypes.c_double)),
        ("p_scale", ctypes.c_double * 2), ("u_prev", ctypes.c_void_p), ("u_prev_stride", ctypes.c_int64),
        ("value_only", ctypes.c_int32), ("cost", ctypes.c_void_p), ("loss", ctypes.c_void_p),
    ]


class FcrBankNoise(ctypes.Structure):
    """fcr_bank_noise (include/fcr.h): the process noise of a noisy bank run (with its model stride) and the states the
    forward stored beside the record, as the noisy adjoints read them."""
    _fields_ = [("process_noise", ctypes.c_void_p), ("process_stride", ctypes.c_int64), ("x_state", ctypes.c_void_p)]


class FcrMpc(ctypes.Structure):
    """fcr_mpc (include/fcr.h): the shooting MPC's horizon, iteration count, integrator, weights and bounds."""
    _fields_ = [
        ("N", ctypes.c_int32), ("K", ctypes.c_int32), ("ts", ctypes.c_double),
        ("substeps", ctypes.c_int32), ("smooth", ctypes.c_int32),
        ("r_u", ctypes.c_double), ("lam0", ctypes.c_double), ("p_bounds", ctypes.c_double * 4),
        ("p_weight", ctypes.c_double), ("p_scale", ctypes.c_double), ("u_bounds", ctypes.c_double * 2),
    ]


class FcrMpcLoop(ctypes.Structure):
    """fcr_mpc_loop (include/fcr.h): the inputs and outputs of the MPC's closed loop."""
    _fields_ = [
        ("B", ctypes.c_int32), ("T", ctypes.c_int32), ("preview", ctypes.c_int32),
        ("x0", ctypes.c_void_p), ("ref", ctypes.c_void_p), ("u_init", ctypes.c_void_p), ("U0", ctypes.c_void_p),
        ("process_noise", ctypes.c_void_p), ("meas_noise", ctypes.c_void_p),
        ("plant", ctypes.c_void_p), ("plant_stride", ctypes.c_int64),
        ("model", ctypes.c_void_p), ("model_stride", ctypes.c_int64),
        ("x", ctypes.c_void_p), ("u", ctypes.c_void_p), ("cost", ctypes.c_void_p), ("grad_inf", ctypes.c_void_p),
        ("accepted", ctypes.c_void_p),
        ("plans", ctypes.c_void_p), ("trace", ctypes.c_void_p), ("trace_u", ctypes.c_void_p),
    ]


class FcrSupervised(ctypes.Structure):
    """fcr_supervised (include/fcr.h): one epoch of the supervised baseline for n_models stacked FNNModels."""
    _fields_ = [
        ("n_models", ctypes.c_int32), ("n_samples", ctypes.c_int32), ("batch_size", ctypes.c_int32),
        ("hidden", ctypes.c_int32), ("loss_kind", ctypes.c_int32), ("train", ctypes.c_int32),
        ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
        ("weight_decay", ctypes.c_double),
        ("X", ctypes.c_void_p), ("y", ctypes.c_void_p), ("perm", ctypes.c_void_p),           # (n,3), (n), (M,n) int32
        ("w_inp", ctypes.c_void_p), ("b_inp", ctypes.c_void_p), ("w_out", ctypes.c_void_p),  # (M,hidden,3), (M,hidden) x 2
        ("exp_avg_w_inp", ctypes.c_void_p), ("exp_avg_b_inp", ctypes.c_void_p), ("exp_avg_w_out", ctypes.c_void_p),
        ("exp_avg_sq_w_inp", ctypes.c_void_p), ("exp_avg_sq_b_inp", ctypes.c_void_p), ("exp_avg_sq_w_out", ctypes.c_void_p),
        ("step", ctypes.c_void_p), ("loss", ctypes.c_void_p),                                # (M) fp32, (M, n_batches)
    ]


class FcrLstmRolloutGrads(ctypes.Structure):
    """fcr_lstm_rollout_grads (include/fcr.h): where fcr_lstm_rollout_backward writes; g_window0 / g_cmd may be NULL."""
    _fields_ = [
        ("g_w_ih", ctypes.c_void_p * 3), ("g_w_hh", ctypes.c_void_p * 3), ("g_fc_w", ctypes.c_void_p),
        ("g_fc_b", ctypes.c_void_p), ("g_window0", ctypes.c_void_p), ("g_cmd", ctypes.c_void_p),
    ]


_vp, _i32, _i64, _sz, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double
_P = ctypes.POINTER
_dims, _po, _wts, _pt, _feas, _press = _P(FcrDims), _P(FcrOptions), _P(FcrWeights), _P(FcrLossTerms), _P(FcrFeasibility), _P(FcrPress)
# (symbol, restype, argtypes) of every call load() declares
_SIGNATURES = (
    ("fcr_workspace_size", _i32, [_dims, _po, _i32, _P(_sz)]),
    ("fcr_wide_kept_windows", _i32, [_dims, _sz, _P(ctypes.c_int32)]),
    ("fcr_forward", _i32, [_dims, _po, _wts] + [_vp] * 10 + [_i32, _vp, _sz, _vp]),
    ("fcr_backward", _i32, [_dims, _po] + [_vp] * 9 + [_sz, _vp]),
    ("fcr_plant_rk4", _i32, [_i32, _i32, _f64, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("fcr_lstm_workspace_size", _i32, [_dims, _i32, _P(_sz)]),
    ("fcr_lstm_forward", _i32, [_dims, _wts, _vp, _vp, _i32, _vp, _sz, _vp]),
    ("fcr_lstm_backward", _i32, [_dims, _wts, _vp, _P(_vp), _P(_vp), _vp, _vp, _vp, _vp, _sz, _vp]),
    ("fcr_lstm_rollout_workspace_size", _i32, [_dims, _P(_sz)]),
    ("fcr_lstm_rollout", _i32, [_dims, _wts, _vp, _vp, _P(ctypes.c_float), _vp, _vp, _vp, _sz, _vp]),
    ("fcr_lstm_rollout_backward_workspace_size", _i32, [_dims, _P(_sz)]),                # pure additions to ABI 8
    ("fcr_lstm_rollout_backward", _i32, [_dims, _wts, _vp, _vp, _P(ctypes.c_float), _vp, _vp, _P(FcrLstmRolloutGrads), _vp,
                                         _sz, _vp]),
    ("fcr_closed_loop_run", _i32, [_P(FcrClosedLoop), _vp]),
    ("fcr_closed_loop_run_bank", _i32, [_P(FcrClosedLoopBank), _vp]),            # a pure addition to ABI 8
    ("fcr_feasibility_project", _i32, [_feas, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fcr_supervised_epoch", _i32, [_P(FcrSupervised), _vp]),
    ("fcr_window_gather", _i32, [_P(FcrWindows), _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("fcr_fnn_workspace_size", _i32, [_i32, _i32, _P(_sz)]),
    ("fcr_fnn_forward", _i32, [_i32, _i32, _i32] + [_vp] * 6),
    ("fcr_fnn_backward", _i32, [_i32, _i32, _i32] + [_vp] * 10 + [_sz, _vp]),
    # M controllers side by side (a pure addition to ABI 8)
    ("fcr_many_workspace_size", _i32, [_dims, _po, _i32, _i32, _P(_sz)]),
    ("fcr_forward_many", _i32, [_dims, _po, _i32, _wts] + [_vp] * 10 + [_i32, _vp, _sz, _vp]),
    ("fcr_backward_many", _i32, [_dims, _po, _i32] + [_vp] * 9 + [_sz, _vp]),
    ("fcr_fnn_forward_many", _i32, [_i32, _i32, _i32, _i32] + [_vp] * 6),
    ("fcr_fnn_backward_many", _i32, [_i32, _i32, _i32, _i32] + [_vp] * 10 + [_sz, _vp]),
    ("fcr_set_small_batch_limit", _i32, [_i32]), ("fcr_get_small_batch_limit", _i32, []),
    ("fcr_set_small_pipe_limit", _i32, [_i32]), ("fcr_get_small_pipe_limit", _i32, []),
    ("fcr_set_small_pipe_sets", _i32, [_i32]), ("fcr_get_small_pipe_sets", _i32, []),
    ("fcr_set_wide_keep_budget", _i64, [_i64]), ("fcr_get_wide_keep_budget", _i64, []),
    ("fcr_last_error", ctypes.c_char_p, []), ("fcr_abi_version", _i32, []),
    ("fcr_wide_bwd_cell_workspace", _i32, [_i32, _i32, _i32, _P(_sz)]),
    ("fcr_wide_bwd_cell", _i32, [_i32, _i32, _i32] + [_vp] * 11 + [_sz, _vp]),
)
# Pure additions to ABI 8 that an FCR_LIB development build may predate, each under the symbol load() probes for: the press
# as data, the loss's terms as data, the differentiable press, its gradients with respect to the press parameters, training a
# bank on the press, the MPC baseline, training on the press under noise
_ADDITIONS = {
    "fcr_press_nominal": (
        ("fcr_press_nominal", None, [_press]),
        ("fcr_plant_rk4_press", _i32, [_i32, _i32, _f64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
        ("fcr_feasibility_project_press", _i32, [_feas, _press, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
        ("fcr_closed_loop_run_bank_press", _i32, [_P(FcrClosedLoopBank), _vp, _i64, _i64, _press, _vp]),
    ),
    "fcr_forward_terms": (
        ("fcr_loss_terms_default", None, [_pt, ctypes.c_float]),
        ("fcr_forward_terms", _i32, [_dims, _po, _wts, _pt] + [_vp] * 10 + [_i32, _vp, _sz, _vp]),
        ("fcr_backward_terms", _i32, [_dims, _po, _pt] + [_vp] * 9 + [_sz, _vp]),
        ("fcr_forward_many_terms", _i32, [_dims, _po, _i32, _wts, _pt] + [_vp] * 10 + [_i32, _vp, _sz, _vp]),
        ("fcr_backward_many_terms", _i32, [_dims, _po, _i32, _pt] + [_vp] * 9 + [_sz, _vp]),
    ),
    "fcr_plant_rk4_vjp": (
        ("fcr_plant_rk4_vjp", _i32, [_i32, _i32, _f64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
        ("fcr_closed_loop_vjp_workspace_size", _i32, [_i32, _i32, _i32, _P(_sz)]),
        ("fcr_closed_loop_vjp", _i32, [_P(FcrClosedLoopGrad), _vp, _sz, _vp]),
    ),
    "fcr_plant_rk4_vjp_press": (
        ("fcr_plant_rk4_vjp_press", _i32, [_i32, _i32, _f64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
        ("fcr_closed_loop_vjp_press", _i32, [_P(FcrClosedLoopGrad), _vp, _vp, _sz, _vp]),
        ("fcr_press_grad_sum_workspace_size", _i32, [_i32, _P(_sz)]),
        ("fcr_press_grad_sum", _i32, [_i32, _vp, _vp, _vp, _sz, _vp]),
    ),
    "fcr_closed_loop_bank_vjp": (                            # training a bank on the press
        ("fcr_closed_loop_bank_vjp_workspace_size", _i32, [_i32, _i32, _i32, _i32, _P(_sz)]),
        ("fcr_closed_loop_bank_vjp", _i32, [_P(FcrClosedLoopBankGrad), _vp, _vp, _vp, _sz, _vp]),
        ("fcr_closed_loop_bank_loss_vjp", _i32, [_P(FcrClosedLoopBankGrad), _P(FcrPressLoss), _vp, _sz, _vp]),
    ),
    "fcr_mpc_solve": (                                       # the MPC baseline on the press
        ("fcr_mpc_workspace_size", _i32, [_i32, _i32, _P(_sz)]),
        ("fcr_mpc_solve", _i32, [_P(FcrMpc), _i32, _vp, _vp, _vp, _vp, _vp, _i64] + [_vp] * 7 + [_vp, _sz, _vp]),
        ("fcr_mpc_closed_loop", _i32, [_P(FcrMpc), _P(FcrMpcLoop), _vp, _sz, _vp]),
    ),
    "fcr_closed_loop_bank_vjp_noise": (                      # training on the press under noise
        ("fcr_closed_loop_run_bank_press_state", _i32, [_P(FcrClosedLoopBank), _vp, _i64, _i64, _press, _vp, _vp]),
        ("fcr_closed_loop_bank_vjp_noise", _i32, [_P(FcrClosedLoopBankGrad), _P(FcrBankNoise), _vp, _vp, _vp, _sz, _vp]),
        ("fcr_closed_loop_bank_loss_vjp_noise", _i32,
         [_P(FcrClosedLoopBankGrad), _P(FcrBankNoise), _P(FcrPressLoss), _vp, _sz, _vp]),
    ),
}


class NativeError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def load() -> ctypes.CDLL:
    """Load libfcr.so once (raises NativeError with build instructions if absent)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if LIB_PATH != _IN_TREE:
            if os.environ.get("FCR_DEV") != "1":
                raise NativeError(f"FCR_LIB={LIB_PATH} names a development build; set FCR_DEV=1 to load it "
                                  "(unset FCR_LIB for the in-tree library)")
            sys.stderr.write(f"forging_control_amd: FCR_LIB development build {LIB_PATH}\n")
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no fallback path.")
        lib = ctypes.CDLL(LIB_PATH)
        for probe, rows in [(None, _SIGNATURES)] + list(_ADDITIONS.items()):
            # An FCR_LIB development build of ABI 8 from before an addition (an A/B timing against an earlier commit)
            # loads without it; the calls it lacks then raise AttributeError.
            if probe is None or LIB_PATH == _IN_TREE or hasattr(lib, probe):
                for name, restype, argtypes in rows:
                    fn = getattr(lib, name)
                    fn.restype, fn.argtypes = restype, argtypes
        if lib.fcr_abi_version() != ABI_VERSION:
            raise NativeError(f"libfcr ABI {lib.fcr_abi_version()} != expected {ABI_VERSION}")
        _lib = lib
        return lib


def check(rc: int, what: str) -> None:
    if rc != FCR_OK:
        msg = load().fcr_last_error().decode(errors="replace")
        raise NativeError(f"{what} failed ({ERRORS.get(rc, rc)}): {msg}")


def stream(device) -> ctypes.c_void_p:
    """The current HIP stream of ``device``, as the ``void *stream`` every launching call takes."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def set_small_batch_limit(max_batch: int) -> int:
    """fcr_set_small_batch_limit: the process-wide DEFAULT small-batch limit (B <= it runs the small-batch kernels,
    0 = never) of calls whose options inherit it; returns the old value. Per call: MPCLoss(small_batch_limit=...)."""
    return int(load().fcr_set_small_batch_limit(int(max_batch)))


def small_batch_limit() -> int:
    """The process-wide default small-batch limit (fcr_get_small_batch_limit: read-only)."""
    return int(load().fcr_get_small_batch_limit())


def set_small_pipe_limit(max_batch: int) -> int:
    """fcr_set_small_pipe_limit: B <= it (and <= 32 groups) runs the small-batch family's layer-pipelined geometry
    (csrc/fcr_pipe.h), 0 = never; process-wide; returns the old value."""
    return int(load().fcr_set_small_pipe_limit(int(max_batch)))


def small_pipe_limit() -> int:
    """The process-wide layer-pipelined small-batch limit (fcr_get_small_pipe_limit: read-only)."""
    return int(load().fcr_get_small_pipe_limit())


def set_small_pipe_sets(sets: int) -> int:
    """fcr_set_small_pipe_sets: caps the pipelined geometry's window sets (forward <= 4, backward <= 3; 0 = the most
    that fit); process-wide; returns the old value. Results are bit-identical for every value."""
    return int(load().fcr_set_small_pipe_sets(int(sets)))


def small_pipe_sets() -> int:
    """The process-wide window-set setting (fcr_get_small_pipe_sets: read-only; 0 = automatic)."""
    return int(load().fcr_get_small_pipe_sets())


def set_wide_keep_budget(nbytes: int) -> int:
    """fcr_set_wide_keep_budget (H > 52): the process-wide DEFAULT bytes of kept windows a backward-enabled workspace
    may add, so their backward skips the recompute (< 0 = the library's policy: half the device memory free at its
    first sizing, at most 40 % of the device; 0 = none); returns the old budget. Per call: MPCLoss(wide_keep_budget=...)."""
    return int(load().fcr_set_wide_keep_budget(int(nbytes)))


def wide_keep_budget() -> int:
    """The process-wide default keep budget (fcr_get_wide_keep_budget: read-only)."""
    return int(load().fcr_get_wide_keep_budget())


KERNEL_FAMILIES = {0: None, 1: "small", 2: "fused", 3: "wide"}


def workspace_bytes(dims: FcrDims, with_backward: bool, opts: FcrOptions | None = None) -> int:
    out = ctypes.c_size_t(0)
    check(load().fcr_workspace_size(ctypes.byref(dims), ctypes.byref(opts) if opts is not None else None,
                                    int(bool(with_backward)), ctypes.byref(out)), "fcr_workspace_size")
    return int(out.value)


def many_workspace_bytes(dims: FcrDims, n_models: int, with_backward: bool, opts: FcrOptions | None = None) -> int:
    """fcr_many_workspace_size: scratch of fcr_forward_many (+ fcr_backward_many) for n_models models of shape dims."""
    out = ctypes.c_size_t(0)
    check(load().fcr_many_workspace_size(ctypes.byref(dims), ctypes.byref(opts) if opts is not None else None,
                                         int(n_models), int(bool(with_backward)), ctypes.byref(out)),
          "fcr_many_workspace_size")
    return int(out.value)


def kept_windows(dims: FcrDims, ws_bytes: int) -> int:
    """fcr_wide_kept_windows: windows (of N) a backward-enabled H > 52 workspace of ws_bytes keeps."""
    out = ctypes.c_int32(0)
    check(load().fcr_wide_kept_windows(ctypes.byref(dims), int(ws_bytes), ctypes.byref(out)), "fcr_wide_kept_windows")
    return int(out.value)
