// fcr_train.hip — C ABI of training a bank of controllers on the press (fcr_press_train.h): the
// adjoint of the closed loop for M models under incoming gradients (fcr_closed_loop_bank_vjp) or under the MPC loss
// evaluated on the record (fcr_closed_loop_bank_loss_vjp), their workspace query, and both on a run made under pre-drawn
// noise (fcr_closed_loop_bank_vjp_noise, fcr_closed_loop_bank_loss_vjp_noise; §7.18: the same function with one more
// argument, the reverse launch being fcr_press_noise.hip's). Validation before any device call,
// by the checks the press rows share (fcr_press_host.h); stream-ordered launches; no allocation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr.h"
#include "fcr_host.h"
#include "fcr_plant.h"
#include "fcr_press_host.h"

// fcr_press_grad.h's non-template kernels have external host stubs and are compiled into fcr_grad.hip; this unit reads
// the header for its __device__ functions only, so here those kernels get internal linkage (no second host stub under
// the same name) and are never launched.
#pragma push_macro("__global__")
#undef __global__
#define __global__ static __attribute__((global))
#include "fcr_press_grad.h"
#pragma pop_macro("__global__")

#include "fcr_press_noise_host.h"
#include "fcr_press_train.h"

using namespace fcr;

namespace {

constexpr int kMaxModels = 65535;   // the model is blockIdx.y

template <bool TABLE>
using Press = std::conditional_t<TABLE, plant::Coeffs, plant::Nominal>;

int cost_blocks(int B) { return (B + press_grad::kGradBlock - 1) / press_grad::kGradBlock; }

size_t param_workspace(int M, int B, int T, int hidden) {
    return align_up((size_t)M * press_grad::param_blocks((long long)B * T) * hidden * 5 * sizeof(double));
}

size_t bank_workspace(int M, int B, int T, int hidden) {
    return param_workspace(M, B, T, hidden) + align_up((size_t)M * cost_blocks(B) * sizeof(double));
}

int check_models(const char *who, int M, int B, int T) {
    if (M < 0) return fail(FCR_EINVAL, "%s: n_models=%d must be >= 0", who, M);
    if (M > kMaxModels) return fail(FCR_EUNSUPPORTED, "%s: n_models=%d: built for 0..%d", who, M, kMaxModels);
    if ((long long)M * B * (T + 1) * 5 > (1LL << 40)) return fail(FCR_EINVAL, "%s: n_models*B*(T+1) too large", who);
    return FCR_OK;
}

// the fused loss's own arguments, the terms rows included (read from the host copy)
int check_loss(const char *who, const fcr_press_loss *l, int M, int B) {
    if (!(l->p_scale[0] > 0.0) || !(l->p_scale[1] > 0.0) || l->p_scale[0] - l->p_scale[0] != 0.0 ||
        l->p_scale[1] - l->p_scale[1] != 0.0)
        return fail(FCR_EINVAL, "%s: p_scale=(%g, %g) must be positive and finite", who, l->p_scale[0], l->p_scale[1]);
    if (l->terms_stride != 0 && l->terms_stride < 6)
        return fail(FCR_EINVAL, "%s: terms_stride=%lld must be 0 (one row for all models) or >= 6", who, (long long)l->terms_stride);
    if (l->u_prev_stride != 0 && l->u_prev_stride < B)
        return fail(FCR_EINVAL, "%s: u_prev_stride=%lld must be 0 (shared) or >= B", who, (long long)l->u_prev_stride);
    if (!l->u_prev && l->u_prev_stride)
        return fail(FCR_EINVAL, "%s: u_prev_stride=%lld without u_prev", who, (long long)l->u_prev_stride);
    if (M == 0) return FCR_OK;
    if (!l->terms_host) return fail(FCR_EINVAL, "%s: terms_host is NULL", who);
    const int rows = l->terms_stride ? M : 1;
    for (int m = 0; m < rows; ++m) {
        const double *r = l->terms_host + (size_t)m * 6;
        for (int i = 0; i < 6; ++i)
            if (r[i] != r[i]) return fail(FCR_EINVAL, "%s: terms row %d holds a NaN (field %d)", who, m, i);
        if (r[0] - r[0] != 0.0) return fail(FCR_EINVAL, "%s: terms row %d: alpha=%g must be finite", who, m, r[0]);
        if (r[1] > r[2] || r[3] > r[4])
            return fail(FCR_EINVAL, "%s: terms row %d: a lower bound is above its upper bound (p1 %g..%g, p2 %g..%g)", who, m,
                        r[1], r[2], r[3], r[4]);
        if (!(r[5] >= 0.0) || r[5] - r[5] != 0.0)
            return fail(FCR_EINVAL, "%s: terms row %d: weight=%g must be finite and >= 0", who, m, r[5]);
    }
    return FCR_OK;
}

// the noisy run's own arguments (fcr_bank_noise): where the adjoint reads the process noise and the forward's states
int check_noise(const char *who, const fcr_bank_noise *n, int B, int T) {
    if (!n) return fail(FCR_EINVAL, "%s: noise is NULL", who);
    if (n->process_stride < 0 || (n->process_stride && n->process_stride < (long long)B * T * 5))
        return fail(FCR_EINVAL, "%s: process_stride=%lld must be 0 (shared) or >= B * T * 5 = %lld", who,
                    (long long)n->process_stride, (long long)B * T * 5);
    if (!n->process_noise && n->process_stride)
        return fail(FCR_EINVAL, "%s: process_stride=%lld without process_noise", who, (long long)n->process_stride);
    if ((((uintptr_t)n->process_noise) | ((uintptr_t)n->x_state)) & 7)
        return fail(FCR_EINVAL, "%s: process_noise and x_state must be 8-byte aligned (fp64)", who);
    return FCR_OK;
}

// the entry points under their own names: l = NULL is the general product (g_x, g_u), else the fused loss; noisy: the
// adjoint of the run under pre-drawn noise (nz; fcr_press_noise.hip's kernels), everything else as without
int bank_vjp(const char *who, const fcr_closed_loop_bank_grad *c, const double *g_x, const double *g_u,
             const fcr_press_loss *l, bool fused, void *ws, size_t ws_bytes, void *stream,
             const fcr_bank_noise *nz = nullptr, bool noisy = false) {
    if (const int rc = check_loop(who, c, press_grad::kMaxHidden, true)) return rc;
    if (noisy)
        if (const int rc = check_noise(who, nz, c->B, c->T)) return rc;
    if (const int rc = check_models(who, c->n_models, c->B, c->T)) return rc;
    if (const int rc = check_table_strides(who, c->stride_model, c->stride_traj, c->B)) return rc;
    if (const int rc = check_table_pointer(who, c->press, false, c->stride_traj)) return rc;
    if (!c->press && c->stride_model)
        return fail(FCR_EINVAL, "%s: stride_model=%lld without a parameter table", who, (long long)c->stride_model);
    if (c->ref_stride < 0 || (c->ref_stride && c->ref_stride < (long long)c->B * c->T))
        return fail(FCR_EINVAL, "%s: ref_stride=%lld must be 0 (shared) or >= B * T = %lld", who, (long long)c->ref_stride,
                    (long long)c->B * c->T);
    if (c->truncate < 0) return fail(FCR_EINVAL, "%s: truncate=%d must be >= 0 (0 = none)", who, c->truncate);
    if (fused && !l) return fail(FCR_EINVAL, "%s: loss is NULL", who);
    if (fused)
        if (const int rc = check_loss(who, l, c->n_models, c->B)) return rc;
    const int M = c->n_models, B = c->B, T = c->T, H = c->ctrl_hidden;
    if (M == 0) return FCR_OK;
    const bool value_only = fused && l->value_only;
    const bool rows = B > 0 && T > 0;
    if (!value_only && (!c->g_w_inp || !c->g_b_inp || !c->g_w_out)) {
        if (B == 0 && !(fused && l->loss)) return FCR_OK;      // an empty batch with nothing to zero
        if (B > 0) return fail(FCR_EINVAL, "%s: a parameter gradient is NULL", who);
    }
    if (B > 0 && (!c->x || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (B > 0 && fused && (!l->terms || !l->cost || !l->loss)) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (B > 0 && !fused && !g_x) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (rows && (!c->ref || !c->u || (!value_only && !c->dv) || (!fused && !g_u)))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    uintptr_t bits = ((uintptr_t)c->x) | ((uintptr_t)c->u) | ((uintptr_t)c->ref) | ((uintptr_t)g_x) | ((uintptr_t)g_u) |
                     ((uintptr_t)c->g_x0) | ((uintptr_t)c->dv) | ((uintptr_t)c->g_w_inp) | ((uintptr_t)c->g_b_inp) |
                     ((uintptr_t)c->g_w_out);
    if (fused) bits |= ((uintptr_t)l->terms) | ((uintptr_t)l->u_prev) | ((uintptr_t)l->cost) | ((uintptr_t)l->loss);
    if (bits & 7) return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    const size_t need = bank_workspace(M, B, T, H);
    if (need && !ws) return fail(FCR_EINVAL, "%s: the workspace is NULL", who);
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "%s: the workspace has %zu bytes, %zu are needed", who, ws_bytes, need);
    if (((uintptr_t)ws) & 7) return fail(FCR_EINVAL, "%s: the workspace must be 8-byte aligned", who);

    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)ws, *cost_part = (double *)((char *)ws + param_workspace(M, B, T, H));
    press_train::BankGradArgs a{M, B, T, c->substeps, H, c->truncate, c->ts / c->substeps, c->ref, (long long)c->ref_stride,
                                c->ctrl_w_inp, c->ctrl_b_inp, c->ctrl_w_out, c->in_scale[0], c->in_scale[1], c->ref_scale,
                                c->out_scale, c->x, c->u, c->press, (long long)c->stride_model, (long long)c->stride_traj,
                                c->g_x0, c->dv};
    const dim3 block(press_grad::kGradBlock), grid(cost_blocks(B), M);
    const bool kept = c->substeps == press_grad::kKeptSubsteps;
    if (B > 0 && fused) {
        const press_train::LossSeed seed{l->terms, (long long)l->terms_stride, l->p_scale[0], l->p_scale[1], l->u_prev,
                                         (long long)l->u_prev_stride, l->cost};
        if (value_only) {
            hipLaunchKernelGGL(press_train::press_loss_value_kernel, grid, block, 0, s, a, seed);
            if (const int rc = launch_check("press_loss_value_kernel")) return rc;
        } else if (noisy) {
            const press_noise::NoiseGrad n{nz->process_noise, (long long)nz->process_stride, nz->x_state};
            if (const int rc = press_noise::launch_bank_vjp(a, nullptr, &seed, n, c->smooth, kept, c->press != nullptr, grid, s))
                return rc;
        } else {   // T = 0 launches too: zero cost and g_x0
            const auto k = select([](auto sm, auto kp, auto table) {
                return &press_train::closed_loop_bank_vjp_kernel<sm(), kp(), Press<table()>, press_train::LossSeed>; },
                c->smooth, kept, c->press != nullptr);
            hipLaunchKernelGGL(k, grid, block, 0, s, a, seed);
            if (const int rc = launch_check("closed_loop_bank_vjp_kernel<LossSeed>")) return rc;
        }
        hipLaunchKernelGGL(press_train::cost_sum_kernel, grid, dim3(press_grad::kSumLanes), 0, s, B,
                           (const double *)l->cost, cost_part);
        if (const int rc = launch_check("cost_sum_kernel")) return rc;
    } else if (B > 0) {   // T = 0 launches too: g_x0 = g_x[:, :, 0]
        const press_train::TensorSeed seed{g_x, g_u};
        if (noisy) {
            const press_noise::NoiseGrad n{nz->process_noise, (long long)nz->process_stride, nz->x_state};
            if (const int rc = press_noise::launch_bank_vjp(a, &seed, nullptr, n, c->smooth, kept, c->press != nullptr, grid, s))
                return rc;
        } else {
            const auto k = select([](auto sm, auto kp, auto table) {
                return &press_train::closed_loop_bank_vjp_kernel<sm(), kp(), Press<table()>, press_train::TensorSeed>; },
                c->smooth, kept, c->press != nullptr);
            hipLaunchKernelGGL(k, grid, block, 0, s, a, seed);
            if (const int rc = launch_check("closed_loop_bank_vjp_kernel<TensorSeed>")) return rc;
        }
    }
    if (fused && l->loss) {   // B = 0: zeros
        hipLaunchKernelGGL(press_train::loss_reduce_kernel, dim3((M + press_grad::kSumLanes - 1) / press_grad::kSumLanes),
                           dim3(press_grad::kSumLanes), 0, s, M, B, (const double *)cost_part, cost_blocks(B), l->loss);
        if (const int rc = launch_check("loss_reduce_kernel")) return rc;
    }
    if (value_only || !c->g_w_inp || !c->g_b_inp || !c->g_w_out) return FCR_OK;
    const int blocks = rows ? press_grad::param_blocks((long long)B * T) : 0;
    if (blocks) {
        hipLaunchKernelGGL(press_train::param_grad_bank_kernel, dim3(blocks, M), block, 0, s, a, part);
        if (const int rc = launch_check("param_grad_bank_kernel")) return rc;
    }
    // no rows: the three gradients are zeroed
    hipLaunchKernelGGL(press_train::param_reduce_bank_kernel,
                       dim3((H * 5 + press_grad::kGradBlock - 1) / press_grad::kGradBlock, M), block, 0, s,
                       (const double *)part, blocks, H, c->g_w_inp, c->g_b_inp, c->g_w_out);
    return launch_check("param_reduce_bank_kernel");
}

}  // namespace

extern "C" {

int fcr_closed_loop_bank_vjp_workspace_size(int32_t n_models, int32_t B, int32_t T, int32_t ctrl_hidden, size_t *bytes) {
    const char *who = "fcr_closed_loop_bank_vjp_workspace_size";
    if (!bytes) return fail(FCR_EINVAL, "%s: bytes is NULL", who);
    *bytes = 0;
    if (const int rc = check_batch(who, B, T, "T", false)) return rc;
    if (const int rc = check_models(who, n_models, B, T)) return rc;
    if (ctrl_hidden < 1 || ctrl_hidden > press_grad::kMaxHidden)
        return fail(FCR_EUNSUPPORTED, "%s: ctrl_hidden=%d: built for 1..%d", who, ctrl_hidden, press_grad::kMaxHidden);
    *bytes = bank_workspace(n_models, B, T, ctrl_hidden);
    return FCR_OK;
}

int fcr_closed_loop_bank_vjp(const fcr_closed_loop_bank_grad *args, const double *g_x, const double *g_u, void *ws,
                             size_t ws_bytes, void *stream) {
    return bank_vjp("fcr_closed_loop_bank_vjp", args, g_x, g_u, nullptr, false, ws, ws_bytes, stream);
}

int fcr_closed_loop_bank_loss_vjp(const fcr_closed_loop_bank_grad *args, const fcr_press_loss *loss, void *ws,
                                  size_t ws_bytes, void *stream) {
    return bank_vjp("fcr_closed_loop_bank_loss_vjp", args, nullptr, nullptr, loss, true, ws, ws_bytes, stream);
}

int fcr_closed_loop_bank_vjp_noise(const fcr_closed_loop_bank_grad *args, const fcr_bank_noise *noise, const double *g_x,
                                   const double *g_u, void *ws, size_t ws_bytes, void *stream) {
    return bank_vjp("fcr_closed_loop_bank_vjp_noise", args, g_x, g_u, nullptr, false, ws, ws_bytes, stream, noise, true);
}

int fcr_closed_loop_bank_loss_vjp_noise(const fcr_closed_loop_bank_grad *args, const fcr_bank_noise *noise,
                                        const fcr_press_loss *loss, void *ws, size_t ws_bytes, void *stream) {
    return bank_vjp("fcr_closed_loop_bank_loss_vjp_noise", args, nullptr, nullptr, loss, true, ws, ws_bytes, stream, noise,
                    true);
}

}  // extern "C"
