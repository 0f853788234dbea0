// fcr_grad.hip — C ABI of the press's adjoint (fcr_press_grad.h): the vector-Jacobian product of the open-loop RK4
// rollout (fcr_plant_rk4_vjp) and of the controller + press closed loop (fcr_closed_loop_vjp), each also with the
// gradients of the 28 press parameters (*_press; fcr_press_grad_sum: their fixed-order sum). Validation before any
// device call, by the checks the press rows share (fcr_press_host.h); stream-ordered launches; no allocation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr.h"
#include "fcr_host.h"
#include "fcr_press_grad.h"
#include "fcr_press_host.h"

using namespace fcr;

namespace {

size_t param_workspace(int B, int T, int hidden) {
    return align_up((size_t)press_grad::param_blocks((long long)B * T) * hidden * 5 * sizeof(double));
}

// the press policy of an adjoint kernel: the table's rows, or the reference's press (press = NULL)
template <bool TABLE>
using Press = std::conditional_t<TABLE, plant::Coeffs, plant::Nominal>;

// a parameter table's stride and pointer (NULL = the reference's press; then the stride must be 0), or a message
int check_table(const char *who, const double *press, long long stride_traj, int B) {
    if (const int rc = check_table_strides(who, 0, stride_traj, B)) return rc;
    return check_table_pointer(who, press, false, stride_traj);
}

// fcr_plant_rk4_vjp (g_press = NULL, want_press false) and fcr_plant_rk4_vjp_press under their own names
int plant_vjp(const char *who, bool want_press, int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth,
              const double *x, const double *u, const double *g_x, const double *press, int64_t stride_traj, double *g_x0,
              double *g_u, double *g_press, void *stream) {
    if (const int rc = check_batch(who, B, S, "S")) return rc;
    if (const int rc = check_step(who, "", ts, substeps)) return rc;
    if (const int rc = check_smooth(who, smooth)) return rc;
    if (const int rc = check_table(who, press, stride_traj, B)) return rc;
    if (B == 0) return FCR_OK;
    if (want_press)
        if (const int rc = check_table_pointer(who, press, true)) return rc;
    if (!x || !g_x || !g_x0 || (S > 0 && (!u || !g_u)) || (want_press && !g_press))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)x) | ((uintptr_t)u) | ((uintptr_t)g_x) | ((uintptr_t)g_x0) | ((uintptr_t)g_u) | ((uintptr_t)g_press)) & 7)
        return fail(FCR_EINVAL, "%s: buffers must be 8-byte aligned (fp64)", who);
    const dim3 grid((B + press_grad::kGradBlock - 1) / press_grad::kGradBlock), block(press_grad::kGradBlock);
    const bool kept = substeps == press_grad::kKeptSubsteps;
    // S = 0 launches too: g_x0 = g_x[:, 0] (and g_press = 0)
    if (want_press) {
        const auto k = select([](auto sm, auto kp) { return &press_grad::plant_rk4_vjp_press_kernel<sm(), kp()>; }, smooth, kept);
        hipLaunchKernelGGL(k, grid, block, 0, (hipStream_t)stream, B, S, ts / substeps, substeps, x, u, g_x, press,
                           (long long)stride_traj, g_x0, g_u, g_press);
        return launch_check("plant_rk4_vjp_press_kernel");
    }
    const auto k = select([](auto sm, auto kp, auto table) {
        return &press_grad::plant_rk4_vjp_kernel<sm(), kp(), Press<table()>>; },
        smooth, kept, press != nullptr);
    hipLaunchKernelGGL(k, grid, block, 0, (hipStream_t)stream, B, S, ts / substeps, substeps, x, u, g_x, press,
                       (long long)stride_traj, g_x0, g_u);
    return launch_check("plant_rk4_vjp_kernel");
}

// fcr_closed_loop_vjp and fcr_closed_loop_vjp_press under their own names
int loop_vjp(const char *who, bool want_press, const fcr_closed_loop_grad *c, double *g_press, void *ws, size_t ws_bytes,
             void *stream) {
    if (const int rc = check_loop(who, c, press_grad::kMaxHidden, true)) return rc;
    if (const int rc = check_table(who, c->press, c->stride_traj, c->B)) return rc;
    if (!c->g_w_inp || !c->g_b_inp || !c->g_w_out) {
        if (c->B == 0) return FCR_OK;                          // an empty batch with nothing to zero
        return fail(FCR_EINVAL, "%s: a parameter gradient is NULL", who);
    }
    if ((((uintptr_t)c->g_w_inp) | ((uintptr_t)c->g_b_inp) | ((uintptr_t)c->g_w_out)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    const bool rows = c->B > 0 && c->T > 0;
    if (want_press && c->B > 0)
        if (const int rc = check_table_pointer(who, c->press, true)) return rc;
    if (c->B > 0 && (!c->x || !c->g_x || !c->g_x0 || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out ||
                     (want_press && !g_press)))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (rows && (!c->ref || !c->u || !c->g_u || !c->dv)) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)c->x) | ((uintptr_t)c->u) | ((uintptr_t)c->ref) | ((uintptr_t)c->g_x) | ((uintptr_t)c->g_u) |
         ((uintptr_t)c->g_x0) | ((uintptr_t)c->dv) | ((uintptr_t)g_press)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    const size_t need = param_workspace(c->B, c->T, c->ctrl_hidden);
    if (need && !ws) return fail(FCR_EINVAL, "%s: the workspace is NULL", who);
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "%s: the workspace has %zu bytes, %zu are needed", who, ws_bytes, need);
    if (((uintptr_t)ws) & 7) return fail(FCR_EINVAL, "%s: the workspace must be 8-byte aligned", who);

    hipStream_t s = (hipStream_t)stream;
    press_grad::LoopGradArgs a{c->B, c->T, c->substeps, c->ctrl_hidden, c->ts / c->substeps, c->ref, c->ctrl_w_inp,
                               c->ctrl_b_inp, c->ctrl_w_out, c->in_scale[0], c->in_scale[1], c->ref_scale, c->out_scale,
                               c->x, c->u, c->g_x, c->g_u, c->press, (long long)c->stride_traj, c->g_x0, c->dv};
    const dim3 block(press_grad::kGradBlock), grid((c->B + press_grad::kGradBlock - 1) / press_grad::kGradBlock);
    const bool kept = c->substeps == press_grad::kKeptSubsteps;
    if (c->B > 0 && want_press) {   // T = 0 launches too: g_x0 = g_x[:, 0] (and g_press = 0)
        const auto k = select([](auto sm, auto kp) { return &press_grad::closed_loop_vjp_press_kernel<sm(), kp()>; },
                              c->smooth, kept);
        hipLaunchKernelGGL(k, grid, block, 0, s, a, g_press);
        if (const int rc = launch_check("closed_loop_vjp_press_kernel")) return rc;
    } else if (c->B > 0) {
        const auto k = select([](auto sm, auto kp, auto table) {
            return &press_grad::closed_loop_vjp_kernel<sm(), kp(), Press<table()>>; },
            c->smooth, kept, c->press != nullptr);
        hipLaunchKernelGGL(k, grid, block, 0, s, a);
        if (const int rc = launch_check("closed_loop_vjp_kernel")) return rc;
    }
    const int blocks = rows ? press_grad::param_blocks((long long)c->B * c->T) : 0;
    if (blocks) {
        hipLaunchKernelGGL(press_grad::param_grad_kernel, dim3(blocks), block, 0, s, a, (double *)ws);
        if (const int rc = launch_check("param_grad_kernel")) return rc;
    }
    // no rows: the three gradients are zeroed
    hipLaunchKernelGGL(press_grad::param_reduce_kernel,
                       dim3((c->ctrl_hidden * 5 + press_grad::kGradBlock - 1) / press_grad::kGradBlock), block, 0, s,
                       (const double *)ws, blocks, c->ctrl_hidden, c->g_w_inp, c->g_b_inp, c->g_w_out);
    return launch_check("param_reduce_kernel");
}

size_t sum_workspace(int B) {
    return align_up((size_t)((B + press_grad::kGradBlock - 1) / press_grad::kGradBlock) * plant::kPressFields * sizeof(double));
}

}  // namespace

extern "C" {

int fcr_plant_rk4_vjp(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x, const double *u,
                      const double *g_x, const double *press, int64_t stride_traj, double *g_x0, double *g_u,
                      void *stream) {
    return plant_vjp("fcr_plant_rk4_vjp", false, B, S, ts, substeps, smooth, x, u, g_x, press, stride_traj, g_x0, g_u,
                     nullptr, stream);
}

int fcr_plant_rk4_vjp_press(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x,
                            const double *u, const double *g_x, const double *press, int64_t stride_traj, double *g_x0,
                            double *g_u, double *g_press, void *stream) {
    return plant_vjp("fcr_plant_rk4_vjp_press", true, B, S, ts, substeps, smooth, x, u, g_x, press, stride_traj, g_x0, g_u,
                     g_press, stream);
}

int fcr_closed_loop_vjp_workspace_size(int32_t B, int32_t T, int32_t ctrl_hidden, size_t *bytes) {
    const char *who = "fcr_closed_loop_vjp_workspace_size";
    if (!bytes) return fail(FCR_EINVAL, "%s: bytes is NULL", who);
    *bytes = 0;
    if (const int rc = check_batch(who, B, T, "T", false)) return rc;
    if (ctrl_hidden < 1 || ctrl_hidden > press_grad::kMaxHidden)
        return fail(FCR_EUNSUPPORTED, "%s: ctrl_hidden=%d: built for 1..%d", who, ctrl_hidden, press_grad::kMaxHidden);
    *bytes = param_workspace(B, T, ctrl_hidden);
    return FCR_OK;
}

int fcr_closed_loop_vjp(const fcr_closed_loop_grad *args, void *ws, size_t ws_bytes, void *stream) {
    return loop_vjp("fcr_closed_loop_vjp", false, args, nullptr, ws, ws_bytes, stream);
}

int fcr_closed_loop_vjp_press(const fcr_closed_loop_grad *args, double *g_press, void *ws, size_t ws_bytes, void *stream) {
    return loop_vjp("fcr_closed_loop_vjp_press", true, args, g_press, ws, ws_bytes, stream);
}

int fcr_press_grad_sum_workspace_size(int32_t B, size_t *bytes) {
    const char *who = "fcr_press_grad_sum_workspace_size";
    if (!bytes) return fail(FCR_EINVAL, "%s: bytes is NULL", who);
    *bytes = 0;
    if (B < 0) return fail(FCR_EINVAL, "%s: B=%d must be >= 0", who, B);
    *bytes = sum_workspace(B);
    return FCR_OK;
}

int fcr_press_grad_sum(int32_t B, const double *g_press, double *g_row, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "fcr_press_grad_sum";
    if (B < 0) return fail(FCR_EINVAL, "%s: B=%d must be >= 0", who, B);
    if (!g_row) {
        if (B == 0) return FCR_OK;                             // an empty batch with nothing to zero
        return fail(FCR_EINVAL, "%s: g_row is NULL", who);
    }
    if (B > 0 && !g_press) return fail(FCR_EINVAL, "%s: g_press is NULL", who);
    if ((((uintptr_t)g_press) | ((uintptr_t)g_row)) & 7) return fail(FCR_EINVAL, "%s: buffers must be 8-byte aligned (fp64)", who);
    const size_t need = sum_workspace(B);
    if (need && !ws) return fail(FCR_EINVAL, "%s: the workspace is NULL", who);
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "%s: the workspace has %zu bytes, %zu are needed", who, ws_bytes, need);
    if (((uintptr_t)ws) & 7) return fail(FCR_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (B + press_grad::kGradBlock - 1) / press_grad::kGradBlock;
    if (blocks) {
        hipLaunchKernelGGL(press_grad::press_grad_sum_kernel, dim3(blocks), dim3(press_grad::kSumLanes), 0, s, B, g_press,
                           (double *)ws);
        if (const int rc = launch_check("press_grad_sum_kernel")) return rc;
    }
    // B = 0: g_row is zeroed
    hipLaunchKernelGGL(press_grad::press_grad_reduce_kernel, dim3(1), dim3(press_grad::kSumLanes), 0, s, (const double *)ws,
                       blocks, g_row);
    return launch_check("press_grad_reduce_kernel");
}

}  // extern "C"
