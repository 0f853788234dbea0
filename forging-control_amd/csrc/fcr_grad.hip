// fcr_grad.hip — C ABI of the press's adjoint (fcr_press_grad.h): the vector-Jacobian product of the open-loop RK4
// rollout (fcr_plant_rk4_vjp) and of the controller + press closed loop (fcr_closed_loop_vjp). Validation before any
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

}  // namespace

extern "C" {

int fcr_plant_rk4_vjp(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x, const double *u,
                      const double *g_x, const double *press, int64_t stride_traj, double *g_x0, double *g_u,
                      void *stream) {
    const char *who = "fcr_plant_rk4_vjp";
    if (const int rc = check_batch(who, B, S, "S")) return rc;
    if (const int rc = check_step(who, "", ts, substeps)) return rc;
    if (const int rc = check_smooth(who, smooth)) return rc;
    if (const int rc = check_table(who, press, stride_traj, B)) return rc;
    if (B == 0) return FCR_OK;
    if (!x || !g_x || !g_x0 || (S > 0 && (!u || !g_u))) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)x) | ((uintptr_t)u) | ((uintptr_t)g_x) | ((uintptr_t)g_x0) | ((uintptr_t)g_u)) & 7)
        return fail(FCR_EINVAL, "%s: buffers must be 8-byte aligned (fp64)", who);
    const auto k = select([](auto sm, auto kept, auto table) {
        return &press_grad::plant_rk4_vjp_kernel<sm(), kept(), Press<table()>>; },
        smooth, substeps == press_grad::kKeptSubsteps, press != nullptr);
    const dim3 grid((B + press_grad::kGradBlock - 1) / press_grad::kGradBlock);
    // S = 0 launches too: g_x0 = g_x[:, 0]
    hipLaunchKernelGGL(k, grid, dim3(press_grad::kGradBlock), 0, (hipStream_t)stream, B, S, ts / substeps, substeps, x, u, g_x,
                       press, (long long)stride_traj, g_x0, g_u);
    return launch_check("plant_rk4_vjp_kernel");
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

int fcr_closed_loop_vjp(const fcr_closed_loop_grad *c, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "fcr_closed_loop_vjp";
    if (const int rc = check_loop(who, c, press_grad::kMaxHidden, true)) return rc;
    if (const int rc = check_table(who, c->press, c->stride_traj, c->B)) return rc;
    if (!c->g_w_inp || !c->g_b_inp || !c->g_w_out) {
        if (c->B == 0) return FCR_OK;                          // an empty batch with nothing to zero
        return fail(FCR_EINVAL, "%s: a parameter gradient is NULL", who);
    }
    if ((((uintptr_t)c->g_w_inp) | ((uintptr_t)c->g_b_inp) | ((uintptr_t)c->g_w_out)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    const bool rows = c->B > 0 && c->T > 0;
    if (c->B > 0 && (!c->x || !c->g_x || !c->g_x0 || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (rows && (!c->ref || !c->u || !c->g_u || !c->dv)) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)c->x) | ((uintptr_t)c->u) | ((uintptr_t)c->ref) | ((uintptr_t)c->g_x) | ((uintptr_t)c->g_u) |
         ((uintptr_t)c->g_x0) | ((uintptr_t)c->dv)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    const size_t need = param_workspace(c->B, c->T, c->ctrl_hidden);
    if (need && !ws) return fail(FCR_EINVAL, "%s: the workspace is NULL", who);
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "%s: the workspace has %zu bytes, %zu are needed", who, ws_bytes, need);
    if (((uintptr_t)ws) & 7) return fail(FCR_EINVAL, "%s: the workspace must be 8-byte aligned", who);

    hipStream_t s = (hipStream_t)stream;
    press_grad::LoopGradArgs a{c->B, c->T, c->substeps, c->ctrl_hidden, c->ts / c->substeps, c->ref, c->ctrl_w_inp,
                               c->ctrl_b_inp, c->ctrl_w_out, c->in_scale[0], c->in_scale[1], c->ref_scale, c->out_scale,
                               c->x, c->u, c->g_x, c->g_u, c->press, (long long)c->stride_traj, c->g_x0, c->dv};
    const dim3 block(press_grad::kGradBlock);
    if (c->B > 0) {   // T = 0 launches too: g_x0 = g_x[:, 0]
        const auto k = select([](auto sm, auto kept, auto table) {
            return &press_grad::closed_loop_vjp_kernel<sm(), kept(), Press<table()>>; },
            c->smooth, c->substeps == press_grad::kKeptSubsteps, c->press != nullptr);
        hipLaunchKernelGGL(k, dim3((c->B + press_grad::kGradBlock - 1) / press_grad::kGradBlock), block, 0, s, a);
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

}  // extern "C"
