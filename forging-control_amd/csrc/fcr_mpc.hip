// fcr_mpc.hip — C ABI of the model-predictive baseline on the press (fcr_mpc.h): one horizon for B
// problems (fcr_mpc_solve), the T-step closed loop around the same solver (fcr_mpc_closed_loop), and their workspace
// query. Validation before any device call, by the checks the press rows share (fcr_press_host.h); stream-ordered
// launches; no allocation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcr.h"
#include "fcr_host.h"
#include "fcr_plant.h"
#include "fcr_press_host.h"

// fcr_plant.h's and fcr_press_grad.h's non-template kernels have external host stubs and are compiled into fcr_rows.hip
// and fcr_grad.hip; this unit reads the headers for their __device__ functions only, so here those kernels get internal
// linkage (no second host stub under the same name) and are never launched.
#pragma push_macro("__global__")
#undef __global__
#define __global__ static __attribute__((global))
#include "fcr_press_grad.h"
#pragma pop_macro("__global__")

#include "fcr_mpc.h"

using namespace fcr;

namespace {

template <bool TABLE>
using Press = std::conditional_t<TABLE, plant::Coeffs, plant::Nominal>;

int blocks_of(int B) { return (B + mpc::kMpcBlock - 1) / mpc::kMpcBlock; }

size_t workspace(int B, int N) { return align_up((size_t)B * mpc::Layout(N).total * sizeof(double)); }

bool finite(double v) { return v - v == 0.0; }

int check_horizon(const char *who, int N) {
    if (N < 1 || N > mpc::kMaxHorizon) return fail(FCR_EINVAL, "%s: N=%d must be 1..%d", who, N, mpc::kMaxHorizon);
    return FCR_OK;
}

// the solver's own fields -> the kernels' arguments, or a message
int check_mpc(const char *who, const fcr_mpc *m, mpc::MpcArgs *out) {
    if (!m) return fail(FCR_EINVAL, "%s: mpc is NULL", who);
    if (const int rc = check_horizon(who, m->N)) return rc;
    if (m->K < 1 || m->K > mpc::kMaxIters) return fail(FCR_EINVAL, "%s: K=%d must be 1..%d", who, m->K, mpc::kMaxIters);
    if (const int rc = check_step(who, "", m->ts, m->substeps)) return rc;
    if (const int rc = check_smooth(who, m->smooth)) return rc;
    if (!(m->r_u >= 0.0) || !finite(m->r_u)) return fail(FCR_EINVAL, "%s: r_u=%g must be finite and >= 0", who, m->r_u);
    if (!(m->lam0 > 0.0) || !finite(m->lam0)) return fail(FCR_EINVAL, "%s: lam0=%g must be finite and > 0", who, m->lam0);
    const double *p = m->p_bounds;
    for (int i = 0; i < 4; ++i)
        if (p[i] != p[i]) return fail(FCR_EINVAL, "%s: p_bounds[%d] is a NaN", who, i);
    if (p[0] > p[1] || p[2] > p[3])
        return fail(FCR_EINVAL, "%s: a lower pressure bound is above its upper bound (p1 %g..%g, p2 %g..%g)", who, p[0], p[1],
                    p[2], p[3]);
    if (!(m->p_weight >= 0.0) || !finite(m->p_weight))
        return fail(FCR_EINVAL, "%s: p_weight=%g must be finite and >= 0", who, m->p_weight);
    if (!(m->p_scale > 0.0) || !finite(m->p_scale))
        return fail(FCR_EINVAL, "%s: p_scale=%g must be finite and > 0", who, m->p_scale);
    if (m->u_bounds[0] != m->u_bounds[0] || m->u_bounds[1] != m->u_bounds[1] || m->u_bounds[0] > m->u_bounds[1])
        return fail(FCR_EINVAL, "%s: u_bounds=(%g, %g) must be lo <= hi", who, m->u_bounds[0], m->u_bounds[1]);
    // w = 0 removes the four hinge rows: their bounds go to infinity
    const bool off = m->p_weight == 0.0;
    *out = mpc::MpcArgs{m->N, m->K, m->substeps, m->ts / m->substeps, sqrt(m->r_u), m->lam0,
                        off ? -INFINITY : p[0], off ? INFINITY : p[1], off ? -INFINITY : p[2], off ? INFINITY : p[3],
                        sqrt(m->p_weight), 1.0 / m->p_scale, m->u_bounds[0], m->u_bounds[1]};
    return FCR_OK;
}

int check_press(const char *who, const char *what, const double *press, long long stride) {
    if (stride < 0 || stride % plant::kPressFields)
        return fail(FCR_EINVAL, "%s: %s_stride=%lld must be 0 (shared) or a multiple of %d", who, what, stride,
                    plant::kPressFields);
    if (!press && stride) return fail(FCR_EINVAL, "%s: %s_stride=%lld without a parameter table", who, what, stride);
    if (((uintptr_t)press) & 7) return fail(FCR_EINVAL, "%s: the %s table must be 8-byte aligned (fp64)", who, what);
    return FCR_OK;
}

int check_workspace(const char *who, int B, int N, const void *ws, size_t ws_bytes) {
    const size_t need = workspace(B, N);
    if (!ws) return fail(FCR_EINVAL, "%s: the workspace is NULL", who);
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "%s: the workspace has %zu bytes, %zu are needed", who, ws_bytes, need);
    if (((uintptr_t)ws) & 7) return fail(FCR_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    return FCR_OK;
}

}  // namespace

extern "C" {

int fcr_mpc_workspace_size(int32_t B, int32_t N, size_t *bytes) {
    const char *who = "fcr_mpc_workspace_size";
    if (!bytes) return fail(FCR_EINVAL, "%s: bytes is NULL", who);
    *bytes = 0;
    if (B < 0) return fail(FCR_EINVAL, "%s: B=%d must be >= 0", who, B);
    if (const int rc = check_horizon(who, N)) return rc;
    *bytes = workspace(B, N);
    return FCR_OK;
}

int fcr_mpc_solve(const fcr_mpc *m, int32_t B, const double *x0, const double *ref, const double *u_prev, const double *U0,
                  const double *model, int64_t model_stride, double *U, double *cost, double *grad_inf, int32_t *accepted,
                  double *lam, double *trace, double *trace_u, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "fcr_mpc_solve";
    mpc::MpcArgs a;
    if (const int rc = check_mpc(who, m, &a)) return rc;
    if (const int rc = check_batch(who, B, m->N, "N")) return rc;
    if (const int rc = check_press(who, "model", model, (long long)model_stride)) return rc;
    if ((trace == nullptr) != (trace_u == nullptr)) return fail(FCR_EINVAL, "%s: trace and trace_u go together", who);
    if (B == 0) return FCR_OK;
    if (!x0 || !ref || !u_prev || !U || !cost || !grad_inf || !accepted || !lam)
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    const uintptr_t bits = ((uintptr_t)x0) | ((uintptr_t)ref) | ((uintptr_t)u_prev) | ((uintptr_t)U0) | ((uintptr_t)U) |
                           ((uintptr_t)cost) | ((uintptr_t)grad_inf) | ((uintptr_t)lam) | ((uintptr_t)trace) |
                           ((uintptr_t)trace_u);
    if (bits & 7) return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    if (const int rc = check_workspace(who, B, m->N, ws, ws_bytes)) return rc;
    const mpc::SolveArgs s{B, x0, ref, u_prev, U0, model, (long long)model_stride, U, cost, grad_inf, lam, accepted, trace,
                           trace_u, (double *)ws};
    const auto k = select([](auto sm, auto table) { return &mpc::mpc_solve_kernel<sm(), Press<table()>>; }, m->smooth != 0,
                          model != nullptr);
    hipLaunchKernelGGL(k, dim3(blocks_of(B)), dim3(mpc::kMpcBlock), 0, (hipStream_t)stream, a, s);
    return launch_check("mpc_solve_kernel");
}

int fcr_mpc_closed_loop(const fcr_mpc *m, const fcr_mpc_loop *l, void *ws, size_t ws_bytes, void *stream) {
    const char *who = "fcr_mpc_closed_loop";
    mpc::MpcArgs a;
    if (const int rc = check_mpc(who, m, &a)) return rc;
    if (!l) return fail(FCR_EINVAL, "%s: loop is NULL", who);
    if (const int rc = check_batch(who, l->B, l->T, "T")) return rc;
    if ((long long)l->B * (l->T > 0 ? l->T : 1) * m->K * (m->N > 5 ? m->N : 5) > (1LL << 40))
        return fail(FCR_EINVAL, "%s: B*T*K*N too large", who);
    if (l->preview != 0 && l->preview != 1) return fail(FCR_EINVAL, "%s: preview=%d must be 0 or 1", who, l->preview);
    if (const int rc = check_press(who, "plant", l->plant, (long long)l->plant_stride)) return rc;
    if (const int rc = check_press(who, "model", l->model, (long long)l->model_stride)) return rc;
    if ((l->trace == nullptr) != (l->trace_u == nullptr)) return fail(FCR_EINVAL, "%s: trace and trace_u go together", who);
    const int B = l->B, T = l->T;
    if (B == 0) return FCR_OK;
    if (!l->x0 || !l->x) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (T > 0 && (!l->ref || !l->u_init || !l->u || !l->cost || !l->grad_inf || !l->accepted))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    const uintptr_t bits = ((uintptr_t)l->x0) | ((uintptr_t)l->ref) | ((uintptr_t)l->u_init) | ((uintptr_t)l->U0) |
                           ((uintptr_t)l->process_noise) | ((uintptr_t)l->meas_noise) | ((uintptr_t)l->x) | ((uintptr_t)l->u) |
                           ((uintptr_t)l->cost) | ((uintptr_t)l->grad_inf) | ((uintptr_t)l->plans) | ((uintptr_t)l->trace) |
                           ((uintptr_t)l->trace_u);
    if (bits & 7) return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if (T == 0) {   // x[:,0] = x0 and nothing else
        if (hipMemcpyAsync(l->x, l->x0, (size_t)B * 5 * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(FCR_EHIP, "%s: copying x0 failed", who);
        return FCR_OK;
    }
    if (const int rc = check_workspace(who, B, m->N, ws, ws_bytes)) return rc;
    const mpc::LoopArgs la{B, T, l->preview, l->x0, l->ref, l->u_init, l->U0, l->process_noise, l->meas_noise, l->plant, l->model,
                           (long long)l->plant_stride, (long long)l->model_stride, l->x, l->u, l->cost, l->grad_inf,
                           l->accepted, l->plans, l->trace, l->trace_u, (double *)ws};
    // either press given as a table: both run as tables (a NULL one reads the reference's row)
    const auto k = select([](auto sm, auto table, auto noise) {
        return &mpc::mpc_closed_loop_kernel<sm(), Press<table()>, Press<table()>, noise()>; },
        m->smooth != 0, l->plant != nullptr || l->model != nullptr, l->process_noise != nullptr || l->meas_noise != nullptr);
    hipLaunchKernelGGL(k, dim3(blocks_of(B)), dim3(mpc::kMpcBlock), 0, s, a, la);
    return launch_check("mpc_closed_loop_kernel");
}

}  // extern "C"
