// fcr_rows.hip — C ABI of the SURVEY.md §8(f) rows that need no rollout state: the batched press plant
// (fcr_plant.h), the controller + press closed loop (fcr_closed_loop.h), its feasibility recovery
// (fcr_feasibility.h), the training-window gather (fcr_window.h) and the supervised baseline's epoch (fcr_supervised.h). Validation before any device call; stream-ordered launches; no allocation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr.h"
#include "fcr_closed_loop.h"
#include "fcr_feasibility.h"
#include "fcr_host.h"
#include "fcr_plant.h"
#include "fcr_supervised.h"
#include "fcr_window.h"

using namespace fcr;

namespace {

// ts / substeps of an RK4 integrator (what: "" or the name of whose they are), or a message
int check_step(const char *who, const char *what, double ts, int substeps) {
    if (substeps < 1 || substeps > 4096) return fail(FCR_EINVAL, "%s: %ssubsteps=%d must be 1..4096", who, what, substeps);
    if (!(ts > 0.0) || ts > 1e6) return fail(FCR_EINVAL, "%s: %sts=%g must be a positive time step", who, what, ts);
    return FCR_OK;
}

// fcr_feasibility -> the kernels' arguments (bounds scaled as the reference's NLP scales them), or a message
int feasibility_args(const char *who, const fcr_feasibility *f, feasibility::FeasArgs *out) {
    if (!(f->p1_lo < f->p1_hi)) return fail(FCR_EINVAL, "%s: p1 bounds lo=%g must be < hi=%g", who, f->p1_lo, f->p1_hi);
    if (!(f->p2_lo < f->p2_hi)) return fail(FCR_EINVAL, "%s: p2 bounds lo=%g must be < hi=%g", who, f->p2_lo, f->p2_hi);
    if (!(f->u_lo < f->u_hi)) return fail(FCR_EINVAL, "%s: u_lo=%g must be < u_hi=%g", who, f->u_lo, f->u_hi);
    if (const int rc = check_step(who, "feasibility ", f->ts, f->substeps)) return rc;
    if (f->expand < 1 || f->expand > 20) return fail(FCR_EINVAL, "%s: expand=%d must be 1..20", who, f->expand);
    if (f->bisect < 1 || f->bisect > 60) return fail(FCR_EINVAL, "%s: bisect=%d must be 1..60", who, f->bisect);
    *out = feasibility::FeasArgs{f->p1_lo * feasibility::kPScale, f->p1_hi * feasibility::kPScale,
                                 f->p2_lo * feasibility::kPScale, f->p2_hi * feasibility::kPScale,
                                 f->u_lo, f->u_hi, f->ts / f->substeps, f->substeps, f->expand, f->bisect};
    return FCR_OK;
}

static_assert(sizeof(fcr_press) == plant::kPressFields * sizeof(double), "fcr_press is one row of a parameter table");

// a host-side press (the model a projection integrates) -> its coefficients, or a message
int press_model(const char *who, const fcr_press *model, plant::UniformParams *out) {
    fcr_press nominal;
    fcr_press_nominal(&nominal);
    const double *row = (const double *)(model ? model : &nominal);
    static const char *const names[plant::kPressFields] = {
        "m_mass", "b_damp", "ft", "d1", "d2", "g", "kb", "v1_0", "v2_0", "kl_1", "kl_2", "cd", "rho", "d",
        "ps", "pt", "mu", "k", "w0", "h0", "b0", "t_def", "t1", "m0", "m1", "m2", "m3", "m4"};
    static const int positive[] = {0, 3, 4, 7, 8, 12, 18, 19, 20, 22};   // divided by, or under a root
    for (int i = 0; i < plant::kPressFields; ++i)
        if (!(row[i] - row[i] == 0.0)) return fail(FCR_EINVAL, "%s: model field %s=%g is not finite", who, names[i], row[i]);
    for (const int i : positive)
        if (!(row[i] > 0.0)) return fail(FCR_EINVAL, "%s: model field %s=%g must be positive", who, names[i], row[i]);
    *out = plant::derive(row);
    return FCR_OK;
}

// a parameter table's pointer, checked once the call is known not to be empty (B = 0 reads no row), or a message
int press_pointer(const char *who, const double *press) {
    if (!press) return fail(FCR_EINVAL, "%s: the parameter table is NULL", who);
    if (((uintptr_t)press) & 7) return fail(FCR_EINVAL, "%s: the parameter table must be 8-byte aligned (fp64)", who);
    return FCR_OK;
}

// a parameter table's strides (include/fcr.h), or a message
int press_strides(const char *who, long long stride_model, long long stride_traj, int B) {
    if (stride_model < 0 || stride_traj < 0)
        return fail(FCR_EINVAL, "%s: a parameter stride is negative (model %lld, trajectory %lld)", who, stride_model, stride_traj);
    if (stride_traj % plant::kPressFields)
        return fail(FCR_EINVAL, "%s: stride_traj=%lld must be 0 (shared) or a multiple of %d", who, stride_traj, plant::kPressFields);
    if (stride_model && (stride_model % plant::kPressFields || stride_model < (long long)B * stride_traj))
        return fail(FCR_EINVAL, "%s: stride_model=%lld must be 0 (shared) or a multiple of %d that is >= B * stride_traj = %lld",
                    who, stride_model, plant::kPressFields, (long long)B * stride_traj);
    return FCR_OK;
}

// fcr_closed_loop_run_bank (table = null: the reference's press, the kernels without parameters) and
// fcr_closed_loop_run_bank_press (table, model: checked by the caller)
int run_bank(const char *who, const fcr_closed_loop_bank *c, const closed_loop::PressTable *table,
             const plant::UniformParams *model, void *stream);

}  // namespace

extern "C" {

void fcr_press_nominal(fcr_press *out) {
    if (!out) return;
    *out = fcr_press{plant::M_MASS, plant::B_DAMP, plant::FT, plant::D1, plant::D2, plant::G, plant::KB, plant::V1_0,
                     plant::V2_0, plant::KL_1, plant::KL_2, plant::CD, plant::RHO, plant::D, plant::PS, plant::PT,
                     plant::MU, plant::K, plant::W0, plant::H0, plant::B0, plant::T_DEF, plant::T1, plant::M0,
                     plant::M1, plant::M2, plant::M3, plant::M4};
}

int fcr_plant_rk4_press(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x0,
                        const double *u, double *x, const double *press, int64_t stride_traj, void *stream) {
    const char *who = "fcr_plant_rk4_press";
    if (B < 0 || S < 0) return fail(FCR_EINVAL, "%s: B=%d, S=%d must be >= 0", who, B, S);
    if (const int rc = check_step(who, "", ts, substeps)) return rc;
    if (smooth != 0 && smooth != 1) return fail(FCR_EINVAL, "%s: smooth=%d must be 0 or 1", who, smooth);
    if ((long long)B * (S + 1) * 5 > (1LL << 40)) return fail(FCR_EINVAL, "%s: B*(S+1) too large", who);
    if (const int rc = press_strides(who, 0, stride_traj, B)) return rc;
    if (B == 0) return FCR_OK;
    if (const int rc = press_pointer(who, press)) return rc;
    if (!x0 || !x || (S > 0 && !u)) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)x0) | ((uintptr_t)u) | ((uintptr_t)x)) & 7)
        return fail(FCR_EINVAL, "%s: buffers must be 8-byte aligned (fp64)", who);
    const dim3 grid((B + plant::kPlantBlock - 1) / plant::kPlantBlock);
    hipLaunchKernelGGL(smooth ? plant::plant_rk4_press_kernel<true> : plant::plant_rk4_press_kernel<false>, grid,
                       dim3(plant::kPlantBlock), 0, (hipStream_t)stream, B, S, ts / substeps, substeps, x0, u, x, press,
                       (long long)stride_traj);
    return launch_check("plant_rk4_press_kernel");
}

int fcr_plant_rk4(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x0,
                  const double *u, double *x, void *stream) {
    if (B < 0 || S < 0) return fail(FCR_EINVAL, "fcr_plant_rk4: B=%d, S=%d must be >= 0", B, S);
    if (const int rc = check_step("fcr_plant_rk4", "", ts, substeps)) return rc;
    if (smooth != 0 && smooth != 1) return fail(FCR_EINVAL, "fcr_plant_rk4: smooth=%d must be 0 or 1", smooth);
    if ((long long)B * (S + 1) * 5 > (1LL << 40)) return fail(FCR_EINVAL, "fcr_plant_rk4: B*(S+1) too large");
    if (B == 0) return FCR_OK;
    if (!x0 || !x || (S > 0 && !u)) return fail(FCR_EINVAL, "fcr_plant_rk4: a required pointer is NULL");
    if ((((uintptr_t)x0) | ((uintptr_t)u) | ((uintptr_t)x)) & 7)
        return fail(FCR_EINVAL, "fcr_plant_rk4: buffers must be 8-byte aligned (fp64)");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((B + plant::kPlantBlock - 1) / plant::kPlantBlock);
    const double dt = ts / substeps;
    hipLaunchKernelGGL(smooth ? plant::plant_rk4_kernel<true> : plant::plant_rk4_kernel<false>, grid,
                       dim3(plant::kPlantBlock), 0, s, B, S, dt, substeps, x0, u, x);
    return launch_check("plant_rk4_kernel");
}

int fcr_window_gather(const fcr_windows *t, int32_t B, const int64_t *idx, float *x, float *y, float *z,
                      int32_t *bad, void *stream) {
    if (!t) return fail(FCR_EINVAL, "fcr_window_gather: tables is NULL");
    if (t->rows < 1 || t->traj_len < 1 || t->rows % t->traj_len)
        return fail(FCR_EINVAL, "fcr_window_gather: rows=%lld must be a positive multiple of traj_len=%d",
                    (long long)t->rows, t->traj_len);
    if (t->lookback < 1 || t->lookback > 4096) return fail(FCR_EINVAL, "fcr_window_gather: lookback=%d must be 1..4096", t->lookback);
    if (t->nx < 0 || t->ny < 0 || t->nz < 0 || t->nx > 4096 || t->ny > 4096 || t->nz > 4096)
        return fail(FCR_EINVAL, "fcr_window_gather: feature counts %d/%d/%d must be 0..4096", t->nx, t->ny, t->nz);
    if (B < 0) return fail(FCR_EINVAL, "fcr_window_gather: B=%d must be >= 0", B);
    if ((t->nx && !t->X) || (t->ny && !t->Y) || (t->nz && !t->Z) || !bad ||
        (B && (!idx || (t->nx && !x) || (t->ny && !y) || (t->nz && !z))))
        return fail(FCR_EINVAL, "fcr_window_gather: a required pointer is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, sizeof(int32_t), s) != hipSuccess) return fail(FCR_EHIP, "hipMemsetAsync failed");
    const long long per = t->nx + t->ny + (long long)t->lookback * t->nz;
    if (B == 0 || per == 0) return FCR_OK;
    window::WinArgs a{t->X, t->Y, t->Z, (long long)t->rows, t->traj_len, t->lookback, t->nx, t->ny, t->nz,
                      B, (const long long *)idx, x, y, z, bad};
    const long long n = (long long)B * per;
    if (n > (1LL << 40)) return fail(FCR_EINVAL, "fcr_window_gather: batch too large");
    hipLaunchKernelGGL(window::window_gather_kernel, dim3((unsigned)((n + window::kWinBlock - 1) / window::kWinBlock)),
                       dim3(window::kWinBlock), 0, s, a);
    return launch_check("window_gather_kernel");
}

int fcr_closed_loop_run(const fcr_closed_loop *c, void *stream) {
    if (!c) return fail(FCR_EINVAL, "fcr_closed_loop_run: args is NULL");
    if (c->B < 0 || c->T < 0) return fail(FCR_EINVAL, "fcr_closed_loop_run: B=%d, T=%d must be >= 0", c->B, c->T);
    if (const int rc = check_step("fcr_closed_loop_run", "", c->ts, c->substeps)) return rc;
    if (c->smooth != 0 && c->smooth != 1) return fail(FCR_EINVAL, "fcr_closed_loop_run: smooth=%d must be 0 or 1", c->smooth);
    if (c->ctrl_hidden < 1 || c->ctrl_hidden > closed_loop::kClMaxHidden)
        return fail(FCR_EUNSUPPORTED, "fcr_closed_loop_run: ctrl_hidden=%d: built for 1..%d", c->ctrl_hidden,
                    closed_loop::kClMaxHidden);
    if (!(c->in_scale[0] > 0.0) || !(c->in_scale[1] > 0.0) || !(c->ref_scale > 0.0) || !(c->out_scale > 0.0))
        return fail(FCR_EINVAL, "fcr_closed_loop_run: scaler scales must be positive");
    if (c->B == 0) return FCR_OK;
    if (!c->x0 || !c->x || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out || (c->T > 0 && (!c->ref || !c->u)))
        return fail(FCR_EINVAL, "fcr_closed_loop_run: a required pointer is NULL");
    if ((((uintptr_t)c->x0) | ((uintptr_t)c->ref) | ((uintptr_t)c->x) | ((uintptr_t)c->u)) & 7)
        return fail(FCR_EINVAL, "fcr_closed_loop_run: fp64 buffers must be 8-byte aligned");
    if ((((uintptr_t)c->process_noise) | ((uintptr_t)c->meas_noise)) & 7)
        return fail(FCR_EINVAL, "fcr_closed_loop_run: noise buffers must be 8-byte aligned (fp64)");
    feasibility::FeasArgs fa{};
    if (c->feasibility) {
        if (const int rc = feasibility_args("fcr_closed_loop_run", c->feasibility, &fa)) return rc;
        if (c->T > 0 && (!c->u_nn || !c->feas_flag))
            return fail(FCR_EINVAL, "fcr_closed_loop_run: u_nn or feas_flag is NULL with feasibility set");
        if ((((uintptr_t)c->u_nn) & 7) || (((uintptr_t)c->feas_flag) & 3))
            return fail(FCR_EINVAL, "fcr_closed_loop_run: u_nn must be 8-byte and feas_flag 4-byte aligned");
    }
    closed_loop::ClArgs a{c->B, c->T, c->substeps, c->ctrl_hidden, c->ts / c->substeps, c->x0, c->ref,
                          c->ctrl_w_inp, c->ctrl_b_inp, c->ctrl_w_out, c->in_scale[0], c->in_scale[1],
                          c->ref_scale, c->out_scale, c->x, c->u};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((c->B + closed_loop::kClBlock - 1) / closed_loop::kClBlock);
    const dim3 block(closed_loop::kClBlock);
    // one loop (closed_loop::loop_body), instantiated per [smooth] and, with recovery, [noise]; T = 0 only copies x0
    const bool sm = c->smooth, noise = c->T > 0 && (c->process_noise || c->meas_noise), recover = c->T > 0 && c->feasibility;
    if (recover) {
        using feasibility::closed_loop_recover_kernel;
        static constexpr decltype(&closed_loop_recover_kernel<false, false>) k[2][2] = {
            {closed_loop_recover_kernel<false, false>, closed_loop_recover_kernel<false, true>},
            {closed_loop_recover_kernel<true, false>, closed_loop_recover_kernel<true, true>}};
        hipLaunchKernelGGL(k[sm][noise], grid, block, 0, s, a, fa, c->process_noise, c->meas_noise, c->u_nn, c->feas_flag);
    } else if (noise) {
        hipLaunchKernelGGL(sm ? closed_loop::closed_loop_noise_kernel<true> : closed_loop::closed_loop_noise_kernel<false>,
                           grid, block, 0, s, a, c->process_noise, c->meas_noise);
    } else {
        hipLaunchKernelGGL(sm ? closed_loop::closed_loop_kernel<true> : closed_loop::closed_loop_kernel<false>, grid, block,
                           0, s, a);
    }
    return launch_check(recover ? "closed_loop_recover_kernel" : (noise ? "closed_loop_noise_kernel" : "closed_loop_kernel"));
}

int fcr_closed_loop_run_bank(const fcr_closed_loop_bank *c, void *stream) {
    return run_bank("fcr_closed_loop_run_bank", c, nullptr, nullptr, stream);
}

int fcr_closed_loop_run_bank_press(const fcr_closed_loop_bank *c, const double *press, int64_t stride_model,
                                   int64_t stride_traj, const fcr_press *model, void *stream) {
    const char *who = "fcr_closed_loop_run_bank_press";
    if (!c) return fail(FCR_EINVAL, "%s: args is NULL", who);
    if (const int rc = press_strides(who, stride_model, stride_traj, c->B)) return rc;
    plant::UniformParams mp;
    if (const int rc = press_model(who, model, &mp)) return rc;
    const closed_loop::PressTable table{press, (long long)stride_model, (long long)stride_traj};
    return run_bank(who, c, &table, &mp, stream);
}

int fcr_feasibility_project_press(const fcr_feasibility *f, const fcr_press *model, int32_t B, const double *x,
                                  const double *u_nn, double *u, int32_t *flag, double *v, void *stream) {
    const char *who = "fcr_feasibility_project_press";
    if (!f) return fail(FCR_EINVAL, "%s: parameters is NULL", who);
    if (B < 0) return fail(FCR_EINVAL, "%s: B=%d must be >= 0", who, B);
    feasibility::FeasArgs fa{};
    if (const int rc = feasibility_args(who, f, &fa)) return rc;
    plant::UniformParams mp;
    if (const int rc = press_model(who, model, &mp)) return rc;
    if (B == 0) return FCR_OK;
    if (!x || !u_nn || !u || !flag) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (((((uintptr_t)x) | ((uintptr_t)u_nn) | ((uintptr_t)u) | ((uintptr_t)v)) & 7) || (((uintptr_t)flag) & 3))
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte and flag 4-byte aligned", who);
    hipLaunchKernelGGL(feasibility::feasibility_project_press_kernel,
                       dim3((B + feasibility::kFeasBlock - 1) / feasibility::kFeasBlock), dim3(feasibility::kFeasBlock), 0,
                       (hipStream_t)stream, fa, mp, B, x, u_nn, u, flag, v);
    return launch_check("feasibility_project_press_kernel");
}

}  // extern "C"

namespace {

int run_bank(const char *who, const fcr_closed_loop_bank *c, const closed_loop::PressTable *table,
             const plant::UniformParams *model, void *stream) {
    if (!c) return fail(FCR_EINVAL, "%s: args is NULL", who);
    if (c->n_models < 0) return fail(FCR_EINVAL, "%s: n_models=%d must be >= 0", who, c->n_models);
    if (c->B < 0 || c->T < 0) return fail(FCR_EINVAL, "%s: B=%d, T=%d must be >= 0", who, c->B, c->T);
    if (const int rc = check_step(who, "", c->ts, c->substeps)) return rc;
    if (c->smooth != 0 && c->smooth != 1) return fail(FCR_EINVAL, "%s: smooth=%d must be 0 or 1", who, c->smooth);
    if (c->ctrl_hidden < 1 || c->ctrl_hidden > closed_loop::kClMaxHidden)
        return fail(FCR_EUNSUPPORTED, "%s: ctrl_hidden=%d: built for 1..%d", who, c->ctrl_hidden, closed_loop::kClMaxHidden);
    if (!(c->in_scale[0] > 0.0) || !(c->in_scale[1] > 0.0) || !(c->ref_scale > 0.0) || !(c->out_scale > 0.0))
        return fail(FCR_EINVAL, "%s: scaler scales must be positive", who);
    if (!(c->p1_lo < c->p1_hi) || !(c->p2_lo < c->p2_hi))
        return fail(FCR_EINVAL, "%s: pressure bounds p1 [%g, %g], p2 [%g, %g] need lo < hi", who, c->p1_lo, c->p1_hi,
                    c->p2_lo, c->p2_hi);
    if (c->x0_stride < 0 || c->ref_stride < 0 || c->process_noise_stride < 0 || c->meas_noise_stride < 0)
        return fail(FCR_EINVAL, "%s: a model stride is negative", who);
    feasibility::FeasArgs fa{};
    if (c->feasibility)
        if (const int rc = feasibility_args(who, c->feasibility, &fa)) return rc;
    const long long bpm = ((long long)c->B + closed_loop::kClBlock - 1) / closed_loop::kClBlock;
    if (c->n_models * bpm > INT32_MAX || (long long)c->n_models * c->B * ((long long)c->T + 1) * 5 > (1LL << 40))
        return fail(FCR_EINVAL, "%s: n_models*B*(T+1) too large", who);
    if (c->n_models == 0 || c->B == 0) return FCR_OK;
    if (table)
        if (const int rc = press_pointer(who, table->press)) return rc;
    if (!c->x0 || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out || !c->traj_stats || !c->traj_counts || !c->x_final ||
        !c->summary || (c->T > 0 && !c->ref))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    const bool recover = c->T > 0 && c->feasibility;
    if (c->x ? (c->T > 0 && (!c->u || (recover && (!c->u_nn || !c->feas_flag)))) : (c->u || c->u_nn || c->feas_flag))
        return fail(FCR_EINVAL, "%s: x, u (and u_nn, feas_flag with feasibility) are stored together: all set, or all NULL "
                                "to store nothing per step", who);
    if ((((uintptr_t)c->x0) | ((uintptr_t)c->ref) | ((uintptr_t)c->x) | ((uintptr_t)c->u) | ((uintptr_t)c->u_nn) |
         ((uintptr_t)c->process_noise) | ((uintptr_t)c->meas_noise) | ((uintptr_t)c->traj_stats) | ((uintptr_t)c->x_final) |
         ((uintptr_t)c->summary)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    if ((((uintptr_t)c->feas_flag) | ((uintptr_t)c->traj_counts) | ((uintptr_t)c->ctrl_w_inp) | ((uintptr_t)c->ctrl_b_inp) |
         ((uintptr_t)c->ctrl_w_out)) & 3)
        return fail(FCR_EINVAL, "%s: int32 and fp32 buffers must be 4-byte aligned", who);
    closed_loop::ClArgs a{c->B, c->T, c->substeps, c->ctrl_hidden, c->ts / c->substeps, c->x0, c->ref,
                          c->ctrl_w_inp, c->ctrl_b_inp, c->ctrl_w_out, c->in_scale[0], c->in_scale[1],
                          c->ref_scale, c->out_scale, c->x, c->u};
    const closed_loop::BankStrides st{c->x0_stride, c->ref_stride, c->process_noise_stride, c->meas_noise_stride};
    const closed_loop::StatsArgs sa{c->p1_lo, c->p1_hi, c->p2_lo, c->p2_hi, c->traj_stats, c->traj_counts, c->x_final};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(c->n_models * bpm)), block(closed_loop::kClBlock);
    // the single-model call's choice of instantiation; T = 0 copies x0 and writes zero statistics
    const bool sm = c->smooth, noise = c->T > 0 && (c->process_noise || c->meas_noise), store = c->x != nullptr;
    if (table && recover) {
        using feasibility::closed_loop_bank_recover_press_kernel;
        static constexpr decltype(&closed_loop_bank_recover_press_kernel<false, false, false>) k[2][2][2] = {
            {{closed_loop_bank_recover_press_kernel<false, false, false>, closed_loop_bank_recover_press_kernel<false, false, true>},
             {closed_loop_bank_recover_press_kernel<false, true, false>, closed_loop_bank_recover_press_kernel<false, true, true>}},
            {{closed_loop_bank_recover_press_kernel<true, false, false>, closed_loop_bank_recover_press_kernel<true, false, true>},
             {closed_loop_bank_recover_press_kernel<true, true, false>, closed_loop_bank_recover_press_kernel<true, true, true>}}};
        hipLaunchKernelGGL(k[sm][noise][store], grid, block, 0, s, a, fa, st, sa, c->process_noise, c->meas_noise, c->u_nn,
                           c->feas_flag, *table, *model);
    } else if (table) {
        using closed_loop::closed_loop_bank_press_kernel;
        static constexpr decltype(&closed_loop_bank_press_kernel<false, false, false>) k[2][2][2] = {
            {{closed_loop_bank_press_kernel<false, false, false>, closed_loop_bank_press_kernel<false, false, true>},
             {closed_loop_bank_press_kernel<false, true, false>, closed_loop_bank_press_kernel<false, true, true>}},
            {{closed_loop_bank_press_kernel<true, false, false>, closed_loop_bank_press_kernel<true, false, true>},
             {closed_loop_bank_press_kernel<true, true, false>, closed_loop_bank_press_kernel<true, true, true>}}};
        hipLaunchKernelGGL(k[sm][noise][store], grid, block, 0, s, a, st, sa, c->process_noise, c->meas_noise, *table);
    } else if (recover) {
        using feasibility::closed_loop_bank_recover_kernel;
        static constexpr decltype(&closed_loop_bank_recover_kernel<false, false, false>) k[2][2][2] = {
            {{closed_loop_bank_recover_kernel<false, false, false>, closed_loop_bank_recover_kernel<false, false, true>},
             {closed_loop_bank_recover_kernel<false, true, false>, closed_loop_bank_recover_kernel<false, true, true>}},
            {{closed_loop_bank_recover_kernel<true, false, false>, closed_loop_bank_recover_kernel<true, false, true>},
             {closed_loop_bank_recover_kernel<true, true, false>, closed_loop_bank_recover_kernel<true, true, true>}}};
        hipLaunchKernelGGL(k[sm][noise][store], grid, block, 0, s, a, fa, st, sa, c->process_noise, c->meas_noise, c->u_nn,
                           c->feas_flag);
    } else {
        using closed_loop::closed_loop_bank_kernel;
        static constexpr decltype(&closed_loop_bank_kernel<false, false, false>) k[2][2][2] = {
            {{closed_loop_bank_kernel<false, false, false>, closed_loop_bank_kernel<false, false, true>},
             {closed_loop_bank_kernel<false, true, false>, closed_loop_bank_kernel<false, true, true>}},
            {{closed_loop_bank_kernel<true, false, false>, closed_loop_bank_kernel<true, false, true>},
             {closed_loop_bank_kernel<true, true, false>, closed_loop_bank_kernel<true, true, true>}}};
        hipLaunchKernelGGL(k[sm][noise][store], grid, block, 0, s, a, st, sa, c->process_noise, c->meas_noise);
    }
    if (const int rc = launch_check(table ? (recover ? "closed_loop_bank_recover_press_kernel" : "closed_loop_bank_press_kernel")
                                          : (recover ? "closed_loop_bank_recover_kernel" : "closed_loop_bank_kernel")))
        return rc;
    const closed_loop::RedArgs ra{c->B, c->T, c->ref_stride, c->ref, c->traj_stats, c->traj_counts, c->summary};
    hipLaunchKernelGGL(closed_loop::loop_stats_reduce_kernel, dim3(c->n_models), dim3(closed_loop::kRedBlock), 0, s, ra);
    return launch_check("loop_stats_reduce_kernel");
}

}  // namespace

extern "C" {

int fcr_feasibility_project(const fcr_feasibility *f, int32_t B, const double *x, const double *u_nn, double *u,
                            int32_t *flag, double *v, void *stream) {
    if (!f) return fail(FCR_EINVAL, "fcr_feasibility_project: parameters is NULL");
    if (B < 0) return fail(FCR_EINVAL, "fcr_feasibility_project: B=%d must be >= 0", B);
    feasibility::FeasArgs fa{};
    if (const int rc = feasibility_args("fcr_feasibility_project", f, &fa)) return rc;
    if (B == 0) return FCR_OK;
    if (!x || !u_nn || !u || !flag) return fail(FCR_EINVAL, "fcr_feasibility_project: a required pointer is NULL");
    if (((((uintptr_t)x) | ((uintptr_t)u_nn) | ((uintptr_t)u) | ((uintptr_t)v)) & 7) || (((uintptr_t)flag) & 3))
        return fail(FCR_EINVAL, "fcr_feasibility_project: fp64 buffers must be 8-byte and flag 4-byte aligned");
    hipLaunchKernelGGL(feasibility::feasibility_project_kernel, dim3((B + feasibility::kFeasBlock - 1) / feasibility::kFeasBlock),
                       dim3(feasibility::kFeasBlock), 0, (hipStream_t)stream, fa, B, x, u_nn, u, flag, v);
    return launch_check("feasibility_project_kernel");
}

int fcr_supervised_epoch(const fcr_supervised *c, void *stream) {
    if (!c) return fail(FCR_EINVAL, "fcr_supervised_epoch: args is NULL");
    if (c->n_models < 0) return fail(FCR_EINVAL, "fcr_supervised_epoch: n_models=%d must be >= 0", c->n_models);
    if (c->n_samples < 1 || c->n_samples > (1 << 30))
        return fail(FCR_EINVAL, "fcr_supervised_epoch: n_samples=%d must be 1..2^30", c->n_samples);
    if (c->batch_size < 1) return fail(FCR_EINVAL, "fcr_supervised_epoch: batch_size=%d must be >= 1", c->batch_size);
    if (c->hidden < 1 || c->hidden > fnn::kFnnMaxHidden)
        return fail(FCR_EUNSUPPORTED, "fcr_supervised_epoch: hidden=%d: built for 1..%d", c->hidden, fnn::kFnnMaxHidden);
    if (c->loss_kind != FCR_LOSS_L1 && c->loss_kind != FCR_LOSS_MSE)
        return fail(FCR_EINVAL, "fcr_supervised_epoch: loss_kind=%d must be FCR_LOSS_L1 or FCR_LOSS_MSE", c->loss_kind);
    if (c->train != 0 && c->train != 1) return fail(FCR_EINVAL, "fcr_supervised_epoch: train=%d must be 0 or 1", c->train);
    if (c->train) {
        if (!(c->lr >= 0.0) || !(c->eps >= 0.0) || !(c->weight_decay >= 0.0) || !(c->beta1 >= 0.0 && c->beta1 < 1.0) ||
            !(c->beta2 >= 0.0 && c->beta2 < 1.0))
            return fail(FCR_EINVAL, "fcr_supervised_epoch: AdamW needs lr, eps, weight_decay >= 0 and betas in [0, 1)");
    }
    if (c->n_models == 0) return FCR_OK;
    if (!c->X || !c->y || !c->w_inp || !c->b_inp || !c->w_out || !c->loss)
        return fail(FCR_EINVAL, "fcr_supervised_epoch: a required pointer is NULL");
    if (c->train && !c->perm) return fail(FCR_EINVAL, "fcr_supervised_epoch: perm is NULL with train set");
    if (c->train && (!c->exp_avg_w_inp || !c->exp_avg_b_inp || !c->exp_avg_w_out || !c->exp_avg_sq_w_inp ||
                     !c->exp_avg_sq_b_inp || !c->exp_avg_sq_w_out || !c->step))
        return fail(FCR_EINVAL, "fcr_supervised_epoch: a moment or step pointer is NULL with train set");
    const int nb = (int)(((long long)c->n_samples + c->batch_size - 1) / c->batch_size);
    supervised::SlArgs a{c->n_samples, c->batch_size, nb, c->hidden, c->lr, c->beta1, c->beta2,
                         (float)(1.0 - c->lr * c->weight_decay), (float)c->eps, c->X, c->y, c->perm,
                         c->w_inp, c->b_inp, c->w_out, c->exp_avg_w_inp, c->exp_avg_b_inp, c->exp_avg_w_out,
                         c->exp_avg_sq_w_inp, c->exp_avg_sq_b_inp, c->exp_avg_sq_w_out, c->step, c->loss};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(c->n_models), block(supervised::kSlBlock);
    if (c->train && c->loss_kind == FCR_LOSS_L1)
        hipLaunchKernelGGL((supervised::sl_epoch_kernel<supervised::kLossL1, true>), grid, block, 0, s, a);
    else if (c->train)
        hipLaunchKernelGGL((supervised::sl_epoch_kernel<supervised::kLossMse, true>), grid, block, 0, s, a);
    else if (c->loss_kind == FCR_LOSS_L1)
        hipLaunchKernelGGL((supervised::sl_epoch_kernel<supervised::kLossL1, false>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((supervised::sl_epoch_kernel<supervised::kLossMse, false>), grid, block, 0, s, a);
    return launch_check("sl_epoch_kernel");
}

}  // extern "C"
