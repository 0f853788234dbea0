// fcr_rows.hip — C ABI of the SURVEY.md §8(f) rows that need no rollout state: the batched press plant
// (fcr_plant.h), the controller + press closed loop (fcr_closed_loop.h), its feasibility recovery
// (fcr_feasibility.h), the training-window gather (fcr_window.h) and the supervised baseline's epoch (fcr_supervised.h).
// Validation before any device call; stream-ordered launches; no allocation. The press rows' checks and their choice of
// a kernel instantiation are fcr_press_host.h's, shared with fcr_grad.hip; an entry point and its *_press twin are one
// function below, and the single-model loop and the bank fill the kernels' arguments from one place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr.h"
#include "fcr_closed_loop.h"
#include "fcr_feasibility.h"
#include "fcr_host.h"
#include "fcr_plant.h"
#include "fcr_press_host.h"
#include "fcr_press_noise_host.h"
#include "fcr_supervised.h"
#include "fcr_window.h"

using namespace fcr;

namespace {

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

// fcr_plant_rk4 (table = false: the reference's press, the kernel without parameters) and fcr_plant_rk4_press
int plant_rk4(const char *who, bool table, int B, int S, double ts, int substeps, int smooth, const double *x0,
              const double *u, double *x, const double *press, long long stride_traj, void *stream) {
    if (const int rc = check_batch(who, B, S, "S")) return rc;
    if (const int rc = check_step(who, "", ts, substeps)) return rc;
    if (const int rc = check_smooth(who, smooth)) return rc;
    if (table)
        if (const int rc = check_table_strides(who, 0, stride_traj, B)) return rc;
    if (B == 0) return FCR_OK;
    if (table)
        if (const int rc = check_table_pointer(who, press, true)) return rc;
    if (!x0 || !x || (S > 0 && !u)) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)x0) | ((uintptr_t)u) | ((uintptr_t)x)) & 7)
        return fail(FCR_EINVAL, "%s: buffers must be 8-byte aligned (fp64)", who);
    const dim3 grid((B + plant::kPlantBlock - 1) / plant::kPlantBlock), block(plant::kPlantBlock);
    hipStream_t s = (hipStream_t)stream;
    const double dt = ts / substeps;
    if (table) {
        const auto k = select([](auto sm) { return &plant::plant_rk4_press_kernel<sm()>; }, smooth);
        hipLaunchKernelGGL(k, grid, block, 0, s, B, S, dt, substeps, x0, u, x, press, stride_traj);
    } else {
        const auto k = select([](auto sm) { return &plant::plant_rk4_kernel<sm()>; }, smooth);
        hipLaunchKernelGGL(k, grid, block, 0, s, B, S, dt, substeps, x0, u, x);
    }
    return launch_check(table ? "plant_rk4_press_kernel" : "plant_rk4_kernel");
}

// fcr_feasibility_project (with_model = false: the kernel without parameters) and fcr_feasibility_project_press (model
// NULL: the reference's press through the kernel with parameters)
int project(const char *who, bool with_model, const fcr_feasibility *f, const fcr_press *model, int B, const double *x,
            const double *u_nn, double *u, int32_t *flag, double *v, void *stream) {
    if (!f) return fail(FCR_EINVAL, "%s: parameters is NULL", who);
    if (B < 0) return fail(FCR_EINVAL, "%s: B=%d must be >= 0", who, B);
    feasibility::FeasArgs fa{};
    if (const int rc = feasibility_args(who, f, &fa)) return rc;
    plant::UniformParams mp;
    if (with_model)
        if (const int rc = press_model(who, model, &mp)) return rc;
    if (B == 0) return FCR_OK;
    if (!x || !u_nn || !u || !flag) return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if (((((uintptr_t)x) | ((uintptr_t)u_nn) | ((uintptr_t)u) | ((uintptr_t)v)) & 7) || (((uintptr_t)flag) & 3))
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte and flag 4-byte aligned", who);
    const dim3 grid((B + feasibility::kFeasBlock - 1) / feasibility::kFeasBlock), block(feasibility::kFeasBlock);
    if (with_model)
        hipLaunchKernelGGL(feasibility::feasibility_project_press_kernel, grid, block, 0, (hipStream_t)stream, fa, mp, B, x,
                           u_nn, u, flag, v);
    else
        hipLaunchKernelGGL(feasibility::feasibility_project_kernel, grid, block, 0, (hipStream_t)stream, fa, B, x, u_nn, u,
                           flag, v);
    return launch_check(with_model ? "feasibility_project_press_kernel" : "feasibility_project_kernel");
}

// The loop kernels' arguments and their choice of instantiation from the fields fcr_closed_loop and fcr_closed_loop_bank
// share. T = 0 only copies x0 (the bank: and writes zero statistics), so it runs the plain instantiation
struct Loop {
    closed_loop::ClArgs a;
    bool smooth, noise, recover;
};
template <class C>
Loop loop_of(const C *c) {
    return {{c->B, c->T, c->substeps, c->ctrl_hidden, c->ts / c->substeps, c->x0, c->ref, c->ctrl_w_inp, c->ctrl_b_inp,
             c->ctrl_w_out, c->in_scale[0], c->in_scale[1], c->ref_scale, c->out_scale, c->x, c->u},
            c->smooth != 0, c->T > 0 && (c->process_noise || c->meas_noise), c->T > 0 && c->feasibility};
}

// fcr_closed_loop_run_bank (table = null: the reference's press, the kernels without parameters) and
// fcr_closed_loop_run_bank_press (table's strides and model: checked by the caller)
// and fcr_closed_loop_run_bank_press_state (state: the storing run that also writes the unperturbed states to x_state,
// fcr_press_noise.hip's kernels; table = null there too is the reference's press)
int run_bank(const char *who, const fcr_closed_loop_bank *c, const closed_loop::PressTable *table,
             const plant::UniformParams *model, void *stream, bool state = false, double *x_state = nullptr) {
    if (state && c->feasibility)
        return fail(FCR_EUNSUPPORTED, "%s: x_state is stored by the loop without feasibility recovery", who);
    if (c->n_models < 0) return fail(FCR_EINVAL, "%s: n_models=%d must be >= 0", who, c->n_models);
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
        if (const int rc = check_table_pointer(who, table->press, true)) return rc;
    if (!c->x0 || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out || !c->traj_stats || !c->traj_counts || !c->x_final ||
        !c->summary || (c->T > 0 && !c->ref))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    const Loop l = loop_of(c);
    if (c->x ? (c->T > 0 && (!c->u || (l.recover && (!c->u_nn || !c->feas_flag)))) : (c->u || c->u_nn || c->feas_flag))
        return fail(FCR_EINVAL, "%s: x, u (and u_nn, feas_flag with feasibility) are stored together: all set, or all NULL "
                                "to store nothing per step", who);
    if ((((uintptr_t)c->x0) | ((uintptr_t)c->ref) | ((uintptr_t)c->x) | ((uintptr_t)c->u) | ((uintptr_t)c->u_nn) |
         ((uintptr_t)c->process_noise) | ((uintptr_t)c->meas_noise) | ((uintptr_t)c->traj_stats) | ((uintptr_t)c->x_final) |
         ((uintptr_t)c->summary)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    if ((((uintptr_t)c->feas_flag) | ((uintptr_t)c->traj_counts) | ((uintptr_t)c->ctrl_w_inp) | ((uintptr_t)c->ctrl_b_inp) |
         ((uintptr_t)c->ctrl_w_out)) & 3)
        return fail(FCR_EINVAL, "%s: int32 and fp32 buffers must be 4-byte aligned", who);
    if (state && (!x_state || !c->x)) return fail(FCR_EINVAL, "%s: x_state is stored beside x: both are required", who);
    if (((uintptr_t)x_state) & 7) return fail(FCR_EINVAL, "%s: x_state must be 8-byte aligned (fp64)", who);
    const closed_loop::BankStrides st{c->x0_stride, c->ref_stride, c->process_noise_stride, c->meas_noise_stride};
    const closed_loop::StatsArgs sa{c->p1_lo, c->p1_hi, c->p2_lo, c->p2_hi, c->traj_stats, c->traj_counts, c->x_final};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(c->n_models * bpm)), block(closed_loop::kClBlock);
    const bool store = c->x != nullptr;
    const char *what;
    if (state) {
        if (const int rc = press_noise::launch_bank_state(l.a, st, sa, c->process_noise, c->meas_noise, table, l.smooth,
                                                          x_state, grid, s))
            return rc;
        what = "closed_loop_bank_state_kernel";
    } else if (table && l.recover) {
        const auto k = select([](auto sm, auto noise, auto store) {
            return &feasibility::closed_loop_bank_recover_press_kernel<sm(), noise(), store()>; }, l.smooth, l.noise, store);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a, fa, st, sa, c->process_noise, c->meas_noise, c->u_nn, c->feas_flag,
                           *table, *model);
        what = "closed_loop_bank_recover_press_kernel";
    } else if (table) {
        const auto k = select([](auto sm, auto noise, auto store) {
            return &closed_loop::closed_loop_bank_press_kernel<sm(), noise(), store()>; }, l.smooth, l.noise, store);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a, st, sa, c->process_noise, c->meas_noise, *table);
        what = "closed_loop_bank_press_kernel";
    } else if (l.recover) {
        const auto k = select([](auto sm, auto noise, auto store) {
            return &feasibility::closed_loop_bank_recover_kernel<sm(), noise(), store()>; }, l.smooth, l.noise, store);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a, fa, st, sa, c->process_noise, c->meas_noise, c->u_nn, c->feas_flag);
        what = "closed_loop_bank_recover_kernel";
    } else {
        const auto k = select([](auto sm, auto noise, auto store) {
            return &closed_loop::closed_loop_bank_kernel<sm(), noise(), store()>; }, l.smooth, l.noise, store);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a, st, sa, c->process_noise, c->meas_noise);
        what = "closed_loop_bank_kernel";
    }
    if (const int rc = launch_check(what)) return rc;
    const closed_loop::RedArgs ra{c->B, c->T, c->ref_stride, c->ref, c->traj_stats, c->traj_counts, c->summary};
    hipLaunchKernelGGL(closed_loop::loop_stats_reduce_kernel, dim3(c->n_models), dim3(closed_loop::kRedBlock), 0, s, ra);
    return launch_check("loop_stats_reduce_kernel");
}

}  // namespace

extern "C" {

void fcr_press_nominal(fcr_press *out) {
    if (!out) return;
    *out = fcr_press{plant::M_MASS, plant::B_DAMP, plant::FT, plant::D1, plant::D2, plant::G, plant::KB, plant::V1_0,
                     plant::V2_0, plant::KL_1, plant::KL_2, plant::CD, plant::RHO, plant::D, plant::PS, plant::PT,
                     plant::MU, plant::K, plant::W0, plant::H0, plant::B0, plant::T_DEF, plant::T1, plant::M0,
                     plant::M1, plant::M2, plant::M3, plant::M4};
}

int fcr_plant_rk4(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x0,
                  const double *u, double *x, void *stream) {
    return plant_rk4("fcr_plant_rk4", false, B, S, ts, substeps, smooth, x0, u, x, nullptr, 0, stream);
}

int fcr_plant_rk4_press(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x0,
                        const double *u, double *x, const double *press, int64_t stride_traj, void *stream) {
    return plant_rk4("fcr_plant_rk4_press", true, B, S, ts, substeps, smooth, x0, u, x, press, stride_traj, stream);
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

// the single-model kernels write no statistics: this is not the bank with one model
int fcr_closed_loop_run(const fcr_closed_loop *c, void *stream) {
    const char *who = "fcr_closed_loop_run";
    if (const int rc = check_loop(who, c, closed_loop::kClMaxHidden, false)) return rc;
    if (c->B == 0) return FCR_OK;
    if (!c->x0 || !c->x || !c->ctrl_w_inp || !c->ctrl_b_inp || !c->ctrl_w_out || (c->T > 0 && (!c->ref || !c->u)))
        return fail(FCR_EINVAL, "%s: a required pointer is NULL", who);
    if ((((uintptr_t)c->x0) | ((uintptr_t)c->ref) | ((uintptr_t)c->x) | ((uintptr_t)c->u)) & 7)
        return fail(FCR_EINVAL, "%s: fp64 buffers must be 8-byte aligned", who);
    if ((((uintptr_t)c->process_noise) | ((uintptr_t)c->meas_noise)) & 7)
        return fail(FCR_EINVAL, "%s: noise buffers must be 8-byte aligned (fp64)", who);
    feasibility::FeasArgs fa{};
    if (c->feasibility) {
        if (const int rc = feasibility_args(who, c->feasibility, &fa)) return rc;
        if (c->T > 0 && (!c->u_nn || !c->feas_flag))
            return fail(FCR_EINVAL, "%s: u_nn or feas_flag is NULL with feasibility set", who);
        if ((((uintptr_t)c->u_nn) & 7) || (((uintptr_t)c->feas_flag) & 3))
            return fail(FCR_EINVAL, "%s: u_nn must be 8-byte and feas_flag 4-byte aligned", who);
    }
    const Loop l = loop_of(c);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((c->B + closed_loop::kClBlock - 1) / closed_loop::kClBlock), block(closed_loop::kClBlock);
    // one loop (closed_loop::loop_body), instantiated per [smooth] and, with recovery, [noise]
    if (l.recover) {
        const auto k = select([](auto sm, auto noise) { return &feasibility::closed_loop_recover_kernel<sm(), noise()>; },
                              l.smooth, l.noise);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a, fa, c->process_noise, c->meas_noise, c->u_nn, c->feas_flag);
    } else if (l.noise) {
        const auto k = select([](auto sm) { return &closed_loop::closed_loop_noise_kernel<sm()>; }, l.smooth);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a, c->process_noise, c->meas_noise);
    } else {
        const auto k = select([](auto sm) { return &closed_loop::closed_loop_kernel<sm()>; }, l.smooth);
        hipLaunchKernelGGL(k, grid, block, 0, s, l.a);
    }
    return launch_check(l.recover ? "closed_loop_recover_kernel" : (l.noise ? "closed_loop_noise_kernel" : "closed_loop_kernel"));
}

int fcr_closed_loop_run_bank(const fcr_closed_loop_bank *c, void *stream) {
    const char *who = "fcr_closed_loop_run_bank";
    if (const int rc = check_loop(who, c, closed_loop::kClMaxHidden, false)) return rc;
    return run_bank(who, c, nullptr, nullptr, stream);
}

int fcr_closed_loop_run_bank_press(const fcr_closed_loop_bank *c, const double *press, int64_t stride_model,
                                   int64_t stride_traj, const fcr_press *model, void *stream) {
    const char *who = "fcr_closed_loop_run_bank_press";
    if (const int rc = check_loop(who, c, closed_loop::kClMaxHidden, false)) return rc;
    if (const int rc = check_table_strides(who, stride_model, stride_traj, c->B)) return rc;
    plant::UniformParams mp;
    if (const int rc = press_model(who, model, &mp)) return rc;
    const closed_loop::PressTable table{press, (long long)stride_model, (long long)stride_traj};
    return run_bank(who, c, &table, &mp, stream);
}

int fcr_closed_loop_run_bank_press_state(const fcr_closed_loop_bank *c, const double *press, int64_t stride_model,
                                         int64_t stride_traj, const fcr_press *model, double *x_state, void *stream) {
    const char *who = "fcr_closed_loop_run_bank_press_state";
    if (const int rc = check_loop(who, c, closed_loop::kClMaxHidden, false)) return rc;
    if (const int rc = check_table_strides(who, stride_model, stride_traj, c->B)) return rc;
    if (const int rc = check_table_pointer(who, press, false, stride_traj)) return rc;
    if (!press && stride_model)
        return fail(FCR_EINVAL, "%s: stride_model=%lld without a parameter table", who, (long long)stride_model);
    plant::UniformParams mp;
    if (const int rc = press_model(who, model, &mp)) return rc;
    const closed_loop::PressTable table{press, (long long)stride_model, (long long)stride_traj};
    return run_bank(who, c, press ? &table : nullptr, &mp, stream, true, x_state);
}

int fcr_feasibility_project(const fcr_feasibility *f, int32_t B, const double *x, const double *u_nn, double *u,
                            int32_t *flag, double *v, void *stream) {
    return project("fcr_feasibility_project", false, f, nullptr, B, x, u_nn, u, flag, v, stream);
}

int fcr_feasibility_project_press(const fcr_feasibility *f, const fcr_press *model, int32_t B, const double *x,
                                  const double *u_nn, double *u, int32_t *flag, double *v, void *stream) {
    return project("fcr_feasibility_project_press", true, f, model, B, x, u_nn, u, flag, v, stream);
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
