// fcr_press_host.h — host-only: the argument checks the press rows' entry points share (fcr_rows.hip: plant, closed
// loop, bank, projection; fcr_grad.hip: their adjoints), and the one way a launch picks a kernel template's instantiation
// from run-time flags. Every check takes the entry point's name, fails through fail() and makes no device call.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "fcr.h"
#include "fcr_host.h"
#include "fcr_plant.h"

namespace fcr {

// ts / substeps of an RK4 integrator (what: "" or the name of whose they are), or a message
inline int check_step(const char *who, const char *what, double ts, int substeps) {
    if (substeps < 1 || substeps > 4096) return fail(FCR_EINVAL, "%s: %ssubsteps=%d must be 1..4096", who, what, substeps);
    if (!(ts > 0.0) || ts > 1e6) return fail(FCR_EINVAL, "%s: %sts=%g must be a positive time step", who, what, ts);
    return FCR_OK;
}

inline int check_smooth(const char *who, int smooth) {
    if (smooth != 0 && smooth != 1) return fail(FCR_EINVAL, "%s: smooth=%d must be 0 or 1", who, smooth);
    return FCR_OK;
}

// B trajectories of S steps (steps: the entry point's name of S, "S" or "T"): the ranges and, with `bound`, the size of
// the (B, S+1, 5) record
inline int check_batch(const char *who, int B, int S, const char *steps, bool bound = true) {
    if (B < 0 || S < 0) return fail(FCR_EINVAL, "%s: B=%d, %s=%d must be >= 0", who, B, steps, S);
    if (bound && (long long)B * (S + 1) * 5 > (1LL << 40)) return fail(FCR_EINVAL, "%s: B*(%s+1) too large", who, steps);
    return FCR_OK;
}

// the fields fcr_closed_loop, fcr_closed_loop_bank and fcr_closed_loop_grad begin with: batch, step, smooth and the
// controller block (its width against the caller's kernels' maximum, the four scales). bound: as check_batch
template <class C>
int check_loop(const char *who, const C *c, int max_hidden, bool bound) {
    if (!c) return fail(FCR_EINVAL, "%s: args is NULL", who);
    if (const int rc = check_batch(who, c->B, c->T, "T", bound)) return rc;
    if (const int rc = check_step(who, "", c->ts, c->substeps)) return rc;
    if (const int rc = check_smooth(who, c->smooth)) return rc;
    if (c->ctrl_hidden < 1 || c->ctrl_hidden > max_hidden)
        return fail(FCR_EUNSUPPORTED, "%s: ctrl_hidden=%d: built for 1..%d", who, c->ctrl_hidden, max_hidden);
    if (!(c->in_scale[0] > 0.0) || !(c->in_scale[1] > 0.0) || !(c->ref_scale > 0.0) || !(c->out_scale > 0.0))
        return fail(FCR_EINVAL, "%s: scaler scales must be positive", who);
    return FCR_OK;
}

// a parameter table's strides (include/fcr.h), or a message
inline int check_table_strides(const char *who, long long stride_model, long long stride_traj, int B) {
    if (stride_model < 0 || stride_traj < 0)
        return fail(FCR_EINVAL, "%s: a parameter stride is negative (model %lld, trajectory %lld)", who, stride_model, stride_traj);
    if (stride_traj % plant::kPressFields)
        return fail(FCR_EINVAL, "%s: stride_traj=%lld must be 0 (shared) or a multiple of %d", who, stride_traj, plant::kPressFields);
    if (stride_model && (stride_model % plant::kPressFields || stride_model < (long long)B * stride_traj))
        return fail(FCR_EINVAL, "%s: stride_model=%lld must be 0 (shared) or a multiple of %d that is >= B * stride_traj = %lld",
                    who, stride_model, plant::kPressFields, (long long)B * stride_traj);
    return FCR_OK;
}

// a parameter table's pointer, or a message. required (*_press): NULL is refused — asked once the call is known not to be
// empty, B = 0 reads no row. Otherwise (*_vjp) NULL is the reference's press, and then the stride must be 0
inline int check_table_pointer(const char *who, const double *press, bool required, long long stride_traj = 0) {
    if (!press && required) return fail(FCR_EINVAL, "%s: the parameter table is NULL", who);
    if (!press && stride_traj) return fail(FCR_EINVAL, "%s: stride_traj=%lld without a parameter table", who, stride_traj);
    if (((uintptr_t)press) & 7) return fail(FCR_EINVAL, "%s: the parameter table must be 8-byte aligned (fp64)", who);
    return FCR_OK;
}

static_assert(sizeof(fcr_press) == plant::kPressFields * sizeof(double), "fcr_press is one row of a parameter table");

// a host-side press (the model a projection integrates; NULL: the reference's) -> its coefficients, or a message
inline int press_model(const char *who, const fcr_press *model, plant::UniformParams *out) {
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

// Run-time flags -> template arguments: select(f, a, b, ...) is f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...).
// A kernel family names its template once, in f, which returns the instantiation's address; every combination of the
// flags is instantiated, exactly the entries of a k[2]...[2] table of them.
template <class F>
constexpr auto select(F f) {
    return f();
}
template <class F, class... Flags>
constexpr auto select(F f, bool flag, Flags... flags) {
    return flag ? select([f](auto... rest) { return f(std::true_type{}, rest...); }, flags...)
                : select([f](auto... rest) { return f(std::false_type{}, rest...); }, flags...);
}

}  // namespace fcr
