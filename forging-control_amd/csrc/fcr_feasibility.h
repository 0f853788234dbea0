// fcr_feasibility.h — the reference's feasibility recovery as an on-GPU projection, one lane per state, and the
// closed loop that applies it at every step ("Feasibility recovery").
//
// Reference: FeasibilityRecovery.feasibility_recover solves, per step and trajectory, the NLP of UL/Main.py:584-657
// with CasADi/IPOPT: one scalar u, two slacks s >= 0 that appear in the cost (:624) and in no constraint (:641-646),
// so s = 0 at the optimum, and what is left is
//   min (u_NN - u)^2   s.t.   LB <= p1(X1), p1(X2), p2(X1), p2(X2) <= UB,   X1 = F(x, u), X2 = F(X1, u)
// with F = Ruge_Kuta(TS, forging_model) (M = 4, the non-smooth model) and the bounds 0 / 32e6 (:118-119) — the
// projection of one number onto a feasible set on the line. With the pressures scaled by 1/32e6 (:603-610)
//   v(x, u) = max over {p1(X1), p1(X2), p2(X1), p2(X2)} of max(lo - p, p - hi),
// u is feasible iff v <= 0 (a NaN v is infeasible), and the search below finds the feasible point nearest u_NN
// wherever the feasible set is an interval on the probed side:
//   flag 0  v(x, u_NN) <= 0: u_NN itself, bit for bit (the NLP has no bound on u);
//   flag 1  for k = 0..expand probe c- = clip(u_NN - d 2^k), c+ = clip(u_NN + d 2^k), d = (u_hi - u_lo)/2^expand,
//           stop at the first k with a feasible probe (both: the nearer, ties to c-), bisect between it and the
//           previous (infeasible) probe on that side `bisect` times; the result is the feasible end;
//   flag 2  no probe feasible: clip(u_NN, u_lo, u_hi), the reference's `except` branch.
//
// Cost: one v is 2 steps x substeps x 4 = 32 right-hand sides beside the plant step's 16; a lane that needs the
// search runs up to 2 (expand + 1) + bisect = 52 more. The search is ONE loop of fixed trip count over "the next
// candidate" with per-lane predicates (no early return), so the integrator is inlined once, not once per phase,
// and a wave leaves an iteration as soon as none of its lanes needs it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr_closed_loop.h"
#include "fcr_plant.h"

namespace fcr {
namespace feasibility {

constexpr int kFeasBlock = 256;
constexpr double kPScale = 1.0 / 32e6;          // scaling_factors['p1'] = ['p2'], UL/Main.py:607-608

struct FeasArgs {
    double lo1, hi1, lo2, hi2;                  // scaled by kPScale on the host
    double u_lo, u_hi, dt;
    int substeps, expand, bisect;
};

struct Projected {
    double u, v;
    int flag;
};

__device__ __forceinline__ double clip(double c, double lo, double hi) { return c < lo ? lo : (c > hi ? hi : c); }

// max that keeps a NaN once it has one (np.maximum), so a NaN pressure makes v NaN and v <= 0 false
__device__ __forceinline__ double nan_max(double v, double t) { return (t > v || t != t) ? t : v; }

// P: the press the projection's model integrates (plant::Nominal, or plant::UniformParams: one set per launch)
template <class P = plant::Nominal>
__device__ __forceinline__ double violation(const double (&x)[5], double u, const FeasArgs &f, P p = {}) {
    double xs[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) xs[i] = x[i];
    double v = -HUGE_VAL;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        plant::rk4_step<false, false>(xs, u, f.dt, f.substeps, nullptr, p);
        const double p1 = xs[2] * kPScale, p2 = xs[3] * kPScale;
        v = nan_max(v, nan_max(f.lo1 - p1, p1 - f.hi1));
        v = nan_max(v, nan_max(f.lo2 - p2, p2 - f.hi2));
    }
    return v;
}

template <class P = plant::Nominal>
__device__ __forceinline__ Projected project(const double (&x)[5], double u_nn, const FeasArgs &f, P p = {}) {
    const double delta = (f.u_hi - f.u_lo) / (double)(1 << f.expand);
    const int n_probe = 2 * (f.expand + 1), n_it = 1 + n_probe + f.bisect;
    double a = u_nn, g = u_nn, vg = 0.0;        // the bracket: a infeasible, g feasible (once found)
    double v0 = 0.0, cm = u_nn, vm = 0.0;       // v(u_nn); this k's c- and its v
    double prev_m = u_nn, prev_p = u_nn, vlast_m = 0.0, vlast_p = 0.0;
    bool need = true, found = false;            // need: u_nn infeasible; found: a feasible probe brackets the crossing
#pragma unroll 1
    for (int it = 0; it < n_it; ++it) {
        const int k = (it - 1) >> 1;
        const bool probing = it >= 1 && it <= n_probe, plus = probing && ((it - 1) & 1);   // c- first, then c+
        const bool minus = probing && !plus;
        double c = u_nn;
        if (probing) {
            const double step = delta * (double)(1 << k);
            c = clip(minus ? u_nn - step : u_nn + step, f.u_lo, f.u_hi);
        } else if (it > n_probe) {
            c = 0.5 * (a + g);
        }
        const bool active = it == 0 || (probing ? need && !found : found);
        if (active) {
            const double vc = violation(x, c, f, p);
            const bool ok = vc <= 0.0;
            if (it == 0) {
                v0 = vc;
                need = !ok;
            } else if (minus) {
                cm = c;
                vm = vc;
            } else if (plus) {
                const bool ok_m = vm <= 0.0;
                if (ok_m || ok) {
                    const bool take_m = ok_m && (!ok || fabs(u_nn - cm) <= fabs(c - u_nn));
                    g = take_m ? cm : c;
                    vg = take_m ? vm : vc;
                    a = k == 0 ? u_nn : (take_m ? prev_m : prev_p);
                    found = true;
                }
                prev_m = cm;
                prev_p = c;
                vlast_m = vm;
                vlast_p = vc;
            } else if (ok) {
                g = c;
                vg = vc;
            } else {
                a = c;
            }
        }
    }
    Projected r;
    if (!need) {
        r.u = u_nn, r.v = v0, r.flag = 0;
    } else if (found) {
        r.u = g, r.v = vg, r.flag = 1;
    } else {   // clip(u_nn) is u_nn inside the range and the last probe on its side outside it
        r.u = clip(u_nn, f.u_lo, f.u_hi);
        r.v = u_nn > f.u_hi ? vlast_p : (u_nn < f.u_lo ? vlast_m : v0);
        r.flag = 2;
    }
    return r;
}

// The stand-alone projection: x (B,5), u_nn (B) -> u (B), flag (B), v (B) or null.
__global__ __launch_bounds__(kFeasBlock) void feasibility_project_kernel(FeasArgs f, int B, const double *__restrict__ x,
                                                                         const double *__restrict__ u_nn,
                                                                         double *__restrict__ u, int32_t *__restrict__ flag,
                                                                         double *__restrict__ v) {
    const int b = blockIdx.x * kFeasBlock + threadIdx.x;
    if (b >= B) return;
    double xs[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) xs[i] = x[(size_t)b * 5 + i];
    const Projected r = project(xs, u_nn[b], f);
    u[b] = r.u;
    flag[b] = r.flag;
    if (v) v[b] = r.v;
}

// feasibility_project_kernel on a model press other than the reference's: its coefficients by value, in scalar registers.
__global__ __launch_bounds__(kFeasBlock) void feasibility_project_press_kernel(FeasArgs f, plant::UniformParams p, int B,
                                                                               const double *__restrict__ x,
                                                                               const double *__restrict__ u_nn,
                                                                               double *__restrict__ u,
                                                                               int32_t *__restrict__ flag,
                                                                               double *__restrict__ v) {
    const int b = blockIdx.x * kFeasBlock + threadIdx.x;
    if (b >= B) return;
    double xs[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) xs[i] = x[(size_t)b * 5 + i];
    const Projected r = project(xs, u_nn[b], f, p);
    u[b] = r.u;
    flag[b] = r.flag;
    if (v) v[b] = r.v;
}

// The command policy of the loop with recovery (closed_loop::loop_body): the projection of the controller's command
// from the record the controller read, between the controller and the press. Stores u_nn, u and flag. The projection's
// own model has no noise, is always the non-smooth one, has its own step (FeasArgs) and its own press P — the model's,
// which need not be the press the loop steps.
template <class P = plant::Nominal>
struct ProjectedCommand {
    FeasArgs f;
    double *u, *u_nn;
    int32_t *flag;
    P p;
    __device__ __forceinline__ ProjectedCommand row(size_t r) const { return {f, u + r, u_nn + r, flag + r, p}; }
    __device__ __forceinline__ double operator()(const double (&m)[5], double un, int t) const {
        const Projected r = project(m, un, f, p);
        u_nn[t] = un;
        u[t] = r.u;
        flag[t] = r.flag;
        return r.u;
    }
    // as called under closed_loop::LaneStats: the stores are optional, the flag goes to the lane's counts
    __device__ __forceinline__ double operator()(const double (&m)[5], double un, int t, bool store, int &fl) const {
        const Projected r = project(m, un, f, p);
        if (store) {
            u_nn[t] = un;
            u[t] = r.u;
            flag[t] = r.flag;
        }
        fl = r.flag;
        return r.u;
    }
};

template <bool SMOOTH, bool NOISE>
__global__ __launch_bounds__(closed_loop::kClBlock) void closed_loop_recover_kernel(closed_loop::ClArgs a, FeasArgs f,
                                                                                    const double *wn, const double *vn,
                                                                                    double *u_nn, int32_t *flag) {
    closed_loop::loop_body<SMOOTH, NOISE>(a, wn, vn, ProjectedCommand<>{f, a.u, u_nn, flag});
}

// closed_loop_bank_kernel with recovery: u_nn and flag are model-major like a.u, and null with it.
template <bool SMOOTH, bool NOISE, bool STORE>
__global__ __launch_bounds__(closed_loop::kClBlock) void closed_loop_bank_recover_kernel(
    closed_loop::ClArgs a, FeasArgs f, closed_loop::BankStrides strides, closed_loop::StatsArgs stats, const double *wn,
    const double *vn, double *u_nn, int32_t *flag) {
    closed_loop::loop_body<SMOOTH, NOISE>(a, wn, vn, ProjectedCommand<>{f, a.u, u_nn, flag},
                                          closed_loop::BankModel(a.B, strides), closed_loop::LaneStats<STORE>(stats));
}

// closed_loop_bank_recover_kernel where every trajectory has its own press and the projection integrates `model`.
template <bool SMOOTH, bool NOISE, bool STORE>
__global__ __launch_bounds__(closed_loop::kClBlock) void closed_loop_bank_recover_press_kernel(
    closed_loop::ClArgs a, FeasArgs f, closed_loop::BankStrides strides, closed_loop::StatsArgs stats, const double *wn,
    const double *vn, double *u_nn, int32_t *flag, closed_loop::PressTable press, plant::UniformParams model) {
    closed_loop::loop_body<SMOOTH, NOISE>(a, wn, vn, ProjectedCommand<plant::UniformParams>{f, a.u, u_nn, flag, model},
                                          closed_loop::BankPressModel(a.B, strides, press), closed_loop::LaneStats<STORE>(stats));
}

}  // namespace feasibility
}  // namespace fcr
