// fcr_mpc.h — the model-predictive baseline on the press: a shooting MPC with the reference's objective
// on the project's own RK4 press, solved per trajectory by a fixed number of Levenberg-Marquardt iterations.
// Forward: fcr_plant.h (rk4_step); step Jacobians: fcr_press_grad.h (rk4_step_vjp under unit cotangents, so the
// conventions at the singular points are that file's own). Both are read only.
//
// Problem of one lane: state x_0, previous command u_prev, references r_1..r_N, a press (the controller's MODEL);
// unknowns U = (u_0..u_{N-1}); x_{k+1} = rk4_step(x_k, u_k). Residuals: e_k = x_k[1] - r_k (k = 1..N);
// d_k = sqrt(r_u) (u_k - u_{k-1}), u_{-1} = u_prev (k = 0..N-1); per k = 1..N the squared hinges
// sqrt(w) relu((x_k[c] - hi)/s_p), sqrt(w) relu((lo - x_k[c])/s_p) for c = 2, 3 (an infinite bound is off, relu'(0) = 0).
// cost = sum residual^2.
//
// One iteration from (U, lambda, c): roll out keeping x_0..x_N; A_k = dx_{k+1}/dx_k, b_k = dx_{k+1}/du_k by five
// rk4_step_vjp per step; H = J^T J, g = J^T r from the residual rows (s = e_c; j = k-1..0: row[j] = b_j^T s, s = A_j^T s)
// and the bidiagonal command rows; active set {i: (U_i <= u_lo and g_i > 0) or (U_i >= u_hi and g_i < 0)}: row and column
// zeroed, H_ii = 1, g_i = 0; (H + lambda diag(H)) delta = -g by Cholesky, diag taken BEFORE the substitution; a pivot
// that is not positive and finite rejects; U' = clip(U + delta); accept iff cost(U') < c (false for NaN): lambda *= 0.3
// (floor 1e-12), else lambda *= 10 (cap 1e12). After a rejection U is unchanged, so is its linearisation: it is reused.
// K iterations always; every loop bound is a launch argument or a constant.
//
// One lane owns one trajectory. Its matrices live in a caller-provided workspace in global memory laid out
// [element][lane] (element e of lane b at ws[e * B + b]): a wave's loads and stores of one element coalesce, and nothing
// indexed at run time stands in the private segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr_plant.h"
#include "fcr_press_grad.h"

namespace fcr {
namespace mpc {

constexpr int kMpcBlock = 64;     // one wave per block: B = 300 spreads over 5 compute units
constexpr int kMaxHorizon = 32;   // the active set is a 32-bit mask
constexpr int kMaxIters = 64;

struct MpcArgs {
    int N, K, substeps;
    double dt, sru, lam0;         // sru = sqrt(r_u)
    double lo1, hi1, lo2, hi2;    // Pa; +-inf = off
    double sw, inv_sp;            // sqrt(w), 1 / s_p
    double u_lo, u_hi;
};

// element offsets of one lane's workspace
struct Layout {
    int x, a, b, h, l, g, u, ut, d, total;
    __host__ __device__ explicit Layout(int N) {
        const int tri = N * (N + 1) / 2;
        x = 0;                    // x_0..x_N
        a = x + 5 * (N + 1);      // A_k[i][m], k < N
        b = a + 25 * N;           // b_k[i]
        h = b + 5 * N;            // H, packed lower triangle
        l = h + tri;              // its damped copy / Cholesky factor
        g = l + tri;
        u = g + N;                // U
        ut = u + N;               // the trial point U'
        d = ut + N;               // a residual's row; the step delta
        total = d + N;
    }
};

struct Lane {
    double *p;                    // ws + b
    size_t stride;                // B
    __device__ __forceinline__ double &operator[](int e) const { return p[(size_t)e * stride]; }
};

// r_k, k = 1..N: p[min(first + (k-1) step, last)]
struct Ref {
    const double *p;
    int first, last, step;
    __device__ __forceinline__ double operator()(int k) const {
        const int i = first + (k - 1) * step;
        return p[i < last ? i : last];
    }
};

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // j <= i

// the press row of a table lane: NULL = the reference's constants as a row (derive() of it gives Nominal's doubles)
__device__ __forceinline__ plant::Coeffs table_press(const double *press, long long stride, int b) {
    if (press) return plant::derive(press + (size_t)b * stride);
    const double row[plant::kPressFields] = {
        plant::M_MASS, plant::B_DAMP, plant::FT, plant::D1, plant::D2, plant::G, plant::KB, plant::V1_0, plant::V2_0,
        plant::KL_1, plant::KL_2, plant::CD, plant::RHO, plant::D, plant::PS, plant::PT, plant::MU, plant::K, plant::W0,
        plant::H0, plant::B0, plant::T_DEF, plant::T1, plant::M0, plant::M1, plant::M2, plant::M3, plant::M4};
    return plant::derive(row);
}
template <class P>
__device__ __forceinline__ P press_of(const double *press, long long stride, int b) {
    if constexpr (plant::kLiteral<P>) return {};
    else return table_press(press, stride, b);
}

// one pressure's hinge pair at value v: the residual and its slope d residual / d v (0, 0 inside the bounds)
__device__ __forceinline__ void hinge(const MpcArgs &a, double v, double lo, double hi, double &res, double &slope) {
    res = 0.0;
    slope = 0.0;
    if (v > hi) {
        res = a.sw * ((v - hi) * a.inv_sp);
        slope = a.sw * a.inv_sp;
    } else if (v < lo) {
        res = a.sw * ((lo - v) * a.inv_sp);
        slope = -(a.sw * a.inv_sp);
    }
}

// cost of the commands at w[at..at+N); STORE: x_0..x_N are kept
template <bool SMOOTH, bool STORE, class P>
__device__ __forceinline__ double rollout_cost(const MpcArgs &a, const Lane &w, const Layout &o, int at, const double (&x0)[5],
                                               double u_prev, const Ref &ref, P pm) {
    double x[5], c = 0.0, up = u_prev;
#pragma unroll
    for (int i = 0; i < 5; ++i) x[i] = x0[i];
    for (int k = 0; k < a.N; ++k) {
        const double u = w[at + k];
        if (STORE) {
#pragma unroll
            for (int i = 0; i < 5; ++i) w[o.x + k * 5 + i] = x[i];
        }
        const double d = a.sru * (u - up);
        c += d * d;
        up = u;
        plant::rk4_step<SMOOTH, false>(x, u, a.dt, a.substeps, nullptr, pm);
        const double e = x[1] - ref(k + 1);
        c += e * e;
        double r, s;
        hinge(a, x[2], a.lo1, a.hi1, r, s);
        c += r * r;
        hinge(a, x[3], a.lo2, a.hi2, r, s);
        c += r * r;
    }
    if (STORE) {
#pragma unroll
        for (int i = 0; i < 5; ++i) w[o.x + a.N * 5 + i] = x[i];
    }
    return c;
}

// A_k, b_k at the stored states, then H = J^T J and g = J^T r at U
template <bool SMOOTH, class P>
__device__ __forceinline__ void linearise(const MpcArgs &a, const Lane &w, const Layout &o, double u_prev, const Ref &ref,
                                          P pm) {
    const int N = a.N;
    const bool kept = a.substeps == press_grad::kKeptSubsteps;
    press_grad::NoCoeffGrad gc;
    for (int k = 0; k < N; ++k) {
        double xk[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) xk[i] = w[o.x + k * 5 + i];
        const double u = w[o.u + k];
#pragma nounroll
        for (int c = 0; c < 5; ++c) {                        // row c of [A_k | b_k]: the unit cotangent e_c
            double lam[5], gu = 0.0;
#pragma unroll
            for (int i = 0; i < 5; ++i) lam[i] = i == c ? 1.0 : 0.0;
            if (kept) press_grad::rk4_step_vjp<SMOOTH, true>(xk, u, a.dt, a.substeps, lam, gu, pm, gc);
            else press_grad::rk4_step_vjp<SMOOTH, false>(xk, u, a.dt, a.substeps, lam, gu, pm, gc);
#pragma unroll
            for (int i = 0; i < 5; ++i) w[o.a + k * 25 + c * 5 + i] = lam[i];
            w[o.b + k * 5 + c] = gu;
        }
    }
    const int nt = N * (N + 1) / 2;
    for (int i = 0; i < nt; ++i) w[o.h + i] = 0.0;
    for (int i = 0; i < N; ++i) w[o.g + i] = 0.0;
    // tracking and hinge rows of x_k, k = 1..N: component 1 (speed), 2 and 3 (pressures)
    for (int k = 1; k <= N; ++k) {
#pragma nounroll
        for (int c = 1; c <= 3; ++c) {
            const double v = w[o.x + k * 5 + c];
            double res, slope;
            if (c == 1) {
                res = v - ref(k);
                slope = 1.0;
            } else {
                hinge(a, v, c == 2 ? a.lo1 : a.lo2, c == 2 ? a.hi1 : a.hi2, res, slope);
            }
            if (slope == 0.0) continue;
            double s[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) s[i] = i == c ? slope : 0.0;
            for (int j = k - 1; j >= 0; --j) {
                double rj = 0.0, sn[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    rj += w[o.b + j * 5 + i] * s[i];
#pragma unroll
                    for (int m = 0; m < 5; ++m) sn[m] += w[o.a + j * 25 + i * 5 + m] * s[i];
                }
                w[o.d + j] = rj;
#pragma unroll
                for (int i = 0; i < 5; ++i) s[i] = sn[i];
            }
            for (int i = 0; i < k; ++i) {
                const double ri = w[o.d + i];
                w[o.g + i] += ri * res;
                for (int j = 0; j <= i; ++j) w[o.h + tri(i, j)] += ri * w[o.d + j];
            }
        }
    }
    // the command rows d_k = sru (u_k - u_{k-1}): +sru at k, -sru at k-1
    const double ru = a.sru * a.sru;
    double up = u_prev;
    for (int k = 0; k < N; ++k) {
        const double u = w[o.u + k];
        const double gd = a.sru * (a.sru * (u - up));
        up = u;
        w[o.h + tri(k, k)] += ru;
        w[o.g + k] += gd;
        if (k > 0) {
            w[o.h + tri(k - 1, k - 1)] += ru;
            w[o.h + tri(k, k - 1)] -= ru;
            w[o.g + k - 1] -= gd;
        }
    }
}

// active set at U (a bit per command), and |g|_inf over the others
__device__ __forceinline__ unsigned active_set(const MpcArgs &a, const Lane &w, const Layout &o, double &ginf) {
    unsigned act = 0u;
    ginf = 0.0;
    for (int i = 0; i < a.N; ++i) {
        const double u = w[o.u + i], g = w[o.g + i];
        if ((u <= a.u_lo && g > 0.0) || (u >= a.u_hi && g < 0.0)) act |= 1u << i;
        else ginf = fabs(g) > ginf || g != g ? fabs(g) : ginf;   // a NaN stays
    }
    return act;
}

// (H_act + lam diag(H)) delta = -g_act by Cholesky into w[o.d..]; false: a pivot was not positive and finite
__device__ __forceinline__ bool damped_step(const MpcArgs &a, const Lane &w, const Layout &o, unsigned act, double lam) {
    const int N = a.N;
    for (int i = 0; i < N; ++i) {
        const bool ai = (act >> i) & 1u;
        for (int j = 0; j < i; ++j) w[o.l + tri(i, j)] = (ai || ((act >> j) & 1u)) ? 0.0 : w[o.h + tri(i, j)];
        const double hii = w[o.h + tri(i, i)];
        w[o.l + tri(i, i)] = (ai ? 1.0 : hii) + lam * hii;
        w[o.d + i] = ai ? 0.0 : -w[o.g + i];
    }
    bool ok = true;
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = w[o.l + tri(i, j)];
            for (int k = 0; k < j; ++k) s -= w[o.l + tri(i, k)] * w[o.l + tri(j, k)];
            if (j == i) {
                if (!(s > 0.0) || s - s != 0.0) ok = false;
                w[o.l + tri(i, i)] = sqrt(s);
            } else {
                w[o.l + tri(i, j)] = s / w[o.l + tri(j, j)];
            }
        }
    }
    for (int i = 0; i < N; ++i) {                             // L y = rhs
        double s = w[o.d + i];
        for (int k = 0; k < i; ++k) s -= w[o.l + tri(i, k)] * w[o.d + k];
        w[o.d + i] = s / w[o.l + tri(i, i)];
    }
    for (int i = N - 1; i >= 0; --i) {                        // L^T delta = y
        double s = w[o.d + i];
        for (int k = i + 1; k < N; ++k) s -= w[o.l + tri(k, i)] * w[o.d + k];
        w[o.d + i] = s / w[o.l + tri(i, i)];
    }
    return ok;
}

struct SolveOut {
    double cost, grad_inf, lam;
    int accepted;
};

// K iterations from the U in the workspace (w[o.u..]), which ends as the solution. trace (K,5) / trace_u (K,N) of this
// solve, or null: per iteration (c, c', lambda before, accepted, pivot failure; c' = inf at a pivot failure) and U after it.
template <bool SMOOTH, class P>
__device__ __forceinline__ SolveOut mpc_solve_device(const MpcArgs &a, const Lane &w, const Layout &o, const double (&x0)[5],
                                                     double u_prev, const Ref &ref, P pm, double *trace, double *trace_u) {
    SolveOut out{0.0, 0.0, a.lam0, 0};
    double c = 0.0;
    bool fresh = true;                                        // U has moved since its linearisation
    unsigned act = 0u;
    for (int it = 0; it < a.K; ++it) {
        if (fresh) {
            c = rollout_cost<SMOOTH, true>(a, w, o, o.u, x0, u_prev, ref, pm);
            linearise<SMOOTH>(a, w, o, u_prev, ref, pm);
            act = active_set(a, w, o, out.grad_inf);
            fresh = false;
        }
        const double lam = out.lam;
        const bool ok = damped_step(a, w, o, act, lam);
        double cn = __builtin_inf();
        bool accept = false;
        if (ok) {
            for (int i = 0; i < a.N; ++i) w[o.ut + i] = fmin(fmax(w[o.u + i] + w[o.d + i], a.u_lo), a.u_hi);
            cn = rollout_cost<SMOOTH, false>(a, w, o, o.ut, x0, u_prev, ref, pm);
            accept = cn < c;
        }
        if (trace) {
            double *tr = trace + (size_t)it * 5;
            tr[0] = c;
            tr[1] = cn;
            tr[2] = lam;
            tr[3] = accept ? 1.0 : 0.0;
            tr[4] = ok ? 0.0 : 1.0;
        }
        if (accept) {
            for (int i = 0; i < a.N; ++i) w[o.u + i] = w[o.ut + i];
            c = cn;
            out.lam = fmax(lam * 0.3, 1e-12);
            out.accepted += 1;
            fresh = true;
        } else {
            out.lam = fmin(lam * 10.0, 1e12);
        }
        if (trace_u)
            for (int i = 0; i < a.N; ++i) trace_u[(size_t)it * a.N + i] = w[o.u + i];
    }
    out.cost = c;
    return out;
}

// ---- one horizon for B problems ----
struct SolveArgs {
    int B;
    const double *x0, *ref, *u_prev, *U0;                     // (B,5), (B,N), (B), (B,N) or null (u_prev repeated)
    const double *model;                                      // P = Coeffs: the table or null (the reference's row)
    long long model_stride;
    double *U, *cost, *grad_inf, *lam;                        // (B,N), (B) x 3
    int *accepted;                                            // (B)
    double *trace, *trace_u;                                  // (B,K,5), (B,K,N) or null
    double *ws;
};

template <bool SMOOTH, class P>
__global__ __launch_bounds__(kMpcBlock) void mpc_solve_kernel(MpcArgs a, SolveArgs s) {
    const int b = blockIdx.x * kMpcBlock + threadIdx.x;
    if (b >= s.B) return;
    const P pm = press_of<P>(s.model, s.model_stride, b);
    const Layout o(a.N);
    const Lane w{s.ws + b, (size_t)s.B};
    double x0[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) x0[i] = s.x0[(size_t)b * 5 + i];
    const double up = s.u_prev[b];
    // the starting plan is projected into the box (u_prev itself may lie outside): every returned U is inside it
    for (int i = 0; i < a.N; ++i) w[o.u + i] = fmin(fmax(s.U0 ? s.U0[(size_t)b * a.N + i] : up, a.u_lo), a.u_hi);
    const Ref ref{s.ref + (size_t)b * a.N, 0, a.N - 1, 1};
    const SolveOut r = mpc_solve_device<SMOOTH>(a, w, o, x0, up, ref, pm,
                                                s.trace ? s.trace + (size_t)b * a.K * 5 : nullptr,
                                                s.trace_u ? s.trace_u + (size_t)b * a.K * a.N : nullptr);
    for (int i = 0; i < a.N; ++i) s.U[(size_t)b * a.N + i] = w[o.u + i];
    s.cost[b] = r.cost;
    s.grad_inf[b] = r.grad_inf;
    s.lam[b] = r.lam;
    s.accepted[b] = r.accepted;
}

// ---- the closed loop: T solves around the true press ----
struct LoopArgs {
    int B, T, preview;
    const double *x0, *ref, *u_init, *U0;                     // (B,5), (B,T), (B), (B,N) or null (u_init repeated)
    const double *wn, *vn;                                    // (B,T,5) process / measurement noise or null (NOISE only)
    const double *plant, *model;                              // tables or null
    long long plant_stride, model_stride;
    double *x, *u, *cost, *grad_inf;                          // (B,T+1,5), (B,T) x 3
    int *accepted;                                            // (B,T)
    double *plans, *trace, *trace_u;                          // (B,T,N), (B,T,K,5), (B,T,K,N) or null
    double *ws;
};

// x[:,0] = x0; per step: the record m_t (x_t, + v[t-1] under NOISE) -> horizon references -> solve from m_t with
// u_prev = u_{t-1} and the previous plan shifted by one -> u_t = U[0] -> the true press steps (f + w[t] under NOISE).
template <bool SMOOTH, class PP, class PM, bool NOISE>
__global__ __launch_bounds__(kMpcBlock) void mpc_closed_loop_kernel(MpcArgs a, LoopArgs s) {
    const int b = blockIdx.x * kMpcBlock + threadIdx.x;
    if (b >= s.B) return;
    const PP pp = press_of<PP>(s.plant, s.plant_stride, b);
    const PM pm = press_of<PM>(s.model, s.model_stride, b);
    const Layout o(a.N);
    const Lane w{s.ws + b, (size_t)s.B};
    double x[5], m[5];
    double *xo = s.x + (size_t)b * (s.T + 1) * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = s.x0[(size_t)b * 5 + i];
        m[i] = x[i];
        xo[i] = x[i];
    }
    const size_t row = (size_t)b * s.T;
    double up = s.u_init[b];
    // the starting plan is projected into the box (u_init itself may lie outside): every applied u_t is inside it
    for (int i = 0; i < a.N; ++i) w[o.u + i] = fmin(fmax(s.U0 ? s.U0[(size_t)b * a.N + i] : up, a.u_lo), a.u_hi);
    for (int t = 0; t < s.T; ++t) {
        if (t > 0) {
            for (int i = 0; i + 1 < a.N; ++i) w[o.u + i] = w[o.u + i + 1];   // the last entry stays: repeated
        }
        const Ref ref{s.ref + row, t, s.T - 1, s.preview ? 1 : 0};
        const SolveOut r = mpc_solve_device<SMOOTH>(a, w, o, m, up, ref, pm,
                                                    s.trace ? s.trace + (row + t) * a.K * 5 : nullptr,
                                                    s.trace_u ? s.trace_u + (row + t) * a.K * a.N : nullptr);
        const double u = w[o.u];
        if (s.plans)
            for (int i = 0; i < a.N; ++i) s.plans[(row + t) * a.N + i] = w[o.u + i];
        s.u[row + t] = u;
        s.cost[row + t] = r.cost;
        s.grad_inf[row + t] = r.grad_inf;
        s.accepted[row + t] = r.accepted;
        up = u;
        double wt[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, vt[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (NOISE) {
            const size_t nt = (row + t) * 5;
            if (s.wn) {
#pragma unroll
                for (int i = 0; i < 5; ++i) wt[i] = s.wn[nt + i];
            }
            if (s.vn) {
#pragma unroll
                for (int i = 0; i < 5; ++i) vt[i] = s.vn[nt + i];
            }
        }
        plant::rk4_step<SMOOTH, NOISE>(x, u, a.dt, a.substeps, wt, pp);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            m[i] = NOISE ? x[i] + vt[i] : x[i];
            xo[(size_t)(t + 1) * 5 + i] = m[i];
        }
    }
}

}  // namespace mpc
}  // namespace fcr
