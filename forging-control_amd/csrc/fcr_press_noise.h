// fcr_press_noise.h — training on the press under pre-drawn process and measurement noise: the adjoint
// of the noisy RK4 step, the bank's reverse loop on a noisy run, and the forward kernels that store the unperturbed state
// beside the record. fcr_plant.h, fcr_closed_loop.h, fcr_press_grad.h and fcr_press_train.h are only read: rhs_vjp,
// lane_press, the seed policies and BankGradArgs are their own, and the controller chain below is
// closed_loop_bank_vjp_kernel's line for line.
//
// Forward (fcr_closed_loop.h's loop_body, §7.5.1), per trajectory with w (T,5), v (T,5), state s_0 = x0, record m_0 = x0:
//   u_t = controller(m_t[1], m_t[4], ref[t]);  s_{t+1} = rk4_step<NOISE>(s_t, u_t, w_t);  m_{t+1} = s_{t+1} + v_t = x[:, t+1].
// w_t is held over the step and enters every stage, k = f(X, u) + w_t, so the stage points are
//   X2 = (s + dt/2 k1) + dt/2 w,  X3 = (s + dt/2 k2) + dt/2 w,  X4 = (s + dt k3) + dt w
// and the sub-step's Jacobian is the noise-free one evaluated at those shifted points: w is a constant and adds no term
// of its own. The reverse loop runs t = T-1 .. 0 with lambda = dL/ds_{t+1} (= dL/dm_{t+1}: v is additive):
//   seed on the RECORD m_{t+1};  (lambda, du) = rk4_step_vjp_noise at (s_t, u_t, w_t);  the controller chain and its masks
//   from the RECORD m_t, its input cotangents added to lambda[1], lambda[4];  truncation as in fcr_press_train.h.
// s_t is read from x_state, which the forward kernels below store ((m - v) is not the forward's bits); x_state = NULL: no
// measurement noise, the record is the state. w and v are constants: no gradient is produced for them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr_closed_loop.h"
#include "fcr_press_noise_host.h"
#include "fcr_press_train.h"

namespace fcr {
namespace press_noise {

using press_grad::kGradBlock;
using press_grad::kKeptSubsteps;
using press_grad::kMaxHidden;

// substep_vjp (fcr_press_grad.h) of the sub-step under process noise: hw = dt/2 w, dw = dt w as rk4_step forms them, the
// stage points in the forward's expression order ((x + c k) + c w, plant::plus_noise).
template <bool SMOOTH, class P, class G>
__device__ __forceinline__ void substep_vjp_noise(const double (&x)[5], double u, double dt, const double (&hw)[5],
                                                  const double (&dw)[5], double (&lam)[5], double &gu, P p, G &gc) {
    double k[5], x2[5], x3[5], x4[5];
    plant::forging_rhs<SMOOTH>(x, u, k, p);
#pragma unroll
    for (int i = 0; i < 5; ++i) x2[i] = plant::plus_noise<true>(x[i] + dt / 2 * k[i], hw[i]);
    plant::forging_rhs<SMOOTH>(x2, u, k, p);
#pragma unroll
    for (int i = 0; i < 5; ++i) x3[i] = plant::plus_noise<true>(x[i] + dt / 2 * k[i], hw[i]);
    plant::forging_rhs<SMOOTH>(x3, u, k, p);
#pragma unroll
    for (int i = 0; i < 5; ++i) x4[i] = plant::plus_noise<true>(x[i] + dt * k[i], dw[i]);
    double a[5], mu[5], sum[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        a[i] = dt / 6 * lam[i];
        mu[i] = 0.0;
    }
    press_grad::rhs_vjp<SMOOTH>(x4, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] = mu[i];
        a[i] = dt / 3 * lam[i] + dt * mu[i];
        mu[i] = 0.0;
    }
    press_grad::rhs_vjp<SMOOTH>(x3, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] += mu[i];
        a[i] = dt / 3 * lam[i] + dt / 2 * mu[i];
        mu[i] = 0.0;
    }
    press_grad::rhs_vjp<SMOOTH>(x2, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] += mu[i];
        a[i] = dt / 6 * lam[i] + dt / 2 * mu[i];
        mu[i] = 0.0;
    }
    press_grad::rhs_vjp<SMOOTH>(x, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) lam[i] += sum[i] + mu[i];
}

// rk4_step_vjp (fcr_press_grad.h) of the sampling step from the stored state st under the held command u and the held
// noise w: the sub-steps' entry states are recomputed with the forward's own noisy step.
template <bool SMOOTH, bool KEPT, class P, class G>
__device__ __forceinline__ void rk4_step_vjp_noise(const double (&st)[5], double u, double dt, int substeps,
                                                   const double (&w)[5], double (&lam)[5], double &gu, P p, G &gc) {
    double hw[5], dw[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        hw[i] = dt / 2 * w[i];
        dw[i] = dt * w[i];
    }
    if constexpr (KEPT) {
        // e1..e3 picked by compare-and-select and both loops rolled, as in rk4_step_vjp and for its reason
        double e1[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, e2[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, e3[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, e[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) e[i] = st[i];
#pragma nounroll
        for (int m = 1; m < kKeptSubsteps; ++m) {
            plant::rk4_step<SMOOTH, true>(e, u, dt, 1, w, p);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                e1[i] = m == 1 ? e[i] : e1[i];
                e2[i] = m == 2 ? e[i] : e2[i];
                e3[i] = m == 3 ? e[i] : e3[i];
            }
        }
#pragma nounroll
        for (int m = kKeptSubsteps - 1; m >= 0; --m) {
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] = m == 3 ? e3[i] : (m == 2 ? e2[i] : (m == 1 ? e1[i] : st[i]));
            substep_vjp_noise<SMOOTH>(e, u, dt, hw, dw, lam, gu, p, gc);
        }
    } else {
        for (int m = substeps - 1; m >= 0; --m) {
            double e[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] = st[i];
            plant::rk4_step<SMOOTH, true>(e, u, dt, m, w, p);
            substep_vjp_noise<SMOOTH>(e, u, dt, hw, dw, lam, gu, p, gc);
        }
    }
}

// closed_loop_bank_vjp_kernel (fcr_press_train.h) on a noisy run. The seed and the controller read the record; the plant is
// linearised at the state, with the step's noise.
template <bool SMOOTH, bool KEPT, class P, class Seed>
__global__ __launch_bounds__(kGradBlock) void closed_loop_bank_vjp_noise_kernel(press_train::BankGradArgs a, Seed seed,
                                                                                NoiseGrad n) {
    __shared__ float w[kMaxHidden * 5];        // [j] = (w_inp[j][0..2], b_inp[j], w_out[j]) of model blockIdx.y
    const int m = blockIdx.y;
    {
        const float *wi = a.w_inp + (size_t)m * a.hidden * 3, *bi = a.b_inp + (size_t)m * a.hidden;
        const float *wo = a.w_out + (size_t)m * a.hidden;
        for (int i = threadIdx.x; i < a.hidden; i += kGradBlock) {
            w[i * 5 + 0] = wi[i * 3 + 0];
            w[i * 5 + 1] = wi[i * 3 + 1];
            w[i * 5 + 2] = wi[i * 3 + 2];
            w[i * 5 + 3] = bi[i];
            w[i * 5 + 4] = wo[i];
        }
    }
    __syncthreads();
    const int b = blockIdx.x * kGradBlock + threadIdx.x;
    if (b >= a.B) return;
    const P p = press_grad::lane_press<P>(a.press + (size_t)m * a.stride_model, a.stride_traj, b);
    const size_t mb = (size_t)m * a.B + b, row = mb * a.T;
    const double *xb = a.x + mb * (a.T + 1) * 5, *ub = a.u + row;
    const double *sb = n.x_state ? n.x_state + mb * (a.T + 1) * 5 : nullptr;
    const double *wb = n.w ? n.w + (size_t)m * n.w_stride + (size_t)b * a.T * 5 : nullptr;
    const double *rb = a.ref + (size_t)m * a.ref_stride + (size_t)b * a.T;
    const double os = (double)(float)a.out_scale;             // the forward multiplies by the float32 scale
    typename Seed::Lane s(seed, a, m, b);
    double lam[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double xn[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, un = 0.0, ut = 0.0;
    if (a.T > 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) xn[i] = xb[(size_t)a.T * 5 + i];
        ut = ub[a.T - 1];
    }
    press_grad::NoCoeffGrad gc;
    for (int t = a.T - 1; t >= 0; --t) {
        double xt[5], st[5], wt[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // the record, the state, the step's noise
#pragma unroll
        for (int i = 0; i < 5; ++i) xt[i] = xb[(size_t)t * 5 + i];
        if (sb) {
#pragma unroll
            for (int i = 0; i < 5; ++i) st[i] = sb[(size_t)t * 5 + i];
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i) st[i] = xt[i];
        }
        if (wb) {
#pragma unroll
            for (int i = 0; i < 5; ++i) wt[i] = wb[(size_t)t * 5 + i];
        }
        const double rt = rb[t];
        const double up = t > 0 ? ub[t - 1] : s.before(ut);
        double du = s.step(t, xn, rt, un, ut, up, lam);
        rk4_step_vjp_noise<SMOOTH, KEPT>(st, ut, a.dt, a.substeps, wt, lam, du, p, gc);
        const float s0 = (float)(xt[1] / a.in_scale0), s1 = (float)(xt[4] / a.in_scale1);
        const float s2 = (float)(rt / a.ref_scale);
        float v = 0.0f;
        for (int j = 0; j < a.hidden; ++j) {
            const float *wj = w + j * 5;
            float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
            z = z > 0.0f ? z : 0.0f;
            v = fmaf(wj[4], z, v);
        }
        const double dv = (v > -1.0f && v < 1.0f) ? du * os : 0.0;
        a.dv[row + t] = dv;
        if (dv != 0.0) {
            double g0 = 0.0, g1 = 0.0;
            for (int j = 0; j < a.hidden; ++j) {
                const float *wj = w + j * 5;
                const float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
                if (z > 0.0f) {
                    const double dz = dv * (double)wj[4];
                    g0 = fma(dz, (double)wj[0], g0);
                    g1 = fma(dz, (double)wj[1], g1);
                }
            }
            lam[1] += g0 / a.in_scale0;
            lam[4] += g1 / a.in_scale1;
        }
        // truncated back-propagation, as in closed_loop_bank_vjp_kernel
        if (a.truncate > 0 && t > 0 && t % a.truncate == 0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) lam[i] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) xn[i] = xt[i];
        un = ut;
        ut = up;
    }
    s.finish(lam);
    if (a.g_x0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) a.g_x0[mb * 5 + i] = lam[i];
    }
    s.done();
}

// closed_loop_bank_kernel / closed_loop_bank_press_kernel (fcr_closed_loop.h) under noise, storing, and with the
// unperturbed states written to x_state (M,B,T+1,5) beside the record. (The body is repeated, not shared: with a policy
// for the extra store added to loop_body, defaulted to nothing, all 32 bank kernels came out with other instructions.)
// It is loop_body<SMOOTH, true, PlainCommand, Model, LaneStats<true>> line for line — the same expressions in the same
// order, so x, u and the statistics are those kernels' bits — plus the two stores of x. TABLE: every trajectory's own press.
template <bool SMOOTH, class Model>
__device__ __forceinline__ void state_loop_body(closed_loop::ClArgs a, const double *wn, const double *vn, Model model,
                                                closed_loop::LaneStats<true> stats, double *x_state) {
    using namespace closed_loop;
    __shared__ float w[kClMaxHidden * 5];        // [j] = (w_inp[j][0..2], b_inp[j], w_out[j])
    const float *w_inp = a.w_inp + (size_t)model.model() * 3 * a.hidden, *b_inp = a.b_inp + (size_t)model.model() * a.hidden,
                *w_out = a.w_out + (size_t)model.model() * a.hidden;
    for (int i = threadIdx.x; i < a.hidden; i += kClBlock) {
        w[i * 5 + 0] = w_inp[i * 3 + 0];
        w[i * 5 + 1] = w_inp[i * 3 + 1];
        w[i * 5 + 2] = w_inp[i * 3 + 2];
        w[i * 5 + 3] = b_inp[i];
        w[i * 5 + 4] = w_out[i];
    }
    __syncthreads();
    const int b = model.block() * kClBlock + threadIdx.x;
    if (b >= a.B) return;
    const auto pp = model.press(b);                // this lane's press
    const size_t g = (size_t)model.model() * a.B + b;   // the row of the (model-major) outputs
    double x[5], m[5];                            // the press's state; the record the controller reads
    double *o = a.x + g * (a.T + 1) * 5, *so = x_state + g * (a.T + 1) * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = a.x0[model.x0() + (size_t)b * 5 + i];
        m[i] = x[i];
        o[i] = x[i];
        so[i] = x[i];
    }
    const size_t row = (size_t)b * a.T;
    const double *rb = a.ref + model.ref() + row;
    const PlainCommand command = PlainCommand{a.u}.row(g * a.T);
    for (int t = 0; t < a.T; ++t) {
        const float s0 = (float)(m[1] / a.in_scale0), s1 = (float)(m[4] / a.in_scale1);
        const double r = rb[t];
        const float s2 = (float)(r / a.ref_scale);
        float v = 0.0f;
        for (int j = 0; j < a.hidden; ++j) {
            const float *wj = w + j * 5;
            float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
            z = z > 0.0f ? z : 0.0f;
            v = fmaf(wj[4], z, v);
        }
        v = fminf(fmaxf(v, -1.0f), 1.0f);                   // Hardtanh
        const double un = (double)(v * (float)a.out_scale); // inverse_transform on the float32 output
        int flag = 0;
        const double u = command(m, un, t, true, flag);
        double wt[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, vt[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const size_t nt = (row + t) * 5;
        if (wn) {
#pragma unroll
            for (int i = 0; i < 5; ++i) wt[i] = wn[model.w() + nt + i];
        }
        if (vn) {
#pragma unroll
            for (int i = 0; i < 5; ++i) vt[i] = vn[model.v() + nt + i];
        }
        plant::rk4_step<SMOOTH, true>(x, u, a.dt, a.substeps, wt, pp);
        o += 5;
        so += 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            m[i] = x[i] + vt[i];
            o[i] = m[i];
            so[i] = x[i];
        }
        stats.step(r, m, u, flag, t);
    }
    stats.finish(g, x, a.T);
}

template <bool SMOOTH, bool TABLE>
__global__ __launch_bounds__(closed_loop::kClBlock) void closed_loop_bank_state_kernel(
    closed_loop::ClArgs a, closed_loop::BankStrides strides, closed_loop::StatsArgs stats, const double *wn,
    const double *vn, closed_loop::PressTable press, double *x_state) {
    using namespace closed_loop;
    if constexpr (TABLE)
        state_loop_body<SMOOTH>(a, wn, vn, BankPressModel(a.B, strides, press), LaneStats<true>(stats), x_state);
    else
        state_loop_body<SMOOTH>(a, wn, vn, BankModel(a.B, strides), LaneStats<true>(stats), x_state);
}

}  // namespace press_noise
}  // namespace fcr
