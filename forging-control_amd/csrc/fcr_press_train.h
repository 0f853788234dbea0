// fcr_press_train.h — training a bank of controllers on the press: the adjoint of the closed loop for
// M models in one launch, seeded either by incoming gradient tensors (TensorSeed: the general vector-Jacobian product)
// or by the MPC loss evaluated on the stored record (LossSeed: the loss's cotangents are formed in registers, the
// per-trajectory cost is accumulated in the same pass, nothing but the record is read), with optional truncated
// back-propagation; the controllers' parameter gradients for M models in one launch; the fixed-order sum of the cost.
// fcr_press_grad.h is only read: lane_press, rk4_step_vjp, NoCoeffGrad and the constants are its own, the controller
// chain below is closed_loop_vjp_kernel's line for line, and param_grad_bank_kernel / param_reduce_bank_kernel are
// param_grad_kernel / param_reduce_kernel with the model as blockIdx.y — the same tiling, the same fp64 fixed-order sums
// and the same per-model partial layout, so model m's gradients are the single-model call's.
//
// One lane owns one trajectory of one model (blockIdx.y), 256 lanes per block; a block stages its model's
// (w_inp, b_inp, w_out) in LDS. The reverse loop runs t = T-1 .. 0 with lambda = dL/dx_{t+1} in registers:
//   seed: lambda += dL/dx[t+1] (direct), du = dL/du_t (direct);  (lambda, du) = rk4_step_vjp(x_t, u_t, lambda);
//   [controller];  write dv;  truncation: lambda = 0 after step t when t > 0 and t % K == 0.
// The loop carries x_{t+1} (the previous iteration's x_t), u_{t+1}, u_t and u_{t-1} in registers, so each element of the
// record is read once: 8 B per element under LossSeed, against 24 B under TensorSeed (the record, g_x and g_u).
//
// The loss (all fp64), for model m and trajectory b, with the model's row (alpha, lo1, hi1, lo2, hi2, w):
//   e_t = (x[t+1,1] - ref[t]) / s_v;  d_t = (u_t - u_{t-1}) / s_u (d_0 = (u_0 - u_prev[b]) / s_u, or 0 without u_prev);
//   c_t = w (relu(lo1 - P1) + relu(P1 - hi1) + relu(lo2 - P2) + relu(P2 - hi2)), P1 = x[t+1,2] / s_p1, P2 = x[t+1,3] / s_p2;
//   cost[m,b] = (1/T) sum_t (e_t^2 + alpha d_t^2 + c_t);  loss[m] = (1/B) sum_b cost[m,b].
// relu'(0) = 0; an infinite bound switches its side off. The factor 1/(T B) is folded into the seeds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr_press_grad.h"

namespace fcr {
namespace press_train {

using press_grad::kGradBlock;
using press_grad::kMaxHidden;

struct BankGradArgs {
    int M, B, T, substeps, hidden, truncate;
    double dt;
    const double *ref;                    // model m: ref + m * ref_stride, (B,T)
    long long ref_stride;
    const float *w_inp, *b_inp, *w_out;   // (M,hidden,3), (M,hidden), (M,hidden)
    double in_scale0, in_scale1, ref_scale, out_scale;
    const double *x, *u;                  // the stored run: (M,B,T+1,5), (M,B,T)
    const double *press;                  // P = Coeffs: row m * stride_model + b * stride_traj
    long long stride_model, stride_traj;
    double *g_x0, *dv;                    // (M,B,5) or NULL; (M,B,T)
};

// ---- seed policies: what the reverse loop adds to lambda and to du at step t ----
// Lane(seed, a, m, b) is a lane's state; step(t, xn, rt, un, ut, up, lam) adds dL/dx[t+1] to lam and returns the direct
// dL/du_t, given xn = x[t+1], rt = ref[t], un / ut / up = u_{t+1} / u_t / u_{t-1} (un is unused at t = T-1; up at t = 0 is
// before(ut)); finish(lam) adds dL/dx[0]; done() stores what the seed accumulates.

// the general vector-Jacobian product: g_x (M,B,T+1,5) and g_u (M,B,T) incoming, closed_loop_vjp_kernel's arithmetic
struct TensorSeed {
    const double *g_x, *g_u;
    struct Lane {
        const double *gb, *gu;
        __device__ __forceinline__ Lane(const TensorSeed &s, const BankGradArgs &a, int m, int b)
            : gb(s.g_x + ((size_t)m * a.B + b) * (a.T + 1) * 5), gu(s.g_u + ((size_t)m * a.B + b) * a.T) {}
        __device__ __forceinline__ double before(double ut) const { return ut; }
        __device__ __forceinline__ double step(int t, const double (&)[5], double, double, double, double, double (&lam)[5]) {
#pragma unroll
            for (int i = 0; i < 5; ++i) lam[i] += gb[(size_t)(t + 1) * 5 + i];
            return gu[t];
        }
        __device__ __forceinline__ void finish(double (&lam)[5]) const {
#pragma unroll
            for (int i = 0; i < 5; ++i) lam[i] += gb[i];
        }
        __device__ __forceinline__ void done() const {}
    };
};

// the fused loss: the model's terms row, the pressure scales, u_prev (B) or (M,B) or NULL -> cost (M,B)
struct LossSeed {
    const double *terms;                  // (M,6) fp64 on the device, row m * terms_stride
    long long terms_stride;
    double p_scale1, p_scale2;
    const double *u_prev;                 // NULL: d_0 = 0; else u_prev[m * u_prev_stride + b]
    long long u_prev_stride;
    double *cost;                         // (M,B)
    struct Lane {
        double alpha, lo1, hi1, lo2, hi2, w;
        double scale, inv_sv, inv_su, inv_p1, inv_p2, acc;
        const double *prev;
        double *out;
        int T;
        __device__ __forceinline__ Lane(const LossSeed &s, const BankGradArgs &a, int m, int b) {
            const double *row = s.terms + (size_t)m * s.terms_stride;
            alpha = row[0], lo1 = row[1], hi1 = row[2], lo2 = row[3], hi2 = row[4], w = row[5];
            T = a.T;
            scale = 1.0 / ((double)a.T * (double)a.B);
            inv_sv = 1.0 / a.ref_scale, inv_su = 1.0 / a.out_scale, inv_p1 = 1.0 / s.p_scale1, inv_p2 = 1.0 / s.p_scale2;
            acc = 0.0;
            prev = s.u_prev ? s.u_prev + (size_t)m * s.u_prev_stride + b : nullptr;
            out = s.cost + (size_t)m * a.B + b;
        }
        __device__ __forceinline__ double before(double ut) const { return prev ? *prev : ut; }
        __device__ __forceinline__ double step(int t, const double (&xn)[5], double rt, double un, double ut, double up,
                                               double (&lam)[5]) {
            const double e = (xn[1] - rt) * inv_sv;
            const double d = (ut - up) * inv_su;
            const double dn = t + 1 < T ? (un - ut) * inv_su : 0.0;
            const double P1 = xn[2] * inv_p1, P2 = xn[3] * inv_p2;
            const double a1 = lo1 - P1, b1 = P1 - hi1, a2 = lo2 - P2, b2 = P2 - hi2;
            const double c = (a1 > 0.0 ? a1 : 0.0) + (b1 > 0.0 ? b1 : 0.0) + (a2 > 0.0 ? a2 : 0.0) + (b2 > 0.0 ? b2 : 0.0);
            acc += e * e + alpha * (d * d) + w * c;
            const double ws = w * scale;
            lam[1] += 2.0 * scale * e * inv_sv;
            lam[2] += ws * ((b1 > 0.0 ? 1.0 : 0.0) - (a1 > 0.0 ? 1.0 : 0.0)) * inv_p1;
            lam[3] += ws * ((b2 > 0.0 ? 1.0 : 0.0) - (a2 > 0.0 ? 1.0 : 0.0)) * inv_p2;
            return 2.0 * scale * alpha * (d - dn) * inv_su;
        }
        __device__ __forceinline__ void finish(double (&)[5]) const {}
        __device__ __forceinline__ void done() const { *out = T > 0 ? acc / (double)T : 0.0; }
    };
};

template <bool SMOOTH, bool KEPT, class P, class Seed>
__global__ __launch_bounds__(kGradBlock) void closed_loop_bank_vjp_kernel(BankGradArgs a, Seed seed) {
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
        double xt[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) xt[i] = xb[(size_t)t * 5 + i];
        const double rt = rb[t];
        const double up = t > 0 ? ub[t - 1] : s.before(ut);
        double du = s.step(t, xn, rt, un, ut, up, lam);
        press_grad::rk4_step_vjp<SMOOTH, KEPT>(xt, ut, a.dt, a.substeps, lam, du, p, gc);
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
        // truncated back-propagation: x_t counts as a constant for the step that started from it (controller included);
        // the direct terms on x_t and u_{t-1} are added by the next iteration, to the step that produced them
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

// The loss alone (no gradients wanted): cost (M,B) from the record, LossSeed::Lane::step's own arithmetic.
__global__ __launch_bounds__(kGradBlock) void press_loss_value_kernel(BankGradArgs a, LossSeed seed) {
    const int m = blockIdx.y, b = blockIdx.x * kGradBlock + threadIdx.x;
    if (b >= a.B) return;
    const size_t mb = (size_t)m * a.B + b;
    const double *xb = a.x + mb * (a.T + 1) * 5, *ub = a.u + mb * a.T;
    const double *rb = a.ref + (size_t)m * a.ref_stride + (size_t)b * a.T;
    LossSeed::Lane s(seed, a, m, b);
    double lam[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, xn[5];
    for (int t = 0; t < a.T; ++t) {
#pragma unroll
        for (int i = 0; i < 5; ++i) xn[i] = xb[(size_t)(t + 1) * 5 + i];
        const double ut = ub[t];
        s.step(t, xn, rb[t], ut, ut, t > 0 ? ub[t - 1] : s.before(ut), lam);
    }
    s.done();
}

// loss[m] = (1/B) sum_b cost[m,b], in fp64 and in a fixed order, as press_grad_sum_kernel sums: block (k, m) adds the
// trajectories 256 k .. 256 k + 255 of model m in order into part[m][k]; loss_reduce_kernel adds a model's blocks in order.
__global__ __launch_bounds__(press_grad::kSumLanes) void cost_sum_kernel(int B, const double *__restrict__ cost,
                                                                         double *__restrict__ part) {
    if (threadIdx.x != 0) return;
    const int m = blockIdx.y;
    const long long first = (long long)blockIdx.x * kGradBlock;
    const long long last = first + kGradBlock < B ? first + kGradBlock : B;
    double sum = 0.0;
    for (long long b = first; b < last; ++b) sum += cost[(size_t)m * B + b];
    part[(size_t)m * gridDim.x + blockIdx.x] = sum;
}

// blocks = 0 (B = 0 or T = 0 handled by the caller's zeroed cost): loss = 0
__global__ __launch_bounds__(press_grad::kSumLanes) void loss_reduce_kernel(int M, int B, const double *__restrict__ part,
                                                                            int blocks, double *__restrict__ loss) {
    const int m = blockIdx.x * press_grad::kSumLanes + threadIdx.x;
    if (m >= M) return;
    double sum = 0.0;
    for (int q = 0; q < blocks; ++q) sum += part[(size_t)m * blocks + q];
    loss[m] = blocks ? sum / (double)B : 0.0;
}

// param_grad_kernel for M models: blockIdx.y = m runs its blocks over model m's B * T rows of the stacked arrays and
// writes model m's partials at part + m * gridDim.x * H * 5 (the single-model layout, one after the other).
__global__ __launch_bounds__(kGradBlock) void param_grad_bank_kernel(BankGradArgs a, double *__restrict__ part) {
    __shared__ float s0[kGradBlock], s1[kGradBlock], s2[kGradBlock];
    __shared__ double dvs[kGradBlock];
    __shared__ double red[kGradBlock * 5];
    const int m = blockIdx.y;
    const int tid = threadIdx.x, H = a.hidden, groups = kGradBlock / H;
    const int g = tid / H, j = tid - g * H;
    const bool on = g < groups;
    const float *wi = a.w_inp + (size_t)m * H * 3, *bi = a.b_inp + (size_t)m * H, *wout = a.w_out + (size_t)m * H;
    const double *xm = a.x + (size_t)m * a.B * (a.T + 1) * 5, *dvm = a.dv + (size_t)m * a.B * a.T;
    const double *rm = a.ref + (size_t)m * a.ref_stride;
    part += (size_t)m * gridDim.x * H * 5;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, bj = 0.0f, wo = 0.0f;
    if (on) {
        w0 = wi[j * 3 + 0], w1 = wi[j * 3 + 1], w2 = wi[j * 3 + 2];
        bj = bi[j], wo = wout[j];
    }
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const long long rows = (long long)a.B * a.T, tiles = (rows + kGradBlock - 1) / kGradBlock;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile * kGradBlock + tid;
        __syncthreads();                                       // the previous tile has been read
        if (r < rows) {
            const long long b = r / a.T, t = r - b * a.T;
            const double *xr = xm + (size_t)(b * (a.T + 1) + t) * 5;
            s0[tid] = (float)(xr[1] / a.in_scale0);
            s1[tid] = (float)(xr[4] / a.in_scale1);
            s2[tid] = (float)(rm[r] / a.ref_scale);
            dvs[tid] = dvm[r];
        } else {
            s0[tid] = s1[tid] = s2[tid] = 0.0f;
            dvs[tid] = 0.0;
        }
        __syncthreads();
        if (on) {
            for (int i = g; i < kGradBlock; i += groups) {
                const double d = dvs[i];
                if (d == 0.0) continue;                        // a saturated (or padding) row adds nothing
                const float z = fmaf(w2, s2[i], fmaf(w1, s1[i], fmaf(w0, s0[i], bj)));
                if (z > 0.0f) {
                    const double dz = d * (double)wo;
                    acc[0] = fma(dz, (double)s0[i], acc[0]);
                    acc[1] = fma(dz, (double)s1[i], acc[1]);
                    acc[2] = fma(dz, (double)s2[i], acc[2]);
                    acc[3] += dz;
                    acc[4] = fma(d, (double)z, acc[4]);
                }
            }
        }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[(size_t)tid * 5 + k] = acc[k];   // tid = g * H + j
    }
    __syncthreads();
    if (tid < H) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double sum = 0.0;
            for (int q = 0; q < groups; ++q) sum += red[(size_t)(q * H + tid) * 5 + k];
            part[((size_t)blockIdx.x * H + tid) * 5 + k] = sum;
        }
    }
}

// param_reduce_kernel for M models: blockIdx.y = m adds model m's `blocks` partials in block order -> row m of
// g_w_inp (M,H,3), g_b_inp (M,H), g_w_out (M,H); blocks = 0: zeros.
__global__ __launch_bounds__(kGradBlock) void param_reduce_bank_kernel(const double *__restrict__ part, int blocks, int H,
                                                                       double *__restrict__ g_w_inp,
                                                                       double *__restrict__ g_b_inp,
                                                                       double *__restrict__ g_w_out) {
    const int idx = blockIdx.x * kGradBlock + threadIdx.x, m = blockIdx.y;
    if (idx >= H * 5) return;
    const int j = idx / 5, k = idx - j * 5;
    part += (size_t)m * blocks * H * 5;
    double sum = 0.0;
    for (int q = 0; q < blocks; ++q) sum += part[((size_t)q * H + j) * 5 + k];
    if (k < 3) g_w_inp[((size_t)m * H + j) * 3 + k] = sum;
    else if (k == 3) g_b_inp[(size_t)m * H + j] = sum;
    else g_w_out[(size_t)m * H + j] = sum;
}

}  // namespace press_train
}  // namespace fcr
