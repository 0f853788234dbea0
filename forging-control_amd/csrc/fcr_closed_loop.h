// fcr_closed_loop.h — the NN controller driving the press, all T steps of B trajectories in one launch
// (SURVEY.md §8(f) ranks 1 + 2 together: the closed-loop evaluation the plant row exists for).
//
// Reference: NeuralNetwork.loop (Functions.py:1075-1240; with its feasibility recovery: fcr_feasibility.h), per step t:
//   X = [y_dot, z, ref_t]; X_new = scalers['input'].transform(X) with the last column replaced by
//   scalers['y_dot'].transform(ref_t) (NN_make_step, Functions.py:1594-1598); u = scalers['output']
//   .inverse_transform(FNN(float32(X_new))) (:1601-1604); x_{t+1} = plant(x_t, u) (:1178-1179; here the
//   reference's own RK4 integrator F of Ruge_Kuta, Functions.py:1743-1781, in place of do-mpc's CVODES).
// The scalers are MaxAbsScalers (UL/Main.py:237-256): transform = x / scale, inverse = x · scale.
//
// One lane owns one trajectory: fp64 state in VGPRs for all T steps, the 3->H->1 controller in fp32 as
// torch evaluates it (weights in LDS, one FMA chain per hidden unit), the plant in fp64. HBM sees the
// reference (8 B) in and u (8 B) + the state (40 B) out per step; with pre-drawn process and measurement noise
// 40 B or 80 B more in.
//
// Every kernel of the family — plain, under the harness's noise, with feasibility recovery — is loop_body below.
// One step: the controller reads the RECORD m = x + v and forms u_NN; the command policy turns it into the command
// to apply (itself, or its projection from the record: fcr_feasibility.h) and stores what it reports; the plant steps
// the unperturbed state x under that command, with the process noise w added to the right-hand side at every RK4
// stage (fcr_plant.h); the new record x + v is written to x[:, t+1]. So the measurement noise v (B,T,5) reaches the
// controller and the projection — the harness feeds make_step's return value back in (Functions.py:1170-1183) —
// while the integration continues from the unperturbed state. w (B,T,5) and v are pre-drawn; either may be null.
// Under NOISE all five components of the record are carried; without it m = x and the compiler keeps one of them.
// Out of scope: the smooth model measures p_eff, not p (template_model.py:154-155); the record here is p + v.
#pragma once
#include <hip/hip_runtime.h>

#include "fcr_plant.h"

namespace fcr {
namespace closed_loop {

constexpr int kClBlock = 256;
constexpr int kClMaxHidden = 256;

struct ClArgs {
    int B, T, substeps, hidden;
    double dt;
    const double *x0, *ref;
    const float *w_inp, *b_inp, *w_out;
    double in_scale0, in_scale1, ref_scale, out_scale;
    double *x, *u;
};

// The command policy of the loop without recovery: u[b,t] = u_NN. A policy holds its (B,T) outputs; row(b·T) is the
// policy of one lane, its pointers at that lane's row, formed once before the loop (indexing [b·T + t] per step
// instead gives the recovering kernels another register budget).
struct PlainCommand {
    double *u;
    __device__ __forceinline__ PlainCommand row(size_t r) const { return {u + r}; }
    __device__ __forceinline__ double operator()(const double (&)[5], double un, int t) const {
        u[t] = un;
        return un;
    }
};

template <bool SMOOTH, bool NOISE, class Command>
__device__ __forceinline__ void loop_body(ClArgs a, const double *wn, const double *vn, Command policy) {
    __shared__ float w[kClMaxHidden * 5];        // [j] = (w_inp[j][0..2], b_inp[j], w_out[j])
    for (int i = threadIdx.x; i < a.hidden; i += kClBlock) {
        w[i * 5 + 0] = a.w_inp[i * 3 + 0];
        w[i * 5 + 1] = a.w_inp[i * 3 + 1];
        w[i * 5 + 2] = a.w_inp[i * 3 + 2];
        w[i * 5 + 3] = a.b_inp[i];
        w[i * 5 + 4] = a.w_out[i];
    }
    __syncthreads();
    const int b = blockIdx.x * kClBlock + threadIdx.x;
    if (b >= a.B) return;
    double x[5], m[5];                            // the press's state; the record the controller and the policy read
    double *o = a.x + (size_t)b * (a.T + 1) * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = a.x0[(size_t)b * 5 + i];
        m[i] = x[i];
        o[i] = x[i];
    }
    const size_t row = (size_t)b * a.T;
    const double *rb = a.ref + row;
    const Command command = policy.row(row);
    for (int t = 0; t < a.T; ++t) {
        // NN_make_step: scaled input in fp64, then float32 for the torch model (Functions.py:1594-1601)
        const float s0 = (float)(m[1] / a.in_scale0), s1 = (float)(m[4] / a.in_scale1), s2 = (float)(rb[t] / a.ref_scale);
        float v = 0.0f;
        for (int j = 0; j < a.hidden; ++j) {   // fc_inp + ReLU, fc_out (no bias) (Functions.py:275-287)
            const float *wj = w + j * 5;
            float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
            z = z > 0.0f ? z : 0.0f;
            v = fmaf(wj[4], z, v);
        }
        v = fminf(fmaxf(v, -1.0f), 1.0f);                   // Hardtanh
        const double un = (double)(v * (float)a.out_scale); // inverse_transform on the float32 output
        const double u = command(m, un, t);
        double wt[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, vt[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (NOISE) {
            const size_t nt = (row + t) * 5;
            if (wn) {
#pragma unroll
                for (int i = 0; i < 5; ++i) wt[i] = wn[nt + i];
            }
            if (vn) {
#pragma unroll
                for (int i = 0; i < 5; ++i) vt[i] = vn[nt + i];
            }
        }
        plant::rk4_step<SMOOTH, NOISE>(x, u, a.dt, a.substeps, wt);
        o += 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            m[i] = NOISE ? x[i] + vt[i] : x[i];
            o[i] = m[i];
        }
    }
}

template <bool SMOOTH>
__global__ __launch_bounds__(kClBlock) void closed_loop_kernel(ClArgs a) {
    loop_body<SMOOTH, false>(a, nullptr, nullptr, PlainCommand{a.u});
}

template <bool SMOOTH>
__global__ __launch_bounds__(kClBlock) void closed_loop_noise_kernel(ClArgs a, const double *wn, const double *vn) {
    loop_body<SMOOTH, true>(a, wn, vn, PlainCommand{a.u});
}

}  // namespace closed_loop
}  // namespace fcr
