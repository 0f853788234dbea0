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
//
// A bank of M controllers is the same body under two more policies, both defaulted so the single-model
// kernels are what they were: BankModel gives a block its model, its local rows and the model's base offsets;
// LaneStats keeps the evaluation's per-trajectory sums in registers and makes the per-step stores optional.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
    // as called under LaneStats: the store is optional, the flag is 0
    __device__ __forceinline__ double operator()(const double (&)[5], double un, int t, bool store, int &flag) const {
        if (store) u[t] = un;
        flag = 0;
        return un;
    }
};

// Which model a block works for. SingleModel: the one model of the single-model kernels, every member a compile-time 0 /
// the identity. BankModel: model m owns blocks m * bpm .. (m + 1) * bpm - 1, bpm = ceil(B / 256); its weights are rows
// m of the stacked (M,hidden,3) / (M,hidden) arrays, its outputs rows m * B .. of the model-major ones, and each of x0,
// ref, w, v starts m * stride elements into its buffer (stride 0: one copy shared by all models).
struct SingleModel {
    __device__ __forceinline__ int model() const { return 0; }
    __device__ __forceinline__ int block() const { return blockIdx.x; }
    __device__ __forceinline__ size_t x0() const { return 0; }
    __device__ __forceinline__ size_t ref() const { return 0; }
    __device__ __forceinline__ size_t w() const { return 0; }
    __device__ __forceinline__ size_t v() const { return 0; }
    __device__ __forceinline__ plant::Nominal press(int) const { return {}; }
};

struct BankStrides {
    long long x0, ref, w, v;
};

struct BankModel {
    int m, blk;
    BankStrides s;
    __device__ __forceinline__ BankModel(int B, BankStrides st) : s(st) {
        const int bpm = (B + kClBlock - 1) / kClBlock;
        m = blockIdx.x / bpm;
        blk = blockIdx.x - m * bpm;
    }
    __device__ __forceinline__ int model() const { return m; }
    __device__ __forceinline__ int block() const { return blk; }
    __device__ __forceinline__ size_t x0() const { return (size_t)m * s.x0; }
    __device__ __forceinline__ size_t ref() const { return (size_t)m * s.ref; }
    __device__ __forceinline__ size_t w() const { return (size_t)m * s.w; }
    __device__ __forceinline__ size_t v() const { return (size_t)m * s.v; }
    __device__ __forceinline__ plant::Nominal press(int) const { return {}; }
};

// Whose press a lane steps: the models above step the reference's, compile-time constants
// (plant::Nominal), as they always did. BankPressModel: lane b's own — row m * stride_model + b * stride_traj (elements;
// 0 = shared, as for x0 / ref / w / v) of a table of plant::kPressFields doubles per row, from which the lane derives its
// coefficients once, before the loop, into registers.
struct PressTable {
    const double *press;
    long long stride_model, stride_traj;
};

struct BankPressModel : BankModel {
    PressTable t;
    __device__ __forceinline__ BankPressModel(int B, BankStrides st, PressTable table) : BankModel(B, st), t(table) {}
    __device__ __forceinline__ plant::LaneParams press(int b) const {
        return plant::derive(t.press + (size_t)m * t.stride_model + (size_t)b * t.stride_traj);
    }
};

// max that keeps a NaN once it has one (np.maximum)
__device__ __forceinline__ double keep_nan_max(double v, double t) { return (t > v || t != t) ? t : v; }

// What a lane accumulates beside the loop. NoStats: nothing, every per-step store is made, and the policy is called as
// it always was. LaneStats (the bank kernels): over t = 0..T-1, with r = ref[b,t], (y, p1, p2) of the record x[:,t+1] as
// stored (measurement noise included) and u the applied command,
//   traj_stats  (.,6) fp64   sum |y - r|, sum (y - r)^2, max |y - r|, sum |u|, sum_{t>=1} (u_t - u_{t-1})^2,
//                            max_t max(p1_lo - p1, p1 - p1_hi, p2_lo - p2, p2 - p2_hi)   (Pa; 0 at T = 0)
//   traj_counts (.,3) int32  steps whose violation is > 0, steps flagged 1, steps flagged 2
//   x_final     (.,5) fp64   the unperturbed state after step T
// written once after the loop. Each square is an explicit fma, so contraction has nothing to decide and a run that
// stores its trajectories and one that does not give the same bits. STORE is a template flag, not a run-time branch:
// the row pointers of x, u, u_nn and flag are eight VGPRs a lane holds over the whole loop, and without them every
// non-storing instantiation fits three waves per SIMD (<= 164 VGPRs), which the storing noisy recovering ones
// (170 / 174) do not.
struct NoStats {
    static constexpr bool kOn = false, kStore = true;
    __device__ __forceinline__ void step(double, const double (&)[5], double, int, int) {}
    __device__ __forceinline__ void finish(size_t, const double (&)[5], int) const {}
};

struct StatsArgs {
    double p1_lo, p1_hi, p2_lo, p2_hi;   // Pa
    double *traj_stats;
    int32_t *traj_counts;
    double *x_final;
};

template <bool STORE>
struct LaneStats {
    static constexpr bool kOn = true, kStore = STORE;
    StatsArgs k;
    double s_abs = 0.0, s_sq = 0.0, e_max = 0.0, s_u = 0.0, s_du = 0.0, v_max = -HUGE_VAL, u_prev = 0.0;
    int n_viol = 0, n_flag1 = 0, n_flag2 = 0;
    __device__ __forceinline__ explicit LaneStats(StatsArgs args) : k(args) {}
    __device__ __forceinline__ void step(double r, const double (&m)[5], double u, int flag, int t) {
        const double e = m[1] - r, ae = fabs(e);
        s_abs += ae;
        s_sq = fma(e, e, s_sq);
        e_max = keep_nan_max(e_max, ae);
        s_u += fabs(u);
        const double d = t > 0 ? u - u_prev : 0.0;
        s_du = fma(d, d, s_du);
        u_prev = u;
        const double viol = keep_nan_max(keep_nan_max(k.p1_lo - m[2], m[2] - k.p1_hi), keep_nan_max(k.p2_lo - m[3], m[3] - k.p2_hi));
        v_max = keep_nan_max(v_max, viol);
        n_viol += viol > 0.0;
        n_flag1 += flag == 1;
        n_flag2 += flag == 2;
    }
    __device__ __forceinline__ void finish(size_t g, const double (&x)[5], int T) const {
        double *s = k.traj_stats + g * 6;
        s[0] = s_abs, s[1] = s_sq, s[2] = e_max, s[3] = s_u, s[4] = s_du, s[5] = T > 0 ? v_max : 0.0;
        int32_t *c = k.traj_counts + g * 3;
        c[0] = n_viol, c[1] = n_flag1, c[2] = n_flag2;
#pragma unroll
        for (int i = 0; i < 5; ++i) k.x_final[g * 5 + i] = x[i];
    }
};

// The policy's command for step t: called as it always was, or (under statistics) with the optional store and the flag.
template <bool STATS, class Command>
__device__ __forceinline__ double apply(const Command &command, const double (&m)[5], double un, int t, bool store, int &flag) {
    if constexpr (STATS) return command(m, un, t, store, flag);
    else return command(m, un, t);
}

template <bool SMOOTH, bool NOISE, class Command, class Model = SingleModel, class Stats = NoStats>
__device__ __forceinline__ void loop_body(ClArgs a, const double *wn, const double *vn, Command policy,
                                          Model model = Model{}, Stats stats = Stats{}) {
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
    constexpr bool store = Stats::kStore;
    double x[5], m[5];                            // the press's state; the record the controller and the policy read
    double *o = a.x + g * (a.T + 1) * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = a.x0[model.x0() + (size_t)b * 5 + i];
        m[i] = x[i];
        if (store) o[i] = x[i];
    }
    const size_t row = (size_t)b * a.T;
    const double *rb = a.ref + model.ref() + row;
    const Command command = policy.row(g * a.T);
    for (int t = 0; t < a.T; ++t) {
        // NN_make_step: scaled input in fp64, then float32 for the torch model (Functions.py:1594-1601)
        const float s0 = (float)(m[1] / a.in_scale0), s1 = (float)(m[4] / a.in_scale1);
        const double r = rb[t];
        const float s2 = (float)(r / a.ref_scale);
        float v = 0.0f;
        for (int j = 0; j < a.hidden; ++j) {   // fc_inp + ReLU, fc_out (no bias) (Functions.py:275-287)
            const float *wj = w + j * 5;
            float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
            z = z > 0.0f ? z : 0.0f;
            v = fmaf(wj[4], z, v);
        }
        v = fminf(fmaxf(v, -1.0f), 1.0f);                   // Hardtanh
        const double un = (double)(v * (float)a.out_scale); // inverse_transform on the float32 output
        int flag = 0;
        const double u = apply<Stats::kOn>(command, m, un, t, store, flag);
        double wt[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, vt[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (NOISE) {
            const size_t nt = (row + t) * 5;
            if (wn) {
#pragma unroll
                for (int i = 0; i < 5; ++i) wt[i] = wn[model.w() + nt + i];
            }
            if (vn) {
#pragma unroll
                for (int i = 0; i < 5; ++i) vt[i] = vn[model.v() + nt + i];
            }
        }
        plant::rk4_step<SMOOTH, NOISE>(x, u, a.dt, a.substeps, wt, pp);
        o += 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            m[i] = NOISE ? x[i] + vt[i] : x[i];
            if (store) o[i] = m[i];
        }
        stats.step(r, m, u, flag, t);
    }
    stats.finish(g, x, a.T);
}

template <bool SMOOTH>
__global__ __launch_bounds__(kClBlock) void closed_loop_kernel(ClArgs a) {
    loop_body<SMOOTH, false>(a, nullptr, nullptr, PlainCommand{a.u});
}

template <bool SMOOTH>
__global__ __launch_bounds__(kClBlock) void closed_loop_noise_kernel(ClArgs a, const double *wn, const double *vn) {
    loop_body<SMOOTH, true>(a, wn, vn, PlainCommand{a.u});
}

// M controllers in one launch (fcr_closed_loop_run_bank): grid M * ceil(B / 256); a.w_inp / b_inp / w_out are the stacked
// weights, a.x / a.u the model-major outputs (STORE) or null (nothing stored per step), wn / vn null or per-model by
// stride.
template <bool SMOOTH, bool NOISE, bool STORE>
__global__ __launch_bounds__(kClBlock) void closed_loop_bank_kernel(ClArgs a, BankStrides strides, StatsArgs stats,
                                                                    const double *wn, const double *vn) {
    loop_body<SMOOTH, NOISE>(a, wn, vn, PlainCommand{a.u}, BankModel(a.B, strides), LaneStats<STORE>(stats));
}

// closed_loop_bank_kernel where every trajectory has its own press (fcr_closed_loop_run_bank_press).
template <bool SMOOTH, bool NOISE, bool STORE>
__global__ __launch_bounds__(kClBlock) void closed_loop_bank_press_kernel(ClArgs a, BankStrides strides, StatsArgs stats,
                                                                          const double *wn, const double *vn,
                                                                          PressTable press) {
    loop_body<SMOOTH, NOISE>(a, wn, vn, PlainCommand{a.u}, BankPressModel(a.B, strides, press), LaneStats<STORE>(stats));
}

// The per-model summary of a bank run from its per-trajectory statistics: one block per model, every sum taken in a
// fixed order (lane tid keeps eight partial sums, the k-th over elements tid + 1024 (8 j + k), j = 0, 1, ...; adds them
// pairwise; then a pairwise tree over the block), so the same call twice gives the same bits. The eight independent
// sums keep eight loads per lane in flight: with one running sum the two passes over ref are bound by one load's
// latency per element (measured: most of a launch at B = 65 536). summary (M,10) over n = B * T steps:
//   MAE, RMSE, R2 = 1 - SSE / SST, max |e|, mean |u|, RMS of du over B (T - 1) terms (0 at T = 1), the worst violation,
//   and the fractions of steps violating, flagged 1, flagged 2.
// SST = sum (r - mean r)^2 is taken from ref in two passes, the mean first (as sklearn's r2_score does), so nothing
// cancels; SST = 0 gives sklearn's 1 (SSE = 0) or 0. n = 0: ten zeros.
constexpr int kRedBlock = 1024, kRedWays = 8;

struct RedArgs {
    int B, T;
    long long ref_stride;
    const double *ref, *traj_stats;
    const int32_t *traj_counts;
    double *summary;
};

template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double *sh) {
    const int tid = threadIdx.x;
    __syncthreads();                             // the previous reduction's result has been read
    sh[tid] = v;
    __syncthreads();
    for (int s = kRedBlock / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = MAX ? keep_nan_max(sh[tid], sh[tid + s]) : sh[tid] + sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// This lane's share of a sum over v[0..n): acc_k = add(acc_k, v[tid + 1024 (8 j + k)]), then ((0+1)+(2+3))+((4+5)+(6+7)).
template <class Add>
__device__ __forceinline__ double strided_sum(const double *v, size_t n, Add add) {
    constexpr size_t kStep = (size_t)kRedBlock * kRedWays;
    double acc[kRedWays];
#pragma unroll
    for (int k = 0; k < kRedWays; ++k) acc[k] = 0.0;
    size_t i = threadIdx.x;
    for (; i + kStep - kRedBlock < n; i += kStep) {   // all eight elements exist
        double r[kRedWays];
#pragma unroll
        for (int k = 0; k < kRedWays; ++k) r[k] = v[i + (size_t)k * kRedBlock];
#pragma unroll
        for (int k = 0; k < kRedWays; ++k) acc[k] = add(acc[k], r[k]);
    }
#pragma unroll
    for (int k = 0; k < kRedWays; ++k)
        if (i + (size_t)k * kRedBlock < n) acc[k] = add(acc[k], v[i + (size_t)k * kRedBlock]);
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

__global__ __launch_bounds__(kRedBlock) void loop_stats_reduce_kernel(RedArgs a) {
    __shared__ double sh[kRedBlock];
    const int tid = threadIdx.x;
    const size_t mdl = blockIdx.x, n = (size_t)a.B * a.T;
    double *out = a.summary + mdl * 10;
    if (n == 0) {
        if (tid < 10) out[tid] = 0.0;
        return;
    }
    const double *ref = a.ref + mdl * a.ref_stride;
    const double mean = block_reduce<false>(strided_sum(ref, n, [](double acc, double r) { return acc + r; }), sh) / (double)n;
    const double sst = block_reduce<false>(strided_sum(ref, n, [mean](double acc, double r) {
                                               const double d = r - mean;
                                               return fma(d, d, acc);
                                           }), sh);
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, cnt[3] = {0.0, 0.0, 0.0}, e_max = 0.0, v_max = -HUGE_VAL;
    for (size_t b = tid; b < (size_t)a.B; b += kRedBlock) {
        const double *ts = a.traj_stats + (mdl * a.B + b) * 6;
        const int32_t *tc = a.traj_counts + (mdl * a.B + b) * 3;
        sum[0] += ts[0], sum[1] += ts[1], sum[2] += ts[3], sum[3] += ts[4];
        e_max = keep_nan_max(e_max, ts[2]);
        v_max = keep_nan_max(v_max, ts[5]);
#pragma unroll
        for (int i = 0; i < 3; ++i) cnt[i] += (double)tc[i];   // exact: a count is at most n < 2^53
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] = block_reduce<false>(sum[i], sh);
#pragma unroll
    for (int i = 0; i < 3; ++i) cnt[i] = block_reduce<false>(cnt[i], sh);
    e_max = block_reduce<true>(e_max, sh);
    v_max = block_reduce<true>(v_max, sh);
    if (tid == 0) {
        const double dn = (double)n, n_du = (double)a.B * (double)(a.T - 1);
        out[0] = sum[0] / dn;
        out[1] = sqrt(sum[1] / dn);
        out[2] = sst != 0.0 ? 1.0 - sum[1] / sst : (sum[1] == 0.0 ? 1.0 : 0.0);
        out[3] = e_max;
        out[4] = sum[2] / dn;
        out[5] = a.T > 1 ? sqrt(sum[3] / n_du) : 0.0;
        out[6] = v_max;
        out[7] = cnt[0] / dn;
        out[8] = cnt[1] / dn;
        out[9] = cnt[2] / dn;
    }
}

}  // namespace closed_loop
}  // namespace fcr
