// fcr_supervised.h — the supervised (behaviour-cloning) baseline's training epoch on gfx950: NeuralNetwork.train_model /
// validate_model of Supervised Learning/Functions.py:396-464 for the 3 -> hidden -> 1 FNNModel (SL/Main.py:143-159),
// every optimizer step of an epoch in ONE launch, one workgroup per independent model.
//
// One step is bs x 5·hidden of arithmetic (256 x 250 at the reference's shape): microseconds of work that torch
// spreads over ~10 launches and a host .item(). Here the model's parameters stay in LDS (the [k][W0 W1 W2 b wout]
// records fnn_sample reads), its AdamW moments in the registers of wave 0 (lane k owns hidden unit k's five
// parameters) and the step counter with them; per batch the lanes are samples for the forward (as fnn_fwd_kernel),
// then hidden units for the parameter sums (as fnn_bwd_kernel), and wave 0 applies torch's AdamW update in place.
// Every sum runs in a fixed order: two launches on the same inputs agree bit for bit.
#pragma once
#include "fcr_common.h"
#include "fcr_fnn_sample.h"

namespace fcr {
namespace supervised {

constexpr int kSlBlock = 256;                 // lanes of a workgroup = samples of one pass over a batch
constexpr int kSlWaves = kSlBlock / kWave;
constexpr int kLossL1 = 0, kLossMse = 1;      // FCR_LOSS_L1 / FCR_LOSS_MSE (include/fcr.h)

struct SlArgs {
    int n, bs, nb, hidden;                    // samples, batch size, batches per epoch = ceil(n / bs), hidden units
    double lr, beta1, beta2;
    float decay, eps;                         // 1 - lr·weight_decay; AdamW's eps
    const float *X, *y;                       // (n,3), (n)
    const int *perm;                          // (M,n) sample order per model, or null: 0..n-1
    float *wi, *bi, *wo;                      // (M,hidden,3), (M,hidden), (M,hidden)
    float *m_wi, *m_bi, *m_wo;                // exp_avg
    float *v_wi, *v_bi, *v_wo;                // exp_avg_sq
    float *step;                              // (M) optimizer steps taken so far (torch keeps it as a float)
    float *loss;                              // (M,nb) the batches' mean losses
};

// beta^k for an integer k >= 0 in fp64 (bias corrections of a run that continues at step k)
__device__ __forceinline__ double ipow(double b, int k) {
    double r = 1.0;
    for (; k > 0; k >>= 1, b *= b)
        if (k & 1) r *= b;
    return r;
}

// fnn_sample over groups of kSlGroup units: the group's count is a constant, so its loop unrolls and its LDS reads issue
// back to back (one latency per group, not per unit); the groups' sums add up in order
constexpr int kSlGroup = 10;
__device__ __forceinline__ float sl_forward(const float (*sp)[5], int hidden, float x0, float x1, float x2) {
    float pre = 0.0f;
    int k0 = 0;
    for (; k0 + kSlGroup <= hidden; k0 += kSlGroup) pre += fnn::fnn_sample(sp + k0, kSlGroup, x0, x1, x2);
    return pre + fnn::fnn_sample(sp + k0, hidden - k0, x0, x1, x2);
}

template <int LOSS, bool TRAIN>
__global__ __launch_bounds__(kSlBlock) void sl_epoch_kernel(SlArgs a) {
    __shared__ float sp[fnn::kFnnMaxHidden][5];
    __shared__ float4 ss[kSlBlock];                                  // staged (x0, x1, x2, dpre) of one pass
    __shared__ float red[kSlWaves][fnn::kFnnMaxHidden][5];
    __shared__ float lred[2][kSlWaves];                              // by batch parity: read while the next batch runs
    const int model = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int hidden = a.hidden, n = a.n, bs = a.bs;
    const size_t mo = (size_t)model * hidden;
    fnn::load_params(sp, hidden, a.wi + mo * kCtrlIn, a.bi + mo, a.wo + mo);
    const int *perm = a.perm ? a.perm + (size_t)model * n : nullptr;
    const bool owner = TRAIN && w == 0 && lane < hidden;             // this lane updates hidden unit `lane`
    float mom[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, var[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    double b1p = 1.0, b2p = 1.0;                                     // beta^step
    int step0 = 0;
    if (TRAIN) {
        step0 = (int)a.step[model];
        if (owner) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                mom[p] = a.m_wi[(mo + lane) * kCtrlIn + p];
                var[p] = a.v_wi[(mo + lane) * kCtrlIn + p];
            }
            mom[3] = a.m_bi[mo + lane];
            var[3] = a.v_bi[mo + lane];
            mom[4] = a.m_wo[mo + lane];
            var[4] = a.v_wo[mo + lane];
            b1p = ipow(a.beta1, step0);
            b2p = ipow(a.beta2, step0);
        }
    }
    // One sample of the pass that starts `off` samples into batch j: (x, y) through the index table. The next pass's
    // sample is fetched while this one is computed, so the two dependent reads (index, then row) hide behind it.
    float nx0 = 0.0f, nx1 = 0.0f, nx2 = 0.0f, ny = 0.0f;
    auto fetch = [&](int j, int off) {
        if (j >= a.nb) return;
        const int b0 = j * bs, left = n - b0, i = off + tid;
        if (i >= (left < bs ? left : bs)) return;
        int s = perm ? perm[b0 + i] : b0 + i;
        s = s < 0 ? 0 : (s >= n ? n - 1 : s);                        // a bad index reads a wrong row, never out of bounds
        const float *x = a.X + (size_t)s * kCtrlIn;
        nx0 = x[0];
        nx1 = x[1];
        nx2 = x[2];
        ny = a.y[s];
    };
    fetch(0, 0);
    __syncthreads();
    const int k = lane < hidden ? lane : 0;
    for (int j = 0; j < a.nb; ++j) {
        const int left = n - j * bs, bsj = left < bs ? left : bs;    // the last batch may be short
        float lsum = 0.0f, acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int off = 0; off < bsj; off += kSlBlock) {
            const int cn = bsj - off < kSlBlock ? bsj - off : kSlBlock;
            const bool last = off + kSlBlock >= bsj;
            const float x0 = nx0, x1 = nx1, x2 = nx2, yv = ny;
            fetch(last ? j + 1 : j, last ? 0 : off + kSlBlock);
            if (tid < cn) {
                const float pre = sl_forward(sp, hidden, x0, x1, x2);
                const float diff = hardtanh(pre) - yv;
                lsum += LOSS == kLossL1 ? fabsf(diff) : diff * diff;
                if (TRAIN) {
                    // d loss·bs_j / d out: sign(diff) with sign(0) = 0 (L1), 2 diff (MSE); Hardtanh' = 1 on (-1, 1)
                    const float g = LOSS == kLossL1 ? (diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f)) : 2.0f * diff;
                    ss[tid] = make_float4(x0, x1, x2, (pre > -1.0f && pre < 1.0f) ? g : 0.0f);
                }
            }
            if (TRAIN) {
                __syncthreads();
                const float W0 = sp[k][0], W1 = sp[k][1], W2 = sp[k][2], bk = sp[k][3];
                // dz_k / wout_k: the unit's own factor wout_k multiplies the finished sums (below). Under L1 the
                // bias sum is then a count of +-1, exact in any order: signs that cancel give a gradient of exactly 0,
                // as in exact arithmetic, where a sum of +-wout_k/bs leaves rounding noise of the size of AdamW's eps
                // and a fresh optimizer turns that noise into a move of lr/10.
                auto add = [&](const float4 s) {
                    const float z = fmaf(W2, s.z, fmaf(W1, s.y, W0 * s.x)) + bk;
                    const float dz = z > 0.0f ? s.w : 0.0f;          // ReLU'(0) = 0
                    acc[0] = fmaf(dz, s.x, acc[0]);
                    acc[1] = fmaf(dz, s.y, acc[1]);
                    acc[2] = fmaf(dz, s.z, acc[2]);
                    acc[3] += dz;
                    acc[4] = fmaf(s.w, relu(z), acc[4]);
                };
                // lanes = hidden units, waves stride the samples (in order: the sums do not depend on the grouping);
                // four records are read before the first is used, so their LDS latencies overlap
                int i = w;
                for (; i + 3 * kSlWaves < cn; i += 4 * kSlWaves) {
                    const float4 s0 = ss[i], s1 = ss[i + kSlWaves], s2 = ss[i + 2 * kSlWaves], s3 = ss[i + 3 * kSlWaves];
                    add(s0);
                    add(s1);
                    add(s2);
                    add(s3);
                }
                for (; i < cn; i += kSlWaves) add(ss[i]);
                if (!last) __syncthreads();                          // the next pass overwrites ss
            }
        }
        // the batch's sums: lanes of a wave (fixed butterfly), then the waves in order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
        if (lane == 0) lred[j & 1][w] = lsum;
        if (TRAIN) {
#pragma unroll
            for (int p = 0; p < 5; ++p) red[w][lane][p] = acc[p];
        }
        __syncthreads();
        const float inv = 1.0f / (float)bsj;
        if (tid == kSlBlock - 1) {
            float s = 0.0f;
#pragma unroll
            for (int ww = 0; ww < kSlWaves; ++ww) s += lred[j & 1][ww];
            a.loss[(size_t)model * a.nb + j] = s * inv;
        }
        if (TRAIN) {
            if (owner) {
                // torch.optim.AdamW, one step (decoupled decay, bias-corrected moments, eps outside the root)
                b1p *= a.beta1;
                b2p *= a.beta2;
                const float step_size = (float)(a.lr / (1.0 - b1p)), bc2 = (float)sqrt(1.0 - b2p);
                const float w1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, w2 = (float)(1.0 - a.beta2);
                const float wk = sp[lane][4];                        // wout_k of this batch's forward
#pragma unroll
                for (int p = 0; p < 5; ++p) {
                    float g = 0.0f;
#pragma unroll
                    for (int ww = 0; ww < kSlWaves; ++ww) g += red[ww][lane][p];
                    g = (p < 4 ? g * wk : g) * inv;
                    mom[p] += (g - mom[p]) * w1;
                    var[p] = fmaf(w2 * g, g, var[p] * b2);
                    const float denom = sqrtf(var[p]) / bc2 + a.eps;
                    sp[lane][p] = fmaf(-step_size, mom[p] / denom, sp[lane][p] * a.decay);
                }
            }
            __syncthreads();                                         // the next batch's forward reads the new sp
        }
    }
    if (owner) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            a.wi[(mo + lane) * kCtrlIn + p] = sp[lane][p];
            a.m_wi[(mo + lane) * kCtrlIn + p] = mom[p];
            a.v_wi[(mo + lane) * kCtrlIn + p] = var[p];
        }
        a.bi[mo + lane] = sp[lane][3];
        a.m_bi[mo + lane] = mom[3];
        a.v_bi[mo + lane] = var[3];
        a.wo[mo + lane] = sp[lane][4];
        a.m_wo[mo + lane] = mom[4];
        a.v_wo[mo + lane] = var[4];
        if (lane == 0) a.step[model] = (float)(step0 + a.nb);
    }
}

}  // namespace supervised
}  // namespace fcr
