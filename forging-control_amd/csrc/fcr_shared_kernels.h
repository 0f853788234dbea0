// fcr_shared_kernels.h — the non-template kernels that more than one engine launches: the range guard, the small
// packs, the loss and controller-gradient reductions. A non-template __global__ has an external host stub, so these are
// compiled into ONE translation unit, fcr_rollout.hip, and every other file launches them through the functions
// fcr_host.h declares (launch_range, launch_pack_all, launch_pack_ctrl, launch_loss_reduce, launch_ctrl_grads,
// launch_grad_reduce). Their items and constants stay in fcr_pack.h, fcr_f16.h and fcr_img.h.
#pragma once
#include "fcr_f16.h"
#include "fcr_img.h"
#include "fcr_pack.h"

namespace fcr {

__global__ __launch_bounds__(64) void range_final_kernel(const float *__restrict__ part, int nblk,
                                                         const float *__restrict__ fcw,
                                                         const float *__restrict__ fcb, int H, float *wsc) {
    range_final_wave(part, nblk, fcw, fcb, H, wsc, threadIdx.x);
}

__global__ __launch_bounds__(kRangeThreads) void range_partial_kernel(const float *__restrict__ states,
                                                                      const float *__restrict__ u0,
                                                                      const float *__restrict__ noise, int B, int N,
                                                                      float *part, const float *fcw = nullptr,
                                                                      const float *fcb = nullptr, int H = 0,
                                                                      float *wsc = nullptr) {
    __shared__ float red[kIn][kRangeThreads];
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
    const size_t stride = (size_t)gridDim.x * blockDim.x, tid0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t rows = (size_t)B * kL;
    for (size_t r = tid0; r < rows; r += stride) {
        const float *p = states + r * kIn;
        m0 = fmaxf(m0, fabsf(p[0]));
        m1 = fmaxf(m1, fabsf(p[1]));
        m2 = fmaxf(m2, fabsf(p[2]));
        m3 = fmaxf(m3, fabsf(p[3]));
        m4 = fmaxf(m4, fabsf(p[4]));
    }
    for (size_t b = tid0; b < (size_t)B; b += stride) m4 = fmaxf(m4, fabsf(u0[b]));
    if (noise)
        for (size_t r = tid0; r < (size_t)B * N; r += stride) {
            const float *p = noise + r * kOut;
            m0 = fmaxf(m0, fabsf(p[0]));
            m1 = fmaxf(m1, fabsf(p[1]));
            m2 = fmaxf(m2, fabsf(p[2]));
            m3 = fmaxf(m3, fabsf(p[3]));
        }
    red[0][threadIdx.x] = m0;
    red[1][threadIdx.x] = m1;
    red[2][threadIdx.x] = m2;
    red[3][threadIdx.x] = m3;
    red[4][threadIdx.x] = m4;
    __syncthreads();
    for (int w = kRangeThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < kIn; ++c) red[c][threadIdx.x] = fmaxf(red[c][threadIdx.x], red[c][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x < kIn) part[blockIdx.x * 8 + threadIdx.x] = red[threadIdx.x][0];
    if (wsc) {   // launched as one block: the final step too (range_final_kernel's, one launch fewer)
        __syncthreads();
        if (threadIdx.x < 64) range_final_wave(part, 1, fcw, fcb, H, wsc, threadIdx.x);
    }
}

__global__ void pack_misc_kernel(PackArgs a) { pack_misc_item(a, blockIdx.x * blockDim.x + threadIdx.x); }

// loss = sum(loss_part[0..nw)) / B, fixed order (one block)
__device__ __forceinline__ void loss_reduce_block(const float *part, int nw, int B, float *loss) {
    __shared__ float red[256];
    float s = 0.0f;
    for (int i = threadIdx.x; i < nw; i += blockDim.x) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] / (float)B;
}
__global__ void loss_reduce_kernel(const float *part, int nw, int B, float *loss) { loss_reduce_block(part, nw, B, loss); }
// M models (fcr_forward_many): block m sums model m's gpm partials in the same order -> loss[m]
__global__ void loss_reduce_many_kernel(const float *part, int gpm, int B, float *loss) {
    loss_reduce_block(part + (size_t)blockIdx.x * gpm, gpm, B, loss + blockIdx.x);
}

// Controller parameter gradients (the in-loss controller calls, Functions.py:1424-1430), from the dv
// the backward kernel stored per (trajectory, step): z = W_inp·[x0, x3, ref] + b is recomputed from
// the stored xhat with the same arithmetic as fnn_pre; dz = dv·w_out·1[z>0]. One block per chunk of
// (trajectory, step) items; a wave's lanes are the hidden units; fixed-order sums everywhere.
// The call fed by step j is u_{j+1}'s, so its reference is r_{j+1} = ref[b * ref_b + (j + 1) * ref_j] (the default:
// X + 2 with strides (3, 0)); the last step feeds no call (dv = 0) and reads r_{N-1}, in bounds.
__device__ __forceinline__ void ctrl_grad_block(const float *ref, long long ref_b, long long ref_j, const float *xhat, const float *dv, const float *fnp,
                                                int B, int N, int hidden, float *part, float *gwi, float *gbi,
                                                float *gwo) {
    __shared__ float sx0[kCtrlItems], sx3[kCtrlItems], sref[kCtrlItems], sdv[kCtrlItems];
    __shared__ float red[kCtrlBlock / kWave][64][5];
    const long long items = (long long)B * N;
    const long long i0 = (long long)blockIdx.x * kCtrlItems;
    const int n = (int)((items - i0) < kCtrlItems ? (items - i0) : kCtrlItems);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const long long it = i0 + i;
        const int bb = (int)(it / N);
        sx0[i] = xhat[it * kOut + 0];
        sx3[i] = xhat[it * kOut + 3];
        const int jn = (int)(it - (long long)bb * N) + 1;
        sref[i] = ref[bb * ref_b + (jn < N ? jn : N - 1) * ref_j];
        sdv[i] = dv[it];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = lane;   // hidden unit
    float W0 = 0.0f, W1 = 0.0f, W2 = 0.0f, bk = 0.0f, wo = 0.0f;
    if (k < hidden) {
        const float *p = fnp + ((k >> 2) * 4 + (k & 3)) * kFnpStride;
        W0 = p[0]; W1 = p[1]; W2 = p[2]; bk = p[3]; wo = p[4];
    }
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, g4 = 0.0f;
    for (int i = w; i < n; i += kCtrlBlock / kWave) {
        const float a = sx0[i], b3 = sx3[i], r = sref[i], d = sdv[i];
        const float z = W0 * a + W1 * b3 + W2 * r + bk;    // == fnn_pre's z
        const float dz = z > 0.0f ? d * wo : 0.0f;
        g0 += dz * a;
        g1 += dz * b3;
        g2 += dz * r;
        g3 += dz;
        g4 += d * (z > 0.0f ? z : 0.0f);
    }
    red[w][lane][0] = g0; red[w][lane][1] = g1; red[w][lane][2] = g2; red[w][lane][3] = g3; red[w][lane][4] = g4;
    __syncthreads();
    if (w == 0 && k < hidden) {
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            float s = 0.0f;
#pragma unroll
            for (int ww = 0; ww < kCtrlBlock / kWave; ++ww) s += red[ww][lane][p];
            grad_out5(part, hidden, k, p, s, gwi, gbi, gwo);
        }
    }
}
__global__ __launch_bounds__(kCtrlBlock) void ctrl_grad_kernel(const float *ref, long long ref_b, long long ref_j,
                                                               const float *xhat, const float *dv,
                                                               const float *fnp, int B, int N, int hidden,
                                                               float *part, float *gwi = nullptr,
                                                               float *gbi = nullptr, float *gwo = nullptr) {
    ctrl_grad_block(ref, ref_b, ref_j, xhat, dv, fnp, B, N, hidden, part, gwi, gbi, gwo);
}
// M models (fcr_backward_many): blockIdx.y = m runs ctrl_grad_kernel's blocks over model m's B * N items of the stacked
// (M, B, ...) arrays with that model's records; `blocks` = the blocks per model (the stride of the partials); model
// m's references start at ref + m * ref_m
__global__ __launch_bounds__(kCtrlBlock) void ctrl_grad_many_kernel(const float *ref, long long ref_m, long long ref_b,
                                                                    long long ref_j, const float *xhat, const float *dv,
                                                                    const float *fnp, int B, int N, int hidden,
                                                                    float *part, int blocks, float *gwi, float *gbi,
                                                                    float *gwo) {
    const size_t m = blockIdx.y, rows = m * B;
    ctrl_grad_block(ref + (long long)m * ref_m, ref_b, ref_j, xhat + rows * N * kOut, dv + rows * N, fnp + m * (kMS * 4 * kFnpStride), B, N, hidden,
                    part + m * blocks * hidden * 5, gwi ? gwi + m * hidden * kCtrlIn : nullptr,
                    gwi ? gbi + m * hidden : nullptr, gwi ? gwo + m * hidden : nullptr);
}

// grads: one block per (unit k, param p); sum over waves in fixed order
__device__ __forceinline__ void grad_reduce_block(const float *part, int nw, int hidden, float *gwi, float *gbi,
                                                  float *gwo) {
    __shared__ float red[256];
    const int kp = blockIdx.x, k = kp / 5, p = kp % 5;
    float s = 0.0f;
    for (int i = threadIdx.x; i < nw; i += blockDim.x) s += part[((size_t)i * hidden + k) * 5 + p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float v = red[0];
        if (p < 3) gwi[k * kCtrlIn + p] = v;
        else if (p == 3) gbi[k] = v;
        else gwo[k] = v;
    }
}
__global__ void grad_reduce_kernel(const float *part, int nw, int hidden, float *gwi, float *gbi,
                                   float *gwo) {
    grad_reduce_block(part, nw, hidden, gwi, gbi, gwo);
}
// M models: blockIdx.y = m sums model m's nw partials -> row m of the stacked gradients
__global__ void grad_reduce_many_kernel(const float *part, int nw, int hidden, float *gwi, float *gbi, float *gwo) {
    const size_t m = blockIdx.y;
    grad_reduce_block(part + m * nw * hidden * 5, nw, hidden, gwi + m * hidden * kCtrlIn, gbi + m * hidden,
                      gwo + m * hidden);
}

// the controller records of M stacked controllers (pack_misc_item's fnp part per model): blockIdx.y = m
__global__ void pack_fnp_many_kernel(const float *cwi, const float *cbi, const float *cwo, int CH, float *fnp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int nf = kMS * 4 * kFnpStride;
    if (idx >= nf) return;
    const size_t m = blockIdx.y;
    const int p = idx % kFnpStride, q = (idx / kFnpStride) & 3, k = 4 * (idx / (kFnpStride * 4)) + q;
    float v = 0.0f;
    if (k < CH) {
        if (p < 3) v = cwi[(m * CH + k) * kCtrlIn + p];
        else if (p == 3) v = cbi[m * CH + k];
        else if (p == 4) v = cwo[m * CH + k];
    }
    fnp[m * nf + idx] = v;
}

// the LSTM weight packs as launches of their own (pack_all_kernel, fcr_rollout.hip, runs the same items as jobs)
__global__ void pack_fwd16_kernel(PackArgs a, int l, _Float16 *dst) {
    pack_fwd16_item(a, l, dst, blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void pack_img_kernel(PackArgs a, int l, _Float16 *dst) {
    pack_img_item(a, l, dst, blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace fcr
