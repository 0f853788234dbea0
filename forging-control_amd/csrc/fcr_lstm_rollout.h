// fcr_lstm_rollout.h — command-driven free run of the LSTM surrogate, all T steps in one launch: the results_LSTM
// track of NeuralNetwork.loop (Functions.py:1196-1231). Beside the press the harness steps the surrogate on its own
// predictions and the controller's command: per step the 10-row window drops its oldest row and gains
// [input.transform(output.inverse_transform(x̂_{t-1})), u_t] (:1198-1207), and x̂_t = LSTM(window_t) + noise
// (simulator_make_step, :969-1011; the fed-back value includes the noise, :1004). For MaxAbs scalers the two
// transforms between steps are one gain per column, out_scale / in_scale.
//
// Built from the fused H <= 52 forward's parts (fcr_fwd.h): fwd16_cell with its split-f16 MFMA products, the
// LDS-resident fragments (layer 0 resident, layers 1 | 2 refilled per phase), the register window ring, the readout,
// 16 trajectories per wave, kFwdWaves waves per workgroup. No controller, no cost, nothing kept for a backward.
// Layer 2 reads layer 1's h sequence back from a per-wave slab of ONE window that every step reuses (a wave reads
// step t's records to the last before it writes step t+1's, in program order), so the workspace does not grow with T.
#pragma once
#include "fcr_common.h"
#include "fcr_f16.h"
#include "fcr_fwd.h"
#include "fcr_pack.h"

namespace fcr {

struct LroArgs {
    int B, T;
    const float *window0, *cmd, *noise;
    float g0, g1, g2, g3;   // gain of the fed-back prediction per output column
    float *xhat;
    f32x4 *hseq;            // [wave][t][record]: layer 1's h of the current window
    Packed p;
};

template <int HS>
struct LroGeo {
    using G = Geo16<HS>;
    static constexpr int LDS = (G::FA1 + G::FA0 + G::FCP + 4) * 4;   // bytes: [layer 1|2 | layer 0 | fc.W | fc.b]
    static_assert(LDS <= 163840, "fragments exceed the 160 KiB LDS");
};

template <int HS>
__global__ __launch_bounds__(kFwdWaves * kWave, kFwdWaves / 4) void fcr_lstm_rollout_kernel(LroArgs a) {
    using G = Geo16<HS>;
    extern __shared__ __attribute__((aligned(16))) float lw[];
    float *lw0 = lw + G::FA1;      // resident layer-0 fragments
    float *lfcp = lw0 + G::FA0;    // resident fc.weight (lane layout) and fc.bias
    float *lfcb = lfcp + G::FCP;
    lds_copy(lw0, a.p.fa[0], G::FA0);
    lds_copy(lfcp, a.p.fcp, G::FCP);
    lds_copy(lfcb, a.p.fcb, 4);
    const int lane = threadIdx.x & 63;
    const int q = lane >> 4, sl = lane & 15;
    const int wave = blockIdx.x * kFwdWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = wave * kTile + sl;
    const bool valid = b < a.B;
    const int bc = valid ? b : a.B - 1;   // out-of-range lanes recompute the last trajectory
    const int T = a.T;

    const float *st = a.window0 + (size_t)bc * kL * kIn;
    const float *cmd = a.cmd + (size_t)bc * T;
    float w0[kL], w1[kL];                                             // window ring, B-operand layout
    const float scq = a.p.wsc[q], sc4 = a.p.wsc[4];   // range guard (fcr_pack.h): the ring holds v 2^-s_c
    const float gsc = sel4(q, a.g0, a.g1, a.g2, a.g3);
#pragma unroll
    for (int t = 0; t < kL; ++t) {
        w0[t] = st[t * kIn + q] * scq;
        w1[t] = (q == 0) ? st[t * kIn + 4] * sc4 : 0.0f;
    }
    float cn = cmd[0];                                                // the command of the step about to run
    float xh0 = 0.0f, xh1 = 0.0f, xh2 = 0.0f, xh3 = 0.0f;

    float c[HS], hout[HS], hp[HS], xc[HS], xn[HS];   // hp, xc, xn: split records (fcr_f16.h)
    const size_t qcell = (size_t)Geo<HS>::QC;        // one cell of the slab, in 16-B units
    const __amdgpu_buffer_rsrc_t rh = wave_rsrc(a.hseq + (size_t)wave * kL * qcell, (size_t)kL * qcell * 16);
#define LRO_O(t) ((uint32_t)((t) * qcell * 16))
    Pace turn;
    turn.turn = (threadIdx.x >> 8) & 1;   // waves w and w+4 share a SIMD: start out of phase
    for (int j = 0; j < T; ++j) {
        const float *lfcp_j = opaque(lfcp), *lfcb_j = opaque(lfcb);
        if (j > 0) {                                                   // Functions.py:1198-1207
#pragma unroll
            for (int k = 0; k < kL - 1; ++k) {
                w0[k] = w0[k + 1];
                w1[k] = w1[k + 1];
            }
            w0[kL - 1] = sel4(q, xh0, xh1, xh2, xh3) * gsc * scq;
        }
        w1[kL - 1] = (q == 0) ? cn * sc4 : 0.0f;                       // step 0: cmd[:,0] replaces the last row's command
        if (j + 1 < T) cn = cmd[j + 1];                                // next command in flight during the step

        // ---- layers 0 and 1 together, time-major: layer 1's input h_t leaves layer 0's cell already split in
        // registers; layer 1's fragments sit beside the resident layer 0 for the phase, layer 2's replace them ----
        {
            lds_fill<G::FA1 * 4, kFwdWaves>(lw, a.p.fa[1]);   // its first barrier also publishes the resident blocks
            float c1[HS], h1[HS];   // layer 1's c and the split record of its h
            {
                const float x0 = w0[0], x1 = w1[0];
                rot_left(w0);
                rot_left(w1);
                fwd16_cell<HS, true, true, false>(lw0, lane, x0, x1, hp, hp, c, hout, turn);
                split_rec<HS>(hout, hp);
                fwd16_cell<HS, false, true, false>(lw, lane, 0.0f, 0.0f, hp, h1, c1, hout, turn);
                split_rec<HS>(hout, h1);
                buf_store_rec<HS>(rh, LRO_O(0), h1, lane);
            }
            for (int t = 1; t < kL; ++t) {
                const float x0 = w0[0], x1 = w1[0];
                rot_left(w0);
                rot_left(w1);
                fwd16_cell<HS, true, false, false>(lw0, lane, x0, x1, hp, hp, c, hout, turn);
                split_rec<HS>(hout, hp);
                fwd16_cell<HS, false, false, false>(lw, lane, 0.0f, 0.0f, hp, h1, c1, hout, turn);
                split_rec<HS>(hout, h1);
                buf_store_rec<HS>(rh, LRO_O(t), h1, lane);
            }
        }
        // ---- layer 2: its input sequence (layer 1's h) streamed back from the slab, one cell ahead ----
        {
            lds_fill<G::FA1 * 4, kFwdWaves>(lw, a.p.fa[2]);
            buf_load_quads<HS>(xc, rh, LRO_O(0), lane);
            buf_load_quads<HS>(xn, rh, LRO_O(1), lane);
            fwd16_cell<HS, false, true, false>(lw, lane, 0.0f, 0.0f, xc, hp, c, hout, turn);
            split_rec<HS>(hout, hp);
#pragma unroll
            for (int r = 0; r < HS; ++r) xc[r] = xn[r];
#pragma unroll 3
            for (int t = 1; t < kL; ++t) {
                buf_load_quads<HS>(xn, rh, LRO_O(t + 1 < kL ? t + 1 : t), lane);
                fwd16_cell<HS, false, false, false>(lw, lane, 0.0f, 0.0f, xc, hp, c, hout, turn);
                if (t + 1 < kL) split_rec<HS>(hout, hp);   // h_9 of layer 2 only feeds the readout (fp32 hout)
#pragma unroll
                for (int r = 0; r < HS; ++r) xc[r] = xn[r];
            }
        }
        // ---- readout fc(h_9 of layer 2) (Functions.py:377) ----
        float xo[kOut];
#pragma unroll
        for (int o = 0; o < kOut; ++o) {
            float p = 0.0f;
#pragma unroll
            for (int r = 0; r < HS; ++r) p += lfcp_j[(o * HS + r) * 4 + q] * hout[r];
            xo[o] = xor_sum_q(p) + lfcb_j[o];
        }
        if (a.noise) {                                                 // Functions.py:1004
            const float *nz = a.noise + ((size_t)bc * T + j) * kOut;
#pragma unroll
            for (int o = 0; o < kOut; ++o) xo[o] += nz[o];
        }
        xh0 = xo[0];
        xh1 = xo[1];
        xh2 = xo[2];
        xh3 = xo[3];
        if (valid) a.xhat[((size_t)b * T + j) * kOut + q] = sel4(q, xh0, xh1, xh2, xh3);
    }
#undef LRO_O
}

// ---------------------------------------------------------------------------------------------
// Range guard (fcr_pack.h) for this rollout. Column c of the window can hold: a value of window0; for c = 4 a
// command; for c < 4 a generated row gain_c x̂_c with |x̂_c| <= sum_k |fc.W[c,k]| + |fc.b[c]| + max |noise_c|
// (|h| < 1). The command column is not bounded by a Hardtanh here, and the noise is scaled by the gain, so the bound
// m_c is formed from the maxima kept apart: partials [block][16] = (window0 / cmd columns 0..4 | noise columns 8..11).
//
// As in the rollout, m_c < 2^14 leaves the column alone (s_c = 0: bit-identical to an unguarded run). Above it the
// column runs on v 2^-s against W_ih0[:, c] 2^s, and here s balances the two operands instead of taking the least
// shift: a harness whose input scaler turns large raw values into O(1) products has W_ih0[:, c] ~ 1/m_c, and such a
// weight times the least 2^s stays far below 2^-3, where the lo half of its f16 split is subnormal (absolute error
// 2^-25, times v 2^-s up to 2^14: 1e-4 of a gate pre-activation, measured). With e_v, e_w the binary exponents of m_c
// and of max |W_ih0[:, c]|, s = (e_v - e_w) / 2 puts both at the same exponent, clamped to e_v - 14 <= s <= 13 - e_w
// (v 2^-s < 2^14; the packed weight, times up to 2 log2(e), < 2^15); where the two bounds cross (|v W| ~ 2^27 and
// beyond, not covered by the rollout's guard either) the value's bound wins.
constexpr int kLroPart = 16;

struct LroRangeArgs {
    float g0, g1, g2, g3;
    const float *fcw, *fcb, *wih0;
    int H;
    float *wsc;
};

__device__ __forceinline__ void lro_range_final_wave(const float *__restrict__ part, int nblk, const LroRangeArgs &r,
                                                     int lane) {
    float mw[kIn], mn[kOut];
#pragma unroll
    for (int c = 0; c < kIn + kOut; ++c) {
        float m = 0.0f;
        for (int i = lane; i < nblk; i += 64) m = fmaxf(m, part[i * kLroPart + (c < kIn ? c : 8 + c - kIn)]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (c < kIn) mw[c] = m;
        else mn[c - kIn] = m;
    }
    if (lane >= 8) return;
    float sc = 1.0f;
    if (lane < kIn) {
        float m = mw[0], n = mn[0];
#pragma unroll
        for (int c = 1; c < kIn; ++c)
            if (lane == c) m = mw[c];
#pragma unroll
        for (int c = 1; c < kOut; ++c)
            if (lane == c) n = mn[c];
        if (lane < kOut) {
            float s = fabsf(r.fcb[lane]);
            const float *w = r.fcw + lane * r.H;
            for (int k = 0; k < r.H; ++k) s += fabsf(w[k]);
            m = fmaxf(m, fabsf(sel4(lane, r.g0, r.g1, r.g2, r.g3)) * (s + n));
        }
        if (isfinite(m) && m >= 16384.0f) {
            float wmax = 0.0f;
            for (int k = 0; k < 4 * r.H; ++k) wmax = fmaxf(wmax, fabsf(r.wih0[k * kIn + lane]));
            const int ev = __builtin_amdgcn_frexp_expf(m);
            int s = ev - 14;
            if (isfinite(wmax) && wmax > 0.0f) {
                const int ew = __builtin_amdgcn_frexp_expf(wmax);
                s = (ev - ew) / 2;
                if (s > 13 - ew) s = 13 - ew;
                if (s < ev - 14) s = ev - 14;
            }
            sc = __builtin_amdgcn_ldexpf(1.0f, -s);
        }
    }
    r.wsc[lane] = sc;
}

__global__ __launch_bounds__(64) void lro_range_final_kernel(const float *__restrict__ part, int nblk, LroRangeArgs r) {
    lro_range_final_wave(part, nblk, r, threadIdx.x);
}

// final != 0: launched as one block, the final step too (one launch fewer at small batches)
__global__ __launch_bounds__(kRangeThreads) void lro_range_partial_kernel(const float *__restrict__ window0,
                                                                          const float *__restrict__ cmd,
                                                                          const float *__restrict__ noise, int B, int T,
                                                                          float *part, int final, LroRangeArgs r) {
    __shared__ float red[kIn + kOut][kRangeThreads];
    float m[kIn + kOut] = {};
    const size_t stride = (size_t)gridDim.x * blockDim.x, tid0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = tid0; i < (size_t)B * kL; i += stride) {
        const float *p = window0 + i * kIn;
#pragma unroll
        for (int c = 0; c < kIn; ++c) m[c] = fmaxf(m[c], fabsf(p[c]));
    }
    for (size_t i = tid0; i < (size_t)B * T; i += stride) m[4] = fmaxf(m[4], fabsf(cmd[i]));
    if (noise)
        for (size_t i = tid0; i < (size_t)B * T; i += stride) {
            const float *p = noise + i * kOut;
#pragma unroll
            for (int c = 0; c < kOut; ++c) m[kIn + c] = fmaxf(m[kIn + c], fabsf(p[c]));
        }
#pragma unroll
    for (int c = 0; c < kIn + kOut; ++c) red[c][threadIdx.x] = m[c];
    __syncthreads();
    for (int w = kRangeThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < kIn + kOut; ++c) red[c][threadIdx.x] = fmaxf(red[c][threadIdx.x], red[c][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x < kIn + kOut)
        part[blockIdx.x * kLroPart + (threadIdx.x < kIn ? threadIdx.x : 8 + threadIdx.x - kIn)] = red[threadIdx.x][0];
    if (final) {
        __syncthreads();
        if (threadIdx.x < 64) lro_range_final_wave(part, 1, r, threadIdx.x);
    }
}

}  // namespace fcr
