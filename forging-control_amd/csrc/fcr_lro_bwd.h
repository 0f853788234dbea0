// fcr_lro_bwd.h — backward of the surrogate's command-driven free run (fcr_lstm_rollout.h), H <= 52: the gradient of
// every LSTM weight, the readout, window0 and the commands, given G = dL/dx̂ (B, T, 4).
//
// The free run's T windows per trajectory are a VIRTUAL BATCH of T·Bp windows (Bp = B rounded up to whole waves of 16),
// step-major: window (t, b) is virtual window t·Bp + b, wave wb of step t is virtual wave t·nwb + wb.
//   lro_windows_kernel  writes that batch from window0, cmd, x̂ and the gain (W_t row j is the row generated at step
//                       s = t - 10 + j, (gain ⊙ x̂_s, cmd[s+1]), or window0's row j + t with cmd[0] in [9, 4]); padding
//                       trajectories repeat the last one.
//   sur_fwd_kernel      (fcr_sur.h, untouched) recomputes the batch with every cell's h, c, the guarded rows and h_9.
//   lro_bwd_kernel      one wave per 16 trajectories loops t = T-1 .. 0 over its own slabs of the virtual batch: per step
//                       sur_bwd_kernel's window backward (the same bwd_cell instantiations with DgOut, the same image
//                       refills) from ȳ_t = G_t + gain ⊙ P_t[0:4], with layer 0's row gradients folded into the rows P
//                       instead of a g_x. The dgate blocks and scales of every cell go into slab t, ȳ into (T·Bp, 4).
// The weight gradients are then ONE sur_wgrad / sur_part_sum / sur_wgrad_finish pass per layer over all T·Bp·10 rows
// and the readout's sur_fc_* pair over ȳ and h_9 (fcr_sur.h, untouched).
//
// The rows P: per wave [T + 10][64 lanes] (column q, column 4 in lane group 0), in the workspace; row r holds the
// accumulated gradient of original row r of window0 (r < 10) or of the row generated at step r - 10. Row j of W_t is row
// t + j; window t is the first (in this reverse order) to reach it iff t = T-1 or j = 0, so no row needs clearing, and
// row t + 10 is complete when step t starts. A lane only ever re-reads what it wrote itself.
#pragma once
#include "fcr_sur.h"

namespace fcr {

struct LroBwdArgs {
    SurArgs s;            // the virtual batch's slabs and packs (s.B = T·Bp)
    int B, T, nwb;        // trajectories, steps, waves per step
    const float *window0, *cmd, *xhat, *g_xhat;
    float g0, g1, g2, g3;
    float *xwin;          // (T·Bp, 10, 5): the virtual batch
    float *ybar;          // (T·Bp, 4): ȳ (0 for padding trajectories)
    f32x2 *rows;          // [nwb][T + 10][64]: P
    float *g_window0;     // (B, 10, 5) or null
    float *g_cmd;         // (B, T) or null
    int zw0, zw1;         // padding waves [zw0, zw1) of the dgate slab the weight-gradient product reads: zeroed
    size_t dg_bytes, dsc_floats;   // per wave (SurGeo<HS>::DG, ::DSC)
};

constexpr int kLroWinBlock = 256;
__global__ __launch_bounds__(kLroWinBlock) void lro_windows_kernel(LroBwdArgs a) {
    const int Bp = a.nwb * kTile;
    const size_t n = (size_t)a.T * Bp * kL, tid = (size_t)blockIdx.x * kLroWinBlock + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kLroWinBlock;
    if (tid < n) {
        const int j = (int)(tid % kL);
        const size_t vb = tid / kL;
        const int t = (int)(vb / Bp), bb = (int)(vb % Bp);
        const int b = bb < a.B ? bb : a.B - 1;
        const int s = t - kL + j;
        float v[kIn];
        if (s >= 0) {
            const float *xh = a.xhat + ((size_t)b * a.T + s) * kOut;
            v[0] = xh[0] * a.g0;
            v[1] = xh[1] * a.g1;
            v[2] = xh[2] * a.g2;
            v[3] = xh[3] * a.g3;
        } else {
            const float *w = a.window0 + ((size_t)b * kL + (j + t)) * kIn;
#pragma unroll
            for (int c = 0; c < kOut; ++c) v[c] = w[c];
            v[4] = w[4];
        }
        if (s >= -1) v[4] = a.cmd[(size_t)b * a.T + s + 1];
        float *o = a.xwin + tid * kIn;
#pragma unroll
        for (int c = 0; c < kIn; ++c) o[c] = v[c];
    }
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 *dg = reinterpret_cast<f32x4 *>(a.s.dgs + (size_t)a.zw0 * a.dg_bytes);
    for (size_t e = tid; e < (size_t)(a.zw1 - a.zw0) * (a.dg_bytes / 16); e += stride) dg[e] = z;
    float *ds = a.s.dsc + (size_t)a.zw0 * a.dsc_floats;
    for (size_t e = tid; e < (size_t)(a.zw1 - a.zw0) * a.dsc_floats; e += stride) ds[e] = 0.0f;
}

// sur_bwd_kernel's body (fcr_sur.h) per step. A wave past the last one of a step (the workgroup's padding) runs on
// zero-sized descriptors: its loads return 0, its stores are dropped, it only keeps the barriers and its share of the
// image refills.
// (HS = 4 is held to the 4 waves per SIMD sur_bwd_kernel<4>'s allocation comes out at, i.e. two workgroups per CU. At
// HS = 8 the same bound — 3, against the 173 registers the loop takes — costs 32 B of scratch and buys nothing: a
// workgroup is 2 waves per SIMD and a second one needs 4, so 154 or 173 registers both run one workgroup per CU.)
template <int HS>
__global__ __launch_bounds__(kBwdWaves * kWave, HS <= 4 ? 4 : kBwdWaves / 4) void lro_bwd_kernel(LroBwdArgs A) {
    using LD = BwdLds<HS, false>;
    using I1 = Img<HS, false>;
    using I0 = Img<HS, true>;
    using SG = SurGeo<HS>;
    const SurArgs &a = A.s;
    extern __shared__ __attribute__((aligned(16))) float lw[];
    float *lfcp = lw + LD::REGION / 4;
    lds_copy(lfcp, a.p.fcp, Geo16<HS>::FCP);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int q = lane >> 4, sl = lane & 15;
    const int wb = blockIdx.x * kBwdWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = wb < A.nwb;
    const int b = wb * kTile + sl;
    const bool valid = b < A.B;
    const int T = A.T;
    const float scq = a.p.wsc[q], sc4 = a.p.wsc[4];   // d/dx = 2^-s_c d/dx' (fcr_pack.h)
    const float gsc = sel4(q, A.g0, A.g1, A.g2, A.g3);
    const ImgLane<I1::U> L1 = img_lane<I1::U>(lds_offset(lw), lane);
    const ImgLane<I0::U> L0 = img_lane<I0::U>(lds_offset(lw), lane);
    const size_t prow = (size_t)(T + kL) * kWave;   // P rows of a wave, in 8-B units
    const __amdgpu_buffer_rsrc_t rp = wave_rsrc(A.rows + (size_t)(live ? wb : 0) * prow, live ? prow * 8 : 0);
    constexpr size_t qcell = (size_t)Geo<HS>::QC;
    Stamps sp = {{0, 0, 0, 0, (unsigned long long)((threadIdx.x >> 8) & 1), 0, 0, 0}};
    for (int t = T - 1; t >= 0; --t) {
        const size_t vw = live ? (size_t)t * A.nwb + wb : 0;   // this wave's slabs of step t
        const bool lastwin = t == T - 1;
        // ȳ_t = G_t + gain ⊙ P_t[0:4]; g_cmd[t+1] = P_t[4] (complete: every later window is done)
        float yq = valid ? A.g_xhat[((size_t)b * T + t) * kOut + q] : 0.0f;
        if (!lastwin) {
            const f32x2 pv = buf_ld2(rp, lane * 8, (uint32_t)((t + kL) * kWave * 8));
            yq += gsc * pv[0];
            if (A.g_cmd && valid && q == 0) A.g_cmd[(size_t)b * T + t + 1] = pv[1];
        }
        if (!valid) yq = 0.0f;   // padding trajectories carry no gradient
        if (live) A.ybar[(vw * kTile + sl) * kOut + q] = yq;
        float dyo[kOut];
#pragma unroll
        for (int o = 0; o < kOut; ++o) dyo[o] = __shfl(yq, o * 16 + sl);
        // dh_9 = fc.W^T ȳ_t
        const float *lfcp_t = opaque(lfcp);
        float dh_out[HS];
#pragma unroll
        for (int r = 0; r < HS; ++r) {
            const float *fp = lfcp_t + r * 4 + q;
            dh_out[r] = fp[0] * dyo[0] + fp[HS * 4] * dyo[1] + fp[2 * HS * 4] * dyo[2] + fp[3 * HS * 4] * dyo[3];
        }
        float dh[HS], dc[HS], dxo[HS], dab[HS];
        NextIn nb;
        nb.rh = wave_rsrc(a.hseq + vw * SG::SEQ, live ? SG::SEQ * 16 : 0);
        nb.rc = wave_rsrc(a.cseq + vw * SG::SEQ, live ? SG::SEQ * 16 : 0);
        nb.rx = wave_rsrc(a.xw + vw * kL * kWave, live ? (size_t)kL * kWave * 8 : 0);
        nb.rd = wave_rsrc(a.dseq + vw * SG::DSEQ, live ? SG::DSEQ * 16 : 0);
        auto hoff = [&](int l, int tt) { return (uint32_t)(((size_t)l * kL + tt) * qcell * 16); };
        auto doff = [&](int lfrom, int tt) { return ((size_t)(2 - lfrom) * kL + tt) * qcell; };
        auto next_of = [&](int l, int tt) {   // the cell processed after (l, tt)
            NextIn n = nb;
            int nl = l, nt = tt - 1;
            if (tt == 0) {
                nt = kL - 1;
                nl = l - 1;
            }
            if (nl < 0) { nl = 2; nt = kL - 1; }   // past the last cell: reload a valid one (harmless)
            n.x = nl == 0 ? (uint32_t)(nt * kWave * 8) : hoff(nl > 0 ? nl - 1 : 0, nt);
            n.h = hoff(nl, nt > 0 ? nt - 1 : 0);
            n.c = n.h;
            n.o = hoff(nl, nt);
            n.d = (uint32_t)((nl < 2 ? doff(nl + 1, nt) : 0) * 16);
            return n;
        };
        DgOut dg;
        dg.r = wave_rsrc(a.dgs + vw * SG::DG, live ? SG::DG : 0);
        dg.rs = wave_rsrc(a.dsc + vw * SG::DSC, live ? SG::DSC * 4 : 0);
        auto dg_at = [&](int l, int tt) {
            DgOut d = dg;
            d.off = (uint32_t)(((size_t)l * kL + tt) * SG::KBB * 2048);
            d.soff = (uint32_t)((l * kL + tt) * 64);
            return d;
        };
        CellIn<HS> ci;
        {
            const NextIn f = next_of(2, kL);   // tt = kL -> (2, 9)
            load_xhd<HS, false, true, false>(ci, f, lane);
            ld_quads<HS>(ci.c, f.rc, f.c, lane);
        }
        float unused0, unused1;
        // ---- layer 2 ----
        lds_fill<I1::BYTES, kBwdWaves>(lw, a.p.img[2]);
#pragma unroll
        for (int r = 0; r < HS; ++r) dh[r] = dc[r] = dab[r] = 0.0f;
        {
            const DgOut d = dg_at(2, kL - 1);
            bwd_cell<HS, false, false, false, false, true, false, false, false, true, true>(
                L1.fb, L1.tb, lane, dh_out, dh, dc, dxo, unused0, unused1, ci, next_of(2, kL - 1), sp, &d);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(2, kL - 1)) * 16), dxo, lane);
        }
        for (int tt = kL - 2; tt >= 2; --tt) {
            const DgOut d = dg_at(2, tt);
            bwd_cell<HS, false, false, false, false, true, false, false, true, true, true>(
                L1.fb, L1.tb, lane, dab, dh, dc, dxo, unused0, unused1, ci, next_of(2, tt), sp, &d);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(2, tt)) * 16), dxo, lane);
        }
        {
            const DgOut d1 = dg_at(2, 1);
            bwd_cell<HS, false, false, false, false, false, false, false, true, true, true>(
                L1.fb, L1.tb, lane, dab, dh, dc, dxo, unused0, unused1, ci, next_of(2, 1), sp, &d1);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(2, 1)) * 16), dxo, lane);
            const DgOut d0 = dg_at(2, 0);
            bwd_cell<HS, false, false, true, false, true, true, false, true, true, true>(
                L1.fb, L1.tb, lane, dab, dh, dc, dxo, unused0, unused1, ci, next_of(2, 0), sp, &d0);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(2, 0)) * 16), dxo, lane);
        }
        // ---- layer 1 ----
        lds_fill<I1::BYTES, kBwdWaves>(lw, a.p.img[1]);
#pragma unroll
        for (int r = 0; r < HS; ++r) dh[r] = dc[r] = 0.0f;
        for (int tt = kL - 1; tt >= 2; --tt) {
            const DgOut d = dg_at(1, tt);
            bwd_cell<HS, false, true, false, false, true, true, false, true, true, true>(
                L1.fb, L1.tb, lane, dab, dh, dc, dxo, unused0, unused1, ci, next_of(1, tt), sp, &d);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(1, tt)) * 16), dxo, lane);
        }
        {
            const DgOut d1 = dg_at(1, 1);
            bwd_cell<HS, false, true, false, false, false, true, false, true, true, true>(
                L1.fb, L1.tb, lane, dab, dh, dc, dxo, unused0, unused1, ci, next_of(1, 1), sp, &d1);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(1, 1)) * 16), dxo, lane);
            const DgOut d0 = dg_at(1, 0);
            bwd_cell<HS, false, true, true, true, true, true, false, true, true, true>(
                L1.fb, L1.tb, lane, dab, dh, dc, dxo, unused0, unused1, ci, next_of(1, 0), sp, &d0);
            buf_store_quads<HS>(nb.rd, (uint32_t)((doff(1, 0)) * 16), dxo, lane);
        }
        // ---- layer 0: the window-row gradients go into the rows P ----
        lds_fill<I0::BYTES, kBwdWaves>(lw, a.p.img[0]);
#pragma unroll
        for (int r = 0; r < HS; ++r) dh[r] = dc[r] = 0.0f;
        auto put_p = [&](int j, float dxq, float dx4) {   // row j of W_t is row t + j
            const uint32_t off = (uint32_t)((t + j) * kWave * 8);
            f32x2 v = {dxq * scq, q == 0 ? dx4 * sc4 : 0.0f};
            if (!(lastwin || j == 0)) v += buf_ld2(rp, lane * 8, off);
            buf_st2(rp, lane * 8, off, v);
        };
        for (int tt = kL - 1; tt >= 2; --tt) {
            float dxq, dx4;
            const DgOut d = dg_at(0, tt);
            bwd_cell<HS, true, true, false, true, true, true, false, true, true, true>(
                L0.fb, L0.tb, lane, dab, dh, dc, dxo, dxq, dx4, ci, next_of(0, tt), sp, &d);
            put_p(tt, dxq, dx4);
        }
        {
            float dxq, dx4;
            const DgOut d1 = dg_at(0, 1);
            bwd_cell<HS, true, true, false, true, false, true, false, true, true, true>(
                L0.fb, L0.tb, lane, dab, dh, dc, dxo, dxq, dx4, ci, next_of(0, 1), sp, &d1);
            put_p(1, dxq, dx4);
            const DgOut d0 = dg_at(0, 0);
            bwd_cell<HS, true, true, true, false, true, false, false, true, false, true>(
                L0.fb, L0.tb, lane, dab, dh, dc, dxo, dxq, dx4, ci, next_of(0, 0), sp, &d0);
            put_p(0, dxq, dx4);
        }
    }
    // rows 0..9 are window0's; [9, 4] was overwritten by cmd[0], whose gradient its share is
    if (!valid) return;
    float *gw = A.g_window0 ? A.g_window0 + (size_t)b * kL * kIn : nullptr;
    for (int r = 0; r < kL; ++r) {
        const f32x2 pv = buf_ld2(rp, lane * 8, (uint32_t)(r * kWave * 8));
        if (gw) {
            gw[r * kIn + q] = pv[0];
            if (q == 0) gw[r * kIn + 4] = r == kL - 1 ? 0.0f : pv[1];
        }
        if (r == kL - 1 && q == 0 && A.g_cmd) A.g_cmd[(size_t)b * T] = pv[1];
    }
}

}  // namespace fcr
