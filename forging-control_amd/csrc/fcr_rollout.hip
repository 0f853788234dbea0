// fcr_rollout.hip — host side of the H <= 52 engines: the rollout (the fused kernels, the small-batch and the
// layer-pipelined families: fcr_fwd.h, fcr_bwd.h, fcr_small.h, fcr_pipe.h) and the surrogate training step on the same
// cells (fcr_sur.h) and its command-driven free run (fcr_lstm_rollout.h); and the kernels every engine shares
// (fcr_shared_kernels.h, pack_all_kernel) behind the launchers fcr_host.h declares. The C ABI in fcr_abi.hip calls in
// through fcr_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "fcr.h"
#include "fcr_bwd.h"
#include "fcr_common.h"
#include "fcr_fwd.h"
#include "fcr_host.h"
#include "fcr_img.h"
#include "fcr_pack.h"
#include "fcr_pipe.h"
#include "fcr_shared_kernels.h"
#include "fcr_small.h"
#include "fcr_sur.h"
#include "fcr_lstm_rollout.h"   // after the others: built from fcr_fwd.h's parts
#include "fcr_lro_bwd.h"

namespace fcr {
namespace {

struct Layout : PackedLayout {
    int nw, nw_pad;
    size_t xhat, dv, loss_part, fnn_part, hseq, cseq, xw, dseq, dxrow, stamp, total;
    size_t pipe_flags, pipe_rows;   // the layer-pipelined small-batch kernels (fcr_pipe.h), L.nw <= kPipeMaxGroups
    int ctrl_blocks;
};

// the layer-pipelined small-batch kernels (fcr_pipe.h) run at most this many 16-trajectory groups (3 workgroups each)
constexpr int kPipeMaxGroups = 32;

Layout make_layout(const fcr_dims *d, int with_backward) {
    Layout L{};
    L.HS = slot_tier(d->H);
    L.nw = (d->B + kTile - 1) / kTile;
    constexpr int kPad = kFwdWaves > kBwdWaves ? kFwdWaves : kBwdWaves;
    L.nw_pad = (L.nw + kPad - 1) / kPad * kPad;  // covers both launch geometries
    Arena take;
    const int HS = L.HS;
    take_packed(take, L, with_backward != 0);
    L.xhat = take(sizeof(float) * (size_t)d->B * d->N * kOut);
    L.loss_part = take(sizeof(float) * L.nw_pad);
    L.dv = take(sizeof(float) * (size_t)d->B * d->N);
    L.ctrl_blocks = (int)(((long long)d->B * d->N + kCtrlItems - 1) / kCtrlItems);
    L.fnn_part = take(sizeof(float) * (size_t)L.ctrl_blocks * d->ctrl_hidden * 5);
    // sequence slabs (fcr_common.h): h of every cell always (layers 0, 1 are the next phase's input);
    // c, the window rows and the backward's dx / window-row-gradient slabs only with a backward
    const size_t qcells = (size_t)L.nw_pad * d->N * kLayers * kL * HS * 16;   // Geo<HS>::QC per cell
    L.hseq = take(sizeof(f32x4) * qcells);
    if (with_backward) {
        L.cseq = take(sizeof(f32x4) * qcells);
        L.xw = take(sizeof(f32x2) * (size_t)L.nw_pad * d->N * kL * kWave);
        L.dseq = take(sizeof(f32x4) * (size_t)L.nw_pad * d->N * 2 * kL * HS * 16);
        // the small-batch backward keeps one copy per wave of its group (fcr_small.h)
        const size_t rows_waves = L.nw_pad > 4 * L.nw ? L.nw_pad : 4 * L.nw;
        L.dxrow = take(sizeof(f32x2) * rows_waves * d->N * kL * kWave);
    }
#if FCR_STAMP
    L.stamp = take(sizeof(unsigned long long) * L.nw_pad * 16);   // [backward 8 | forward 8] per wave
#endif
    if (L.nw <= kPipeMaxGroups) {
        L.pipe_flags = take(sizeof(unsigned) * (size_t)L.nw * kPipeFlags);
        L.pipe_rows = take(sizeof(float) * (size_t)L.nw * d->N * kTile * kPipeRow);
    }
    L.total = take.off;
    return L;
}

template <int HS, bool STORE, bool LP>
int launch_fwd_t(const FwdArgs &fa, const Layout &L, hipStream_t s) {
    const int lds = LP ? Geo16<HS>::LDS_FWD_LP : Geo16<HS>::LDS_FWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_fwd_kernel<HS, STORE, LP>, lds, attr_done, "fwd")) return rc;
    hipLaunchKernelGGL((fcr_fwd_kernel<HS, STORE, LP>), dim3(L.nw_pad / kFwdWaves), dim3(kFwdWaves * kWave),
                       lds, s, fa);
    return launch_check("fcr_fwd_kernel");
}

template <int HS>
int launch_fwd(const FwdArgs &fa, const Layout &L, bool lp, hipStream_t s) {
    if (lp) return fa.cseq ? launch_fwd_t<HS, true, true>(fa, L, s) : launch_fwd_t<HS, false, true>(fa, L, s);
    return fa.cseq ? launch_fwd_t<HS, true, false>(fa, L, s) : launch_fwd_t<HS, false, false>(fa, L, s);
}

template <int HS, bool LP>
int launch_bwd_t(const BwdArgs &ba, const Layout &L, hipStream_t s) {
    const int lds = BwdLds<HS, LP>::BYTES;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_bwd_kernel<HS, LP>, lds, attr_done, "bwd")) return rc;
    hipLaunchKernelGGL((fcr_bwd_kernel<HS, LP>), dim3(L.nw_pad / kBwdWaves), dim3(kBwdWaves * kWave), lds, s, ba);
    return launch_check("fcr_bwd_kernel");
}

template <int HS>
int launch_bwd(const BwdArgs &ba, const Layout &L, bool lp, hipStream_t s) {
    return lp ? launch_bwd_t<HS, true>(ba, L, s) : launch_bwd_t<HS, false>(ba, L, s);
}

// Small-batch kernels (fcr_small.h): one workgroup of ceil(HS/4) waves per 16-trajectory group.
// Used for the fp32-accurate mode at HS = 8, 13 when B <= the call's small-batch limit (fcr_options; the
// process-wide default g_small_max_batch when it inherits): below one wave per SIMD the fused kernels run at one
// wave's sequential latency. A change between a forward and its backward is harmless: every family keeps one
// workspace layout and one record contract (tests/test_gpu_record_contract.py):
//   - a forward with with_backward = 1 guarantees, in window j with t_lo = max(0, 9 - j), the window rows xw of every
//     t, the h records of layers 0 and 2 and the c records of every layer at t >= t_lo - 1 (never c_9, never layer
//     2's h_9), and h1 at t >= t_lo - 1 (the fused fp32 forward writes h1 at every t for its own layer-2 phase; the
//     small-batch and pipelined forwards write every record). What lies before stays a hole of the slab;
//   - every backward family reads only those: the fused backward runs only the cells t >= t_lo (fcr_bwd.h), which
//     read x_t, h_{t-1}, c_{t-1} and their own h_t; the small-batch and pipelined backwards run every cell and clamp
//     the records of the unreached ones to the written set (SbCtx::next_of, fcr_small.h).
int small_limit_of(const fcr_options *o) {
    return (o && o->small_batch_limit >= 0) ? o->small_batch_limit : g_small_max_batch.load(std::memory_order_relaxed);
}
bool use_small(const fcr_dims *d, const Layout &L, const fcr_options *o) {
    return d->precision == FCR_PRECISION_FP32 && (L.HS == 8 || L.HS == 13) && d->B <= small_limit_of(o);
}
// The small-batch family's layer-pipelined geometry (fcr_pipe.h: three workgroups per group that wait on each other)
// for B <= g_pipe_max_batch (default 512; 0 = never): only where every workgroup of the launch is resident at once —
// 3 per group, one per CU by LDS, within half the device's CUs (the other half for whatever else runs).
int device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
bool use_pipe(const fcr_dims *d, const Layout &L, const fcr_options *o) {
    return use_small(d, L, o) && d->B <= g_pipe_max_batch.load(std::memory_order_relaxed) && L.nw <= kPipeMaxGroups &&
           6 * L.nw <= device_cus();
}
// window sets per group (fcr_pipe.h): up to `most` (forward 4, backward 3), as many as fit `per` S workgroups per group
// within half the CUs and S <= N; g_pipe_sets > 0 caps it (tests: every S gives the same bits)
int pipe_sets(const fcr_dims *d, const Layout &L, int most, int per) {
    const int fixed = g_pipe_sets.load(std::memory_order_relaxed);
    int S = fixed > 0 && fixed < most ? fixed : most;
    const int cus = device_cus();
    while (S > 1 && (2 * per * S * L.nw > cus || S > d->N)) --S;
    return S;
}
PipeArgs pipe_args(const Layout &L, char *base) {
    PipeArgs p;
    p.flags = (unsigned *)(base + L.pipe_flags);
    p.rows = (float *)(base + L.pipe_rows);
    p.groups = L.nw;
    p.loss = nullptr;
    return p;
}
// grid: 2 S (forward) / 3 S (backward) workgroups per group, the ids of a group one residue mod 8 apart (pipe_role)
template <int HS, bool STORE, int S>
int launch_pfwd_t(const FwdArgs &fa, const PipeArgs &pa, const Layout &L, hipStream_t s) {
    constexpr int lds = Pipe<HS>::LDS_FWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_pfwd_kernel<HS, STORE, S>, lds, attr_done, "pfwd")) return rc;
    // (the counters were zeroed by this call's pack_all_kernel)
    hipLaunchKernelGGL((fcr_pfwd_kernel<HS, STORE, S>), dim3(16 * S * ((L.nw + 7) / 8)), dim3(Small<HS>::NQ * kWave), lds,
                       s, fa, pa);
    return launch_check("fcr_pfwd_kernel");
}
template <int HS, bool STORE>
int launch_pfwd_s(const FwdArgs &fa, const PipeArgs &pa, const Layout &L, int S, hipStream_t s) {
    if (S == 4) return launch_pfwd_t<HS, STORE, 4>(fa, pa, L, s);
    if (S == 3) return launch_pfwd_t<HS, STORE, 3>(fa, pa, L, s);
    if (S == 2) return launch_pfwd_t<HS, STORE, 2>(fa, pa, L, s);
    return launch_pfwd_t<HS, STORE, 1>(fa, pa, L, s);
}
template <int HS, int S>
int launch_pbwd_t(const BwdArgs &ba, const PipeArgs &pa, const Layout &L, hipStream_t s) {
    constexpr int lds = Pipe<HS>::LDS_BWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_pbwd_kernel<HS, S>, lds, attr_done, "pbwd")) return rc;
    // (the counters were zeroed by the forward's pack_all_kernel; each backward leaves its own zeroed, fcr_pipe.h)
    hipLaunchKernelGGL((fcr_pbwd_kernel<HS, S>), dim3(24 * S * ((L.nw + 7) / 8)), dim3(Small<HS>::NQ * kWave), lds, s, ba,
                       pa);
    return launch_check("fcr_pbwd_kernel");
}
template <int HS>
int launch_pbwd_s(const BwdArgs &ba, const PipeArgs &pa, const Layout &L, int S, hipStream_t s) {
    if (S == 3) return launch_pbwd_t<HS, 3>(ba, pa, L, s);
    if (S == 2) return launch_pbwd_t<HS, 2>(ba, pa, L, s);
    return launch_pbwd_t<HS, 1>(ba, pa, L, s);
}

template <int HS, bool STORE>
int launch_sfwd_t(const FwdArgs &fa, const Layout &L, hipStream_t s) {
    constexpr int lds = Small<HS>::LDS_FWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_sfwd_kernel<HS, STORE>, lds, attr_done, "sfwd")) return rc;
    hipLaunchKernelGGL((fcr_sfwd_kernel<HS, STORE>), dim3(L.nw), dim3(Small<HS>::NQ * kWave), lds, s, fa);
    return launch_check("fcr_sfwd_kernel");
}

template <int HS>
int launch_sbwd_t(const BwdArgs &ba, const Layout &L, hipStream_t s) {
    constexpr int lds = Small<HS>::LDS_BWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_sbwd_kernel<HS>, lds, attr_done, "sbwd")) return rc;
    hipLaunchKernelGGL((fcr_sbwd_kernel<HS>), dim3(L.nw), dim3(Small<HS>::NQ * kWave), lds, s, ba);
    return launch_check("fcr_sbwd_kernel");
}

// The per-call weight packs (pack_fwd16_item, pack_img_item, pack_misc_item) as jobs of one launch:
// block ranges in job order, 256 threads each, the same items the separate kernels ran
enum { kPackFwd16 = 0, kPackImg = 1, kPackMisc = 2 };
struct PackJob {
    int kind, l, blocks;
    _Float16 *dst;
};
struct PackAllArgs {
    PackArgs a;
    int njobs;
    PackJob job[2 * kLayers + 1];
    unsigned *clear;   // or null: the pipelined kernels' progress counters, zeroed by block 0 (fcr_pipe.h)
    int nclear;
};
__global__ __launch_bounds__(256) void pack_all_kernel(PackAllArgs p) {
    if (p.clear && blockIdx.x == 0)
        for (int i = (int)threadIdx.x; i < p.nclear; i += 256) p.clear[i] = 0u;
    int b = blockIdx.x, j = 0;
    while (j + 1 < p.njobs && b >= p.job[j].blocks) b -= p.job[j++].blocks;
    const int idx = b * 256 + (int)threadIdx.x;
    const PackJob &jb = p.job[j];
    if (jb.kind == kPackFwd16) pack_fwd16_item(p.a, jb.l, jb.dst, idx);
    else if (jb.kind == kPackImg) pack_img_item(p.a, jb.l, jb.dst, idx);
    else pack_misc_item(p.a, idx);
}
}  // namespace

void take_packed(Arena &take, PackedLayout &P, bool with_backward) {
    const int HS = P.HS;
    for (int l = 0; l < kLayers; ++l) P.fa[l] = take(f16_fwd_bytes(HS, l));
    if (with_backward)
        for (int l = 0; l < kLayers; ++l) P.img[l] = take(img_bytes(HS, l));
    P.fcp = take(sizeof(float) * kOut * HS * 4);
    P.fcb = take(sizeof(float) * kOut);
    P.fnp = take(sizeof(float) * kMS * 4 * kFnpStride);
    P.wsc = take(sizeof(float) * 8);
    P.rng = take(sizeof(float) * 8 * kRangeBlocks);
}

// Every weight pack of the call in ONE launch (seven launches of ~4 us each were a step's overhead at the
// reference's B = 15)
int launch_pack_all(const fcr_weights *w, int H, int CH, const PackedLayout &P, bool with_backward, char *base,
                    unsigned *clear, int nclear, hipStream_t s) {
    PackAllArgs pk{};
    PackArgs &pa = pk.a;
    pa.H = H;
    pa.HS = P.HS;
    pa.CH = CH;
    for (int l = 0; l < kLayers; ++l) {
        pa.wih[l] = w->w_ih[l];
        pa.whh[l] = w->w_hh[l];
    }
    pa.fcw = w->fc_w;
    pa.fcb = w->fc_b;
    if (CH) {
        pa.cwi = w->ctrl_w_inp;
        pa.cbi = w->ctrl_b_inp;
        pa.cwo = w->ctrl_w_out;
    }
    pa.fcp = (float *)(base + P.fcp);
    pa.fcbo = (float *)(base + P.fcb);
    pa.fnp = (float *)(base + P.fnp);
    pa.wsc = (const float *)(base + P.wsc);
    pk.clear = clear;
    pk.nclear = nclear;
    for (int l = 0; l < kLayers; ++l) {
        const int nf = P.HS * (l == 0 ? (P.HS + 2 + 7) / 8 : (2 * P.HS + 7) / 8) * kWave * 8;   // per (tile, block, lane, k)
        pk.job[pk.njobs++] = PackJob{kPackFwd16, l, (nf + 255) / 256, (_Float16 *)(base + P.fa[l])};
        if (with_backward)
            pk.job[pk.njobs++] = PackJob{kPackImg, l, (img_pack_threads(P.HS, l) + 255) / 256, (_Float16 *)(base + P.img[l])};
    }
    pk.job[pk.njobs++] = PackJob{kPackMisc, 0, 2, nullptr};
    int blocks = 0;
    for (int j = 0; j < pk.njobs; ++j) blocks += pk.job[j].blocks;
    hipLaunchKernelGGL(pack_all_kernel, dim3(blocks), dim3(256), 0, s, pk);
    return launch_check("pack_all_kernel");
}

int launch_pack_ctrl(const fcr_weights *w, int CH, float *fcp, float *fcbo, float *fnp, hipStream_t s) {
    PackArgs pa{};   // pack_misc_item's fc part at 52 units: fc.W is read only for units < 52 < H, in bounds
    pa.H = kMaxSlots * 4;
    pa.HS = kMaxSlots;
    pa.CH = CH;
    pa.fcw = w->fc_w;
    pa.fcb = w->fc_b;
    pa.cwi = w->ctrl_w_inp;
    pa.cbi = w->ctrl_b_inp;
    pa.cwo = w->ctrl_w_out;
    pa.fcp = fcp;
    pa.fcbo = fcbo;
    pa.fnp = fnp;
    hipLaunchKernelGGL(pack_misc_kernel, dim3(2), dim3(256), 0, s, pa);
    return launch_check("pack_misc_kernel");
}

Packed packed_ptrs(const PackedLayout &L, char *ws) {
    Packed p;
    for (int l = 0; l < kLayers; ++l) {
        p.fa[l] = (const float *)(ws + L.fa[l]);
        p.img[l] = (const float *)(ws + L.img[l]);
    }
    p.fcp = (const float *)(ws + L.fcp);
    p.fcb = (const float *)(ws + L.fcb);
    p.fnp = (const float *)(ws + L.fnp);
    p.wsc = (const float *)(ws + L.wsc);
    return p;
}

// window-column scales of the f16 split's range guard (fcr_pack.h) -> wsc[8], from the call's inputs
int launch_range(const fcr_dims *d, const float *states, const float *u0, const float *noise, const float *fcw,
                 const float *fcb, float *part, float *wsc, hipStream_t s) {
    const size_t rows = (size_t)d->B * (d->N > kL ? d->N : kL);
    if (rows <= 16 * kRangeThreads) {   // small batch: one block, the final step inside (one launch)
        hipLaunchKernelGGL(range_partial_kernel, dim3(1), dim3(kRangeThreads), 0, s, states, u0, noise, d->B, d->N,
                           part, fcw, fcb, d->H, wsc);
        return launch_check("range_partial_kernel");
    }
    hipLaunchKernelGGL(range_partial_kernel, dim3(kRangeBlocks), dim3(kRangeThreads), 0, s, states, u0, noise, d->B,
                       d->N, part, nullptr, nullptr, 0, nullptr);
    int rc = launch_check("range_partial_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(range_final_kernel, dim3(1), dim3(64), 0, s, (const float *)part, kRangeBlocks, fcw, fcb, d->H,
                       wsc);
    return launch_check("range_final_kernel");
}

// The controller's weight gradients from the backward's dv: per-block partials, then their fixed-order sum
int launch_ctrl_grads(const fcr_dims *d, const Terms &tm, const float *xhat, const float *dv, const float *fnp, float *part,
                      int ctrl_blocks, float *g_w_inp, float *g_b_inp, float *g_w_out, hipStream_t s) {
    const bool one = ctrl_blocks == 1;   // one block writes the gradients itself (grad_out5)
    hipLaunchKernelGGL(ctrl_grad_kernel, dim3(ctrl_blocks), dim3(kCtrlBlock), 0, s, tm.ref, tm.ref_b, tm.ref_j, xhat, dv,
                       fnp, d->B, d->N, d->ctrl_hidden, part, one ? g_w_inp : nullptr, one ? g_b_inp : nullptr, one ? g_w_out : nullptr);
    if (const int rc = launch_check("ctrl_grad_kernel")) return rc;
    if (one) return FCR_OK;
    return launch_grad_reduce(part, ctrl_blocks, d->ctrl_hidden, g_w_inp, g_b_inp, g_w_out, s);
}

// grads: one block per (unit, parameter), the per-block partials summed in fixed order
int launch_grad_reduce(const float *part, int blocks, int hidden, float *g_w_inp, float *g_b_inp, float *g_w_out,
                       hipStream_t s) {
    hipLaunchKernelGGL(grad_reduce_kernel, dim3(hidden * 5), dim3(256), 0, s, part, blocks, hidden, g_w_inp, g_b_inp,
                       g_w_out);
    return launch_check("grad_reduce_kernel");
}

int launch_loss_reduce(const float *part, int n, int B, float *loss, hipStream_t s) {
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, part, n, B, loss);
    return launch_check("loss_reduce_kernel");
}

int launch_grad_reduce_many(const float *part, int blocks, int hidden, int n_models, float *g_w_inp, float *g_b_inp,
                            float *g_w_out, hipStream_t s) {
    hipLaunchKernelGGL(grad_reduce_many_kernel, dim3(hidden * 5, n_models), dim3(256), 0, s, part, blocks, hidden, g_w_inp,
                       g_b_inp, g_w_out);
    return launch_check("grad_reduce_many_kernel");
}

int pipe_max_sets() { return Pipe<13>::MAX_SETS; }

size_t rollout_workspace(const fcr_dims *d, int with_backward) { return make_layout(d, with_backward).total; }

int rollout_forward(const fcr_dims *d, fcr_options *opts, const Terms &tm, const fcr_weights *w, const float *X, const float *u0,
                    const float *states, const float *noise, float *loss, float *cost, float *command, float *error,
                    float *prediction, float *xhat, int with_backward, char *base, hipStream_t s) {
    int rc;
    const Layout L = make_layout(d, with_backward);
    if ((rc = launch_range(d, states, u0, noise, w->fc_w, w->fc_b, (float *)(base + L.rng), (float *)(base + L.wsc), s)))
        return rc;
    const bool flags = L.nw <= kPipeMaxGroups;   // the pipelined kernels' counters, zeroed for this forward and its backward
    if ((rc = launch_pack_all(w, d->H, d->ctrl_hidden, L, with_backward != 0, base,
                              flags ? (unsigned *)(base + L.pipe_flags) : nullptr, flags ? L.nw * kPipeFlags : 0, s)))
        return rc;

    FwdArgs fa{};
    fa.B = d->B;
    fa.N = d->N;
    fa.tm = tm;
    fa.X = X;
    fa.u0 = u0;
    fa.states = states;
    fa.noise = noise;
    fa.cost = cost;
    fa.command = command;
    fa.error = error;
    fa.prediction = prediction;
    fa.xhat_user = xhat;
    fa.xhat_ws = (float *)(base + L.xhat);
    fa.loss_part = (float *)(base + L.loss_part);
    fa.hseq = (f32x4 *)(base + L.hseq);
    fa.cseq = with_backward ? (f32x4 *)(base + L.cseq) : nullptr;
    fa.xw = with_backward ? (f32x2 *)(base + L.xw) : nullptr;
    fa.p = packed_ptrs(L, base);
#if FCR_STAMP
    fa.stamp = (unsigned long long *)(base + L.stamp) + (size_t)L.nw_pad * 8;
#endif
    const bool small = use_small(d, L, opts);
    note_kernels(opts, small ? FCR_KERNELS_SMALL : FCR_KERNELS_FUSED);
    const bool piped = small && use_pipe(d, L, opts);
    if (piped) {
        PipeArgs pa = pipe_args(L, base);
        pa.loss = loss;
        const int S = pipe_sets(d, L, Pipe<13>::MAX_SETS, 2);
        if (L.HS == 8) rc = with_backward ? launch_pfwd_s<8, true>(fa, pa, L, S, s) : launch_pfwd_s<8, false>(fa, pa, L, S, s);
        else rc = with_backward ? launch_pfwd_s<13, true>(fa, pa, L, S, s) : launch_pfwd_s<13, false>(fa, pa, L, S, s);
    } else if (small) {
        if (L.HS == 8) rc = with_backward ? launch_sfwd_t<8, true>(fa, L, s) : launch_sfwd_t<8, false>(fa, L, s);
        else rc = with_backward ? launch_sfwd_t<13, true>(fa, L, s) : launch_sfwd_t<13, false>(fa, L, s);
    } else {
        switch (L.HS) {
            case 4: rc = launch_fwd<4>(fa, L, d->precision == FCR_PRECISION_F16, s); break;
            case 8: rc = launch_fwd<8>(fa, L, d->precision == FCR_PRECISION_F16, s); break;
            case 13: rc = launch_fwd<13>(fa, L, d->precision == FCR_PRECISION_F16, s); break;
            default: rc = fail(FCR_EUNSUPPORTED, "H=%d", d->H);
        }
    }
    if (rc) return rc;
    if (piped) return FCR_OK;   // the pipelined forward wrote the loss itself
    // the fused kernel writes a (zero) partial for every padded wave; the small one one per group
    return launch_loss_reduce(fa.loss_part, small ? L.nw : L.nw_pad, d->B, loss, s);
}

int rollout_backward(const fcr_dims *d, fcr_options *opts, const Terms &tm, const float *X, const float *states, const float *prediction,
                     const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, char *base,
                     hipStream_t s) {
    int rc;
    const Layout L = make_layout(d, 1);
    BwdArgs ba{};
    ba.B = d->B;
    ba.N = d->N;
    ba.hidden = d->ctrl_hidden;
    ba.tm = tm;
    ba.X = X;
    ba.states = states;
    ba.prediction = prediction;
    ba.xhat = (const float *)(base + L.xhat);
    ba.dloss = dloss;
    ba.hseq = (const f32x4 *)(base + L.hseq);
    ba.cseq = (const f32x4 *)(base + L.cseq);
    ba.xw = (const f32x2 *)(base + L.xw);
    ba.dseq = (f32x4 *)(base + L.dseq);
    ba.dxrow = (f32x2 *)(base + L.dxrow);
    ba.g_u0 = g_u0;
    ba.dv = (float *)(base + L.dv);
#if FCR_STAMP
    ba.stamp = (unsigned long long *)(base + L.stamp);
#endif
    ba.p = packed_ptrs(L, base);
    const bool small = use_small(d, L, opts);
    note_kernels(opts, small ? FCR_KERNELS_SMALL : FCR_KERNELS_FUSED);
    if (small && use_pipe(d, L, opts)) {
        const PipeArgs pa = pipe_args(L, base);
        const int S = pipe_sets(d, L, Pipe<13>::MAX_SETS_BWD, 3);
        rc = L.HS == 8 ? launch_pbwd_s<8>(ba, pa, L, S, s) : launch_pbwd_s<13>(ba, pa, L, S, s);
    } else if (small) {
        rc = L.HS == 8 ? launch_sbwd_t<8>(ba, L, s) : launch_sbwd_t<13>(ba, L, s);
    } else {
        switch (L.HS) {
            case 4: rc = launch_bwd<4>(ba, L, d->precision == FCR_PRECISION_F16, s); break;
            case 8: rc = launch_bwd<8>(ba, L, d->precision == FCR_PRECISION_F16, s); break;
            case 13: rc = launch_bwd<13>(ba, L, d->precision == FCR_PRECISION_F16, s); break;
            default: rc = fail(FCR_EUNSUPPORTED, "H=%d", d->H);
        }
    }
    if (rc) return rc;
    return launch_ctrl_grads(d, tm, ba.xhat, ba.dv, ba.p.fnp, (float *)(base + L.fnn_part), L.ctrl_blocks, g_w_inp, g_b_inp,
                             g_w_out, s);
}

// ------------------------------------------------------------------------------------------------
// M controllers side by side (fcr_forward_many / fcr_backward_many): the one-workgroup small-batch kernels' MANY
// instantiations (fcr_small.h) on a grid of M * gpm groups, gpm = ceil(B / 16). d->B is the batch of ONE model; the
// inputs and outputs are stacked model-major. Shared: the LSTM fragments and images, the readout, the range guard (its
// scale belongs to the shared W_ih0, so it is taken over the stacked batch; s_c = 0 for every input the reference's
// scalers produce, and then nothing differs from M separate calls). Per model: the controller records, the loss, the
// controller gradients, each in the single-model kernels' summation order, so a model's numbers do not depend on M.
namespace {

struct ManyLayout : PackedLayout {
    int gpm, nw, ctrl_blocks;
    size_t fnp_many, xhat, dv, loss_part, fnn_part, hseq, cseq, xw, dseq, dxrow, stamp, total;
};
ManyLayout make_many(const fcr_dims *d, int M, int with_backward) {
    ManyLayout L{};
    L.HS = slot_tier(d->H);
    L.gpm = (d->B + kTile - 1) / kTile;
    L.nw = M * L.gpm;
    const size_t rows = (size_t)M * d->B;
    Arena take;
    take_packed(take, L, with_backward != 0);
    L.fnp_many = take(sizeof(float) * (size_t)M * kMS * 4 * kFnpStride);
    L.xhat = take(sizeof(float) * rows * d->N * kOut);
    L.loss_part = take(sizeof(float) * L.nw);
    L.dv = take(sizeof(float) * rows * d->N);
    L.ctrl_blocks = (int)(((long long)d->B * d->N + kCtrlItems - 1) / kCtrlItems);
    L.fnn_part = take(sizeof(float) * (size_t)M * L.ctrl_blocks * d->ctrl_hidden * 5);
    const size_t qcells = (size_t)L.nw * d->N * kLayers * kL * L.HS * 16;   // Geo<HS>::QC per cell
    L.hseq = take(sizeof(f32x4) * qcells);
    if (with_backward) {
        L.cseq = take(sizeof(f32x4) * qcells);
        L.xw = take(sizeof(f32x2) * (size_t)L.nw * d->N * kL * kWave);
        L.dseq = take(sizeof(f32x4) * (size_t)L.nw * d->N * 2 * kL * L.HS * 16);
        L.dxrow = take(sizeof(f32x2) * (size_t)4 * L.nw * d->N * kL * kWave);   // one copy per wave of a group
    }
#if FCR_STAMP
    L.stamp = take(sizeof(unsigned long long) * L.nw * 4 * 16);
#endif
    L.total = take.off;
    return L;
}

template <int HS, bool STORE>
int launch_sfwd_many_t(const FwdArgs &fa, const ManyLayout &L, hipStream_t s) {
    constexpr int lds = Small<HS>::LDS_FWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_sfwd_kernel<HS, STORE, true>, lds, attr_done, "sfwd_many")) return rc;
    hipLaunchKernelGGL((fcr_sfwd_kernel<HS, STORE, true>), dim3(L.nw), dim3(Small<HS>::NQ * kWave), lds, s, fa);
    return launch_check("fcr_sfwd_kernel<MANY>");
}
template <int HS>
int launch_sbwd_many_t(const BwdArgs &ba, const ManyLayout &L, hipStream_t s) {
    constexpr int lds = Small<HS>::LDS_BWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_sbwd_kernel<HS, true>, lds, attr_done, "sbwd_many")) return rc;
    hipLaunchKernelGGL((fcr_sbwd_kernel<HS, true>), dim3(L.nw), dim3(Small<HS>::NQ * kWave), lds, s, ba);
    return launch_check("fcr_sbwd_kernel<MANY>");
}

}  // namespace

bool many_supported(const fcr_dims *d) {
    const int HS = slot_tier(d->H);
    return !is_wide(d) && (HS == 8 || HS == 13);
}

size_t many_workspace(const fcr_dims *d, int n_models, int with_backward) {
    return make_many(d, n_models, with_backward).total;
}

int many_forward(const fcr_dims *d, int M, const Terms &tm, const fcr_weights *w, const float *X, const float *u0, const float *states,
                 const float *noise, float *loss, float *cost, float *command, float *error, float *prediction,
                 float *xhat, int with_backward, char *base, hipStream_t s) {
    int rc;
    const ManyLayout L = make_many(d, M, with_backward);
    fcr_dims all = *d;   // the range guard over the stacked batch
    all.B = M * d->B;
    if ((rc = launch_range(&all, states, u0, noise, w->fc_w, w->fc_b, (float *)(base + L.rng), (float *)(base + L.wsc), s)))
        return rc;
    // the shared packs once (no controller: CH = 0), then the M controllers' records
    if ((rc = launch_pack_all(w, d->H, 0, L, with_backward != 0, base, nullptr, 0, s))) return rc;
    constexpr int nf = kMS * 4 * kFnpStride;
    hipLaunchKernelGGL(pack_fnp_many_kernel, dim3((nf + 255) / 256, M), dim3(256), 0, s, w->ctrl_w_inp, w->ctrl_b_inp,
                       w->ctrl_w_out, d->ctrl_hidden, (float *)(base + L.fnp_many));
    if ((rc = launch_check("pack_fnp_many_kernel"))) return rc;

    FwdArgs fa{};
    fa.B = d->B;
    fa.N = d->N;
    fa.tm = tm;
    fa.X = X;
    fa.u0 = u0;
    fa.states = states;
    fa.noise = noise;
    fa.cost = cost;
    fa.command = command;
    fa.error = error;
    fa.prediction = prediction;
    fa.xhat_user = xhat;
    fa.xhat_ws = (float *)(base + L.xhat);
    fa.loss_part = (float *)(base + L.loss_part);
    fa.hseq = (f32x4 *)(base + L.hseq);
    fa.cseq = with_backward ? (f32x4 *)(base + L.cseq) : nullptr;
    fa.xw = with_backward ? (f32x2 *)(base + L.xw) : nullptr;
    fa.p = packed_ptrs(L, base);
    fa.p.fnp = (const float *)(base + L.fnp_many);
#if FCR_STAMP
    fa.stamp = (unsigned long long *)(base + L.stamp) + (size_t)L.nw * 4 * 8;
#endif
    if (L.HS == 8) rc = with_backward ? launch_sfwd_many_t<8, true>(fa, L, s) : launch_sfwd_many_t<8, false>(fa, L, s);
    else rc = with_backward ? launch_sfwd_many_t<13, true>(fa, L, s) : launch_sfwd_many_t<13, false>(fa, L, s);
    if (rc) return rc;
    hipLaunchKernelGGL(loss_reduce_many_kernel, dim3(M), dim3(256), 0, s, (const float *)fa.loss_part, L.gpm, d->B, loss);
    return launch_check("loss_reduce_many_kernel");
}

int many_backward(const fcr_dims *d, int M, const Terms &tm, const float *X, const float *states, const float *prediction,
                  const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, char *base,
                  hipStream_t s) {
    int rc;
    const ManyLayout L = make_many(d, M, 1);
    BwdArgs ba{};
    ba.B = d->B;
    ba.N = d->N;
    ba.hidden = d->ctrl_hidden;
    ba.tm = tm;
    ba.X = X;
    ba.states = states;
    ba.prediction = prediction;
    ba.xhat = (const float *)(base + L.xhat);
    ba.dloss = dloss;
    ba.hseq = (const f32x4 *)(base + L.hseq);
    ba.cseq = (const f32x4 *)(base + L.cseq);
    ba.xw = (const f32x2 *)(base + L.xw);
    ba.dseq = (f32x4 *)(base + L.dseq);
    ba.dxrow = (f32x2 *)(base + L.dxrow);
    ba.g_u0 = g_u0;
    ba.dv = (float *)(base + L.dv);
#if FCR_STAMP
    ba.stamp = (unsigned long long *)(base + L.stamp);
#endif
    ba.p = packed_ptrs(L, base);
    ba.p.fnp = (const float *)(base + L.fnp_many);
    rc = L.HS == 8 ? launch_sbwd_many_t<8>(ba, L, s) : launch_sbwd_many_t<13>(ba, L, s);
    if (rc) return rc;
    float *part = (float *)(base + L.fnn_part);
    const bool one = L.ctrl_blocks == 1;   // one block per model writes that model's gradients itself (grad_out5)
    hipLaunchKernelGGL(ctrl_grad_many_kernel, dim3(L.ctrl_blocks, M), dim3(kCtrlBlock), 0, s, tm.ref, tm.ref_m, tm.ref_b, tm.ref_j,
                       ba.xhat, (const float *)ba.dv,
                       ba.p.fnp, d->B, d->N, d->ctrl_hidden, part, L.ctrl_blocks, one ? g_w_inp : nullptr,
                       one ? g_b_inp : nullptr, one ? g_w_out : nullptr);
    if ((rc = launch_check("ctrl_grad_many_kernel"))) return rc;
    if (one) return FCR_OK;
    return launch_grad_reduce_many(part, L.ctrl_blocks, d->ctrl_hidden, M, g_w_inp, g_b_inp, g_w_out, s);
}

namespace {

// ------------------------------------------------------------------------------------------------
// LSTM surrogate, H <= 52: the rollout's fused split-f16 cells over one window (fcr_sur.h). Workspace:
// the packed fragments / images / readout as the rollout packs them, the window-batch slabs, and for the
// backward the dgate slab, its scales and the weight-gradient partials.
struct SurLayout : PackedLayout {   // (fnp: written as zeros by the shared pack job, unused)
    int nw, nw_pad, groups;
    size_t hseq, cseq, xw, htop, dseq, dgs, dsc, part, total;
};
inline int sur_kbb(int HS) { return (HS + 1) / 2; }
// weight-gradient k-blocks: groups of kSurKW backward waves x kL / kSurKC step groups (a missing last wave of a
// group reads a padding wave of the slabs, whose dgates and scales the backward wrote as zero)
inline int sur_nkb(int nw) { return (nw + kSurKW - 1) / kSurKW * (kL / kSurKC); }
inline size_t sur_part_floats(int HS, bool l0) {
    const int RA = (2 * HS + 3) / 4, NT = l0 ? RA + 1 : 2 * RA;
    return (size_t)16 * HS * 16 * NT;
}
SurLayout make_sur(const fcr_dims *d, int with_backward) {
    SurLayout L{};
    L.HS = slot_tier(d->H);
    L.nw = (d->B + kTile - 1) / kTile;
    constexpr int kPad = kFwdWaves > kBwdWaves ? kFwdWaves : kBwdWaves;
    L.nw_pad = (L.nw + kPad - 1) / kPad * kPad;
    const int nkb = sur_nkb(L.nw);
    L.groups = nkb < kSurWgMaxGroups ? nkb : kSurWgMaxGroups;
    Arena take;
    const int HS = L.HS;
    const size_t cells = (size_t)L.nw_pad * kLayers * kL;
    take_packed(take, L, with_backward != 0);
    L.hseq = take(sizeof(f32x4) * cells * HS * 16);
    if (with_backward) {
        L.cseq = take(sizeof(f32x4) * cells * HS * 16);
        L.xw = take(sizeof(f32x2) * (size_t)L.nw_pad * kL * kWave);
        L.htop = take(sizeof(float) * (size_t)d->B * d->H);
        L.dseq = take(sizeof(f32x4) * (size_t)L.nw_pad * 2 * kL * HS * 16);
        L.dgs = take(cells * sur_kbb(HS) * 2048);
        L.dsc = take(sizeof(float) * cells * 16);
        const size_t pf = sur_part_floats(HS, false) > sur_part_floats(HS, true) ? sur_part_floats(HS, false)
                                                                                 : sur_part_floats(HS, true);
        const size_t fcf = (size_t)((d->B + kFcRows - 1) / kFcRows) * (kOut * d->H + kOut);   // readout partials
        const size_t wgf = (size_t)L.groups * pf;
        L.part = take(sizeof(float) * (wgf > fcf ? wgf : fcf));
    }
    L.total = take.off;
    return L;
}
SurArgs sur_args(const fcr_dims *d, const SurLayout &L, char *base) {
    SurArgs a{};
    a.B = d->B;
    a.H = d->H;
    a.hseq = (f32x4 *)(base + L.hseq);
    if (L.cseq) {
        a.cseq = (f32x4 *)(base + L.cseq);
        a.xw = (f32x2 *)(base + L.xw);
        a.htop = (float *)(base + L.htop);
        a.dseq = (f32x4 *)(base + L.dseq);
        a.dgs = base + L.dgs;
        a.dsc = (float *)(base + L.dsc);
    }
    a.p = packed_ptrs(L, base);
    return a;
}

template <int HS>
int sur_forward_t(const SurArgs &a, const SurLayout &L, bool store, hipStream_t s) {
    constexpr int lds = SurGeo<HS>::LDS_FWD;
    static std::atomic<unsigned long long> attr_done[2] = {{0}, {0}};
    const void *fn = store ? (const void *)sur_fwd_kernel<HS, true> : (const void *)sur_fwd_kernel<HS, false>;
    if (const int rc = lds_attr(fn, lds, attr_done[store], "sur_fwd")) return rc;
    if (store) hipLaunchKernelGGL((sur_fwd_kernel<HS, true>), dim3(L.nw_pad / kFwdWaves), dim3(kFwdWaves * kWave), lds, s, a);
    else hipLaunchKernelGGL((sur_fwd_kernel<HS, false>), dim3(L.nw_pad / kFwdWaves), dim3(kFwdWaves * kWave), lds, s, a);
    return launch_check("sur_fwd_kernel");
}

template <int HS, bool L0>
int sur_wgrad_t(const SurArgs &a, const SurLayout &L, int l, float *part, float *g_ih, float *g_hh, hipStream_t s) {
    using W = SurWg<HS, L0>;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)sur_wgrad_kernel<HS, L0>, W::LDS, attr_done, "sur_wgrad")) return rc;
    const int nkb = sur_nkb(L.nw);
    hipLaunchKernelGGL((sur_wgrad_kernel<HS, L0>), dim3(L.groups), dim3(kSurWgThreads), W::LDS, s, a, l, nkb, part);
    int rc = launch_check("sur_wgrad_kernel");
    if (rc) return rc;
    if (L.groups > 1) {   // the partials summed into the first (coalesced, fixed order), then decoded from it
        hipLaunchKernelGGL(sur_part_sum_kernel, dim3((W::PART / 4 + 255) / 256), dim3(256), 0, s, part, L.groups, W::PART);
        if ((rc = launch_check("sur_part_sum_kernel"))) return rc;
    }
    const int nin = L0 ? kIn : a.H;
    const int n = 4 * a.H * (nin + a.H);
    hipLaunchKernelGGL((sur_wgrad_finish_kernel<HS, L0>), dim3((n + 255) / 256), dim3(256), 0, s, (const float *)part, 1,
                       a.H, a.p.wsc, g_ih, g_hh);
    return launch_check("sur_wgrad_finish_kernel");
}

// the weight gradients of the three layers from the dgate slab a backward kernel left
template <int HS>
int sur_wgrads_t(const SurArgs &a, const SurLayout &L, float *const *g_w_ih, float *const *g_w_hh, float *part,
                 hipStream_t s) {
    int rc;
    if ((rc = sur_wgrad_t<HS, false>(a, L, 2, part, g_w_ih[2], g_w_hh[2], s))) return rc;
    if ((rc = sur_wgrad_t<HS, false>(a, L, 1, part, g_w_ih[1], g_w_hh[1], s))) return rc;
    return sur_wgrad_t<HS, true>(a, L, 0, part, g_w_ih[0], g_w_hh[0], s);
}

template <int HS>
int sur_backward_t(const SurArgs &a, const SurLayout &L, float *const *g_w_ih, float *const *g_w_hh, float *part,
                   hipStream_t s) {
    constexpr int lds = SurGeo<HS>::LDS_BWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)sur_bwd_kernel<HS>, lds, attr_done, "sur_bwd")) return rc;
    hipLaunchKernelGGL((sur_bwd_kernel<HS>), dim3(L.nw_pad / kBwdWaves), dim3(kBwdWaves * kWave), lds, s, a);
    const int rc = launch_check("sur_bwd_kernel");
    if (rc) return rc;
    return sur_wgrads_t<HS>(a, L, g_w_ih, g_w_hh, part, s);
}

// readout: d fc.W = dy^T h_9, d fc.b = sum dy (per-tile partials in the weight-gradient scratch, fixed-order sum)
int sur_readout_grads(const fcr_dims *d, const float *dy, const float *htop, float *part, float *g_fc_w, float *g_fc_b,
                      hipStream_t s) {
    const int nfb = (d->B + kFcRows - 1) / kFcRows;
    hipLaunchKernelGGL(sur_fc_partial_kernel, dim3(nfb), dim3(256), 0, s, dy, htop, d->B, d->H, part);
    if (const int rc = launch_check("sur_fc_partial_kernel")) return rc;
    hipLaunchKernelGGL(sur_fc_final_kernel, dim3(kOut * d->H + kOut), dim3(256), 0, s, (const float *)part, nfb, d->H, g_fc_w,
                       g_fc_b);
    return launch_check("sur_fc_final_kernel");
}

}  // namespace

size_t sur_workspace(const fcr_dims *d, int with_backward) { return make_sur(d, with_backward).total; }

int sur_forward(const fcr_dims *d, const fcr_weights *w, const float *x, float *y, int with_backward, char *base,
                hipStream_t s) {
    const SurLayout L = make_sur(d, with_backward);
    int rc;
    // range guard of the window columns from the batch itself (u0 = x: its first B values are window values, so the
    // column-4 bound stays a bound)
    if ((rc = launch_range(d, x, x, nullptr, w->fc_w, w->fc_b, (float *)(base + L.rng), (float *)(base + L.wsc), s)))
        return rc;
    if ((rc = launch_pack_all(w, d->H, 0, L, with_backward != 0, base, nullptr, 0, s))) return rc;
    SurArgs a = sur_args(d, L, base);
    a.x = x;
    a.y = y;
    switch (L.HS) {
        case 4: return sur_forward_t<4>(a, L, with_backward != 0, s);
        case 8: return sur_forward_t<8>(a, L, with_backward != 0, s);
        default: return sur_forward_t<13>(a, L, with_backward != 0, s);
    }
}

int sur_backward(const fcr_dims *d, const float *dy, float *const *g_w_ih, float *const *g_w_hh, float *g_fc_w,
                 float *g_fc_b, float *g_x, char *base, hipStream_t s) {
    const SurLayout L = make_sur(d, 1);
    SurArgs a = sur_args(d, L, base);
    a.dy = dy;
    a.g_x = g_x;
    float *part = (float *)(base + L.part);
    int rc;
    switch (L.HS) {
        case 4: rc = sur_backward_t<4>(a, L, g_w_ih, g_w_hh, part, s); break;
        case 8: rc = sur_backward_t<8>(a, L, g_w_ih, g_w_hh, part, s); break;
        default: rc = sur_backward_t<13>(a, L, g_w_ih, g_w_hh, part, s);
    }
    if (rc) return rc;
    return sur_readout_grads(d, dy, a.htop, part, g_fc_w, g_fc_b, s);
}

static void sur_slabs(const fcr_dims *d, char *base, SurArgs *a) { *a = sur_args(d, make_sur(d, 1), base); }

static int sur_grads_of_dgates(const fcr_dims *d, const float *dy, float *const *g_w_ih, float *const *g_w_hh, float *g_fc_w,
                        float *g_fc_b, char *base, hipStream_t s) {
    const SurLayout L = make_sur(d, 1);
    const SurArgs a = sur_args(d, L, base);
    float *part = (float *)(base + L.part);
    int rc;
    switch (L.HS) {
        case 4: rc = sur_wgrads_t<4>(a, L, g_w_ih, g_w_hh, part, s); break;
        case 8: rc = sur_wgrads_t<8>(a, L, g_w_ih, g_w_hh, part, s); break;
        default: rc = sur_wgrads_t<13>(a, L, g_w_ih, g_w_hh, part, s);
    }
    if (rc) return rc;
    return sur_readout_grads(d, dy, a.htop, part, g_fc_w, g_fc_b, s);
}

namespace {

// ------------------------------------------------------------------------------------------------
// Command-driven surrogate rollout (fcr_lstm_rollout.h). Workspace: the packed forward fragments and readout as the
// rollout packs them, the range guard's partials and layer 1's h slab of ONE window per wave — nothing scales with T.
struct LroLayout : PackedLayout {
    int nw, nw_pad;
    size_t rpart, hseq, total;
};
LroLayout make_lro(const fcr_dims *d) {
    LroLayout L{};
    L.HS = slot_tier(d->H);
    L.nw = (d->B + kTile - 1) / kTile;
    L.nw_pad = (L.nw + kFwdWaves - 1) / kFwdWaves * kFwdWaves;
    Arena take;
    take_packed(take, L, false);
    L.rpart = take(sizeof(float) * kLroPart * kRangeBlocks);
    L.hseq = take(sizeof(f32x4) * (size_t)L.nw_pad * kL * L.HS * 16);   // Geo<HS>::QC per cell
    L.total = take.off;
    return L;
}

template <int HS>
int launch_lro_t(const LroArgs &a, const LroLayout &L, hipStream_t s) {
    constexpr int lds = LroGeo<HS>::LDS;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)fcr_lstm_rollout_kernel<HS>, lds, attr_done, "lstm_rollout")) return rc;
    hipLaunchKernelGGL((fcr_lstm_rollout_kernel<HS>), dim3(L.nw_pad / kFwdWaves), dim3(kFwdWaves * kWave), lds, s, a);
    return launch_check("fcr_lstm_rollout_kernel");
}

}  // namespace

size_t lro_workspace(const fcr_dims *d) { return make_lro(d).total; }

int lro_forward(const fcr_dims *d, const fcr_weights *w, const float *window0, const float *cmd, const float *gain,
                const float *noise, float *xhat, char *base, hipStream_t s) {
    const LroLayout L = make_lro(d);
    int rc;
    LroArgs a{};
    a.B = d->B;
    a.T = d->N;
    a.window0 = window0;
    a.cmd = cmd;
    a.noise = noise;
    a.g0 = gain ? gain[0] : 1.0f;
    a.g1 = gain ? gain[1] : 1.0f;
    a.g2 = gain ? gain[2] : 1.0f;
    a.g3 = gain ? gain[3] : 1.0f;
    a.xhat = xhat;
    a.hseq = (f32x4 *)(base + L.hseq);
    a.p = packed_ptrs(L, base);
    // range guard of the window columns from everything this rollout can put into them (fcr_lstm_rollout.h)
    float *part = (float *)(base + L.rpart), *wsc = (float *)(base + L.wsc);
    const size_t rows = (size_t)d->B * (d->N > kL ? d->N : kL);
    const LroRangeArgs rg{a.g0, a.g1, a.g2, a.g3, w->fc_w, w->fc_b, w->w_ih[0], d->H, wsc};
    const bool one = rows <= 16 * kRangeThreads;   // small batch: one block, the final step inside (one launch)
    hipLaunchKernelGGL(lro_range_partial_kernel, dim3(one ? 1 : kRangeBlocks), dim3(kRangeThreads), 0, s, window0, cmd,
                       noise, d->B, d->N, part, one ? 1 : 0, rg);
    if ((rc = launch_check("lro_range_partial_kernel"))) return rc;
    if (!one) {
        hipLaunchKernelGGL(lro_range_final_kernel, dim3(1), dim3(64), 0, s, (const float *)part, kRangeBlocks, rg);
        if ((rc = launch_check("lro_range_final_kernel"))) return rc;
    }
    if ((rc = launch_pack_all(w, d->H, 0, L, false, base, nullptr, 0, s))) return rc;
    switch (L.HS) {
        case 4: return launch_lro_t<4>(a, L, s);
        case 8: return launch_lro_t<8>(a, L, s);
        default: return launch_lro_t<13>(a, L, s);
    }
}

}  // namespace fcr


// ------------------------------------------------------------------------------------------------
// Backward of the command-driven surrogate rollout (fcr_lro_bwd.h): the kernels that lay the rollout's windows out as a
// virtual batch and run the reverse over it, strung together with the surrogate step's forward and weight-gradient
// kernels above.
// Workspace: sur_workspace at B' = T*Bp (Bp = B rounded up to 16), then the virtual batch (B',10,5), the recomputed
// outputs (B',4, unused), ybar (B',4) and the rows P [Bp/16][T+10][64] of 8 bytes, each slab 256-byte aligned.
// Launches per call, whatever T: lro_windows, the forward's range guard (1, or 2 above 409 windows), pack_all, sur_fwd,
// lro_bwd, per layer sur_wgrad + sur_part_sum + sur_wgrad_finish, sur_fc_partial, sur_fc_final: 16 or 17.
namespace fcr {
namespace {

struct LroBwdLayout {
    fcr_dims dv;   // the virtual batch's dims: B = T·Bp
    int nwb;       // waves per step
    size_t xwin, yrec, ybar, rows, total;
};
LroBwdLayout make_lro_bwd(const fcr_dims *d) {
    LroBwdLayout L{};
    L.nwb = (d->B + kTile - 1) / kTile;
    L.dv = *d;
    L.dv.B = d->N * L.nwb * kTile;
    L.dv.N = 1;
    Arena take;
    take.off = sur_workspace(&L.dv, 1);
    const size_t Bv = (size_t)L.dv.B;
    L.xwin = take(sizeof(float) * Bv * kL * kIn);
    L.yrec = take(sizeof(float) * Bv * kOut);
    L.ybar = take(sizeof(float) * Bv * kOut);
    L.rows = take(sizeof(f32x2) * (size_t)L.nwb * (d->N + kL) * kWave);
    L.total = take.off;
    return L;
}

template <int HS>
int launch_lro_bwd_t(LroBwdArgs &a, hipStream_t s) {
    using SG = SurGeo<HS>;
    a.dg_bytes = SG::DG;
    a.dsc_floats = SG::DSC;
    const size_t items = (size_t)a.s.B * kL;
    hipLaunchKernelGGL(lro_windows_kernel, dim3((unsigned)((items + kLroWinBlock - 1) / kLroWinBlock)), dim3(kLroWinBlock), 0,
                       s, a);
    return launch_check("lro_windows_kernel");
}
template <int HS>
int launch_lro_cells_t(const LroBwdArgs &a, hipStream_t s) {
    constexpr int lds = SurGeo<HS>::LDS_BWD;
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)lro_bwd_kernel<HS>, lds, attr_done, "lro_bwd")) return rc;
    hipLaunchKernelGGL((lro_bwd_kernel<HS>), dim3((a.nwb + kBwdWaves - 1) / kBwdWaves), dim3(kBwdWaves * kWave), lds, s, a);
    return launch_check("lro_bwd_kernel");
}

}  // namespace

bool lro_bwd_fits(const fcr_dims *d) {   // the virtual batch within the surrogate step's index range
    const long long nwb = (d->B + kTile - 1) / kTile;
    return (long long)d->N * nwb * kTile <= (1LL << 30);
}

size_t lro_bwd_workspace(const fcr_dims *d) { return make_lro_bwd(d).total; }

int lro_backward(const fcr_dims *d, const fcr_weights *w, const float *window0, const float *cmd, const float *gain,
                 const float *xhat, const float *g_xhat, const fcr_lstm_rollout_grads *out, char *base, hipStream_t s) {
    const LroBwdLayout L = make_lro_bwd(d);
    const int HS = slot_tier(d->H);
    LroBwdArgs a{};
    sur_slabs(&L.dv, base, &a.s);
    a.B = d->B;
    a.T = d->N;
    a.nwb = L.nwb;
    a.window0 = window0;
    a.cmd = cmd;
    a.xhat = xhat;
    a.g_xhat = g_xhat;
    a.g0 = gain ? gain[0] : 1.0f;
    a.g1 = gain ? gain[1] : 1.0f;
    a.g2 = gain ? gain[2] : 1.0f;
    a.g3 = gain ? gain[3] : 1.0f;
    a.xwin = (float *)(base + L.xwin);
    a.ybar = (float *)(base + L.ybar);
    a.rows = (f32x2 *)(base + L.rows);
    a.g_window0 = out->g_window0;
    a.g_cmd = out->g_cmd;
    // the weight-gradient product reads whole groups of kSurKW waves: the one past the last step's is zeroed
    a.zw0 = d->N * L.nwb;
    a.zw1 = (a.zw0 + kSurKW - 1) / kSurKW * kSurKW;
    int rc;
    switch (HS) {
        case 4: rc = launch_lro_bwd_t<4>(a, s); break;
        case 8: rc = launch_lro_bwd_t<8>(a, s); break;
        default: rc = launch_lro_bwd_t<13>(a, s);
    }
    if (rc) return rc;
    // the stored forward over the virtual batch (its own range guard and packs; the outputs are not used)
    if ((rc = sur_forward(&L.dv, w, a.xwin, (float *)(base + L.yrec), 1, base, s))) return rc;
    switch (HS) {
        case 4: rc = launch_lro_cells_t<4>(a, s); break;
        case 8: rc = launch_lro_cells_t<8>(a, s); break;
        default: rc = launch_lro_cells_t<13>(a, s);
    }
    if (rc) return rc;
    return sur_grads_of_dgates(&L.dv, a.ybar, out->g_w_ih, out->g_w_hh, out->g_fc_w, out->g_fc_b, base, s);
}

}  // namespace fcr

#if FCR_STAMP
// diagnostic builds: byte offset (in ws) of the per-wave cycle sums [nw_pad][8] of the backward
extern "C" {
size_t fcr_debug_stamp_offset(const fcr_dims *d) { return fcr::make_layout(d, 1).stamp; }
size_t fcr_debug_dseq_offset(const fcr_dims *d) { return fcr::make_layout(d, 1).dseq; }
size_t fcr_debug_dxrow_offset(const fcr_dims *d) { return fcr::make_layout(d, 1).dxrow; }
}  // extern "C"
#endif
