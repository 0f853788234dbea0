// fcr_wide.hip — host side of the H > 52 ("wide") engines: the rollout's per-cell forward and backward, the surrogate
// training step on the same cells, and the fcr_wide_bwd_cell test hook; with the kernels they launch (fcr_wide.h,
// fcr_wgemm.h, fcr_wbwd.h, fcr_wgrad.h, fcr_surrogate.h). The C ABI in fcr_abi.hip calls in through fcr_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "fcr.h"
#include "fcr_common.h"
#include "fcr_host.h"
#include "fcr_surrogate.h"
#include "fcr_wbwd.h"
#include "fcr_wgemm.h"
#include "fcr_wgrad.h"
#include "fcr_wide.h"

namespace fcr {
namespace {

// ---------------------------------------------------------------------------------------------
// H > 52: the batch-wide path (fcr_wide.h, fcr_wgemm.h, fcr_wbwd.h)
// ---------------------------------------------------------------------------------------------
// Every kernel of the rollout's wide path runs at Hp = H padded to whole 64-unit blocks of the forward cell kernel
// (fcr_wgemm.h): the padding units have zero weights in and out, so their gates stay i = f = o = 1/2, g = 0, c = h = 0
// and every product they enter gains exact zeros (the H <= 52 tiers pad the same way, slot_tier). The split weights,
// the readout's fc.W and the window-row gradient's W_ih0 are packed padded per call; the caller's tensors keep H.
int wide_hp(int H) { return (H + kWgU - 1) / kWgU * kWgU; }
// The fused backward cell's column blocks (fcr_wbwd.h): 256 output columns per workgroup in every geometry (WbG256,
// WbG256w). (Round 5 measured 512 columns x 64 trajectories for layers >= 1 — each cell's dgates formed once instead
// of per column block, at twice the A reads per trajectory — 3 % slower at config 5; commit e9dc1d2 builds it with
// -DFCR_WB512=1.)
constexpr int kWbCols = WbG256::kM;
static_assert(WbG256w::kM == kWbCols, "every backward geometry has the same column blocks");
// row-bound slots: one per column block of the writing launch (every block writes its slot, 0 where it has no such
// columns). dh of layer l: its own cells' [0, 2 Hp) (layer 0: [0, Hp)); the input gradient: layer l + 1's [0, Hp)
int wb_hslots(int l, int Hp) { return ((l ? 2 * Hp : Hp) + kWbCols - 1) / kWbCols; }
int wb_dslots(int Hp) { return (Hp + kWbCols - 1) / kWbCols; }
// the slots allocated: the most any geometry writes
int wide_nslots(int Hp) { return (2 * Hp + WbG256::kM - 1) / WbG256::kM; }

// What the rollout's and the surrogate's wide workspaces lay out alike: the per-call weight packs and the scratch of
// the fused backward cells (wb_cell)
struct WideShared {
    int Hp, ns;
    size_t fcw;     // fc.W padded [kOut][Hp]
    size_t fw[3];   // forward split weights per layer: [2][4Hp][K] (W_hi, W_lo; K = kx + Hp, wide_split_fw_kernel)
    size_t bt[3];   // backward product A per layer: [NO][4Hp / 32][hi 32 | lo 32] (NO = Hp for layer 0, else 2Hp)
    size_t w0p;     // W_ih0 packed [Hp][4][kIn] (the fused layer-0 cell's window-row gradient)
    size_t dH, dC, DC2, D[2], E0, RMc, RMh, RMd;
};
// the weight packs (bt and w0p only with a backward), then the backward cells' scratch, in workspace order
void take_wide_packs(Arena &take, WideShared &S, bool with_backward) {
    const size_t F16 = sizeof(_Float16), Hp = (size_t)S.Hp;
    for (int l = 0; l < kLayers; ++l) {
        const size_t K = (l == 0 ? kWgRecX0 : Hp) + Hp;
        S.fw[l] = take(F16 * 2 * 4 * Hp * K);
        if (with_backward) S.bt[l] = take(F16 * 2 * (l == 0 ? Hp : 2 * Hp) * 4 * Hp);
    }
    if (with_backward) S.w0p = take(sizeof(float) * Hp * 4 * kIn);
}
void take_wide_bwd(Arena &take, WideShared &S, size_t B) {
    const size_t F = sizeof(float), Hp = (size_t)S.Hp;
    S.dH = take(F * B * Hp);
    S.dC = take(F * B * Hp);
    S.DC2 = take(F * B * Hp);
    S.D[0] = take(F * kL * B * 2 * Hp);   // per t: [input gradient of the layer above | its dh_{t-1}]
    S.D[1] = take(F * kL * B * 2 * Hp);
    S.E0 = take(F * B * Hp);              // layer 0's dh_{t-1}
    S.RMc = take(F * 2 * B);              // [t & 1][B]            row bound of |dc|
    S.RMh = take(F * 2 * S.ns * B);       // [t & 1][slot][B]      of |dh|, per column block of its writer
    S.RMd = take(F * 2 * kL * S.ns * B);  // [l & 1][t][slot][B]   of |input gradient| for the layer below
}

struct WideLayout : WideShared {
    int keep, ctrl_blocks;
    size_t fcb, cwi, cbi, cwo, fcp, fcbo, fnp, wsc, rng, xhat, tot, cmd, err, Hs, Cs, WR, HR, total;
    size_t Act, rowg, dv, fnn_part;
    // kept windows (the last `keep` of N): the forward's gate pre-activations and c per cell
    // [keep][3][10][B][4Hp] / [keep][3][10][B][Hp], so the backward skips their recompute (wide_keep_fit)
    size_t KA, KC;
};

WideLayout make_wide(const fcr_dims *d, int with_backward, int keep = 0) {
    WideLayout L{};
    Arena take;
    const size_t B = d->B, N = d->N, F = sizeof(float), F16 = sizeof(_Float16);
    const size_t Hp = (size_t)wide_hp(d->H);
    L.Hp = (int)Hp;
    L.ns = wide_nslots((int)Hp);
    L.fcw = take(F * kOut * Hp);
    L.fcb = take(F * kOut);
    L.cwi = take(F * d->ctrl_hidden * kCtrlIn);
    L.cbi = take(F * d->ctrl_hidden);
    L.cwo = take(F * d->ctrl_hidden);
    L.fcp = take(F * kOut * kMaxSlots * 4);
    L.fcbo = take(F * kOut);
    L.fnp = take(F * kMS * 4 * kFnpStride);
    L.wsc = take(F * 8);
    L.rng = take(F * 8 * kRangeBlocks);
    L.xhat = take(F * B * N * kOut);
    L.tot = take(F * B);
    L.cmd = take(F * B);
    L.err = take(F * B);
    L.Hs = take(F * B * Hp);                               // fp32 h of the readout's cell (2, 9)
    L.Cs = take(F * kLayers * kL * B * Hp);                // c of every cell of the current window
    L.WR = take(F16 * kL * B * 2 * kWgRecX0);              // layer 0's window records
    L.HR = take(F16 * 2 * kL * B * 2 * Hp);                // h records of two layers (layer l in slot l & 1)
    take_wide_packs(take, L, with_backward != 0);
    if (with_backward) {
        L.Act = take(F * kLayers * kL * B * 4 * Hp);
        take_wide_bwd(take, L, B);
        L.rowg = take(F * (N + kL - 1) * B * kIn);
        L.dv = take(F * B * N);
        L.ctrl_blocks = (int)(((long long)B * N + kCtrlItems - 1) / kCtrlItems);
        L.fnn_part = take(F * (size_t)L.ctrl_blocks * d->ctrl_hidden * 5);
        if (keep > 0) {
            L.keep = keep;
            L.KA = take(F * (size_t)keep * kLayers * kL * B * 4 * Hp);
            L.KC = take(F * (size_t)keep * kLayers * kL * B * Hp);
        }
    }
    L.total = take.off;
    return L;
}

// a kept window's slabs (window j of the last L.keep)
float *kept_act(const WideLayout &L, char *base, const fcr_dims *d, int j) {
    return (float *)(base + L.KA) + (size_t)(j - (d->N - L.keep)) * kLayers * kL * d->B * 4 * L.Hp;
}
float *kept_c(const WideLayout &L, char *base, const fcr_dims *d, int j) {
    return (float *)(base + L.KC) + (size_t)(j - (d->N - L.keep)) * kLayers * kL * d->B * L.Hp;
}

// The wide path's per-call packs of the current weights, all at the padded Hp; `pieces` picks them: the forward split
// weights of every layer (kPkFw), the backward product's A of layer l (kPkBt << l) and W_ih0 (kPkW0) — kPkBwd: all of
// the backward's — and the readout's fc.W (kPkFc). Launched layer by layer (fw, then bt), then W_ih0, then fc.W
enum { kPkFw = 1, kPkFc = 2, kPkW0 = 4, kPkBt = 8, kPkBwd = kPkW0 | 7 * kPkBt };
int wide_pack(const fcr_weights *w, int H, const WideShared &S, int pieces, char *base, const float *wsc, hipStream_t s) {
    const int Hp = S.Hp;
    int rc;
    auto grid = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };
    for (int l = 0; l < kLayers; ++l) {
        if (pieces & kPkFw) {
            const size_t K = (l == 0 ? kWgRecX0 : Hp) + Hp, n = (size_t)4 * Hp * K;
            _Float16 *fw = (_Float16 *)(base + S.fw[l]);
            hipLaunchKernelGGL(wide_split_fw_kernel, grid(n), dim3(256), 0, s, w->w_ih[l], w->w_hh[l], H, Hp, (int)(l == 0),
                               wsc, fw, fw + n);
            if ((rc = launch_check("wide_split_fw_kernel"))) return rc;
        }
        if (pieces & (kPkBt << l)) {
            const int NO = l == 0 ? Hp : 2 * Hp;
            const size_t nbt = (size_t)NO * 4 * Hp;
            _Float16 *bt = (_Float16 *)(base + S.bt[l]);
            hipLaunchKernelGGL(wide_split_bt_kernel, grid(nbt), dim3(256), 0, s, l == 0 ? (const float *)nullptr : w->w_ih[l],
                               w->w_hh[l], H, Hp, NO, bt);
            if ((rc = launch_check("wide_split_bt_kernel"))) return rc;
        }
    }
    if (pieces & kPkW0) {
        hipLaunchKernelGGL(wide_pack_w0_kernel, grid((size_t)4 * Hp * kIn), dim3(256), 0, s, w->w_ih[0], H, Hp,
                           (float *)(base + S.w0p));
        if ((rc = launch_check("wide_pack_w0_kernel"))) return rc;
    }
    if (pieces & kPkFc) {
        hipLaunchKernelGGL(wide_pad_fc_kernel, grid((size_t)kOut * Hp), dim3(256), 0, s, w->fc_w, H, Hp, (float *)(base + S.fcw));
        if ((rc = launch_check("wide_pad_fc_kernel"))) return rc;
    }
    return FCR_OK;
}

WideArgs wide_args(const fcr_dims *d, const WideLayout &L, char *base) {
    WideArgs a{};
    a.B = d->B;
    a.N = d->N;
    a.H = L.Hp;   // every wide kernel runs at the padded size
    a.CH = d->ctrl_hidden;
    a.fcw = (const float *)(base + L.fcw);
    a.fcb = (const float *)(base + L.fcb);
    a.cwi = (const float *)(base + L.cwi);
    a.cbi = (const float *)(base + L.cbi);
    a.cwo = (const float *)(base + L.cwo);
    a.xhat = (float *)(base + L.xhat);
    a.tot = (float *)(base + L.tot);
    a.cmd = (float *)(base + L.cmd);
    a.err = (float *)(base + L.err);
    a.Hs = (float *)(base + L.Hs);
    a.Cs = (float *)(base + L.Cs);
    a.Act = L.Act ? (float *)(base + L.Act) : nullptr;
    a.dH = L.dH ? (float *)(base + L.dH) : nullptr;
    a.dC = L.dC ? (float *)(base + L.dC) : nullptr;
    a.rowg = L.rowg ? (float *)(base + L.rowg) : nullptr;
    a.dv = L.dv ? (float *)(base + L.dv) : nullptr;
    a.wsc = (const float *)(base + L.wsc);
    a.wr = (_Float16 *)(base + L.WR);
    return a;
}

// One forward cell of the wide path: the cell's split-f16 GEMM and update as one hand-written kernel (fcr_wgemm.h)
int launch_wgemm_cell(const WgArgs &wa, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done{0};
    if (const int rc = lds_attr((const void *)wide_cell_fwd_kernel, kWgLds, attr_done, "wgemm")) return rc;
    if (wa.H % kWgU || wa.kx % kWgK || wa.K != wa.kx + wa.H || wa.B <= 0 || !wa.W || !wa.xr || !wa.c_out || !wa.h_rec)
        return fail(FCR_EINVAL, "wide_cell_fwd_kernel: K %d kx %d H %d B %d off its tiling", wa.K, wa.kx, wa.H, wa.B);
    const int nx = (wa.B + kWgN - 1) / kWgN, ny = wa.H / kWgU;
    hipLaunchKernelGGL(wide_cell_fwd_kernel, dim3((unsigned)(nx * ny)), dim3(kWgThreads), kWgLds, s, wa);
    return launch_check("wide_cell_fwd_kernel");
}

// One backward cell of the fused path (fcr_wbwd.h): dgates formed in the product's prologue, out = dG [W_ih | W_hh]
// (columns [0, NO), NO = 0: the dgate part only) in true units. Geometries: layers >= 1 on 256 columns x 256
// trajectories (WbG256w: A staged once per 256 trajectories, backward −5.4 % at config 5, round5_c5_n256_ab_*.log)
// where its halved workgroup count still fills the chip (B >= 32 768: >= 256 workgroups at two column blocks; the
// surrogate's B = 256 step: 3.2 ms on WbG256 against 4.1) and the cell does not also write its dgates (the surrogate's
// B = 65 536 step 2 % slower on it); everything else, layer 0 included, on 256 x 128 (WbG256). (Layer 0 on WbG256w
// spills ~320 registers in its W_ih0 accumulation at the 12-wave budget: backward +57 %, round5_c5_l0w_ab_keepall.log;
// commit e9dc1d2 builds it with -DFCR_WB_L0_N256=1.)
int launch_fb(const WbArgs &wa, bool l0, hipStream_t s) {
    static std::atomic<unsigned long long> attr_done[4] = {{0}, {0}, {0}, {0}};
    const bool w0g = l0 && wa.H > kWbW0LdsUnits;   // layer 0 with W_ih0 read from global memory
    const bool n256 = !l0 && wa.NB >= 32768 && !wa.dg;
    enum { kL1 = 0, kL0 = 1, kL0Global = 2, kL1N256 = 3 };
    const int kind = l0 ? (w0g ? kL0Global : kL0) : (n256 ? kL1N256 : kL1);
    const void *fn = kind == kL1       ? (const void *)wide_bwd_fused_kernel<WbG256, false>
                     : kind == kL0     ? (const void *)wide_bwd_fused_kernel<WbG256, true, false>
                     : kind == kL1N256 ? (const void *)wide_bwd_fused_kernel<WbG256w, false>
                                       : (const void *)wide_bwd_fused_kernel<WbG256, true, true>;
    if (const int rc = lds_attr(fn, kind == kL1N256 ? kWbLds256w : kWbLds256, attr_done[kind], "wbwd")) return rc;
    if (wa.NO < 0 || wa.NO > 2 * wa.H || wa.NO % 8 || wa.H % 8 || wa.NB <= 0 || (wa.rm_h && wa.nrh < 1) ||
        (wa.rm_d && wa.nrd < 1) || (l0 && (!wa.wih0 || !wa.rowg)))
        return fail(FCR_EINVAL, "wide_bwd_fused_kernel: NO %d H %d B %d off its tiling", wa.NO, wa.H, wa.NB);
    const int N = kind == kL1N256 ? WbG256w::kN : WbG256::kN;
    const dim3 grid((unsigned)((wa.NB + N - 1) / N * (wa.NO > 0 ? (wa.NO + kWbCols - 1) / kWbCols : 1)));
    if (kind == kL1N256)
        hipLaunchKernelGGL((wide_bwd_fused_kernel<WbG256w, false>), grid, dim3(WbG256w::kThreads), wb_lds_bytes<WbG256w>(false, wa.H), s, wa);
    else if (kind == kL1)
        hipLaunchKernelGGL((wide_bwd_fused_kernel<WbG256, false>), grid, dim3(WbG256::kThreads), wb_lds_bytes<WbG256>(false, wa.H), s, wa);
    else if (kind == kL0)
        hipLaunchKernelGGL((wide_bwd_fused_kernel<WbG256, true, false>), grid, dim3(WbG256::kThreads), wb_lds_bytes<WbG256>(true, wa.H), s, wa);
    else
        hipLaunchKernelGGL((wide_bwd_fused_kernel<WbG256, true, true>), grid, dim3(WbG256::kThreads), wb_lds_bytes<WbG256>(true, wa.H), s, wa);
    return launch_check("wide_bwd_fused_kernel");
}

// What a backward cell's product writes (WbArgs NO, h0, h1, d1), at hidden size Hp; has_prev: the cell has a step
// before it (t > 0), so dh_{t-1} is wanted. Layers >= 1: [input gradient | dh_{t-1}] (t = 0: the former only);
// layer 0: dh_{t-1} (t = 0: none) — its window-row gradient goes through wa.wih0 / wa.rowg
void wb_outputs(WbArgs &wa, bool l0, int Hp, bool has_prev) {
    if (!l0) {
        wa.NO = has_prev ? 2 * Hp : Hp;
        wa.h0 = Hp;
        wa.h1 = has_prev ? 2 * Hp : Hp;
        wa.d1 = Hp;
    } else {
        wa.NO = has_prev ? Hp : 0;
        wa.h0 = 0;
        wa.h1 = Hp;
        wa.d1 = 0;
    }
}

// The backward cells' scratch of a wide workspace (WideShared) as pointers
struct WbBufs {
    const _Float16 *bt[kLayers];
    const float *w0p;
    float *dH, *DC[2], *D[2], *E0, *RMc, *RMh, *RMd;
    int ns, B, Hp;
};
WbBufs wb_bufs(const WideShared &S, char *base, int B) {
    WbBufs b{};
    for (int l = 0; l < kLayers; ++l) b.bt[l] = (const _Float16 *)(base + S.bt[l]);
    b.w0p = (const float *)(base + S.w0p);
    b.dH = (float *)(base + S.dH);
    b.DC[0] = (float *)(base + S.dC);
    b.DC[1] = (float *)(base + S.DC2);
    b.D[0] = (float *)(base + S.D[0]);
    b.D[1] = (float *)(base + S.D[1]);
    b.E0 = (float *)(base + S.E0);
    b.RMc = (float *)(base + S.RMc);
    b.RMh = (float *)(base + S.RMh);
    b.RMd = (float *)(base + S.RMd);
    b.ns = S.ns;
    b.B = B;
    b.Hp = S.Hp;
    return b;
}

// The fused backward cell (layer l, step t) of one window, layers 2..0 and t = 9..0 in launch order. Act, Cs: the
// window's gate activations and c ([3][10][B][4Hp] / [3][10][B][Hp]); rowg: the row of the window-row gradient layer 0
// adds to at this step; dG: where the cells also write their dgates ([10][B][4Hp]), or null. Before the window's first
// cell b.dH holds the head's dh of cell (2, 9) and slot 0 of b.RMh its row bound
WbArgs wb_cell(const WbBufs &b, int l, int t, const float *Act, const float *Cs, float *rowg, float *dG) {
    const int B = b.B, Hp = b.Hp, ns = b.ns;
    const size_t cell = (size_t)B * Hp, c_off = ((size_t)l * kL + t) * cell;
    // dh_t below t = 9 comes from cell t+1's product: layer 0 columns 0..Hp-1 of E0, layers >= 1 columns
    // Hp..2Hp-1 of D[l-1] row t+1; the layer above's input gradient from D[l] row t
    // (t = 9: the head's dh for layer 2, zero below it, passed as null like the zero dc_9 and their bounds)
    const bool top9 = t == kL - 1 && l == kLayers - 1, zero9 = t == kL - 1 && l < kLayers - 1;
    WbArgs wa{};
    wa.A = b.bt[l];
    wa.NB = B;
    wa.H = Hp;
    wa.act = Act + c_off * 4;
    wa.c_prev = t > 0 ? Cs + c_off - cell : nullptr;
    // (D rows are k8 rows of 2Hp columns: column Hp starts at + Hp B = + cell)
    wa.dh = top9 ? b.dH : zero9 ? nullptr : l == 0 ? b.E0 : b.D[l - 1] + (size_t)(t + 1) * 2 * cell + cell;
    wa.din = l < kLayers - 1 ? b.D[l] + (size_t)t * 2 * cell : nullptr;
    wa.dC = t == kL - 1 ? nullptr : b.DC[(t + 1) & 1];   // t writes buffer t & 1
    wa.dC_out = b.DC[t & 1];
    wa.rm_c = t == kL - 1 ? nullptr : b.RMc + (size_t)((t + 1) & 1) * B;
    wa.rm_c_out = t > 0 ? b.RMc + (size_t)(t & 1) * B : nullptr;
    // dh's bound: the head's one slot at t = 9 (parity (9 + 1) & 1 = 0; none below layer 2), else the column blocks of
    // cell t + 1's product
    wa.rm_h = zero9 ? nullptr : b.RMh + (size_t)((t + 1) & 1) * ns * B;
    wa.nrh = t == kL - 1 ? 1 : wb_hslots(l, Hp);
    wa.rm_h_out = t > 0 ? b.RMh + (size_t)(t & 1) * ns * B : nullptr;
    wa.rm_d = l < kLayers - 1 ? b.RMd + ((size_t)((l + 1) & 1) * kL + t) * ns * B : nullptr;
    wa.nrd = wb_dslots(Hp);
    wa.rm_d_out = l > 0 ? b.RMd + ((size_t)(l & 1) * kL + t) * ns * B : nullptr;
    wa.dg = dG ? dG + (size_t)t * cell * 4 : nullptr;
    wb_outputs(wa, l == 0, Hp, t > 0);
    if (l > 0) {   // into D[l-1] row t
        wa.out = b.D[l - 1] + (size_t)t * 2 * cell;
    } else {       // dh_{t-1} into E0
        wa.out = b.E0;
        wa.wih0 = b.w0p;
        wa.rowg = rowg;
    }
    return wa;
}

// |v| row maxima over the first n columns of B rows of stride ld, or of k8 rows (ld = 0; fcr_wide.h), one wave per
// row: the row bounds fcr_wide_bwd_cell hands the fused backward cell, which the rollout gets from the kernels that
// wrote those rows (the surrogate: its head's dh_9)
__global__ __launch_bounds__(256) void row_absmax_kernel(const float *__restrict__ v, int n, int ld, int B,
                                                         float *__restrict__ out) {
    const int b = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    float m = 0.0f;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, fabsf(v[ld ? (size_t)b * ld + i : k8(B, b, i)]));
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) out[b] = m;
}

// torch rows [B][ld] (first n columns) <-> k8 rows [n/8][B][8] (fcr_wide.h): the test hook's layout conversion
__global__ void k8_rows_kernel(const float *__restrict__ src, int B, int n, int ld, float *__restrict__ dst, int to_k8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * n) return;
    const int b = (int)(i / n), u = (int)(i % n);
    if (to_k8) dst[k8(B, b, u)] = src[(size_t)b * ld + u];
    else dst[(size_t)b * ld + u] = src[k8(B, b, u)];
}

// fcr_wide_bwd_cell (test hook): the scratch of one standalone fused backward cell
struct CellHookLayout {
    size_t bt, w0, rm, rows, total;
};
CellHookLayout cell_hook_layout(int B, int H, int layer0) {
    CellHookLayout L{};
    Arena take;
    const size_t NP = layer0 ? H : 2 * (size_t)H;
    L.bt = take(sizeof(_Float16) * 2 * NP * 4 * H);
    L.w0 = take(sizeof(float) * 4 * H * kIn);
    L.rm = take(sizeof(float) * 3 * (size_t)B);   // rm_c [B], rm_h [1][B], rm_d [1][B]
    // k8 copies of c_prev, dh, din, dc, dc_out (B H each) and out (B NP)
    L.rows = take(sizeof(float) * (size_t)B * (5 * (size_t)H + NP));
    L.total = take.off;
    return L;
}

// One window's 30 cells, forward (the rollout, and the backward's recompute of a window that was not kept): layer by
// layer, t = 0..9, each cell one wide_cell_fwd_kernel launch. keep_act: the cells' gate activations into `Act` (the
// backward's dgates read them, as autograd reads the activations its forward saved).
// S.fw: the layers' split weights; HR: h records of `slots` layers (layer l in slot l % slots: the rollout keeps two,
// the surrogate all three for its weight gradients)
int wide_cells(const WideArgs &a, const WideShared &S, char *base, _Float16 *HR, int slots, bool keep_act,
               hipStream_t s) {
    const int B = a.B, Hp = S.Hp;
    const size_t cell = (size_t)B * Hp;
    auto rec = [&](int l, int t) { return HR + ((size_t)(l % slots) * kL + t) * B * 2 * Hp; };   // h record of (l, t)
    int rc;
    for (int l = 0; l < kLayers; ++l) {
        const size_t K = (l == 0 ? kWgRecX0 : Hp) + Hp;
        for (int t = 0; t < kL; ++t) {
            WgArgs wa{};
            wa.W = (const _Float16 *)(base + S.fw[l]);
            wa.K = (int)K;
            wa.kx = l == 0 ? kWgRecX0 : Hp;
            wa.xr = l == 0 ? a.wr + (size_t)t * B * 2 * kWgRecX0 : rec(l - 1, t);
            wa.hr = t > 0 ? rec(l, t - 1) : nullptr;
            wa.B = B;
            wa.H = Hp;
            wa.c_prev = t > 0 ? a.Cs + ((size_t)l * kL + t - 1) * cell : nullptr;
            wa.c_out = a.Cs + ((size_t)l * kL + t) * cell;
            wa.h_out = (l == kLayers - 1 && t == kL - 1) ? a.Hs : nullptr;
            wa.act = keep_act ? a.Act + ((size_t)l * kL + t) * cell * 4 : nullptr;
            wa.h_rec = rec(l, t);
            if ((rc = launch_wgemm_cell(wa, s))) return rc;
        }
    }
    return FCR_OK;
}

// the rollout's window cells (two record slots)
int wide_window_cells(const WideArgs &a, const WideLayout &L, char *base, bool keep_act, hipStream_t s) {
    return wide_cells(a, L, base, (_Float16 *)(base + L.HR), 2, keep_act, s);
}

// H > 52: the surrogate's step on the rollout's wide kernels (no vendor library): the forward cells of fcr_wgemm.h
// over the window batch (every cell's activations, c and h records kept), the fused backward cells of fcr_wbwd.h
// (which also write each cell's dgates), and the weight gradients as reductions over all 10 B (step, sample) rows
// on the fp32 matrix cores (fcr_wgrad.h). Hidden size padded to Hp as on the rollout's wide path.
struct SurWideLayout : WideShared {
    size_t wsc, rng, xt, WR, HR, Cs, Act, Hs, rowg, dG, fcpart, part, part_floats, total;
};
constexpr int kSurFcSlices = 64;   // batch slices of the readout's weight gradient (fixed: deterministic)

// n slices of one weight-gradient reduction: enough workgroups to fill the chip, whole kWgrN steps per slice
struct WgSplit {
    int S;
    long long n_per;
};
WgSplit wg_split(long long n, int R, int K) {
    // K <= kWgrSmallK (wgrad_small_kernel): one thread per row r, so many n slices for parallelism
    const bool small = K <= kWgrSmallK;
    const long long tiles = small ? (R + 255) / 256 : (long long)((R + kWgrT - 1) / kWgrT) * ((K + kWgrT - 1) / kWgrT);
    long long S = ((small ? 2048 : 512) + tiles - 1) / tiles;
    S = S < 1 ? 1 : (S > (small ? 1024 : 64) ? (small ? 1024 : 64) : S);
    long long per = (n + S - 1) / S;
    per = (per + kWgrN - 1) / kWgrN * kWgrN;
    return {(int)((n + per - 1) / per), per};
}

SurWideLayout make_surw(const fcr_dims *d, int with_backward) {
    SurWideLayout L{};
    Arena take;
    const size_t B = d->B, F = sizeof(float), F16 = sizeof(_Float16), Hp = (size_t)wide_hp(d->H);
    L.Hp = (int)Hp;
    L.ns = wide_nslots((int)Hp);
    L.fcw = take(F * kOut * Hp);
    L.wsc = take(F * 8);
    L.rng = take(F * 8 * kRangeBlocks);
    L.xt = take(F * kL * B * kIn);
    L.WR = take(F16 * kL * B * 2 * kWgRecX0);
    L.HR = take(F16 * kLayers * kL * B * 2 * Hp);
    L.Cs = take(F * kLayers * kL * B * Hp);
    // the gate activations only for the backward (the forward-only call's cells run with keep_act off)
    L.Act = with_backward ? take(F * kLayers * kL * B * 4 * Hp) : 0;
    L.Hs = take(F * B * Hp);
    take_wide_packs(take, L, with_backward != 0);
    if (with_backward) {
        take_wide_bwd(take, L, B);
        L.rowg = take(F * kL * B * kIn);
        L.dG = take(F * kL * B * 4 * Hp);   // one layer's dgates, every step
        L.fcpart = take(F * kSurFcSlices * kOut * Hp);
        // the largest set of weight-gradient partials over every reduction surw_backward runs: n = 10 B rows (W_ih)
        // and 9 B rows (W_hh), K = kIn (layer 0's W_ih) and H. wg_split rounds each slice up to whole kWgrN steps,
        // so the 9 B reduction can take MORE slices than the 10 B one (H = 256, B = 110: 31 against 18)
        size_t pf = 0;
        for (long long n : {(long long)kL * B, (long long)(kL - 1) * B})
            for (int K : {kIn, d->H}) {
                const WgSplit w = wg_split(n, 4 * (int)Hp, K);
                const size_t a = (size_t)w.S * 4 * Hp * K;
                pf = a > pf ? a : pf;
            }
        L.part = take(F * pf);
        L.part_floats = pf;
    }
    L.total = take.off;
    return L;
}

// one weight gradient: dW [4H][K] = sum_n A[n][.] X[n][.] (fcr_wgrad.h), X fp32 rows or split records
int surw_wgrad(const float *A, long long n, int Hp, int H, int K, const float *X, int ldx, const _Float16 *XR,
               float *part, size_t part_floats, float *dW, hipStream_t s) {
    const WgSplit sp = wg_split(n, 4 * Hp, K);
    if ((size_t)sp.S * 4 * Hp * K > part_floats)   // make_surw sizes L.part for every (n, K) this runs with
        return fail(FCR_EWORKSPACE, "surrogate weight-gradient partials exceed their workspace slab");
    WgradArgs g{};
    g.A = A;
    g.lda = 4 * Hp;
    g.X = X;
    g.XR = XR;
    g.ldx = ldx;
    g.Hx = Hp;
    g.n = n;
    g.R = 4 * Hp;
    g.K = K;
    g.n_per = sp.n_per;
    g.part = part;
    int rc;
    if (K <= kWgrSmallK && X) {
        hipLaunchKernelGGL(wgrad_small_kernel, dim3((unsigned)((4 * Hp + 255) / 256), (unsigned)sp.S), dim3(256), 0, s, g);
        rc = launch_check("wgrad_small_kernel");
    } else {
        static std::atomic<unsigned long long> attr_done{0};
        if ((rc = lds_attr((const void *)wgrad_kernel, kWgrLds, attr_done, "wgrad"))) return rc;
        hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)((4 * Hp + kWgrT - 1) / kWgrT), (unsigned)((K + kWgrT - 1) / kWgrT),
                                              (unsigned)sp.S),
                           dim3(kWgrThreads), kWgrLds, s, g);
        rc = launch_check("wgrad_kernel");
    }
    if (rc) return rc;
    const long long e = (long long)4 * H * K;
    hipLaunchKernelGGL(wgrad_sum_pad_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, (const float *)part, sp.S,
                       H, Hp, K, dW);
    return launch_check("wgrad_sum_pad_kernel");
}

}  // namespace

size_t wide_workspace(const fcr_dims *d, int with_backward, int keep) { return make_wide(d, with_backward, keep).total; }

// The number of kept windows a workspace of ws_bytes holds (the most that fit): the forward and the
// backward each derive it from the ws_bytes they are given, so they agree with no state between them.
int wide_keep_fit(const fcr_dims *d, size_t ws_bytes) {
    for (int k = d->N; k > 0; --k)
        if (make_wide(d, 1, k).total <= ws_bytes) return k;
    return 0;
}

// Default cap of a backward-enabled wide workspace: half of the memory that was FREE on the device the first
// time one was sized there (cached per device, so the count does not drift as torch's cache holds the last
// call's workspace), and never more than kWideDefaultFrac of the device's total. Ranks sharing a device each
// see what the others left; what exceeds the cap recomputes instead of keeping (the floor workspace stays).
constexpr double kWideDefaultFrac = 0.40;
long long wide_default_cap() {
    static std::mutex mu;
    static long long cap_of[64];
    static bool have[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (!have[dev]) {
        size_t free_b = 0, total_b = 0;
        long long cap = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            cap = (long long)(free_b / 2);
            const long long lim = (long long)((double)total_b * kWideDefaultFrac);
            if (cap > lim) cap = lim;
        }
        cap_of[dev] = cap;
        have[dev] = true;
    }
    return cap_of[dev];
}

int wide_forward(const fcr_dims *d, const Terms &tm, const fcr_weights *w, const float *X, const float *u0, const float *states,
                 const float *noise, float *loss, float *cost, float *command, float *error, float *prediction,
                 float *xhat, int with_backward, char *base, size_t ws_bytes, hipStream_t s) {
    const WideLayout L = make_wide(d, with_backward, with_backward ? wide_keep_fit(d, ws_bytes) : 0);
    const size_t F = sizeof(float);
    int rc;
    // private copies of every parameter the backward needs (fcr_backward takes no weights)
    auto cp = [&](size_t off, const float *src, size_t n) {
        return hipMemcpyAsync(base + off, src, n * F, hipMemcpyDeviceToDevice, s);
    };
    if (cp(L.fcb, w->fc_b, kOut) || cp(L.cwi, w->ctrl_w_inp, d->ctrl_hidden * kCtrlIn) ||
        cp(L.cbi, w->ctrl_b_inp, d->ctrl_hidden) || cp(L.cwo, w->ctrl_w_out, d->ctrl_hidden))
        return fail(FCR_EHIP, "hipMemcpyAsync (parameters) failed");
    // controller records for ctrl_grad_kernel (the fc part is unused on this path)
    if ((rc = launch_pack_ctrl(w, d->ctrl_hidden, (float *)(base + L.fcp), (float *)(base + L.fcbo), (float *)(base + L.fnp), s)))
        return rc;
    if ((rc = launch_range(d, states, u0, noise, w->fc_w, w->fc_b, (float *)(base + L.rng), (float *)(base + L.wsc), s)))
        return rc;
    if ((rc = wide_pack(w, d->H, L, kPkFw | kPkFc | (with_backward ? kPkBwd : 0), base, (const float *)(base + L.wsc), s))) return rc;
    WideArgs a = wide_args(d, L, base);
    a.tm = tm;
    a.X = X;
    a.u0 = u0;
    a.states = states;
    a.noise = noise;
    a.pred = prediction;
    const int nb = (d->B + 255) / 256;
    for (int j = 0; j < d->N; ++j) {
        hipLaunchKernelGGL(wide_window_kernel<true>, dim3(nb), dim3(256), 0, s, a, j);
        if ((rc = launch_check("wide_window_kernel"))) return rc;
        if (j >= d->N - L.keep) {   // kept window: pre-activations and c into its own slabs for the backward
            WideArgs ak = a;
            ak.Act = kept_act(L, base, d, j);
            ak.Cs = kept_c(L, base, d, j);
            if ((rc = wide_window_cells(ak, L, base, true, s))) return rc;
        } else if ((rc = wide_window_cells(a, L, base, false, s))) {
            return rc;
        }
        hipLaunchKernelGGL(wide_readout_kernel, dim3((unsigned)(((size_t)d->B * kRoLanes + 255) / 256)), dim3(256), 0, s, a, j,
                           (const float *)a.Hs);
        if ((rc = launch_check("wide_readout_kernel"))) return rc;
    }
    hipLaunchKernelGGL(wide_finish_kernel, dim3(nb), dim3(256), 0, s, a, cost, command, error, xhat);
    if ((rc = launch_check("wide_finish_kernel"))) return rc;
    return launch_loss_reduce(cost, d->B, d->B, loss, s);
}

int wide_backward(const fcr_dims *d, const Terms &tm, const float *X, const float *states, const float *prediction,
                  const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, char *base,
                  size_t ws_bytes, hipStream_t s) {
    const WideLayout L = make_wide(d, 1, wide_keep_fit(d, ws_bytes));
    const int B = d->B, nb = (B + 255) / 256;
    int rc;
    WideArgs a = wide_args(d, L, base);
    a.tm = tm;
    a.X = X;
    a.states = states;
    a.pred = (float *)prediction;
    a.dloss = dloss;
    if (hipMemsetAsync(a.rowg, 0, sizeof(float) * (size_t)(d->N + kL - 1) * B * kIn, s) != hipSuccess)
        return fail(FCR_EHIP, "hipMemsetAsync failed");
    const WbBufs wb = wb_bufs(L, base, B);
    for (int j = d->N - 1; j >= 0; --j) {
        hipLaunchKernelGGL(wide_head_kernel, dim3((unsigned)(((size_t)B * kRoLanes + 255) / 256)), dim3(256), 0, s, a, j,
                           wb.RMh);   // slot 0 of parity (9 + 1) & 1 = 0: layer 2's t = 9 reads it
        if ((rc = launch_check("wide_head_kernel"))) return rc;
        if (j >= d->N - L.keep) {   // kept by the forward: no recompute
            a.Act = kept_act(L, base, d, j);
            a.Cs = kept_c(L, base, d, j);
        } else {
            a.Act = (float *)(base + L.Act);
            a.Cs = (float *)(base + L.Cs);
            hipLaunchKernelGGL(wide_window_kernel<false>, dim3(nb), dim3(256), 0, s, a, j);
            if ((rc = launch_check("wide_window_kernel"))) return rc;
            if ((rc = wide_window_cells(a, L, base, true, s))) return rc;   // checkpoint: recompute the window
        }
        for (int l = kLayers - 1; l >= 0; --l)
            for (int t = kL - 1; t >= 0; --t)   // layer 0's window-row gradient into rowg row j + t
                if ((rc = launch_fb(wb_cell(wb, l, t, a.Act, a.Cs, a.rowg + (size_t)(j + t) * B * kIn, nullptr), l == 0, s)))
                    return rc;
    }
    hipLaunchKernelGGL(wide_gu0_kernel, dim3(nb), dim3(256), 0, s, a, g_u0);
    if ((rc = launch_check("wide_gu0_kernel"))) return rc;
    return launch_ctrl_grads(d, tm, a.xhat, a.dv, (const float *)(base + L.fnp), (float *)(base + L.fnn_part), L.ctrl_blocks,
                             g_w_inp, g_b_inp, g_w_out, s);
}

size_t surw_workspace(const fcr_dims *d, int with_backward) { return make_surw(d, with_backward).total; }

int surw_forward(const fcr_dims *d, const fcr_weights *w, const float *x, float *y, int with_backward, char *base,
                 hipStream_t s) {
    const SurWideLayout L = make_surw(d, with_backward);
    const int B = d->B, Hp = L.Hp;
    int rc;
    // range guard of the window columns from the batch itself (as the H <= 52 step: u0 = x, fcr_pack.h)
    if ((rc = launch_range(d, x, x, nullptr, w->fc_w, w->fc_b, (float *)(base + L.rng), (float *)(base + L.wsc), s)))
        return rc;
    hipLaunchKernelGGL(sur_window_rec_kernel, dim3((unsigned)((B * kL + 255) / 256)), dim3(256), 0, s, x,
                       (const float *)(base + L.wsc), B, (_Float16 *)(base + L.WR), (float *)(base + L.xt));
    if ((rc = launch_check("sur_window_rec_kernel"))) return rc;
    if ((rc = wide_pack(w, d->H, L, kPkFw | kPkFc, base, (const float *)(base + L.wsc), s))) return rc;
    WideArgs a{};
    a.B = B;
    a.N = 1;
    a.H = Hp;
    a.Cs = (float *)(base + L.Cs);
    a.Act = with_backward ? (float *)(base + L.Act) : nullptr;
    a.Hs = (float *)(base + L.Hs);
    a.wr = (_Float16 *)(base + L.WR);
    if ((rc = wide_cells(a, L, base, (_Float16 *)(base + L.HR), kLayers, with_backward != 0, s))) return rc;
    hipLaunchKernelGGL(surrogate::readout_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const float *)a.Hs,
                       (const float *)(base + L.fcw), w->fc_b, y, B, Hp);
    return launch_check("readout_kernel");
}

int surw_backward(const fcr_dims *d, const fcr_weights *w, const float *dy, float *const *g_w_ih, float *const *g_w_hh,
                  float *g_fc_w, float *g_fc_b, float *g_x, char *base, hipStream_t s) {
    const SurWideLayout L = make_surw(d, 1);
    const int B = d->B, H = d->H, Hp = L.Hp;
    const size_t cell = (size_t)B * Hp;
    int rc;
    auto grid = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // the backward's packs (the forward's split weights and padded fc.W are still in ws)
    if ((rc = wide_pack(w, H, L, kPkBwd, base, nullptr, s))) return rc;
    const float *Hs = (const float *)(base + L.Hs), *fcw = (const float *)(base + L.fcw);
    // readout: d fc.W = dy^T h_9 (fixed batch slices), d fc.b = sum dy, dh_9 = dy fc.W (its row bound: slot 0)
    const int b_per = (B + kSurFcSlices - 1) / kSurFcSlices;
    float *fcpart = (float *)(base + L.fcpart);
    hipLaunchKernelGGL(fc_wgrad_part_kernel, dim3((unsigned)((Hp + 255) / 256), kSurFcSlices), dim3(256), 0, s, dy, Hs, B,
                       Hp, b_per, fcpart);
    hipLaunchKernelGGL(fc_wgrad_sum_kernel, grid((size_t)kOut * H), dim3(256), 0, s, (const float *)fcpart,
                       kSurFcSlices, H, Hp, g_fc_w);
    hipLaunchKernelGGL(surrogate::bias_grad_kernel, dim3(kOut), dim3(surrogate::kSurBlock), 0, s, dy, g_fc_b, B);
    const WbBufs wb = wb_bufs(L, base, B);
    hipLaunchKernelGGL(sur_head_kernel, grid(cell), dim3(256), 0, s, dy, fcw, B, Hp, wb.dH);
    hipLaunchKernelGGL(row_absmax_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, (const float *)wb.dH, Hp, 0, B,
                       wb.RMh);
    if ((rc = launch_check("readout backward"))) return rc;
    float *rowg = (float *)(base + L.rowg), *dG = (float *)(base + L.dG);
    float *part = (float *)(base + L.part);
    const float *Cs = (const float *)(base + L.Cs), *Act = (const float *)(base + L.Act);
    const _Float16 *HR = (const _Float16 *)(base + L.HR);
    if (hipMemsetAsync(rowg, 0, sizeof(float) * kL * B * kIn, s) != hipSuccess) return fail(FCR_EHIP, "hipMemsetAsync failed");
    for (int l = kLayers - 1; l >= 0; --l) {
        for (int t = kL - 1; t >= 0; --t)   // rowg row t: dL/dx of window row t; the cells' dgates into dG
            if ((rc = launch_fb(wb_cell(wb, l, t, Act, Cs, rowg + (size_t)t * B * kIn, dG), l == 0, s))) return rc;
        // the layer's weight gradients over all (step, sample) rows: x_t = the window rows (layer 0, fp32) or the
        // layer below's h records; h_{t-1} = this layer's records of steps 0..8 against the dgates of steps 1..9
        const long long n10 = (long long)kL * B, n9 = (long long)(kL - 1) * B;
        if ((rc = surw_wgrad(dG, n10, Hp, H, l == 0 ? kIn : H, l == 0 ? (const float *)(base + L.xt) : nullptr, kIn,
                             l == 0 ? nullptr : HR + (size_t)(l - 1) * kL * B * 2 * Hp, part, L.part_floats, g_w_ih[l],
                             s)))
            return rc;
        if ((rc = surw_wgrad(dG + (size_t)B * 4 * Hp, n9, Hp, H, H, nullptr, 0, HR + (size_t)l * kL * B * 2 * Hp, part,
                             L.part_floats, g_w_hh[l], s)))
            return rc;
    }
    if (g_x) {   // the window-row gradients [t][B][5] -> (B, 10, 5)
        const long long nx = (long long)B * kL * kIn;
        hipLaunchKernelGGL(surrogate::window_transpose_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s,
                           (const float *)rowg, g_x, B, kIn, true);
        if ((rc = launch_check("window_transpose_kernel"))) return rc;
    }
    return FCR_OK;
}

size_t cell_hook_workspace(int B, int H, int layer0) { return cell_hook_layout(B, H, layer0).total; }

// One backward cell of the H > 52 path exactly as wide_backward launches it (launch_fb, fcr_wbwd.h), on caller-given
// inputs: the standalone form the per-element tests of tests/test_wide_cell.py compare with an fp64 product
int wide_bwd_cell_hook(int B, int H, int layer0, const float *w_ih, const float *w_hh, const float *act,
                       const float *c_prev, const float *dh, const float *din, const float *dc, float *out,
                       float *dc_out, float *rowg, char *base, hipStream_t s) {
    const CellHookLayout L = cell_hook_layout(B, H, layer0);
    // the cell's packs as a workspace's (wide_pack), at Hp = H: the given weights stand for layer 0 or a layer above it
    const int l = layer0 ? 0 : 1;
    fcr_weights w{};
    w.w_ih[l] = w_ih;
    w.w_hh[l] = w_hh;
    WideShared S{};
    S.Hp = H;
    S.bt[l] = L.bt;
    S.w0p = L.w0;
    int rc = wide_pack(&w, H, S, (kPkBt << l) | (layer0 ? kPkW0 : 0), base, nullptr, s);
    if (rc) return rc;
    float *rm = (float *)(base + L.rm);
    float *rm_c = rm, *rm_h = rm + B, *rm_d = rm + 2 * (size_t)B;
    const dim3 rg((unsigned)((B + 3) / 4)), rb(256);
    hipLaunchKernelGGL(row_absmax_kernel, rg, rb, 0, s, dc, H, H, B, rm_c);
    hipLaunchKernelGGL(row_absmax_kernel, rg, rb, 0, s, dh, H, H, B, rm_h);
    if (din) hipLaunchKernelGGL(row_absmax_kernel, rg, rb, 0, s, din, H, H, B, rm_d);
    if ((rc = launch_check("row_absmax_kernel"))) return rc;
    // the cell reads and writes k8 rows: the caller's rows are converted around it
    float *rows = (float *)(base + L.rows);
    const size_t cell = (size_t)B * H;
    auto to_k8 = [&](const float *src, float *dst) -> const float * {
        if (!src) return nullptr;
        hipLaunchKernelGGL(k8_rows_kernel, dim3((unsigned)((cell + 255) / 256)), dim3(256), 0, s, src, B, H, H, dst, 1);
        return dst;
    };
    WbArgs wa{};
    wa.A = (const _Float16 *)(base + L.bt);
    wa.NB = B;
    wa.H = H;
    wa.act = act;
    wa.c_prev = to_k8(c_prev, rows);
    wa.dh = to_k8(dh, rows + cell);
    wa.din = to_k8(din, rows + 2 * cell);
    wa.dC = to_k8(dc, rows + 3 * cell);
    wa.dC_out = rows + 4 * cell;
    if ((rc = launch_check("k8_rows_kernel"))) return rc;
    wa.rm_c = rm_c;
    wa.rm_h = rm_h;
    wa.rm_d = din ? rm_d : nullptr;
    wa.nrh = 1;
    wa.nrd = 1;
    wa.out = rows + 5 * cell;
    wb_outputs(wa, layer0 != 0, H, c_prev != nullptr);
    if (layer0) {   // and the window-row gradient
        if (hipMemsetAsync(rowg, 0, sizeof(float) * kIn * (size_t)B, s) != hipSuccess)
            return fail(FCR_EHIP, "hipMemsetAsync failed");
        wa.wih0 = (const float *)(base + L.w0);
        wa.rowg = rowg;
    }
    if ((rc = launch_fb(wa, layer0 != 0, s))) return rc;
    hipLaunchKernelGGL(k8_rows_kernel, dim3((unsigned)((cell + 255) / 256)), dim3(256), 0, s, (const float *)wa.dC_out, B,
                       H, H, dc_out, 0);
    if (wa.NO > 0)
        hipLaunchKernelGGL(k8_rows_kernel, dim3((unsigned)(((size_t)B * wa.NO + 255) / 256)), dim3(256), 0, s,
                           (const float *)wa.out, B, wa.NO, layer0 ? H : 2 * H, out, 0);
    return launch_check("k8_rows_kernel");
}

}  // namespace fcr

#if FCR_WB_STAMP
extern "C" {
// diagnostic builds only (scripts/stamp_wb.py): the fused backward cell's section sums (fcr_wbwd.h), then zeroed
int fcr_debug_wb_stamp(unsigned long long *out16) {
    using namespace fcr;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(fcr_wb_stamp), 16 * sizeof(unsigned long long)) != hipSuccess)
        return FCR_EHIP;
    static const unsigned long long zero[16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(fcr_wb_stamp), zero, sizeof(zero)) == hipSuccess ? FCR_OK : FCR_EHIP;
}
}  // extern "C"
#endif
