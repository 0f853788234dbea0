// fcr_host.h — host-side declarations shared by the library's translation units. Each .hip file compiles the kernels
// of one family and the host code that launches them:
//   fcr_abi.hip      the C ABI (include/fcr.h): argument checks, process defaults, the controller (fcr_fnn.h)
//   fcr_rollout.hip  the H <= 52 rollout (fused, small-batch, pipelined kernels), the H <= 52 surrogate step
//                    (fcr_sur.h), the backward of its free run (fcr_lro_bwd.h) and the kernels every engine shares
//                    (fcr_shared_kernels.h)
//   fcr_wide.hip     the H > 52 rollout, the H > 52 surrogate step and the fcr_wide_bwd_cell test hook
//   fcr_rows.hip     plant, closed loop and bank, feasibility projection, window gather, the supervised baseline's epoch
//   fcr_grad.hip     the press's adjoint: vector-Jacobian products of the plant rollout and the closed loop
//   fcr_train.hip    the bank's adjoint and the fused loss on the press; fcr_mpc.hip the MPC baseline
//   fcr_press_noise.hip  the kernels of training under noise; launched from fcr_rows.hip and fcr_train.hip through
//                    fcr_press_noise_host.h
// What one file needs of another goes through the functions below. The argument checks fcr_rows.hip and fcr_grad.hip
// share, and their choice of a kernel instantiation from run-time flags, are in the host-only fcr_press_host.h: it
// includes fcr_plant.h, so only those two files include it.
// (The H <= 52 surrogate's kernels stay with the rollout's: compiled in a file of their own, sur_fwd_kernel<13> and
// sur_bwd_kernel come out with another instruction schedule and register allocation — they inline the same cell
// functions as fcr_fwd_kernel / fcr_bwd_kernel, and the compiler's order of doing so follows what else is in the file.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "fcr.h"
#include "fcr_common.h"

namespace fcr {

// ---- fcr_abi.hip ----
// Record a message in the thread-local last-error buffer (fcr_last_error) and return `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// FCR_OK, or FCR_EHIP with the launch error of the kernel just enqueued.
int launch_check(const char *what);
// hipFuncSetAttribute(max dynamic LDS) once per (kernel instantiation, device); `done`: the caller's static mask
int lds_attr(const void *fn, int bytes, std::atomic<unsigned long long> &done, const char *what);
// process-wide defaults of the per-call options (fcr_set_small_batch_limit, fcr_set_small_pipe_limit,
// fcr_set_small_pipe_sets, fcr_set_wide_keep_budget)
extern std::atomic<int> g_small_max_batch, g_pipe_max_batch, g_pipe_sets;
extern std::atomic<long long> g_wide_keep_budget;

// Kernels are instantiated for 4, 8 and 13 unit slots (H <= 16, 32, 52); a smaller H runs in the next
// tier with its padding units' weights zero — their gates stay at i = f = o = 1/2, g = 0, so c = h = 0
// and they add nothing to any product (tests/test_gpu_parity.py: H = 40 against the oracle).
constexpr int kMaxSlots = 13;
constexpr int kMaxWideH = 2048;   // H > 4*kMaxSlots: the GEMM-per-cell path (fcr_wide.h)
inline bool is_wide(const fcr_dims *d) { return d->H > 4 * kMaxSlots; }
inline int slot_tier(int H) { return H <= 16 ? 4 : (H <= 32 ? 8 : 13); }
// the kernel family a call ran, reported in its options (FCR_KERNELS_*)
inline void note_kernels(fcr_options *o, int family) {
    if (o) o->kernels = family;
}

// A workspace layout: slabs handed out in call order, each 256-byte aligned; `off` ends as the total
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
struct Arena {
    size_t off = 0;
    size_t operator()(size_t bytes) {
        const size_t o = off;
        off += align_up(bytes);
        return o;
    }
};

// ---- fcr_rollout.hip ----
// The H <= 52 weight packs as the rollout and the surrogate lay them out, first in their workspaces: split-f16
// forward fragments and (with a backward) images per layer, the readout, the controller records, the window-column
// scales and the range guard's partials
struct PackedLayout {
    int HS;
    size_t fa[3], img[3], fcp, fcb, fnp, wsc, rng;
};
void take_packed(Arena &take, PackedLayout &P, bool with_backward);
Packed packed_ptrs(const PackedLayout &P, char *base);
// window-column scales of the f16 split's range guard (fcr_pack.h) -> wsc[8], from the call's inputs
int launch_range(const fcr_dims *d, const float *states, const float *u0, const float *noise, const float *fcw,
                 const float *fcb, float *part, float *wsc, hipStream_t s);
// every pack of PackedLayout in one launch (CH = 0: no controller); clear: nclear words zeroed by the same launch, or null
int launch_pack_all(const fcr_weights *w, int H, int CH, const PackedLayout &P, bool with_backward, char *base,
                    unsigned *clear, int nclear, hipStream_t s);
// the controller records alone (the H > 52 rollout: ctrl_grad_kernel reads fnp; fcp / fcbo are scratch of 52 units)
int launch_pack_ctrl(const fcr_weights *w, int CH, float *fcp, float *fcbo, float *fnp, hipStream_t s);
// loss = sum(part[0..n)) / B in fixed order
int launch_loss_reduce(const float *part, int n, int B, float *loss, hipStream_t s);
// The controller's weight gradients from the backward's dv: per-block partials, then their fixed-order sum
int launch_ctrl_grads(const fcr_dims *d, const Terms &tm, const float *xhat, const float *dv, const float *fnp, float *part,
                      int ctrl_blocks, float *g_w_inp, float *g_b_inp, float *g_w_out, hipStream_t s);
int launch_grad_reduce(const float *part, int blocks, int hidden, float *g_w_inp, float *g_b_inp, float *g_w_out,
                       hipStream_t s);
// M stacked controllers (blockIdx.y = model): model m's `blocks` partials -> row m of the stacked gradients
int launch_grad_reduce_many(const float *part, int blocks, int hidden, int n_models, float *g_w_inp, float *g_b_inp,
                            float *g_w_out, hipStream_t s);
int pipe_max_sets();   // the most window sets the pipelined forward runs (fcr_pipe.h)
size_t rollout_workspace(const fcr_dims *d, int with_backward);
// tm: the loss's terms as the kernels take them (fcr_common.h; resolved and checked by fcr_abi.hip)
int rollout_forward(const fcr_dims *d, fcr_options *opts, const Terms &tm, const fcr_weights *w, const float *X, const float *u0,
                    const float *states, const float *noise, float *loss, float *cost, float *command, float *error,
                    float *prediction, float *xhat, int with_backward, char *base, hipStream_t s);
int rollout_backward(const fcr_dims *d, fcr_options *opts, const Terms &tm, const float *X, const float *states, const float *prediction,
                     const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, char *base,
                     hipStream_t s);
// M controllers side by side through the one-workgroup small-batch kernels (fcr_small.h, MANY); d->B = one model's batch
bool many_supported(const fcr_dims *d);   // slot tier 8 or 13
size_t many_workspace(const fcr_dims *d, int n_models, int with_backward);
int many_forward(const fcr_dims *d, int n_models, const Terms &tm, const fcr_weights *w, const float *X, const float *u0,
                 const float *states, const float *noise, float *loss, float *cost, float *command, float *error,
                 float *prediction, float *xhat, int with_backward, char *base, hipStream_t s);
int many_backward(const fcr_dims *d, int n_models, const Terms &tm, const float *X, const float *states, const float *prediction,
                  const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, char *base,
                  hipStream_t s);

// ---- fcr_wide.hip ----
size_t wide_workspace(const fcr_dims *d, int with_backward, int keep);
// The number of kept windows a workspace of ws_bytes holds (the most that fit): the forward and the
// backward each derive it from the ws_bytes they are given, so they agree with no state between them.
int wide_keep_fit(const fcr_dims *d, size_t ws_bytes);
long long wide_default_cap();
int wide_forward(const fcr_dims *d, const Terms &tm, const fcr_weights *w, const float *X, const float *u0, const float *states,
                 const float *noise, float *loss, float *cost, float *command, float *error, float *prediction,
                 float *xhat, int with_backward, char *base, size_t ws_bytes, hipStream_t s);
int wide_backward(const fcr_dims *d, const Terms &tm, const float *X, const float *states, const float *prediction,
                  const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, char *base,
                  size_t ws_bytes, hipStream_t s);
size_t surw_workspace(const fcr_dims *d, int with_backward);
int surw_forward(const fcr_dims *d, const fcr_weights *w, const float *x, float *y, int with_backward, char *base,
                 hipStream_t s);
int surw_backward(const fcr_dims *d, const fcr_weights *w, const float *dy, float *const *g_w_ih, float *const *g_w_hh,
                  float *g_fc_w, float *g_fc_b, float *g_x, char *base, hipStream_t s);
size_t cell_hook_workspace(int B, int H, int layer0);
int wide_bwd_cell_hook(int B, int H, int layer0, const float *w_ih, const float *w_hh, const float *act,
                       const float *c_prev, const float *dh, const float *din, const float *dc, float *out,
                       float *dc_out, float *rowg, char *base, hipStream_t s);

// the H <= 52 surrogate step
size_t sur_workspace(const fcr_dims *d, int with_backward);
int sur_forward(const fcr_dims *d, const fcr_weights *w, const float *x, float *y, int with_backward, char *base,
                hipStream_t s);
int sur_backward(const fcr_dims *d, const float *dy, float *const *g_w_ih, float *const *g_w_hh, float *g_fc_w,
                 float *g_fc_b, float *g_x, char *base, hipStream_t s);

// the H <= 52 surrogate's command-driven rollout (fcr_lstm_rollout.h); gain: host float[4] or null (= 1)
size_t lro_workspace(const fcr_dims *d);
int lro_forward(const fcr_dims *d, const fcr_weights *w, const float *window0, const float *cmd, const float *gain,
                const float *noise, float *xhat, char *base, hipStream_t s);

// backward of lro_forward (fcr_lro_bwd.h); out: the caller's fcr_lstm_rollout_grads
bool lro_bwd_fits(const fcr_dims *d);   // T x (B rounded up to 16) windows within the surrogate step's index range
size_t lro_bwd_workspace(const fcr_dims *d);
int lro_backward(const fcr_dims *d, const fcr_weights *w, const float *window0, const float *cmd, const float *gain,
                 const float *xhat, const float *g_xhat, const fcr_lstm_rollout_grads *out, char *base, hipStream_t s);

}  // namespace fcr
