// fcr_abi.hip — the C ABI (include/fcr.h) of the gfx950 rollout engine: every extern "C" entry point with its
// argument checks, the last-error buffer, the process-wide defaults, and the controller's own kernels (fcr_fnn.h).
// The engines behind the entry points are one translation unit per kernel family (fcr_host.h): fcr_rollout.hip
// (H <= 52 rollout and surrogate), fcr_wide.hip (H > 52 rollout and surrogate, the cell test hook); the plant,
// closed-loop and window entry points are in fcr_rows.hip.
//
// Replaces the torch work behind `loss_function(...)` / `loss.backward()` at the reference's
// Unsupervised Learning/Functions.py:646 and :655. All launches are stream-ordered on the caller's stream; nothing
// here allocates or synchronises.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "fcr.h"
#include "fcr_common.h"
#include "fcr_fnn.h"
#include "fcr_host.h"

namespace fcr {

thread_local char g_err[512] = "no error";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int launch_check(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FCR_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return FCR_OK;
}

// hipFuncSetAttribute(max dynamic LDS) once per (kernel instantiation, device): one bit per device in the caller's
// static mask. The mask is atomic (calls on several threads are allowed, include/fcr.h), two first calls that race
// both set the attribute (idempotent), and a second device in the process gets its own bit (devices past 63 set
// it on every call).
int lds_attr(const void *fn, int bytes, std::atomic<unsigned long long> &done, const char *what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    const unsigned long long bit = (dev >= 0 && dev < 64) ? 1ull << dev : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return FCR_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return fail(FCR_EHIP, "hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
    done.fetch_or(bit, std::memory_order_release);
    return FCR_OK;
}

// process-wide defaults of the per-call options (fcr_host.h)
std::atomic<int> g_small_max_batch{8192};
std::atomic<int> g_pipe_max_batch{512};
std::atomic<int> g_pipe_sets{0};
// fcr_set_wide_keep_budget: bytes of kept windows fcr_workspace_size may add; < 0 = the default policy
// (wide_default_cap). The process-wide default of fcr_options.wide_keep_budget.
std::atomic<long long> g_wide_keep_budget{-1};

namespace {

// The checks every entry point makes of its workspace, in this order
int check_ws(const char *name, const void *ws, size_t ws_bytes, size_t need) {
    if (((uintptr_t)ws) & 255) return fail(FCR_EINVAL, "%s: ws must be 256-byte aligned", name);
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "%s: ws has %zu bytes, needs %zu", name, ws_bytes, need);
    return FCR_OK;
}

int check_dims(const fcr_dims *d) {
    if (!d) return fail(FCR_EINVAL, "dims is NULL");
    if (d->B < 1) return fail(FCR_EINVAL, "B=%d must be >= 1", d->B);
    if (d->N < 1) return fail(FCR_EINVAL, "N=%d must be >= 1", d->N);
    if (d->L != kL) return fail(FCR_EUNSUPPORTED, "L=%d: the rollout window is fixed at 10 rows", d->L);
    if (d->layers != kLayers) return fail(FCR_EUNSUPPORTED, "layers=%d: built for 3", d->layers);
    if (d->in_dim != kIn || d->out_dim != kOut || d->ctrl_in != kCtrlIn)
        return fail(FCR_EUNSUPPORTED, "in/out/ctrl_in = %d/%d/%d: built for 5/4/3", d->in_dim,
                    d->out_dim, d->ctrl_in);
    if (d->ctrl_hidden < 1 || d->ctrl_hidden > 4 * kMS)
        return fail(FCR_EUNSUPPORTED, "ctrl_hidden=%d: built for 1..52", d->ctrl_hidden);
    if (d->H < 1 || d->H > kMaxWideH)
        return fail(FCR_EUNSUPPORTED, "H=%d: built for 1..%d", d->H, kMaxWideH);
    if ((long long)d->B * d->N > (1LL << 31)) return fail(FCR_EINVAL, "B*N too large");
    if (d->precision == 2)
        return fail(FCR_EUNSUPPORTED, "precision=2 (f16 forward, fp32-accurate backward) is retired: it ran 1.08x the "
                    "fp32 step at the f16 mode's accuracy; use FCR_PRECISION_F16 (1) or FCR_PRECISION_FP32 (0)");
    if (d->precision != FCR_PRECISION_FP32 && d->precision != FCR_PRECISION_F16)
        return fail(FCR_EINVAL, "precision=%d: FCR_PRECISION_FP32 (0) or FCR_PRECISION_F16 (1)", d->precision);
    if (d->precision != FCR_PRECISION_FP32 && is_wide(d))
        return fail(FCR_EUNSUPPORTED, "reduced precision is built for H <= %d (the fused kernels)", 4 * kMaxSlots);
    return FCR_OK;
}

long long keep_budget_of(const fcr_options *o) {
    if (o && o->wide_keep_budget != FCR_OPT_INHERIT) return o->wide_keep_budget < 0 ? -1 : o->wide_keep_budget;
    return g_wide_keep_budget.load();
}

int check_lstm_dims(const fcr_dims *d) {
    if (!d) return fail(FCR_EINVAL, "dims is NULL");
    if (d->B < 1) return fail(FCR_EINVAL, "B=%d must be >= 1", d->B);
    if (d->L != kL) return fail(FCR_EUNSUPPORTED, "L=%d: the window is fixed at 10 rows", d->L);
    if (d->layers != kLayers) return fail(FCR_EUNSUPPORTED, "layers=%d: built for 3", d->layers);
    if (d->in_dim != kIn || d->out_dim != kOut)
        return fail(FCR_EUNSUPPORTED, "in/out = %d/%d: built for 5/4", d->in_dim, d->out_dim);
    if (d->H < 1 || d->H > kMaxWideH) return fail(FCR_EUNSUPPORTED, "H=%d: built for 1..%d", d->H, kMaxWideH);
    if ((long long)d->B * kL * 4 * d->H > (1LL << 40)) return fail(FCR_EINVAL, "B*H too large");
    return FCR_OK;
}

// fcr_lstm_rollout: the fcr_lstm_* convention with N = T steps; B = 0 is a no-op, so it passes
int check_lro_dims(const fcr_dims *d) {
    if (!d) return fail(FCR_EINVAL, "dims is NULL");
    if (d->B < 0) return fail(FCR_EINVAL, "B=%d must be >= 0", d->B);
    if (d->N < 1) return fail(FCR_EINVAL, "N=%d (the steps T) must be >= 1", d->N);
    if (d->L != kL) return fail(FCR_EUNSUPPORTED, "L=%d: the window is fixed at 10 rows", d->L);
    if (d->layers != kLayers) return fail(FCR_EUNSUPPORTED, "layers=%d: built for 3", d->layers);
    if (d->in_dim != kIn || d->out_dim != kOut)
        return fail(FCR_EUNSUPPORTED, "in/out = %d/%d: built for 5/4", d->in_dim, d->out_dim);
    if (d->H < 1 || is_wide(d))
        return fail(FCR_EUNSUPPORTED, "H=%d: the surrogate rollout is built for 1..%d (the fused cells)", d->H, 4 * kMaxSlots);
    if (d->precision != FCR_PRECISION_FP32)
        return fail(FCR_EUNSUPPORTED, "precision=%d: the surrogate rollout runs FCR_PRECISION_FP32 (0) only", d->precision);
    if ((long long)d->B * d->N > (1LL << 31)) return fail(FCR_EINVAL, "B*N too large");
    return FCR_OK;
}

// fcr_loss_terms -> the kernels' Terms (fcr_common.h), checked before any launch. many: d->B is one model's batch
// and X is stacked (M,B,3), so the default reference's model stride is 3 B.
int resolve_terms(const char *what, const fcr_dims *d, const fcr_loss_terms *t, const float *X, bool many, Terms *out) {
    if (!t) return fail(FCR_EINVAL, "%s: terms is NULL", what);
    Terms tm{};
    tm.row = TermRow{t->alpha, t->p1_lo, t->p1_hi, t->p2_lo, t->p2_hi, t->w_con};
    if (!(many && t->table)) {   // (a table's values live on the device: the caller's to check, include/fcr.h)
        if (!(t->alpha - t->alpha == 0.0f)) return fail(FCR_EINVAL, "%s: terms.alpha=%g must be finite", what, t->alpha);
        if (t->p1_lo != t->p1_lo || t->p1_hi != t->p1_hi || t->p2_lo != t->p2_lo || t->p2_hi != t->p2_hi ||
            t->w_con != t->w_con)
            return fail(FCR_EINVAL, "%s: a loss term is NaN (p1 [%g, %g], p2 [%g, %g], w_con %g)", what, t->p1_lo, t->p1_hi,
                        t->p2_lo, t->p2_hi, t->w_con);
        if (t->p1_lo > t->p1_hi) return fail(FCR_EINVAL, "%s: terms.p1_lo=%g is above p1_hi=%g", what, t->p1_lo, t->p1_hi);
        if (t->p2_lo > t->p2_hi) return fail(FCR_EINVAL, "%s: terms.p2_lo=%g is above p2_hi=%g", what, t->p2_lo, t->p2_hi);
        if (t->w_con < 0.0f || !(t->w_con - t->w_con == 0.0f))
            return fail(FCR_EINVAL, "%s: terms.w_con=%g must be finite and >= 0", what, t->w_con);
    }
    if (many && t->table) {
        if (t->table_stride < 0) return fail(FCR_EINVAL, "%s: terms.table_stride=%lld must be >= 0", what, (long long)t->table_stride);
        tm.table = t->table;
        tm.table_stride = t->table_stride;
    }
    if (t->ref) {
        if (t->ref_stride_b < 0 || t->ref_stride_j < 0 || (many && t->ref_stride_m < 0))
            return fail(FCR_EINVAL, "%s: terms.ref strides must be >= 0", what);
        tm.ref = t->ref;
        tm.ref_b = t->ref_stride_b;
        tm.ref_j = t->ref_stride_j;
        tm.ref_m = many ? t->ref_stride_m : 0;
    } else {
        tm.ref = X + (kCtrlIn - 1);   // Functions.py:1392: X[:, -1] in every step
        tm.ref_b = kCtrlIn;
        tm.ref_j = 0;
        tm.ref_m = many ? (long long)kCtrlIn * d->B : 0;
    }
    *out = tm;
    return FCR_OK;
}

int lstm_weights_ok(const fcr_weights *w) {
    if (!w || !w->fc_w || !w->fc_b) return 0;
    for (int l = 0; l < kLayers; ++l)
        if (!w->w_ih[l] || !w->w_hh[l]) return 0;
    return 1;
}

int cell_hook_check(int B, int H) {
    if (B < 1) return fail(FCR_EINVAL, "fcr_wide_bwd_cell: B=%d", B);
    if (H < 8 || H % 8 || H > kMaxWideH)
        return fail(FCR_EUNSUPPORTED, "fcr_wide_bwd_cell: H=%d off the fused cell's tiling (a multiple of 8)", H);
    return FCR_OK;
}

}  // namespace
}  // namespace fcr

using namespace fcr;

extern "C" {

const char *fcr_last_error(void) { return g_err; }

int fcr_abi_version(void) { return FCR_ABI_VERSION; }

int fcr_set_small_batch_limit(int32_t max_batch) {
    return g_small_max_batch.exchange(max_batch < 0 ? 0 : max_batch);
}

int fcr_get_small_batch_limit(void) { return g_small_max_batch.load(); }
int fcr_set_small_pipe_limit(int32_t max_batch) { return g_pipe_max_batch.exchange(max_batch < 0 ? 0 : max_batch); }
int fcr_get_small_pipe_limit(void) { return g_pipe_max_batch.load(); }
int fcr_set_small_pipe_sets(int32_t sets) {
    return g_pipe_sets.exchange(sets < 0 ? 0 : (sets > pipe_max_sets() ? pipe_max_sets() : sets));
}
int fcr_get_small_pipe_sets(void) { return g_pipe_sets.load(); }

int64_t fcr_set_wide_keep_budget(int64_t bytes) {
    return g_wide_keep_budget.exchange(bytes < 0 ? -1 : bytes);
}

int64_t fcr_get_wide_keep_budget(void) { return g_wide_keep_budget.load(); }

int fcr_wide_kept_windows(const fcr_dims *dims, size_t ws_bytes, int32_t *kept) {
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!kept) return fail(FCR_EINVAL, "kept is NULL");
    *kept = is_wide(dims) ? wide_keep_fit(dims, ws_bytes) : 0;
    return FCR_OK;
}

int fcr_wide_bwd_cell_workspace(int32_t B, int32_t H, int32_t layer0, size_t *bytes) {
    if (const int rc = cell_hook_check(B, H)) return rc;
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    *bytes = cell_hook_workspace(B, H, layer0);
    return FCR_OK;
}

int fcr_wide_bwd_cell(int32_t B, int32_t H, int32_t layer0, const float *w_ih, const float *w_hh, const float *act,
                      const float *c_prev, const float *dh, const float *din, const float *dc, float *out,
                      float *dc_out, float *rowg, void *ws, size_t ws_bytes, void *stream) {
    if (const int rc = cell_hook_check(B, H)) return rc;
    if (!w_hh || !act || !dh || !dc || !dc_out || !ws || (!layer0 && !w_ih) || (layer0 && (!w_ih || !rowg)) ||
        ((c_prev || !layer0) && !out))
        return fail(FCR_EINVAL, "fcr_wide_bwd_cell: a required pointer is NULL");
    if (const int rc = check_ws("fcr_wide_bwd_cell", ws, ws_bytes, cell_hook_workspace(B, H, layer0))) return rc;
    return wide_bwd_cell_hook(B, H, layer0, w_ih, w_hh, act, c_prev, dh, din, dc, out, dc_out, rowg, (char *)ws,
                              (hipStream_t)stream);
}

int fcr_workspace_size(const fcr_dims *dims, const fcr_options *opts, int with_backward, size_t *bytes) {
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    if (!is_wide(dims)) {
        *bytes = rollout_workspace(dims, with_backward);
        return FCR_OK;
    }
    int keep = 0;
    if (with_backward) {   // kept windows within the budget (fcr_set_wide_keep_budget)
        const size_t base = wide_workspace(dims, 1, 0);
        long long budget = keep_budget_of(opts);
        if (budget < 0) {   // default: the whole workspace within wide_default_cap()
            const long long cap = wide_default_cap();
            budget = cap > (long long)base ? cap - (long long)base : 0;
        }
        while (keep < dims->N && wide_workspace(dims, 1, keep + 1) - base <= (size_t)budget) ++keep;
    }
    *bytes = wide_workspace(dims, with_backward, keep);
    return FCR_OK;
}

void fcr_loss_terms_default(fcr_loss_terms *t, float alpha) {
    if (!t) return;
    *t = fcr_loss_terms{};
    t->alpha = alpha;
    t->p1_hi = kP1Max;
    t->p2_hi = kP2Max;
    t->w_con = 1.0f;
}

int fcr_forward(const fcr_dims *d, fcr_options *opts, const fcr_weights *w, const float *X, const float *u0,
                const float *states, const float *noise, float *loss, float *cost, float *command,
                float *error, float *prediction, float *xhat, int with_backward, void *ws,
                size_t ws_bytes, void *stream) {
    if (const int rc = check_dims(d)) return rc;
    fcr_loss_terms t;
    fcr_loss_terms_default(&t, d->alpha);
    return fcr_forward_terms(d, opts, w, &t, X, u0, states, noise, loss, cost, command, error, prediction, xhat,
                             with_backward, ws, ws_bytes, stream);
}

int fcr_forward_terms(const fcr_dims *d, fcr_options *opts, const fcr_weights *w, const fcr_loss_terms *terms,
                      const float *X, const float *u0, const float *states, const float *noise, float *loss, float *cost,
                      float *command, float *error, float *prediction, float *xhat, int with_backward, void *ws,
                      size_t ws_bytes, void *stream) {
    int rc = check_dims(d);
    if (rc) return rc;
    Terms tm;   // (the terms are checked before the pointers: X is not read, only offset)
    if ((rc = resolve_terms("fcr_forward", d, terms, X, false, &tm))) return rc;
    if (!w || !X || !u0 || !states || !loss || !cost || !command || !error || !prediction || !ws)
        return fail(FCR_EINVAL, "fcr_forward: a required pointer is NULL");
    for (int l = 0; l < kLayers; ++l)
        if (!w->w_ih[l] || !w->w_hh[l])
            return fail(FCR_EINVAL, "fcr_forward: LSTM weight of layer %d is NULL", l);
    if (!w->fc_w || !w->fc_b || !w->ctrl_w_inp || !w->ctrl_b_inp || !w->ctrl_w_out)
        return fail(FCR_EINVAL, "fcr_forward: a weight pointer is NULL");
    if (is_wide(d)) {
        if ((rc = check_ws("fcr_forward", ws, ws_bytes, wide_workspace(d, with_backward, 0)))) return rc;
        note_kernels(opts, FCR_KERNELS_WIDE);
        return wide_forward(d, tm, w, X, u0, states, noise, loss, cost, command, error, prediction, xhat, with_backward,
                            (char *)ws, ws_bytes, (hipStream_t)stream);
    }
    if ((rc = check_ws("fcr_forward", ws, ws_bytes, rollout_workspace(d, with_backward)))) return rc;
    return rollout_forward(d, opts, tm, w, X, u0, states, noise, loss, cost, command, error, prediction, xhat, with_backward,
                           (char *)ws, (hipStream_t)stream);
}

int fcr_backward(const fcr_dims *d, fcr_options *opts, const float *X, const float *states, const float *prediction,
                 const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out,
                 void *ws, size_t ws_bytes, void *stream) {
    if (const int rc = check_dims(d)) return rc;
    fcr_loss_terms t;
    fcr_loss_terms_default(&t, d->alpha);
    return fcr_backward_terms(d, opts, &t, X, states, prediction, dloss, g_u0, g_w_inp, g_b_inp, g_w_out, ws, ws_bytes,
                              stream);
}

int fcr_backward_terms(const fcr_dims *d, fcr_options *opts, const fcr_loss_terms *terms, const float *X,
                       const float *states, const float *prediction, const float *dloss, float *g_u0, float *g_w_inp,
                       float *g_b_inp, float *g_w_out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_dims(d);
    if (rc) return rc;
    Terms tm;
    if ((rc = resolve_terms("fcr_backward", d, terms, X, false, &tm))) return rc;
    if (!X || !states || !prediction || !dloss || !g_u0 || !g_w_inp || !g_b_inp || !g_w_out || !ws)
        return fail(FCR_EINVAL, "fcr_backward: a required pointer is NULL");
    if (is_wide(d)) {
        if ((rc = check_ws("fcr_backward", ws, ws_bytes, wide_workspace(d, 1, 0)))) return rc;
        note_kernels(opts, FCR_KERNELS_WIDE);
        return wide_backward(d, tm, X, states, prediction, dloss, g_u0, g_w_inp, g_b_inp, g_w_out, (char *)ws, ws_bytes,
                             (hipStream_t)stream);
    }
    if ((rc = check_ws("fcr_backward", ws, ws_bytes, rollout_workspace(d, 1)))) return rc;
    return rollout_backward(d, opts, tm, X, states, prediction, dloss, g_u0, g_w_inp, g_b_inp, g_w_out, (char *)ws,
                            (hipStream_t)stream);
}

// The checks of the many-model entries, before any launch: the single call's dims, then what the MANY kernels cover
static int many_check(const char *what, const fcr_dims *d, const fcr_options *o, int32_t n_models) {
    if (const int rc = check_dims(d)) return rc;
    if (n_models < 0) return fail(FCR_EINVAL, "%s: n_models=%d must be >= 0", what, n_models);
    if (n_models > 65535) return fail(FCR_EUNSUPPORTED, "%s: n_models=%d: at most 65535 (a grid dimension)", what, n_models);
    if (d->precision != FCR_PRECISION_FP32)
        return fail(FCR_EUNSUPPORTED, "%s: precision=%d: the many-model kernels run FCR_PRECISION_FP32 (0) only", what,
                    d->precision);
    if (!many_supported(d))
        return fail(FCR_EUNSUPPORTED, "%s: H=%d: the many-model kernels are built for the slot tiers 8 and 13 (H 17..52)",
                    what, d->H);
    const int limit = (o && o->small_batch_limit >= 0) ? o->small_batch_limit : g_small_max_batch.load();
    if (d->B > limit)
        return fail(FCR_EUNSUPPORTED, "%s: B=%d is above the small-batch limit %d (the many-model kernels are the "
                    "small-batch family's)", what, d->B, limit);
    if ((long long)n_models * d->B * d->N > (1LL << 31)) return fail(FCR_EINVAL, "%s: n_models*B*N too large", what);
    return FCR_OK;
}

int fcr_many_workspace_size(const fcr_dims *dims, const fcr_options *opts, int32_t n_models, int with_backward,
                            size_t *bytes) {
    if (const int rc = many_check("fcr_many_workspace_size", dims, opts, n_models)) return rc;
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    *bytes = many_workspace(dims, n_models, with_backward);
    return FCR_OK;
}

int fcr_forward_many(const fcr_dims *d, fcr_options *opts, int32_t n_models, const fcr_weights *w, const float *X,
                     const float *u0, const float *states, const float *noise, float *loss, float *cost, float *command,
                     float *error, float *prediction, float *xhat, int with_backward, void *ws, size_t ws_bytes,
                     void *stream) {
    if (const int rc = many_check("fcr_forward_many", d, opts, n_models)) return rc;
    fcr_loss_terms t;
    fcr_loss_terms_default(&t, d->alpha);
    return fcr_forward_many_terms(d, opts, n_models, w, &t, X, u0, states, noise, loss, cost, command, error, prediction,
                                  xhat, with_backward, ws, ws_bytes, stream);
}

int fcr_forward_many_terms(const fcr_dims *d, fcr_options *opts, int32_t n_models, const fcr_weights *w,
                           const fcr_loss_terms *terms, const float *X, const float *u0, const float *states,
                           const float *noise, float *loss, float *cost, float *command, float *error, float *prediction,
                           float *xhat, int with_backward, void *ws, size_t ws_bytes, void *stream) {
    int rc = many_check("fcr_forward_many", d, opts, n_models);
    if (rc) return rc;
    Terms tm;
    if ((rc = resolve_terms("fcr_forward_many", d, terms, X, true, &tm))) return rc;
    if (n_models == 0) return FCR_OK;
    if (!w || !X || !u0 || !states || !loss || !cost || !command || !error || !prediction || !ws)
        return fail(FCR_EINVAL, "fcr_forward_many: a required pointer is NULL");
    for (int l = 0; l < kLayers; ++l)
        if (!w->w_ih[l] || !w->w_hh[l]) return fail(FCR_EINVAL, "fcr_forward_many: LSTM weight of layer %d is NULL", l);
    if (!w->fc_w || !w->fc_b || !w->ctrl_w_inp || !w->ctrl_b_inp || !w->ctrl_w_out)
        return fail(FCR_EINVAL, "fcr_forward_many: a weight pointer is NULL");
    if ((rc = check_ws("fcr_forward_many", ws, ws_bytes, many_workspace(d, n_models, with_backward)))) return rc;
    note_kernels(opts, FCR_KERNELS_SMALL);
    return many_forward(d, n_models, tm, w, X, u0, states, noise, loss, cost, command, error, prediction, xhat, with_backward,
                        (char *)ws, (hipStream_t)stream);
}

int fcr_backward_many(const fcr_dims *d, fcr_options *opts, int32_t n_models, const float *X, const float *states,
                      const float *prediction, const float *dloss, float *g_u0, float *g_w_inp, float *g_b_inp,
                      float *g_w_out, void *ws, size_t ws_bytes, void *stream) {
    if (const int rc = many_check("fcr_backward_many", d, opts, n_models)) return rc;
    fcr_loss_terms t;
    fcr_loss_terms_default(&t, d->alpha);
    return fcr_backward_many_terms(d, opts, n_models, &t, X, states, prediction, dloss, g_u0, g_w_inp, g_b_inp, g_w_out,
                                   ws, ws_bytes, stream);
}

int fcr_backward_many_terms(const fcr_dims *d, fcr_options *opts, int32_t n_models, const fcr_loss_terms *terms,
                            const float *X, const float *states, const float *prediction, const float *dloss,
                            float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out, void *ws, size_t ws_bytes,
                            void *stream) {
    int rc = many_check("fcr_backward_many", d, opts, n_models);
    if (rc) return rc;
    Terms tm;
    if ((rc = resolve_terms("fcr_backward_many", d, terms, X, true, &tm))) return rc;
    if (n_models == 0) return FCR_OK;
    if (!X || !states || !prediction || !dloss || !g_u0 || !g_w_inp || !g_b_inp || !g_w_out || !ws)
        return fail(FCR_EINVAL, "fcr_backward_many: a required pointer is NULL");
    if ((rc = check_ws("fcr_backward_many", ws, ws_bytes, many_workspace(d, n_models, 1)))) return rc;
    note_kernels(opts, FCR_KERNELS_SMALL);
    return many_backward(d, n_models, tm, X, states, prediction, dloss, g_u0, g_w_inp, g_b_inp, g_w_out, (char *)ws,
                         (hipStream_t)stream);
}

int fcr_lstm_workspace_size(const fcr_dims *dims, int with_backward, size_t *bytes) {
    int rc = check_lstm_dims(dims);
    if (rc) return rc;
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    *bytes = is_wide(dims) ? surw_workspace(dims, with_backward) : sur_workspace(dims, with_backward);
    return FCR_OK;
}

int fcr_lstm_forward(const fcr_dims *d, const fcr_weights *w, const float *x, float *y, int with_backward, void *ws,
                     size_t ws_bytes, void *stream) {
    int rc = check_lstm_dims(d);
    if (rc) return rc;
    if (!x || !y || !ws) return fail(FCR_EINVAL, "fcr_lstm_forward: a required pointer is NULL");
    if (!lstm_weights_ok(w)) return fail(FCR_EINVAL, "fcr_lstm_forward: an LSTM/fc weight pointer is NULL");
    const size_t need = is_wide(d) ? surw_workspace(d, with_backward) : sur_workspace(d, with_backward);
    if ((rc = check_ws("fcr_lstm_forward", ws, ws_bytes, need))) return rc;
    if (!is_wide(d))   // H <= 52: the fused kernels (fcr_sur.h)
        return sur_forward(d, w, x, y, with_backward, (char *)ws, (hipStream_t)stream);
    return surw_forward(d, w, x, y, with_backward, (char *)ws, (hipStream_t)stream);
}

int fcr_lstm_backward(const fcr_dims *d, const fcr_weights *w, const float *dy, float *const *g_w_ih,
                      float *const *g_w_hh, float *g_fc_w, float *g_fc_b, float *g_x, void *ws, size_t ws_bytes,
                      void *stream) {
    int rc = check_lstm_dims(d);
    if (rc) return rc;
    if (!dy || !ws || !g_w_ih || !g_w_hh || !g_fc_w || !g_fc_b)
        return fail(FCR_EINVAL, "fcr_lstm_backward: a required pointer is NULL");
    for (int l = 0; l < kLayers; ++l)
        if (!g_w_ih[l] || !g_w_hh[l]) return fail(FCR_EINVAL, "fcr_lstm_backward: gradient of layer %d is NULL", l);
    if (!lstm_weights_ok(w)) return fail(FCR_EINVAL, "fcr_lstm_backward: an LSTM/fc weight pointer is NULL");
    const size_t need = is_wide(d) ? surw_workspace(d, 1) : sur_workspace(d, 1);
    if ((rc = check_ws("fcr_lstm_backward", ws, ws_bytes, need))) return rc;
    if (!is_wide(d)) return sur_backward(d, dy, g_w_ih, g_w_hh, g_fc_w, g_fc_b, g_x, (char *)ws, (hipStream_t)stream);
    return surw_backward(d, w, dy, g_w_ih, g_w_hh, g_fc_w, g_fc_b, g_x, (char *)ws, (hipStream_t)stream);
}

int fcr_lstm_rollout_workspace_size(const fcr_dims *dims, size_t *bytes) {
    int rc = check_lro_dims(dims);
    if (rc) return rc;
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    *bytes = lro_workspace(dims);
    return FCR_OK;
}

int fcr_lstm_rollout(const fcr_dims *d, const fcr_weights *w, const float *window0, const float *cmd, const float *gain,
                     const float *noise, float *xhat, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_lro_dims(d);
    if (rc) return rc;
    if (d->B == 0) return FCR_OK;
    if (!window0 || !cmd || !xhat || !ws) return fail(FCR_EINVAL, "fcr_lstm_rollout: a required pointer is NULL");
    if (!lstm_weights_ok(w)) return fail(FCR_EINVAL, "fcr_lstm_rollout: an LSTM/fc weight pointer is NULL");
    if ((rc = check_ws("fcr_lstm_rollout", ws, ws_bytes, lro_workspace(d)))) return rc;
    return lro_forward(d, w, window0, cmd, gain, noise, xhat, (char *)ws, (hipStream_t)stream);
}

static int check_lro_bwd_dims(const fcr_dims *d) {
    if (const int rc = check_lro_dims(d)) return rc;
    if (!lro_bwd_fits(d)) return fail(FCR_EINVAL, "B*N too large: the backward runs N x (B rounded up to 16) windows, 2^30 at the most");
    return FCR_OK;
}

int fcr_lstm_rollout_backward_workspace_size(const fcr_dims *dims, size_t *bytes) {
    int rc = check_lro_bwd_dims(dims);
    if (rc) return rc;
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    *bytes = lro_bwd_workspace(dims);
    return FCR_OK;
}

int fcr_lstm_rollout_backward(const fcr_dims *d, const fcr_weights *w, const float *window0, const float *cmd,
                              const float *gain, const float *xhat, const float *g_xhat,
                              const fcr_lstm_rollout_grads *out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_lro_bwd_dims(d);
    if (rc) return rc;
    if (d->B == 0) return FCR_OK;
    if (!window0 || !cmd || !xhat || !g_xhat || !out || !ws)
        return fail(FCR_EINVAL, "fcr_lstm_rollout_backward: a required pointer is NULL");
    for (int l = 0; l < kLayers; ++l)
        if (!out->g_w_ih[l] || !out->g_w_hh[l])
            return fail(FCR_EINVAL, "fcr_lstm_rollout_backward: gradient of layer %d is NULL", l);
    if (!out->g_fc_w || !out->g_fc_b) return fail(FCR_EINVAL, "fcr_lstm_rollout_backward: a readout gradient is NULL");
    if (!lstm_weights_ok(w)) return fail(FCR_EINVAL, "fcr_lstm_rollout_backward: an LSTM/fc weight pointer is NULL");
    if ((rc = check_ws("fcr_lstm_rollout_backward", ws, ws_bytes, lro_bwd_workspace(d)))) return rc;
    return lro_backward(d, w, window0, cmd, gain, xhat, g_xhat, out, (char *)ws, (hipStream_t)stream);
}

int fcr_fnn_workspace_size(int32_t B, int32_t hidden, size_t *bytes) {
    if (B < 0 || hidden < 1 || hidden > fnn::kFnnMaxHidden)
        return fail(FCR_EINVAL, "fcr_fnn_workspace_size: B=%d, hidden=%d (1..%d)", B, hidden, fnn::kFnnMaxHidden);
    if (!bytes) return fail(FCR_EINVAL, "bytes is NULL");
    const size_t blocks = ((size_t)B + fnn::kFnnItems - 1) / fnn::kFnnItems;
    *bytes = blocks * (size_t)hidden * 5 * sizeof(float);
    return FCR_OK;
}

static int fnn_check(const char *what, int32_t B, int32_t in_dim, int32_t hidden) {
    if (B < 0) return fail(FCR_EINVAL, "%s: B=%d must be >= 0", what, B);
    if (in_dim != kCtrlIn) return fail(FCR_EUNSUPPORTED, "%s: in_dim=%d: built for %d (UL/Main.py:188)", what, in_dim, kCtrlIn);
    if (hidden < 1 || hidden > fnn::kFnnMaxHidden)
        return fail(FCR_EUNSUPPORTED, "%s: hidden=%d: built for 1..%d", what, hidden, fnn::kFnnMaxHidden);
    return FCR_OK;
}

int fcr_fnn_forward(int32_t B, int32_t in_dim, int32_t hidden, const float *X, const float *w_inp,
                    const float *b_inp, const float *w_out, float *u, void *stream) {
    int rc = fnn_check("fcr_fnn_forward", B, in_dim, hidden);
    if (rc) return rc;
    if (B == 0) return FCR_OK;
    if (!X || !w_inp || !b_inp || !w_out || !u) return fail(FCR_EINVAL, "fcr_fnn_forward: a required pointer is NULL");
    hipLaunchKernelGGL(fnn::fnn_fwd_kernel, dim3((B + fnn::kFnnBlock - 1) / fnn::kFnnBlock), dim3(fnn::kFnnBlock), 0,
                       (hipStream_t)stream, B, hidden, X, w_inp, b_inp, w_out, u);
    return launch_check("fnn_fwd_kernel");
}

int fcr_fnn_backward(int32_t B, int32_t in_dim, int32_t hidden, const float *X, const float *w_inp,
                     const float *b_inp, const float *w_out, const float *g_u, float *g_x, float *g_w_inp,
                     float *g_b_inp, float *g_w_out, void *ws, size_t ws_bytes, void *stream) {
    int rc = fnn_check("fcr_fnn_backward", B, in_dim, hidden);
    if (rc) return rc;
    if (!w_inp || !b_inp || !w_out || !g_w_inp || !g_b_inp || !g_w_out || (B && (!X || !g_u || !ws)))
        return fail(FCR_EINVAL, "fcr_fnn_backward: a required pointer is NULL");
    size_t need = 0;
    if ((rc = fcr_fnn_workspace_size(B, hidden, &need))) return rc;
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "fcr_fnn_backward: ws has %zu bytes, needs %zu", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)((B + fnn::kFnnItems - 1) / fnn::kFnnItems);
    if (blocks) {
        const bool one = blocks == 1;   // one block writes the gradients itself (grad_out5)
        hipLaunchKernelGGL(fnn::fnn_bwd_kernel, dim3(blocks), dim3(fnn::kFnnBlock), 0, s, B, hidden, X, w_inp, b_inp,
                           w_out, g_u, g_x, (float *)ws, one ? g_w_inp : nullptr, one ? g_b_inp : nullptr,
                           one ? g_w_out : nullptr);
        if ((rc = launch_check("fnn_bwd_kernel"))) return rc;
        if (one) return FCR_OK;
    }
    return launch_grad_reduce((const float *)ws, blocks, hidden, g_w_inp, g_b_inp, g_w_out, s);
}

static int fnn_many_check(const char *what, int32_t n_models, int32_t B, int32_t in_dim, int32_t hidden) {
    if (n_models < 0) return fail(FCR_EINVAL, "%s: n_models=%d must be >= 0", what, n_models);
    if (n_models > 65535) return fail(FCR_EUNSUPPORTED, "%s: n_models=%d: at most 65535 (a grid dimension)", what, n_models);
    return fnn_check(what, B, in_dim, hidden);
}

int fcr_fnn_forward_many(int32_t n_models, int32_t B, int32_t in_dim, int32_t hidden, const float *X, const float *w_inp,
                         const float *b_inp, const float *w_out, float *u, void *stream) {
    int rc = fnn_many_check("fcr_fnn_forward_many", n_models, B, in_dim, hidden);
    if (rc) return rc;
    if (B == 0 || n_models == 0) return FCR_OK;
    if (!X || !w_inp || !b_inp || !w_out || !u) return fail(FCR_EINVAL, "fcr_fnn_forward_many: a required pointer is NULL");
    hipLaunchKernelGGL(fnn::fnn_fwd_many_kernel, dim3((B + fnn::kFnnBlock - 1) / fnn::kFnnBlock, n_models),
                       dim3(fnn::kFnnBlock), 0, (hipStream_t)stream, B, hidden, X, w_inp, b_inp, w_out, u);
    return launch_check("fnn_fwd_many_kernel");
}

int fcr_fnn_backward_many(int32_t n_models, int32_t B, int32_t in_dim, int32_t hidden, const float *X, const float *w_inp,
                          const float *b_inp, const float *w_out, const float *g_u, float *g_x, float *g_w_inp,
                          float *g_b_inp, float *g_w_out, void *ws, size_t ws_bytes, void *stream) {
    int rc = fnn_many_check("fcr_fnn_backward_many", n_models, B, in_dim, hidden);
    if (rc) return rc;
    if (n_models == 0) return FCR_OK;
    if (!w_inp || !b_inp || !w_out || !g_w_inp || !g_b_inp || !g_w_out || (B && (!X || !g_u || !ws)))
        return fail(FCR_EINVAL, "fcr_fnn_backward_many: a required pointer is NULL");
    size_t need = 0;
    if ((rc = fcr_fnn_workspace_size(B, hidden, &need))) return rc;
    need *= (size_t)n_models;   // fcr_fnn_workspace_size(B, hidden) per model
    if (ws_bytes < need) return fail(FCR_EWORKSPACE, "fcr_fnn_backward_many: ws has %zu bytes, needs %zu", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)((B + fnn::kFnnItems - 1) / fnn::kFnnItems);
    if (blocks) {
        const bool one = blocks == 1;   // one block per model writes that model's gradients itself (grad_out5)
        hipLaunchKernelGGL(fnn::fnn_bwd_many_kernel, dim3(blocks, n_models), dim3(fnn::kFnnBlock), 0, s, B, hidden, X, w_inp,
                           b_inp, w_out, g_u, g_x, (float *)ws, blocks, one ? g_w_inp : nullptr, one ? g_b_inp : nullptr,
                           one ? g_w_out : nullptr);
        if ((rc = launch_check("fnn_bwd_many_kernel"))) return rc;
        if (one) return FCR_OK;
    }
    return launch_grad_reduce_many((const float *)ws, blocks, hidden, n_models, g_w_inp, g_b_inp, g_w_out, s);
}

}  // extern "C"
