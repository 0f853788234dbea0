/*
 * fcr.h — C ABI of the MI355X-native (gfx950) unsupervised-MPC rollout engine.
 *
 * This library replaces the work torch dispatches inside ONE Python call of the reference,
 *
 *     loss, loss_features = loss_function(simulator, model, X, output, z, device, enable_noise)
 *     ...
 *     loss.backward()
 *
 * at /root/reference/Unsupervised Learning/Functions.py:646 and :655 (MPCLoss.forward,
 * Functions.py:1353-1472, plus its autograd backward). The reference has no FFI of its own (it is
 * pure Python/PyTorch); the binding a maintainer adds is the ctypes stub in INTEGRATION.md, and the
 * Python drop-in `MPCLoss` in forging-control_amd/functions.py is that stub.
 *
 * Conventions (all entry points):
 *   - every pointer is caller-owned DEVICE memory (fp32, contiguous, batch-first exactly as the
 *     reference lays it out), except `dims`/`w` (host structs);
 *   - `stream` is a hipStream_t (passed as void* so this header needs no HIP headers); all work is
 *     stream-ordered on it, nothing synchronises the host;
 *   - no allocation inside a call: scratch comes from `ws` (size from fcr_workspace_size);
 *   - return FCR_OK (0) or a negative FCR_E* code; fcr_last_error() (thread-local) explains it.
 */
#ifndef FCR_H
#define FCR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCR_ABI_VERSION 8   /* 8: fcr_feasibility, fcr_feasibility_project; fcr_closed_loop gains feasibility / u_nn / feas_flag;
                              * fcr_supervised_epoch joined later as a pure addition (no existing call or struct changed): look the symbol up */

enum {
    FCR_OK = 0,
    FCR_EINVAL = -1,      /* bad dims, null pointer, misalignment            */
    FCR_EWORKSPACE = -2,  /* ws too small                                      */
    FCR_EHIP = -3,        /* a HIP runtime call failed                         */
    FCR_EUNSUPPORTED = -4 /* dims valid for the reference but not built here   */
};

/* Problem shape. Reference values: L=10 (Functions.py:1434 hard-codes the 10-row window),
 * layers=3 / H=50 / in_dim=5 / out_dim=4 (UL/Main.py:144-154), ctrl 3->50->1 (UL/Main.py:183-188),
 * N = n_horizon = 10 (UL/template_mpc.py:20), alpha = 20.0 (UL/Main.py:192). */
typedef struct fcr_dims {
    int32_t B;           /* trajectories in the batch                         */
    int32_t N;           /* prediction horizon (MPCLoss.N)                    */
    int32_t L;           /* lookback rows of the LSTM window (must be 10)     */
    int32_t H;           /* LSTM hidden size: 1..52 fused kernels, 53..2048 per-cell GEMM path */
    int32_t layers;      /* LSTM layers (must be 3)                           */
    int32_t in_dim;      /* LSTM input features (must be 5)                   */
    int32_t out_dim;     /* LSTM outputs (must be 4)                          */
    int32_t ctrl_in;     /* controller inputs (must be 3)                     */
    int32_t ctrl_hidden; /* controller hidden units (<= 52)                   */
    float alpha;         /* MPCLoss.alpha, command-variation weight            */
    int32_t precision;   /* FCR_PRECISION_FP32 (0) or FCR_PRECISION_F16 (1), below */
} fcr_dims;

/* Arithmetic of the gate products (fcr_forward/fcr_backward; fcr_lstm_forward/_backward ignore it and run fp32,
 * fcr_lstm_rollout accepts FCR_PRECISION_FP32 only):
 *   FCR_PRECISION_FP32 — fp32-accurate: each operand split into two f16 halves, three f16 MFMAs per
 *                        product, fp32 accumulate (results within 1e-5 of an fp64 evaluation);
 *   FCR_PRECISION_F16  — config 3's reduced-precision mode ("bf16 storage/MFMA fwd"):
 *                        f16 operands (11-bit significand, more than bf16's 8; the backward's per-trajectory
 *                        power-of-two scaling keeps them in range), one MFMA per product, fp32 accumulate;
 *                        H <= 52 only;
 *   (2, the former FCR_PRECISION_F16_FWD — f16 forward, fp32-accurate backward — is retired in ABI v5 and refused
 *   with FCR_EUNSUPPORTED: it ran 1.08x the fp32 step at the all-f16 mode's accuracy, DESIGN.md §4 "Config 3".)
 * Both calls of one step must be given the same dims (the same precision value). */
#define FCR_PRECISION_FP32 0
#define FCR_PRECISION_F16 1

/* Weights, torch layouts (row-major, as state_dict holds them). */
typedef struct fcr_weights {
    const float *ctrl_w_inp; /* FNNModel.fc_inp.weight (ctrl_hidden, ctrl_in)  Functions.py:249 */
    const float *ctrl_b_inp; /* FNNModel.fc_inp.bias   (ctrl_hidden)                            */
    const float *ctrl_w_out; /* FNNModel.fc_out.weight (1, ctrl_hidden), no bias Functions.py:251 */
    const float *w_ih[3];    /* LSTMModel.lstm.weight_ih_l{0,1,2} (4H, in_dim | H)  :325        */
    const float *w_hh[3];    /* LSTMModel.lstm.weight_hh_l{0,1,2} (4H, H)                       */
    const float *fc_w;       /* LSTMModel.fc.weight (out_dim, H)                     :329        */
    const float *fc_b;       /* LSTMModel.fc.bias   (out_dim)                                    */
} fcr_weights;

/* Per-call kernel options of fcr_workspace_size / fcr_forward / fcr_backward (ABI v5). NULL = every field at
 * FCR_OPT_INHERIT. Two users of the library in one process (a training rollout and a validation rollout beside it,
 * on different streams or threads) each pass their own and see nothing of the other's; the process-wide setters
 * below only supply the defaults a field set to FCR_OPT_INHERIT takes. A forward and its backward should be given the
 * same options (both kernel families keep one workspace layout, so a mix is valid, only slower).
 *   small_batch_limit  B <= it runs the small-batch kernels (fp32-accurate mode, H 17..52), 0 = never;
 *                      negative (FCR_OPT_INHERIT): fcr_set_small_batch_limit's value
 *   wide_keep_budget   H > 52, read by fcr_workspace_size only: bytes of kept windows the workspace may add;
 *                      FCR_KEEP_AUTO (-1) the library's policy (fcr_set_wide_keep_budget below), FCR_OPT_INHERIT (-2)
 *                      the process-wide setting
 *   kernels            OUT, written by fcr_forward / fcr_backward: the kernel family the call launched
 *                      (FCR_KERNELS_SMALL, _FUSED or _WIDE) */
#define FCR_OPT_INHERIT (-2)
#define FCR_KEEP_AUTO (-1)
#define FCR_KERNELS_SMALL 1
#define FCR_KERNELS_FUSED 2
#define FCR_KERNELS_WIDE 3
typedef struct fcr_options {
    int32_t small_batch_limit;
    int32_t kernels;
    int64_t wide_keep_budget;
} fcr_options;

/* Bytes of scratch a forward (+ backward when with_backward != 0) needs for `dims` (and, H > 52, opts' keep budget). */
int fcr_workspace_size(const fcr_dims *dims, const fcr_options *opts, int with_backward, size_t *bytes);

/* H > 52: how many of the N windows a backward-enabled workspace of ws_bytes keeps (the forward and the backward
 * each derive this count from the ws_bytes they are given; 0 for H <= 52). */
int fcr_wide_kept_windows(const fcr_dims *dims, size_t ws_bytes, int32_t *kept);

/*
 * Forward rollout = MPCLoss.forward (Functions.py:1353-1472).
 *   X        (B,3)   input_controller [y_dot, z, ref]          (Functions.py:1353, ref = X[:,-1] :1392)
 *   u0       (B,1)   output_controller = controller(X)          (Functions.py:643)
 *   states   (B,L,5) LSTM window [y_dot,p1,p2,z,u]              (Functions.py:1395)
 *   noise    (B,N,4) additive LSTM-output noise, or NULL        (Functions.py:1400-1402,1438-1440)
 * Outputs:
 *   loss (1) mean cost; cost/command/error (B) = loss_features['loss'|'command'|'error'];
 *   prediction (B*N) sample-major = loss_features['prediction']  (Functions.py:1466);
 *   xhat (B,N,4) per-step LSTM predictions (closed-loop state trajectory), or NULL.
 * with_backward != 0 keeps the activations fcr_backward needs in `ws` (which must then not be
 * reused until fcr_backward has run).
 */
int fcr_forward(const fcr_dims *dims, fcr_options *opts, const fcr_weights *w,
                const float *X, const float *u0, const float *states, const float *noise,
                float *loss, float *cost, float *command, float *error,
                float *prediction, float *xhat,
                int with_backward, void *ws, size_t ws_bytes, void *stream);

/*
 * Backward of the last fcr_forward(with_backward=1) on the same `ws` = what loss.backward()
 * (Functions.py:655) delivers: d loss/d u0 (B,1) — handed back to the caller's controller(X) graph —
 * and the gradients of the controller parameters used inside the loss. `dloss` is a DEVICE pointer
 * to the incoming scalar gradient (no host sync). LSTM weight gradients are not computed (the
 * reference computes them but nothing reads them: UL/Main.py:195 optimises only the controller).
 * Parameter gradients are OVERWRITTEN (not accumulated); reduction order is fixed (deterministic).
 */
int fcr_backward(const fcr_dims *dims, fcr_options *opts,
                 const float *X, const float *states, const float *prediction,
                 const float *dloss,
                 float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out,
                 void *ws, size_t ws_bytes, void *stream);

/*
 * The caller's controller call `output = model(X)` (Functions.py:643): FNNModel.forward
 * (Functions.py:261-289) at the reference's shape — Linear(in_dim=3 -> hidden) + ReLU,
 * Linear(hidden -> 1, no bias) + Hardtanh (UL/Main.py:188, width_dim = 1); hidden <= 64.
 *   X (B,3), w_inp (hidden,3), b_inp (hidden), w_out (1,hidden) -> u (B,1)
 * fcr_fnn_backward is its autograd backward for g_u = dL/du (B,1): the parameter gradients
 * (OVERWRITTEN, fixed reduction order) and g_x = dL/dX (B,3), or NULL to skip it. Hardtanh'(±1) = 0,
 * ReLU'(0) = 0 (torch). Scratch: fcr_fnn_workspace_size bytes.
 */
int fcr_fnn_workspace_size(int32_t B, int32_t hidden, size_t *bytes);
int fcr_fnn_forward(int32_t B, int32_t in_dim, int32_t hidden, const float *X, const float *w_inp,
                    const float *b_inp, const float *w_out, float *u, void *stream);
int fcr_fnn_backward(int32_t B, int32_t in_dim, int32_t hidden, const float *X, const float *w_inp,
                     const float *b_inp, const float *w_out, const float *g_u, float *g_x, float *g_w_inp,
                     float *g_b_inp, float *g_w_out, void *ws, size_t ws_bytes, void *stream);

/*
 * M controllers side by side (the reference ships ten seeds of the controller, all trained at B = 15): n_models
 * controllers of one hidden width against ONE shared LSTM surrogate, one rollout launch per pass. A pure addition to
 * ABI v8 (no existing call or struct changed): look the symbols up.
 *   dims       the shape of ONE model's call (dims->B = its batch; every model has the same B)
 *   w          ctrl_w_inp (M,hidden,3), ctrl_b_inp (M,hidden), ctrl_w_out (M,hidden) stacked; the LSTM's as in fcr_weights
 *   X (M,B,3), u0 (M,B,1), states (M,B,L,5), noise (M,B,N,4) or NULL — stacked model-major
 *   loss (M), cost/command/error (M,B), prediction (M,B*N), xhat (M,B,N,4) or NULL
 *   dloss (M) DEVICE floats; g_u0 (M,B,1), g_w_inp (M,hidden,3), g_b_inp (M,hidden), g_w_out (M,hidden), OVERWRITTEN
 * Model m's results are what fcr_forward / fcr_backward return for (controller m, X[m], u0[m], states[m], noise[m]):
 * loss[m] is the mean over its own B trajectories, nothing sums over models, every sum keeps the single call's order
 * (a model's numbers do not depend on M). One thing is shared: the f16 split's range guard scales a window column by
 * the maximum over the STACKED batch, because the scale belongs to the shared W_ih0; for every input the reference's
 * scalers produce that scale is 2^0 and nothing differs from M separate calls.
 * Kernels: the small-batch family's one-workgroup geometry, a 16-trajectory group of one model per workgroup. Refused
 * before any launch: n_models < 0 (FCR_EINVAL); precision other than FCR_PRECISION_FP32, an H outside the slot tiers
 * 8 and 13 (17..52), B above the small-batch limit (opts, else the process default) — FCR_EUNSUPPORTED: run those as
 * n_models single calls. n_models = 0 is a no-op. Scratch: fcr_many_workspace_size bytes, 256-byte aligned.
 * fcr_fnn_forward_many / fcr_fnn_backward_many are fcr_fnn_forward / _backward for the stacked controllers on
 * X (M,B,3) -> u (M,B,1); scratch of the backward: n_models * fcr_fnn_workspace_size(B, hidden) bytes.
 */
int fcr_many_workspace_size(const fcr_dims *dims, const fcr_options *opts, int32_t n_models, int with_backward,
                            size_t *bytes);
int fcr_forward_many(const fcr_dims *dims, fcr_options *opts, int32_t n_models, const fcr_weights *w,
                     const float *X, const float *u0, const float *states, const float *noise,
                     float *loss, float *cost, float *command, float *error,
                     float *prediction, float *xhat,
                     int with_backward, void *ws, size_t ws_bytes, void *stream);
int fcr_backward_many(const fcr_dims *dims, fcr_options *opts, int32_t n_models,
                      const float *X, const float *states, const float *prediction,
                      const float *dloss,
                      float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out,
                      void *ws, size_t ws_bytes, void *stream);
int fcr_fnn_forward_many(int32_t n_models, int32_t B, int32_t in_dim, int32_t hidden, const float *X,
                         const float *w_inp, const float *b_inp, const float *w_out, float *u, void *stream);
int fcr_fnn_backward_many(int32_t n_models, int32_t B, int32_t in_dim, int32_t hidden, const float *X,
                          const float *w_inp, const float *b_inp, const float *w_out, const float *g_u, float *g_x,
                          float *g_w_inp, float *g_b_inp, float *g_w_out, void *ws, size_t ws_bytes, void *stream);

/*
 * The loss's terms as data. A pure addition to ABI v8 (no existing call or struct changed): look the symbols up.
 * For trajectory b, horizon step j = 0 .. N-1 and the scaled prediction xhat_j = (y_dot, p1, p2, z):
 *   err_j = (xhat_j[0] - r_j)^2
 *   con_j = w_con * (relu(p1_lo - p1) + relu(p2_lo - p2) + relu(p1 - p1_hi) + relu(p2 - p2_hi))
 *   tot  += (err_j + alpha * du_j^2) + con_j ;   u_{j+1} = controller(xhat_j[0], xhat_j[3], r_{j+1})
 * fcr_loss_terms_default() gives the reference's loss (Functions.py:1405-1452): p*_lo = 0, p1_hi = 2.122366,
 * p2_hi = 1.036233 (32e6 Pa over the shipped output scaler's max_abs_), w_con = 1, r_j = X[b, 2] at every j; with it
 * (and alpha = dims->alpha) the *_terms calls return the bits of the calls without terms, which are exactly that.
 *   alpha                     replaces dims->alpha, which the *_terms calls IGNORE
 *   p1_lo .. p2_hi, w_con     in the surrogate's scaled units. A bound may be -inf (lo) / +inf (hi): switched off.
 *                             Refused (FCR_EINVAL, before any launch): a NaN, lo > hi, w_con < 0, a non-finite alpha
 *   ref, ref_stride_b/_j      DEVICE floats, r_j of trajectory b = ref[b * ref_stride_b + j * ref_stride_j]; a (B,N)
 *                             array passes (N, 1). NULL = X's column 2 (strides ignored). A plain input: no gradient.
 *                             The backward must be given the forward's terms.
 * The many-model calls only:
 *   table, table_stride       DEVICE floats, model m's six scalars {alpha, p1_lo, p1_hi, p2_lo, p2_hi, w_con} at
 *                             table + m * table_stride (stride 0: one row shared by every model); NULL = the struct's
 *                             own scalars for every model. The table's VALUES are the caller's to check (the library
 *                             does not read device memory on the host); with a table the struct's scalars are unused.
 *   ref_stride_m              model m's references start at ref + m * ref_stride_m: an (M,B,N) array passes
 *                             (B N, N, 1).
 * Workspace sizes are those of the calls without terms.
 */
typedef struct fcr_loss_terms {
    float alpha, p1_lo, p1_hi, p2_lo, p2_hi, w_con;
    const float *ref;
    int64_t ref_stride_b, ref_stride_j;
    const float *table;
    int64_t table_stride, ref_stride_m;
} fcr_loss_terms;
void fcr_loss_terms_default(fcr_loss_terms *terms, float alpha);
int fcr_forward_terms(const fcr_dims *dims, fcr_options *opts, const fcr_weights *w, const fcr_loss_terms *terms,
                      const float *X, const float *u0, const float *states, const float *noise,
                      float *loss, float *cost, float *command, float *error,
                      float *prediction, float *xhat,
                      int with_backward, void *ws, size_t ws_bytes, void *stream);
int fcr_backward_terms(const fcr_dims *dims, fcr_options *opts, const fcr_loss_terms *terms,
                       const float *X, const float *states, const float *prediction,
                       const float *dloss,
                       float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out,
                       void *ws, size_t ws_bytes, void *stream);
int fcr_forward_many_terms(const fcr_dims *dims, fcr_options *opts, int32_t n_models, const fcr_weights *w,
                           const fcr_loss_terms *terms,
                           const float *X, const float *u0, const float *states, const float *noise,
                           float *loss, float *cost, float *command, float *error,
                           float *prediction, float *xhat,
                           int with_backward, void *ws, size_t ws_bytes, void *stream);
int fcr_backward_many_terms(const fcr_dims *dims, fcr_options *opts, int32_t n_models, const fcr_loss_terms *terms,
                            const float *X, const float *states, const float *prediction,
                            const float *dloss,
                            float *g_u0, float *g_w_inp, float *g_b_inp, float *g_w_out,
                            void *ws, size_t ws_bytes, void *stream);

/*
 * Batched forging-press plant: the state update x_{t+1} = F(x_t, u_t) of
 * FeasibilityRecovery.Ruge_Kuta (Functions.py:1743-1781) over the dynamics of forging_model
 * (Functions.py:1615-1740; smooth = 1: template_model.py:19-149, pressures floored by smooth_relu),
 * for B independent trajectories of S steps, in fp64.
 *   x0 (B,5)       initial states [y, y_dot, p1, p2, z]
 *   u  (B,S)       command held over each step
 *   x  (B,S+1,5)   x[:,0] = x0, x[:,t+1] = F(x[:,t], u[:,t])
 *   ts             step (the reference: TS = controller t_step = 0.001, template_mpc.py:23)
 *   substeps       RK4 stages per step (the reference: M = 4, Functions.py:1760)
 * B = 0 is a no-op. Buffers are fp64 device memory, 8-byte aligned.
 */
int fcr_plant_rk4(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth,
                  const double *x0, const double *u, double *x, void *stream);

/*
 * Batched closed-loop evaluation (SURVEY.md §8(f) ranks 1 + 2): NeuralNetwork.loop (Functions.py:
 * 1075-1240) — per step the FNN controller on the MaxAbs-scaled [y_dot, z, ref] (NN_make_step, :1560-1613;
 * fp32 like torch), optionally the feasibility recovery of its command (fcr_feasibility, below), and the
 * press advanced by the RK4 integrator of fcr_plant_rk4 (in place of do-mpc's CVODES) — for B trajectories
 * × T steps, one launch.
 *   x0 (B,5), ref (B,T) unscaled speed references (NeuralNetwork.tvp_fun, :926-966, computed by the
 *   caller); controller weights as fcr_weights; in_scale = scalers['input'].scale_[0:2] (y_dot, z),
 *   ref_scale = scalers['y_dot'].scale_, out_scale = scalers['output'].scale_ (UL/Main.py:237-256);
 *   outputs x (B,T+1,5) with x[:,0] = x0 and u (B,T) the commands applied. fp64 buffers, fp32 weights.
 * Optional pre-drawn noise of the harness (ABI v7; NULL = none, so a zero-initialised struct runs the noise-free
 * loop, bit for bit as before):
 *   process_noise (B,T,5) fp64, in the units of x_dot: do-mpc adds it to the right-hand side (template_model.py:
 *     145-149) and the harness holds it over the sampling step (Functions.py:1176-1183), so every RK4 stage of
 *     step t evaluates f(x,u) + process_noise[b,t];
 *   meas_noise (B,T,5) fp64: x[:,t+1] records x_{t+1} + meas_noise[b,t], the controller reads that record at
 *     step t+1, and the integration continues from the unperturbed state. (The smooth model measures p_eff, not p,
 *     template_model.py:154-155; here the record is p + v.)
 * Optional feasibility recovery (ABI v8; NULL = off, so a zero-initialised struct runs the loop as before):
 *   feasibility  the projection's parameters; when set, every step projects the controller's command from the
 *     state the controller reads (under meas_noise the noisy record, all five components: Functions.py:1170) and
 *     the press is stepped with the projected command; u (B,T) then holds the projected commands;
 *   u_nn (B,T) fp64 the controller's raw commands, feas_flag (B,T) int32 the projection's flags; both are
 *     required when feasibility is set and ignored otherwise.
 */
typedef struct fcr_feasibility fcr_feasibility;
typedef struct fcr_closed_loop {
    int32_t B, T;
    double ts;
    int32_t substeps, smooth;
    const double *x0, *ref;
    const float *ctrl_w_inp, *ctrl_b_inp, *ctrl_w_out;
    int32_t ctrl_hidden;
    double in_scale[2];
    double ref_scale, out_scale;
    double *x, *u;
    const double *process_noise, *meas_noise; /* (B,T,5) each, or NULL (ABI v7) */
    const fcr_feasibility *feasibility;       /* NULL = no recovery (ABI v8) */
    double *u_nn;                             /* (B,T), with feasibility */
    int32_t *feas_flag;                       /* (B,T), with feasibility */
} fcr_closed_loop;

int fcr_closed_loop_run(const fcr_closed_loop *args, void *stream);

/*
 * Feasibility recovery (FeasibilityRecovery.feasibility_recover; the NLP of UL/Main.py:584-657) as a projection.
 * The NLP's slacks are in its cost only, so it is min (u_nn - u)^2 over one scalar u under
 *   p1_lo <= p1(X1), p1(X2) <= p1_hi,  p2_lo <= p2(X1), p2(X2) <= p2_hi,  X1 = F(x,u), X2 = F(X1,u),
 * F = `substeps` RK4 stages over `ts` of the NON-smooth forging_model with u held (Ruge_Kuta, Functions.py:1743-1781).
 * With pressures scaled by 1/32e6, v(x,u) = the largest of max(lo - p, p - hi) over the four pressures; u is feasible
 * iff v <= 0 (NaN: infeasible). Per state, in fp64:
 *   flag 0  v(x, u_nn) <= 0: u = u_nn bit for bit, also outside [u_lo, u_hi] (the NLP does not bound u);
 *   flag 1  for k = 0..expand probe clip(u_nn -/+ d·2^k), d = (u_hi - u_lo)/2^expand, clipped to [u_lo, u_hi]; at the
 *           first k with a feasible probe (both: the nearer, ties to the lower) bisect `bisect` times between it and
 *           the previous probe on its side (u_nn at k = 0); u = the feasible end of the bracket;
 *   flag 2  no probe feasible: u = clip(u_nn, u_lo, u_hi) (the reference's `except` branch).
 * The result is the nearest feasible command wherever the feasible set is an interval on the probed side.
 * Reference values: bounds 0 / 32e6 (UL/Main.py:118-119), u_lo/u_hi = -/+0.2 (Functions.py:1533), ts = 1e-3,
 * substeps = 4; expand = 10, bisect = 30 (a final bracket of 0.4/2^10/2^30).
 */
struct fcr_feasibility {
    double p1_lo, p1_hi, p2_lo, p2_hi; /* Pa; lo < hi                        */
    double u_lo, u_hi;                 /* u_lo < u_hi                        */
    double ts;                         /* the projection's own step          */
    int32_t substeps;                  /* 1..4096                            */
    int32_t expand;                    /* 1..20                              */
    int32_t bisect;                    /* 1..60                              */
};

/* x (B,5), u_nn (B) -> u (B), flag (B) int32 and, unless NULL, v (B) = v(x, u) at the returned u. B = 0 is a no-op. */
int fcr_feasibility_project(const fcr_feasibility *f, int32_t B, const double *x, const double *u_nn, double *u,
                            int32_t *flag, double *v, void *stream);

/*
 * The closed loop for a bank of M controllers, with the evaluation's numbers (a pure addition to ABI 8): what the
 * reference repeats per seed — NeuralNetwork.loop, then metrics / other_metrics (Functions.py:751-822) — for n_models
 * controllers × B trajectories × T steps in one launch plus one small reduction. The fields up to feas_flag are
 * fcr_closed_loop's and mean the same, except:
 *   ctrl_w_inp (M,hidden,3), ctrl_b_inp (M,hidden), ctrl_w_out (M,hidden): the stacked controllers (one hidden width,
 *     one set of scalers);
 *   x0, ref, process_noise, meas_noise: model m reads from base + m * stride ELEMENTS (x0_stride = B*5 for (M,B,5),
 *     0 for one (B,5) shared by all models, and so on);
 *   outputs are model-major: x (M,B,T+1,5), u, u_nn (M,B,T), feas_flag (M,B,T) int32. Model m's rows are what
 *     fcr_closed_loop_run returns for controller m on model m's inputs, bit for bit;
 *   storing is optional: x = NULL skips every per-step store, and then u, u_nn and feas_flag must be NULL too.
 * Always written, once after the loop (t = 0..T-1, r = ref[b,t], (y, p1, p2) from the record x[:,t+1] as stored,
 * measurement noise included, u the applied command):
 *   traj_stats  (M,B,6) fp64   sum |y-r|, sum (y-r)^2, max |y-r|, sum |u|, sum_{t>=1} (u_t - u_{t-1})^2, and the worst
 *                              violation max_t max(p1_lo - p1, p1 - p1_hi, p2_lo - p2, p2 - p2_hi) in Pa
 *   traj_counts (M,B,3) int32  steps with violation > 0, steps flagged 1, steps flagged 2 (0 without feasibility)
 *   x_final     (M,B,5) fp64   the unperturbed state after step T
 *   summary     (M,10)  fp64   over n = B*T: MAE, RMSE, R2 = 1 - SSE/SST (SST = sum (r - mean r)^2, mean first), max |e|,
 *                              mean |u|, RMS of du over B*(T-1) terms (0 at T = 1), the worst violation, and the fractions
 *                              of steps violating, flagged 1, flagged 2. Fixed summation order: same call, same bits.
 * p1_lo .. p2_hi are the bounds the violation is measured against (lo < hi); they need not be the feasibility's.
 * n_models = 0 and B = 0 are no-ops; T = 0 copies x0 (into x unless NULL, and x_final) and writes zero statistics.
 * Stream-ordered; nothing allocates or synchronises.
 */
typedef struct fcr_closed_loop_bank {
    int32_t B, T;
    double ts;
    int32_t substeps, smooth;
    const double *x0, *ref;
    const float *ctrl_w_inp, *ctrl_b_inp, *ctrl_w_out;
    int32_t ctrl_hidden;
    double in_scale[2];
    double ref_scale, out_scale;
    double *x, *u;
    const double *process_noise, *meas_noise;
    const fcr_feasibility *feasibility;
    double *u_nn;
    int32_t *feas_flag;
    int32_t n_models;
    int64_t x0_stride, ref_stride, process_noise_stride, meas_noise_stride;
    double p1_lo, p1_hi, p2_lo, p2_hi;
    double *traj_stats;
    int32_t *traj_counts;
    double *x_final;
    double *summary;
} fcr_closed_loop_bank;

int fcr_closed_loop_run_bank(const fcr_closed_loop_bank *args, void *stream);

/*
 * The press and the workpiece as data (a pure addition to ABI 8). fcr_press holds the 28 physical constants of
 * forging_model / template_model under the reference's names (Functions.py:1636-1695): moving mass, damping, friction,
 * plunger diameters, gravity, bulk modulus, chamber volumes, leakages, valve discharge coefficient, oil density, valve
 * diameter, supply and tank pressure, friction coefficient and K of the deformation resistance, billet width, height
 * and bite, its temperature, the valve's time constant, and the flow-stress coefficients. fcr_press_nominal writes the
 * reference's values, the ones every call without parameters is compiled with. The friction knee (0.5 m/s) and the
 * smooth model's epsilon belong to the model's form and are not parameters.
 *
 * A parameter TABLE is device memory, fp64, 8-byte aligned, 28 doubles per row in the order of the struct's fields; a
 * kernel lane reads ITS trajectory's row once and derives its coefficients from it. Rows are addressed by strides in
 * ELEMENTS, 0 = shared (as x0_stride etc. above): trajectory b of model m reads row
 *   press + m * stride_model + b * stride_traj.
 * B = 0 (or n_models = 0) stays a no-op and reads no row: the table may then be NULL. A stride is 0 or a multiple of 28; stride_model, unless 0, is at least B * stride_traj (and at least 28). Nothing
 * synchronises inside a call, so the rows themselves are not checked: a bad row propagates NaN, as a bad x0 does.
 * A host-side `model` (below) IS checked: every field finite, and m_mass, t1, rho, d1, d2, v1_0, v2_0, w0, h0, b0 > 0
 * (the equations divide by them or take their root).
 *
 *   fcr_plant_rk4_press            fcr_plant_rk4 where trajectory b integrates the press of row b * stride_traj.
 *   fcr_feasibility_project_press  fcr_feasibility_project where the projection integrates `model` (NULL = nominal).
 *   fcr_closed_loop_run_bank_press fcr_closed_loop_run_bank where the loop steps each trajectory's own press (the TRUE
 *                                  plant, from the table) and the feasibility projection, if any, integrates `model`
 *                                  (the controller's idea of the press; NULL = nominal), one set for the launch.
 * With the nominal row everywhere and the nominal model each computes what its counterpart computes, bit for bit.
 */
typedef struct fcr_press {
    double m_mass, b_damp, ft, d1, d2, g, kb, v1_0, v2_0, kl_1, kl_2, cd, rho, d, ps, pt, mu, k, w0, h0, b0, t_def, t1,
        m0, m1, m2, m3, m4;
} fcr_press;

void fcr_press_nominal(fcr_press *out);

int fcr_plant_rk4_press(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x0,
                        const double *u, double *x, const double *press, int64_t stride_traj, void *stream);

int fcr_feasibility_project_press(const fcr_feasibility *f, const fcr_press *model, int32_t B, const double *x,
                                  const double *u_nn, double *u, int32_t *flag, double *v, void *stream);

int fcr_closed_loop_run_bank_press(const fcr_closed_loop_bank *args, const double *press, int64_t stride_model,
                                   int64_t stride_traj, const fcr_press *model, void *stream);

/*
 * The differentiable press (a pure addition to ABI 8): the vector-Jacobian products of fcr_plant_rk4 and of the
 * noise-free fcr_closed_loop_run without recovery, by the hand-written adjoint of the RK4 step. The
 * caller keeps what the forward call stored and passes the gradient of its scalar with respect to every stored value.
 *
 *   fcr_plant_rk4_vjp: x (B,S+1,5) and u (B,S) of fcr_plant_rk4 / fcr_plant_rk4_press, g_x (B,S+1,5) = dL/dx ->
 *     g_x0 (B,5) = dL/dx0 and g_u (B,S) = dL/du. press / stride_traj: the table the forward integrated (NULL, 0: the
 *     reference's press). S = 0: g_x0 = g_x[:,0]. B = 0 is a no-op.
 *   fcr_closed_loop_vjp: the forward's fields, the stored x (B,T+1,5) and u (B,T), g_x and g_u (B,T) ->
 *     g_x0 (B,5); dv (B,T) = dL/d(the controller's clamped fp32 output); and the controller's parameter gradients in
 *     fp64, g_w_inp (ctrl_hidden,3), g_b_inp (ctrl_hidden), g_w_out (ctrl_hidden), summed over all (b,t) in a fixed
 *     order (no atomics: the same call twice gives the same bits). ctrl_hidden is 1..256 as in the forward. ws: device
 *     scratch of fcr_closed_loop_vjp_workspace_size bytes. T = 0: g_x0 = g_x[:,0] and zero parameter gradients; B = 0:
 *     zero parameter gradients (where their pointers are given).
 *
 * Conventions where the derivative is singular: the deformation force is differentiated only where y > 0 && y_dot > 0
 * (at y_dot = 0 its slope is infinite and is taken as 0); the valve flow's derivatives with respect to its pressure
 * difference a and to z are 0 at a = 0, its branch chosen by z >= 0 as in the forward; the friction's slope is FT/0.5
 * where |y_dot| <= 0.5 and 0 elsewhere; the smooth pressure floor's is 0.5 (1 + p / sqrt(p^2 + eps)). The controller's
 * fp32 chain is recomputed from the stored record in the forward's operation order, so its ReLU masks (ReLU'(0) = 0) and
 * Hardtanh mask (1 only for -1 < v < 1) are the forward's; float casts are differentiated as the identity.
 * Not covered: process / measurement noise, feasibility recovery. (Gradients with respect to the press parameters: the
 * *_press calls below.)
 */
int fcr_plant_rk4_vjp(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x, const double *u,
                      const double *g_x, const double *press, int64_t stride_traj, double *g_x0, double *g_u,
                      void *stream);

typedef struct fcr_closed_loop_grad {
    int32_t B, T;
    double ts;
    int32_t substeps, smooth;
    const double *ref;                                   /* (B,T) */
    const float *ctrl_w_inp, *ctrl_b_inp, *ctrl_w_out;
    int32_t ctrl_hidden;
    double in_scale[2];
    double ref_scale, out_scale;
    const double *x, *u;                                 /* the forward's outputs */
    const double *g_x, *g_u;                             /* (B,T+1,5), (B,T): incoming */
    const double *press;                                 /* the forward's table, or NULL: the reference's press */
    int64_t stride_traj;                                 /* elements between trajectories' rows; 0 = shared */
    double *g_x0, *dv;                                   /* (B,5), (B,T) */
    double *g_w_inp, *g_b_inp, *g_w_out;                 /* (ctrl_hidden,3), (ctrl_hidden), (ctrl_hidden) fp64 */
} fcr_closed_loop_grad;

int fcr_closed_loop_vjp_workspace_size(int32_t B, int32_t T, int32_t ctrl_hidden, size_t *bytes);
int fcr_closed_loop_vjp(const fcr_closed_loop_grad *args, void *ws, size_t ws_bytes, void *stream);

/*
 * Gradients with respect to the press (a pure addition to ABI 8): the two calls above, which compute
 * what they compute there, and beside it g_press (B,28) = dL/d(the 28 fields of each trajectory's row, fcr_press's
 * order) — per trajectory whatever the stride: under stride_traj = 0 row b holds trajectory b's share of the shared
 * row's gradient, which fcr_press_grad_sum adds up. press is required (the reference's literals have no gradient).
 * The parameter terms are collected along the same reverse recursion, each right-hand side's (df/dc)^T a over the
 * coefficients derive() forms, then carried to the row through derive()'s Jacobian. Conventions as above: the eleven
 * deformation fields (mu, k, w0, h0, b0, t_def, m0..m4) receive gradient only where y > 0 && y_dot > 0; cd, rho, d, ps
 * and pt receive 0 from a valve at a zero pressure difference, ps and pt by the branch z >= 0 as in the forward; ft
 * receives y_dot / 0.5 inside the knee and 1 outside. S = 0 / T = 0: g_press = 0. B = 0 is a no-op.
 *
 *   fcr_press_grad_sum: g_row (28) = sum over b of g_press (B,28), in fp64 and in a fixed order (blocks of 256
 *     trajectories added in order, then the blocks in order; no atomics: the same call twice gives the same bits).
 *     ws: device scratch of fcr_press_grad_sum_workspace_size bytes. B = 0: g_row = 0 (where given).
 */
int fcr_plant_rk4_vjp_press(int32_t B, int32_t S, double ts, int32_t substeps, int32_t smooth, const double *x,
                            const double *u, const double *g_x, const double *press, int64_t stride_traj, double *g_x0,
                            double *g_u, double *g_press, void *stream);
int fcr_closed_loop_vjp_press(const fcr_closed_loop_grad *args, double *g_press, void *ws, size_t ws_bytes, void *stream);
int fcr_press_grad_sum_workspace_size(int32_t B, size_t *bytes);
int fcr_press_grad_sum(int32_t B, const double *g_press, double *g_row, void *ws, size_t ws_bytes, void *stream);

/*
 * Training a bank of controllers on the press (a pure addition to ABI 8): the adjoint of the noise-free
 * closed loop without recovery for n_models controllers in ONE reverse launch on the record fcr_closed_loop_run_bank /
 * _bank_press stored, then the parameter gradients of all models in one launch and one reduction.
 *
 * fcr_closed_loop_bank_grad: fcr_closed_loop_grad's fields for the stacked models. ctrl_w_inp (M,hidden,3), ctrl_b_inp
 * and ctrl_w_out (M,hidden); x (M,B,T+1,5), u (M,B,T); model m reads its references from ref + m * ref_stride ELEMENTS
 * (0: one (B,T) shared, else >= B*T) and trajectory b of model m the press row press + m * stride_model + b * stride_traj
 * (NULL: the reference's press, both strides 0), as the forward did. truncate = K > 0 is truncated back-propagation:
 * the states x_t at t = K, 2K, ... < T count as constants for the step (controller included) that starts from them,
 * while the direct terms on x_t and u_{t-1} still reach the step that produced them; 0 = none.
 * Outputs: g_x0 (M,B,5) or NULL (not wanted); dv (M,B,T) = dL/d(each controller's clamped fp32 output); g_w_inp
 * (M,hidden,3), g_b_inp (M,hidden), g_w_out (M,hidden) in fp64, model m's the bits fcr_closed_loop_vjp gives for model m
 * alone. ws: device scratch of fcr_closed_loop_bank_vjp_workspace_size bytes (M times the single model's, plus the
 * loss's partial sums). Conventions at the singular points: fcr_closed_loop_vjp's.
 *
 *   fcr_closed_loop_bank_vjp: the general vector-Jacobian product, g_x (M,B,T+1,5) and g_u (M,B,T) incoming.
 *     T = 0: g_x0 = g_x[:,:,0] and zero parameter gradients.
 *   fcr_closed_loop_bank_loss_vjp: the gradient of the MPC loss on the record, whose cotangents are formed in registers
 *     (nothing but the record is read). In fp64, with s_v = ref_scale, s_u = out_scale, (s_p1, s_p2) = p_scale and model
 *     m's row (alpha, p1_lo, p1_hi, p2_lo, p2_hi, w):
 *       e_t = (x[t+1,1] - ref[t]) / s_v;  d_t = (u_t - u_{t-1}) / s_u, d_0 = (u_0 - u_prev[b]) / s_u or 0 (u_prev NULL);
 *       c_t = w (relu(p1_lo - P1) + relu(P1 - p1_hi) + relu(p2_lo - P2) + relu(P2 - p2_hi)), P1 = x[t+1,2] / s_p1,
 *       P2 = x[t+1,3] / s_p2;  cost[m,b] = (1/T) sum_t (e_t^2 + alpha d_t^2 + c_t);  loss[m] = (1/B) sum_b cost[m,b],
 *     summed in a fixed order without atomics (the same call twice gives the same bits). relu'(0) = 0; an infinite bound
 *     switches its side off. terms is the DEVICE table the kernel reads, (M,6) fp64, row m * terms_stride (6, or 0: one
 *     row for all); terms_host is the same rows in HOST memory, which the call checks before any device call: no NaN,
 *     lo <= hi, w >= 0. u_prev: (B) shared (u_prev_stride 0) or (M,B) (stride B), or NULL. value_only != 0: only cost
 *     and loss are computed and every gradient pointer may be NULL. T = 0: zero loss, cost and gradients.
 * n_models = 0 or B = 0 is a no-op; outputs are zeroed where given and not empty. Stream-ordered; nothing allocates.
 */
typedef struct fcr_closed_loop_bank_grad {
    int32_t n_models, B, T;
    double ts;
    int32_t substeps, smooth;
    const double *ref;
    int64_t ref_stride;
    const float *ctrl_w_inp, *ctrl_b_inp, *ctrl_w_out;
    int32_t ctrl_hidden;
    double in_scale[2];
    double ref_scale, out_scale;
    const double *x, *u;                                 /* the forward's outputs */
    const double *press;
    int64_t stride_model, stride_traj;
    int32_t truncate;
    double *g_x0, *dv;
    double *g_w_inp, *g_b_inp, *g_w_out;
} fcr_closed_loop_bank_grad;

typedef struct fcr_press_loss {
    const double *terms;                                 /* device, (M,6) fp64 */
    int64_t terms_stride;
    const double *terms_host;                            /* host, the same rows: n_models of them, or one (stride 0) */
    double p_scale[2];
    const double *u_prev;
    int64_t u_prev_stride;
    int32_t value_only;
    double *cost, *loss;                                 /* (M,B), (M) */
} fcr_press_loss;

int fcr_closed_loop_bank_vjp_workspace_size(int32_t n_models, int32_t B, int32_t T, int32_t ctrl_hidden, size_t *bytes);
int fcr_closed_loop_bank_vjp(const fcr_closed_loop_bank_grad *args, const double *g_x, const double *g_u, void *ws,
                             size_t ws_bytes, void *stream);
int fcr_closed_loop_bank_loss_vjp(const fcr_closed_loop_bank_grad *args, const fcr_press_loss *loss, void *ws,
                                  size_t ws_bytes, void *stream);

/*
 * Training on the press under pre-drawn process and measurement noise (a pure addition to ABI 8). The
 * forward is fcr_closed_loop_run_bank's loop: the controller reads the RECORD m_t = x[:, t], the press steps the
 * unperturbed STATE s_t with process_noise[b,t] added to the right-hand side at every RK4 stage, and x[:, t+1] = s_{t+1} +
 * meas_noise[b,t]. The adjoint seeds on the record (the loss and the metrics are evaluated there; dL/ds = dL/dm, v being
 * additive), takes the controller chain and its masks from the record, and linearises the plant at (s_t, u_t, w_t). The
 * noise is a constant: no gradient is produced for it. Feasibility recovery is not covered.
 *
 *   fcr_closed_loop_run_bank_press_state: fcr_closed_loop_run_bank_press (press NULL, both strides 0: the reference's
 *     press, fcr_closed_loop_run_bank) that stores per step (args->x, args->u required) and also writes the states to
 *     x_state (M,B,T+1,5): x_state[:, :, 0] = x0 and x_state[:, :, t+1] + meas_noise[:, t] == x[:, :, t+1] bit for bit.
 *     x, u and every statistic are the bits of the call without x_state. args->feasibility must be NULL.
 *   fcr_bank_noise: what the adjoint reads of the noisy run beside fcr_closed_loop_bank_grad. process_noise: the
 *     forward's, model m's at process_noise + m * process_stride ELEMENTS (0: one (B,T,5) shared, else >= B*T*5), or NULL
 *     (none was drawn). x_state: the forward's states, or NULL: there was no measurement noise and the record is the state.
 *   fcr_closed_loop_bank_vjp_noise / fcr_closed_loop_bank_loss_vjp_noise: fcr_closed_loop_bank_vjp /
 *     fcr_closed_loop_bank_loss_vjp on such a run: the same arguments, outputs, workspace, conventions, truncation and
 *     empty cases (n_models = 0, B = 0, T = 0); with zero-filled noise they compute what those compute.
 */
typedef struct fcr_bank_noise {
    const double *process_noise;
    int64_t process_stride;
    const double *x_state;
} fcr_bank_noise;

int fcr_closed_loop_run_bank_press_state(const fcr_closed_loop_bank *args, const double *press, int64_t stride_model,
                                         int64_t stride_traj, const fcr_press *model, double *x_state, void *stream);
int fcr_closed_loop_bank_vjp_noise(const fcr_closed_loop_bank_grad *args, const fcr_bank_noise *noise, const double *g_x,
                                   const double *g_u, void *ws, size_t ws_bytes, void *stream);
int fcr_closed_loop_bank_loss_vjp_noise(const fcr_closed_loop_bank_grad *args, const fcr_bank_noise *noise,
                                        const fcr_press_loss *loss, void *ws, size_t ws_bytes, void *stream);

/*
 * The model-predictive baseline on the press (a pure addition to ABI 8): a shooting MPC with the
 * reference's objective on the RK4 press, one lane per trajectory, all in fp64.
 *
 * Problem of one trajectory: state x_0 (5), previous command u_prev, references r_1..r_N and a press row (the
 * controller's MODEL of the press); unknowns U = (u_0..u_{N-1}); x_{k+1} = one sampling step of fcr_plant_rk4 (ts,
 * substeps, smooth) under u_k. Residuals: e_k = x_k[1] - r_k, k = 1..N; d_k = sqrt(r_u) (u_k - u_{k-1}), u_{-1} = u_prev,
 * k = 0..N-1; for k = 1..N the squared hinges sqrt(w) relu((x_k[2] - p1_hi)/s_p), sqrt(w) relu((p1_lo - x_k[2])/s_p) and
 * the same two for x_k[3] with p2_lo, p2_hi (p_bounds = {p1_lo, p1_hi, p2_lo, p2_hi}; an infinite bound switches its row
 * off, relu'(0) = 0, w = p_weight = 0 removes all four, s_p = p_scale). cost = sum residual^2. Command box
 * u_bounds[0] <= u_k <= u_bounds[1] (+-inf = none).
 *
 * The solver runs exactly K Levenberg-Marquardt iterations from lambda = lam0. One iteration from (U, lambda, c = cost(U)):
 * step Jacobians A_k, b_k by the press's adjoint (fcr_plant_rk4_vjp's step under unit cotangents: its conventions at the
 * singular points); H = J^T J, g = J^T r; active set {i: (U_i <= u_lo and g_i > 0) or (U_i >= u_hi and g_i < 0)}: row and
 * column i of H zeroed, H_ii = 1, g_i = 0; (H + lambda diag(H)) delta = -g by Cholesky with diag(H) taken before that
 * substitution; a pivot that is not positive and finite rejects the iteration; U' = clip(U + delta, u_bounds);
 * c' = cost(U'); accept iff c' < c (false for NaN): U = U', c = c', lambda = max(0.3 lambda, 1e-12); else
 * lambda = min(10 lambda, 1e12).
 *
 *   fcr_mpc_solve: one horizon for B problems. x0 (B,5), ref (B,N), u_prev (B), U0 (B,N) the initial guess or NULL
 *     (u_prev repeated); the initial guess is projected into u_bounds on load, so U is inside the box even when no
 *     iteration is accepted, while u_prev in d_0 is taken as given. model: the press rows, trajectory b reads model + b * model_stride (0: one row shared; else a
 *     multiple of 28), NULL = the reference's press. Outputs U (B,N), cost (B), grad_inf (B) = |g|_inf over the
 *     non-active entries at the last point linearised, accepted (B) int32, lam (B). trace (B,K,5) with trace_u (B,K,N),
 *     both or neither (NULL in production): per iteration (c, c', lambda before, accepted 0/1, pivot failure 0/1;
 *     c' = inf at a pivot failure) and U after the iteration.
 *   fcr_mpc_closed_loop: for t = 0..T-1 the record m_t = x[:,t] (x_t, plus meas_noise[b,t-1] as fcr_closed_loop_run
 *     records it) -> r_k = ref[b, min(t+k-1, T-1)] (preview = 1) or ref[b, t] (0) -> a solve from m_t with u_prev = u_{t-1}
 *     (u_init[b] at t = 0) warm-started from the previous plan shifted by one, its last entry repeated (t = 0: U0 or
 *     u_init repeated, projected into u_bounds) -> u_t = U[0] -> the TRUE press steps (row plant + b * plant_stride, NULL = the reference's;
 *     process_noise[b,t] added to every stage as fcr_closed_loop_run does). Outputs x (B,T+1,5), u, cost, grad_inf (B,T),
 *     accepted (B,T) int32; optional plans (B,T,N), the plan after each step's solve, and trace (B,T,K,5) with trace_u
 *     (B,T,K,N). T = 0 writes x[:,0] = x0 only.
 *   ws: device scratch of fcr_mpc_workspace_size(B, N) bytes, the lanes' matrices laid out [element][lane].
 * Refused before any device call, with a message: N outside 1..32, K outside 1..64, a lower bound above its upper one,
 * p_weight < 0, r_u < 0, lam0 <= 0, p_scale <= 0, a stride that is negative or no multiple of 28 or comes without its
 * table, a NULL required pointer, a workspace too small. B = 0 is a no-op. Stream-ordered; nothing allocates.
 */
typedef struct fcr_mpc {
    int32_t N, K;
    double ts;
    int32_t substeps, smooth;
    double r_u, lam0;
    double p_bounds[4];
    double p_weight, p_scale;
    double u_bounds[2];
} fcr_mpc;

typedef struct fcr_mpc_loop {
    int32_t B, T, preview;
    const double *x0, *ref;                              /* (B,5), (B,T) */
    const double *u_init, *U0;                           /* (B); (B,N) or NULL */
    const double *process_noise, *meas_noise;            /* (B,T,5) each, or NULL */
    const double *plant;
    int64_t plant_stride;
    const double *model;
    int64_t model_stride;
    double *x, *u, *cost, *grad_inf;
    int32_t *accepted;
    double *plans, *trace, *trace_u;                     /* optional */
} fcr_mpc_loop;

int fcr_mpc_workspace_size(int32_t B, int32_t N, size_t *bytes);
int fcr_mpc_solve(const fcr_mpc *mpc, int32_t B, const double *x0, const double *ref, const double *u_prev, const double *U0,
                  const double *model, int64_t model_stride, double *U, double *cost, double *grad_inf, int32_t *accepted,
                  double *lam, double *trace, double *trace_u, void *ws, size_t ws_bytes, void *stream);
int fcr_mpc_closed_loop(const fcr_mpc *mpc, const fcr_mpc_loop *loop, void *ws, size_t ws_bytes, void *stream);

/*
 * Training-sample windows: the tables of the concatenated per-trajectory
 * SequenceDatasets (Functions.py:92-132, built by Data.get_individual_dataset :479-516 and
 * ConcatDataset, UL/Main.py:270-279), resident in device memory.
 *   X (rows, nx) features [y_dot, z, ref]; Y (rows, ny) target; Z (rows, nz) recurrent features;
 *   rows = trajectories · traj_len (T_TRAJ rows each); lookback = window rows (10, UL/Main.py:267).
 */
typedef struct fcr_windows {
    int64_t rows;
    int32_t traj_len;
    int32_t lookback;
    int32_t nx, ny, nz;
    const float *X, *Y, *Z;
} fcr_windows;

/*
 * Batch gather = SequenceDataset.__getitem__ (Functions.py:109-132) for every global index idx[b]
 * (trajectory k = idx / traj_len, row i = idx % traj_len):
 *   x[b] = X[i],  y[b] = Y[min(i+1, traj_len-1)],  z[b, j] = Z[max(i-lookback+1+j, 0)]   (rows of trajectory k)
 * into x (B,nx), y (B,ny), z (B,lookback,nz). `bad` (device int32) receives the number of indices outside
 * [0, rows) (their outputs are zero-filled) — the reference raises IndexError for them; the Python layer
 * checks it. Stream-ordered; B = 0 only clears `bad`.
 */
int fcr_window_gather(const fcr_windows *tables, int32_t B, const int64_t *idx,
                      float *x, float *y, float *z, int32_t *bad, void *stream);

/*
 * LSTM surrogate training step: what one iteration of
 * NeuralNetwork.train_model (Model_NN/Functions.py:520-569) asks of LSTMModel (Model_NN/Functions.py:
 * 255-330, trained by Model_NN/Main.py:218-242): the forward on a window batch and loss.backward() into
 * every weight. `dims` uses B, H, L (=10), layers (=3), in_dim (=5), out_dim (=4); the controller fields
 * are ignored. Weights: fcr_weights' w_ih/w_hh/fc_w/fc_b (the controller pointers are ignored).
 *   x  (B,10,5)  windows          y (B,4) = fc(h_9 of the top layer) + b
 * with_backward != 0 keeps every cell's state in `ws` for fcr_lstm_backward.
 */
int fcr_lstm_workspace_size(const fcr_dims *dims, int with_backward, size_t *bytes);
int fcr_lstm_forward(const fcr_dims *dims, const fcr_weights *w, const float *x, float *y,
                     int with_backward, void *ws, size_t ws_bytes, void *stream);

/*
 * Backward of the last fcr_lstm_forward(with_backward=1) on the same `ws` and weights, given dy = dL/dy
 * (B,4): gradients of weight_ih_l{0,1,2} (4H,5|H), weight_hh_l{0,1,2} (4H,H), fc.weight (4,H), fc.bias (4),
 * OVERWRITTEN, fixed reduction order; g_x (B,10,5) = dL/dx, or NULL to skip it.
 */
int fcr_lstm_backward(const fcr_dims *dims, const fcr_weights *w, const float *dy,
                      float *const *g_w_ih, float *const *g_w_hh, float *g_fc_w, float *g_fc_b, float *g_x,
                      void *ws, size_t ws_bytes, void *stream);

/*
 * Command-driven free run of the LSTM surrogate (the results_LSTM track of NeuralNetwork.loop, Functions.py:
 * 1196-1231): T steps on its own predictions and an externally given command sequence, one launch. `dims` as for
 * fcr_lstm_forward with N = T (>= 1); H <= 52 and precision = FCR_PRECISION_FP32 only (FCR_EUNSUPPORTED otherwise).
 *   window0 (B,10,5) scaled window [y_dot,p1,p2,z,u];  cmd (B,T) scaled commands;
 *   gain    HOST float[4] or NULL (= 1): what the harness's scalers['output'].inverse_transform followed by
 *           scalers['input'].transform amount to between steps (:1009, :1198), out_scale / in_scale per column;
 *   noise   (B,T,4) additive output noise, or NULL;   xhat (B,T,4) the predictions.
 * Step 0 runs window0 with the command column of its last row replaced by cmd[:,0] (as fcr_forward does with u0);
 * step t >= 1 drops the oldest row and appends [gain * xhat_{t-1}, cmd[:,t]]; xhat_t = LSTM(window_t) + noise[:,t]
 * (the fed-back value includes the noise, simulator_make_step :1004). The workspace does not grow with T. B = 0 is a
 * no-op.
 */
int fcr_lstm_rollout_workspace_size(const fcr_dims *dims, size_t *bytes);
int fcr_lstm_rollout(const fcr_dims *dims, const fcr_weights *w, const float *window0, const float *cmd,
                     const float *gain, const float *noise, float *xhat, void *ws, size_t ws_bytes, void *stream);

/*
 * Backward of fcr_lstm_rollout: training the surrogate on its free run. Given xhat (B,T,4), the predictions the
 * forward returned for the same window0 / cmd / gain / weights (they already contain the noise, which is therefore not
 * passed), and g_xhat (B,T,4) = dL/dxhat, it writes the gradient of every LSTM weight and the readout (OVERWRITTEN,
 * shapes as fcr_lstm_backward, summed over (step, trajectory, cell) in a fixed order: two calls give the same bits) and,
 * where asked for, of window0 and cmd. g_window0[:,9,4] is exactly 0: that entry is overwritten by cmd[:,0], which
 * receives its share. noise and gain receive no gradient. `dims` as for fcr_lstm_rollout (N = T >= 1; H <= 52 and
 * FCR_PRECISION_FP32 only, FCR_EUNSUPPORTED otherwise). The windows of all T steps are rebuilt from xhat and recomputed
 * with every cell's state kept, so the workspace grows with T (fcr_lstm_rollout_backward_workspace_size); the number of
 * launches does not. Stream-ordered, no allocation, no host synchronisation. B = 0 is a no-op.
 */
typedef struct fcr_lstm_rollout_grads {
    float *g_w_ih[3], *g_w_hh[3], *g_fc_w, *g_fc_b; /* OVERWRITTEN, shapes as fcr_lstm_backward */
    float *g_window0;                               /* (B,10,5) or NULL */
    float *g_cmd;                                   /* (B,T) or NULL */
} fcr_lstm_rollout_grads;
int fcr_lstm_rollout_backward_workspace_size(const fcr_dims *dims, size_t *bytes);
int fcr_lstm_rollout_backward(const fcr_dims *dims, const fcr_weights *w, const float *window0, const float *cmd,
                              const float *gain /* host float[4] or NULL */, const float *xhat /* (B,T,4), the forward's */,
                              const float *g_xhat /* (B,T,4) */, const fcr_lstm_rollout_grads *out,
                              void *ws, size_t ws_bytes, void *stream);

/*
 * Process-wide DEFAULTS of the per-call options (a field set to FCR_OPT_INHERIT takes them).
 * Small batches (fp32-accurate mode, H 17..52): B <= max_batch runs the small-batch kernels, which split each
 * 16-trajectory group's cell over the four waves of a workgroup (the reference trains at B = 15, UL/Main.py:84,297);
 * larger B runs the fused one-wave-per-group kernels. Default 8192; 0 = never (negative clamps to 0). Returns the
 * previous value; fcr_get_small_batch_limit reads it without changing it.
 */
int fcr_set_small_batch_limit(int32_t max_batch);
int fcr_get_small_batch_limit(void);

/* Within the small-batch family, B <= max_batch (and at most 32 groups of 16 trajectories, 3 workgroups each within
 * half the device's CUs) runs the layer-pipelined geometry (csrc/fcr_pipe.h: one workgroup per LSTM layer and window
 * set, the layers and windows as a wavefront; results bit-identical to the one-workgroup-per-group kernels). Default
 * 512; 0 = never.
 * Process-wide; returns the previous value; fcr_get_small_pipe_limit reads it. */
int fcr_set_small_pipe_limit(int32_t max_batch);
int fcr_get_small_pipe_limit(void);

/* The pipelined geometry's window sets S: set s takes windows s, s + S, ... so windows run concurrently (every window
 * is an LSTM run from zero state; only the prediction feedback is serial); the forward runs 2 S workgroups per group
 * (S <= 4), the backward 3 S (S <= 3). 0 (default) = the most that fit (within half the CUs, S <= N); k > 0 caps S at
 * k. Results are bit-identical for every S. Process-wide; returns the previous value; fcr_get_small_pipe_sets reads
 * it. */
int fcr_set_small_pipe_sets(int32_t sets);
int fcr_get_small_pipe_sets(void);

/*
 * H > 52 (the batch-wide GEMM path): how many bytes of "kept windows" fcr_workspace_size(with_backward = 1)
 * may add. The backward recomputes each window's cells from a per-window checkpoint (the rollout's memory
 * floor); a kept window instead holds the forward's gate activations and c for all its 30 cells
 * (30 B 5H floats: 10 GB at B = 65 536, H = 256 — torch's autograd keeps at least that for every window),
 * so its backward skips the recompute (config 5: a third of the step). The last windows are kept, as many
 * as the budget allows (fcr_wide_kept_windows).
 * bytes < 0 (FCR_KEEP_AUTO, the default): as many as keep the whole workspace within half of the memory that was
 * free on the device when a workspace was first sized there (cached per device: a stable count from call to call),
 * and within 40 % of the device's total memory; 0: keep none. The workspace stays allocated from the forward until
 * its backward has run (torch: until RolloutFn.backward releases it). Returns the previous budget.
 */
int64_t fcr_set_wide_keep_budget(int64_t bytes);
int64_t fcr_get_wide_keep_budget(void);

/*
 * TEST HOOK (not a reference interface; nothing on the rollout path calls it): ONE backward cell of the H > 52 path,
 * i.e. the autograd backward of one nn.LSTM cell (Functions.py:325, inside loss.backward() at :655), run by the same
 * kernel and launcher fcr_backward uses (wide_bwd_fused_kernel), on caller-given inputs, so a test can compare every
 * output element with an fp64 evaluation. H % 8 == 0, H <= 2048 (the fused cell's tiling). Per trajectory b:
 *   act (B,H,4) gate activations (i, f, g, o) = (sigmoid, sigmoid, tanh, sigmoid) of each unit's pre-activations, in
 *               the [unit][gate] layout the forward cell saves them;  c_prev (B,H) or NULL (t = 0);
 *   dh (B,H) incoming dh_t of the recurrence;  din (B,H) the layer above's input gradient at t, or NULL;
 *   dc (B,H) carried dc_t;  ->  dc_out (B,H) = dc_{t-1};
 *   layer0 == 0: out (B,2H) = dG [W_ih | W_hh] (input gradient | dh_{t-1}; only the first H columns without c_prev),
 *                w_ih (4H,H), w_hh (4H,H);
 *   layer0 != 0: out (B,H) = dG W_hh (dh_{t-1}; not written without c_prev), rowg (B,5) = dG W_ih0 (overwritten),
 *                w_ih = W_ih0 (4H,5), w_hh (4H,H).
 * dG are the gate gradients of the cell update c = f c_prev + i g, h = o tanh(c) for dh + din and dc. Scratch:
 * fcr_wide_bwd_cell_workspace bytes, 256-byte aligned.
 */
int fcr_wide_bwd_cell_workspace(int32_t B, int32_t H, int32_t layer0, size_t *bytes);
int fcr_wide_bwd_cell(int32_t B, int32_t H, int32_t layer0, const float *w_ih, const float *w_hh, const float *act,
                      const float *c_prev, const float *dh, const float *din, const float *dc, float *out,
                      float *dc_out, float *rowg, void *ws, size_t ws_bytes, void *stream);

/*
 * One epoch of the supervised baseline (Supervised Learning/Functions.py:396-464: NeuralNetwork.train_model and
 * validate_model) for n_models independent 3 -> hidden -> 1 FNNModels (SL/Main.py:143-159) over one sample table, in
 * ONE launch: one workgroup per model keeps its parameters, AdamW moments and step counter on the chip and walks the
 * batches in order (csrc/fcr_supervised.h). Batch j is rows perm[m, j*batch_size : min((j+1)*batch_size, n_samples)]
 * of (X, y), so the last batch may be short and is averaged over its own size (DataLoader(drop_last=False) with a
 * mean-reduced loss). Per batch: out = Hardtanh(w_out . ReLU(w_inp x + b_inp)); loss[m, j] = mean |out - y|
 * (FCR_LOSS_L1, nn.L1Loss) or mean (out - y)^2 (FCR_LOSS_MSE, nn.MSELoss); with train != 0 its autograd gradient
 * (sign(0) = 0, Hardtanh' = 1 on the open interval, ReLU'(0) = 0) and one torch.optim.AdamW step (decoupled decay
 * p *= 1 - lr*weight_decay, bias-corrected moments, eps outside the square root, no amsgrad). Parameters, moments and
 * step are updated IN PLACE when the launch ends; with train == 0 only `loss` is written. Sums run in a fixed order:
 * the same call twice gives the same bits. No workspace. n_models = 0 is a no-op.
 * The entries of perm must lie in [0, n_samples): the caller checks them (the kernel clamps what it reads).
 */
#define FCR_LOSS_L1 0
#define FCR_LOSS_MSE 1
typedef struct fcr_supervised {
    int32_t n_models;     /* independent models, one workgroup each                                   */
    int32_t n_samples;    /* rows of X and y, 1 .. 2^30                                                */
    int32_t batch_size;   /* >= 1; any size (the lanes loop over a batch larger than the workgroup)    */
    int32_t hidden;       /* 1 .. 64                                                                   */
    int32_t loss_kind;    /* FCR_LOSS_L1 or FCR_LOSS_MSE                                               */
    int32_t train;        /* 0: losses only (validate_model); 1: gradient + AdamW step per batch       */
    double lr, beta1, beta2, eps, weight_decay;   /* torch.optim.AdamW's (read with train != 0)        */
    const float *X;       /* (n_samples, 3)                                                            */
    const float *y;       /* (n_samples)                                                               */
    const int32_t *perm;  /* (n_models, n_samples) sample order per model; NULL with train == 0: 0..n-1 */
    float *w_inp;         /* (n_models, hidden, 3)  fc_inp.weight of every model                       */
    float *b_inp;         /* (n_models, hidden)     fc_inp.bias                                        */
    float *w_out;         /* (n_models, hidden)     fc_out.weight                                      */
    float *exp_avg_w_inp, *exp_avg_b_inp, *exp_avg_w_out;            /* AdamW exp_avg, shapes as above; train only   */
    float *exp_avg_sq_w_inp, *exp_avg_sq_b_inp, *exp_avg_sq_w_out;   /* AdamW exp_avg_sq;                train only   */
    float *step;          /* (n_models) optimizer steps taken so far, as torch keeps them (fp32); train only */
    float *loss;          /* (n_models, ceil(n_samples / batch_size)) per-batch losses, overwritten    */
} fcr_supervised;
int fcr_supervised_epoch(const fcr_supervised *args, void *stream);

/* Thread-local description of the last error (never NULL). */
const char *fcr_last_error(void);

/* FCR_ABI_VERSION of the loaded library. */
int fcr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FCR_H */
