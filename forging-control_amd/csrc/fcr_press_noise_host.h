// fcr_press_noise_host.h — what fcr_press_noise.hip (the kernels of training on the press under noise)
// offers the files that hold its entry points' checks: fcr_rows.hip (the forward that stores x_state, beside run_bank)
// and fcr_train.hip (the adjoints, beside bank_vjp, whose parameter-gradient and loss kernels they reuse as they are).
// Plain declarations: the kernels' argument structs are named, not defined, so this header includes no kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace fcr {

namespace closed_loop {
struct ClArgs;
struct BankStrides;
struct StatsArgs;
struct PressTable;
}  // namespace closed_loop

namespace press_train {
struct BankGradArgs;
struct TensorSeed;
struct LossSeed;
}  // namespace press_train

namespace press_noise {

// What the noisy reverse loop reads beside BankGradArgs: model m's process noise at w + m * w_stride ELEMENTS (0: one
// (B,T,5) shared by all models; w NULL: none was drawn) and the forward's states x_state (M,B,T+1,5) (NULL: the record).
struct NoiseGrad {
    const double *w;
    long long w_stride;
    const double *x_state;
};

// closed_loop_bank_vjp_noise_kernel<smooth, kept, table, seed>: exactly one of tensor / loss is set. Enqueues only.
int launch_bank_vjp(const press_train::BankGradArgs &a, const press_train::TensorSeed *tensor,
                    const press_train::LossSeed *loss, const NoiseGrad &n, bool smooth, bool kept, bool table, dim3 grid,
                    hipStream_t s);

// closed_loop_bank_state_kernel<smooth, table != NULL>: the noisy storing bank loop that also writes x_state
int launch_bank_state(const closed_loop::ClArgs &a, const closed_loop::BankStrides &strides,
                      const closed_loop::StatsArgs &stats, const double *wn, const double *vn,
                      const closed_loop::PressTable *table, bool smooth, double *x_state, dim3 grid, hipStream_t s);

}  // namespace press_noise
}  // namespace fcr
