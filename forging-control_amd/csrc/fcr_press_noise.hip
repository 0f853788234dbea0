// fcr_press_noise.hip — the kernels of training on the press under process and measurement noise (fcr_press_noise.h;
// DESIGN.md §7.18) and their launches, in a translation unit of their own so that every other code object is what it was.
// The entry points and their checks are beside their noise-free twins: fcr_closed_loop_run_bank_press_state in
// fcr_rows.hip, fcr_closed_loop_bank_vjp_noise / fcr_closed_loop_bank_loss_vjp_noise in fcr_train.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr.h"
#include "fcr_host.h"
#include "fcr_plant.h"
#include "fcr_press_host.h"

// The non-template kernels of these three headers have external host stubs and are compiled into fcr_rows.hip,
// fcr_grad.hip and fcr_train.hip; this unit reads the headers for their __device__ functions and argument structs, so
// here every kernel of theirs gets internal linkage (no second host stub under the same name) and is never launched.
#pragma push_macro("__global__")
#undef __global__
#define __global__ static __attribute__((global))
#include "fcr_closed_loop.h"
#include "fcr_press_grad.h"
#include "fcr_press_train.h"
#pragma pop_macro("__global__")

#include "fcr_press_noise.h"

namespace fcr {
namespace press_noise {

namespace {
template <bool TABLE>
using Press = std::conditional_t<TABLE, plant::Coeffs, plant::Nominal>;
}

int launch_bank_vjp(const press_train::BankGradArgs &a, const press_train::TensorSeed *tensor,
                    const press_train::LossSeed *loss, const NoiseGrad &n, bool smooth, bool kept, bool table, dim3 grid,
                    hipStream_t s) {
    const dim3 block(kGradBlock);
    if (loss) {
        const auto k = select([](auto sm, auto kp, auto tb) {
            return &closed_loop_bank_vjp_noise_kernel<sm(), kp(), Press<tb()>, press_train::LossSeed>; }, smooth, kept, table);
        hipLaunchKernelGGL(k, grid, block, 0, s, a, *loss, n);
        return launch_check("closed_loop_bank_vjp_noise_kernel<LossSeed>");
    }
    const auto k = select([](auto sm, auto kp, auto tb) {
        return &closed_loop_bank_vjp_noise_kernel<sm(), kp(), Press<tb()>, press_train::TensorSeed>; }, smooth, kept, table);
    hipLaunchKernelGGL(k, grid, block, 0, s, a, *tensor, n);
    return launch_check("closed_loop_bank_vjp_noise_kernel<TensorSeed>");
}

int launch_bank_state(const closed_loop::ClArgs &a, const closed_loop::BankStrides &strides,
                      const closed_loop::StatsArgs &stats, const double *wn, const double *vn,
                      const closed_loop::PressTable *table, bool smooth, double *x_state, dim3 grid, hipStream_t s) {
    const dim3 block(closed_loop::kClBlock);
    const closed_loop::PressTable none{nullptr, 0, 0};
    const auto k = select([](auto sm, auto tb) { return &closed_loop_bank_state_kernel<sm(), tb()>; }, smooth,
                          table != nullptr);
    hipLaunchKernelGGL(k, grid, block, 0, s, a, strides, stats, wn, vn, table ? *table : none, x_state);
    return launch_check("closed_loop_bank_state_kernel");
}

}  // namespace press_noise
}  // namespace fcr
