// fcr_fnn_sample.h — the FNNModel's per-sample forward (Functions.py:261-289) as device functions, shared by the
// controller's kernels (fcr_fnn.h, compiled in fcr_abi.hip) and the supervised epoch (fcr_supervised.h, in fcr_rows.hip).
#pragma once
#include "fcr_common.h"

namespace fcr {
namespace fnn {

constexpr int kFnnBlock = 256;
constexpr int kFnnMaxHidden = 64;   // one wave's lanes are the hidden units in the backward
constexpr int kFnnItems = 256;      // samples per backward block

// params -> LDS records [k][W0 W1 W2 b wout]
__device__ __forceinline__ void load_params(float (*sp)[5], int hidden, const float *W, const float *bi,
                                            const float *wo) {
    for (int i = threadIdx.x; i < hidden * 5; i += blockDim.x) {
        const int k = i / 5, p = i % 5;
        sp[k][p] = p < 3 ? W[k * kCtrlIn + p] : (p == 3 ? bi[k] : wo[k]);
    }
}

// pre-Hardtanh output of one sample (z_k = W_k·x + b_k; pre = Σ_k wout_k relu(z_k))
__device__ __forceinline__ float fnn_sample(const float (*sp)[5], int hidden, float x0, float x1, float x2) {
    float acc = 0.0f;
    for (int k = 0; k < hidden; ++k) {
        const float z = fmaf(sp[k][2], x2, fmaf(sp[k][1], x1, sp[k][0] * x0)) + sp[k][3];
        acc = fmaf(sp[k][4], relu(z), acc);
    }
    return acc;
}

}  // namespace fnn
}  // namespace fcr
