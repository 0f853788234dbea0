// fcr_rowgrad.h — which window-row gradients sum into one row of the extended sequence (fcr_bwd.h's row_grad).
//
// Row rho of the extended sequence (states rows 0..9, then one appended row per step) lies in the windows
// w = max(0, rho - 9) .. min(N - 1, rho), at position t = rho - w; its gradient is the sum of dx(w, t) over them, taken
// from the newest window down (w_hi .. w_lo). The kernel wants every load of that sum in flight before the first add,
// so it runs a fixed kL terms: term i is window w_hi - i while that is >= w_lo, and after that a term that loads an
// in-range entry (clamped to w_lo) and adds +0.0f in its place.
//
// Bit-equality with the run-time-bounded loop: the valid terms come first and in the same order; the running sum
// starts from +0.0f, and a sum that started from +0.0f is never -0.0f (x + y is -0 only if both are), so every
// trailing `sum + 0.0f` returns sum unchanged (NaN included: it stays the NaN it was).
#pragma once
#include "fcr_common.h"

namespace fcr {

struct RowTerm {
    int w, t;     // the dxrow entry the term loads: always inside [0, N) x [0, kL)
    bool valid;   // false: the loaded value is replaced by +0.0f
};

// term i (0 .. kL-1) of row rho's sum over an N-window rollout; rho in kL-1 .. N+kL-2 (the rows with a gradient)
__host__ __device__ constexpr RowTerm row_term(int rho, int N, int i) {
    const int w_hi = rho < N - 1 ? rho : N - 1;
    const int w_lo = rho - (kL - 1) > 0 ? rho - (kL - 1) : 0;
    const int w = w_hi - i;
    const bool valid = w >= w_lo;
    const int wc = valid ? w : w_lo;
    return RowTerm{wc, rho - wc, valid};
}

namespace rowgrad_check {
// the run-time-bounded loop this replaces, term by term
constexpr bool same_as_loop(int N) {
    for (int rho = kL - 1; rho <= N + kL - 2; ++rho) {
        const int w_hi = rho < N - 1 ? rho : N - 1;
        const int w_lo = rho - (kL - 1) > 0 ? rho - (kL - 1) : 0;
        int i = 0;
        for (int w = w_hi; w >= w_lo; --w, ++i) {
            if (i >= kL) return false;
            const RowTerm e = row_term(rho, N, i);
            if (!e.valid || e.w != w || e.t != rho - w || e.t < 0 || e.t >= kL) return false;
        }
        if (i == 0) return false;   // every such row lies in at least one window
        for (; i < kL; ++i) {       // the rest trail, add nothing, and load inside the slab
            const RowTerm e = row_term(rho, N, i);
            if (e.valid || e.w < 0 || e.w >= N || e.t < 0 || e.t >= kL) return false;
        }
    }
    return true;
}
constexpr bool same_as_loop_all() {
    for (int N = 1; N <= 25; ++N)
        if (!same_as_loop(N)) return false;
    return true;
}
static_assert(same_as_loop_all(), "row_term must enumerate row_grad's windows in the old loop's order");
}  // namespace rowgrad_check

}  // namespace fcr
