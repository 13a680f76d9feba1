// What every weight entry asks of one cloud's per-point weights -- finite, >= 0, not all zero -- and their sum: plain C++, no
// HIP type and no HIP header (tests/point_weights_main.cpp compiles it alone).  The messages are the context's
// (hgmm_ctx.h: check_point_weights).
#pragma once
#include <cmath>
#include <cstdint>

namespace hgmm {

enum WeightVerdict { WEIGHTS_OK, WEIGHTS_BAD_VALUE, WEIGHTS_ALL_ZERO, WEIGHTS_SUM_NOT_FINITE };
struct WeightScan { int verdict; int64_t index; double value, sum; };   // (BAD_VALUE) the first offender and what it holds; (OK) the sum

// One pass.  The sum is accumulated in double in INDEX ORDER: it is what the M-steps divide by (pi = m0 / W), bit for bit,
// so neither the order nor the accumulator's type may change.  float input: SUM_NOT_FINITE cannot occur -- n * FLT_MAX is far
// below DBL_MAX for any n an int64_t holds -- so the float32 entries, which never made that test, keep every outcome.
template <class T>
inline WeightScan scan_weights(const T* w, int64_t n) {
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!(w[i] >= 0) || !(w[i] < INFINITY)) return {WEIGHTS_BAD_VALUE, i, (double)w[i], 0.0};   // (NaN fails the first comparison)
        sum += (double)w[i];
    }
    if (!(sum > 0.0)) return {WEIGHTS_ALL_ZERO, -1, 0.0, sum};
    if (!(sum < INFINITY)) return {WEIGHTS_SUM_NOT_FINITE, -1, 0.0, sum};
    return {WEIGHTS_OK, -1, 0.0, sum};
}

}  // namespace hgmm
