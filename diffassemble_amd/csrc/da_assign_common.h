// Distance and ordering of the greedy position assignment, shared by k_greedy_assign (da_assign.hip) and k_score2d
// (da_score2d.hip): both must rank every (piece, cell) pair identically, bit for bit.
#pragma once
#include "da_common.h"

namespace da {

__device__ __forceinline__ float dist2(const float *a, const float *b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1];
    const float d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    // a diverged sample (NaN / Inf poses) must still be assignable: +inf is the "retired" marker of rmin and a NaN
    // never wins a comparison, so non-finite distances rank as the largest finite value (the reference returns
    // some wrong assignment in that case; here the row simply goes last, and nothing indexes out of LDS)
    return d <= 3.402823466e38f ? d : 3.402823466e38f;
}

// lexicographic (value, index) minimum
__device__ __forceinline__ void lexmin(float &v, int &i, float v2, int i2) {
    if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

}  // namespace da
