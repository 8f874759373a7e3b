// u64 and the score's place in a sort key of the evaluator kernels.  Apart from the sort this is all that evalaccum.hip has in common with
// the match kernels; evalmatch.h, which includes this file, holds the rest of the shared code.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned long long u64;

// the score's bits mapped so that a greater score is a smaller number
__device__ __forceinline__ unsigned ce_score_desc(float s) {
    if (s == 0.f) s = 0.f;          // -0 and +0 are one score
    const unsigned b = __float_as_uint(s);
    return ~(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}
