// What the COCO and the LVIS evaluator kernels (cocoeval.hip, lviseval.hip) share: the score's place in a 64-bit sort key and the COCO
// bbox IoU in float64.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned long long u64;

// the score's bits mapped so that a greater score is a smaller number
__device__ __forceinline__ unsigned ce_score_desc(float s) {
    if (s == 0.f) s = 0.f;          // -0 and +0 are one score
    const unsigned b = __float_as_uint(s);
    return ~(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}

// d, g: x, y, w, h
__device__ __forceinline__ double coco_iou(const double dx, const double dy, const double dw, const double dh, const double* __restrict__ g,
                                           const bool crowd) {
#pragma clang fp contract(off)
    const double w = fmin(dx + dw, g[0] + g[2]) - fmax(dx, g[0]);
    if (w <= 0.0) return 0.0;
    const double h = fmin(dy + dh, g[1] + g[3]) - fmax(dy, g[1]);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double da = dw * dh, ga = g[2] * g[3];
    const double u = crowd ? da : (da + ga) - i;
    return __ddiv_rn(i, u);
}
