// The split-operand arithmetic of the DTYPE float32 path (library option f32_split = 1), once: csrc/f32.hip (f32x3_igemm_kernel),
// csrc/f32_wstat.hip, csrc/f32_conv3x3.hip, csrc/dynconv.hip (f32x3_dynconv_kernel) and csrc/localattn.hip (mode 1) all multiply through it.
//
// An fp32 value v becomes two fp16 numbers hi = fp16(v), lo = fp16(v - hi), and a product is accumulated in fp32 as three passes of
// v_mfma_f32_32x32x16_f16 (exact fp16 x fp16 products) in ONE fixed order, the two small terms first:
//     activation lo x weight hi,   activation hi x weight lo,   activation hi x weight hi.
// What is dropped is lo x lo (2^-22 of the product) and the rounding of lo.  The order is by ROLE, not by MFMA operand slot: the kernels
// that keep the weights as the MFMA's first operand (f32_wstat, localattn: the transposed product) run the same three terms in the same
// order, which is what makes them bit-identical to the tiled kernel (tests/test_gpu_f32.py::test_f32_wstat_matches_tiled).
// tests/test_host_logic.py restates the split and the passes in numpy.
#pragma once

#include "common.h"

namespace f32_split {

constexpr float kFp16Max = 65504.f;          // |v| beyond this becomes inf in its hi part where fp32 arithmetic would not

// hi = fp16(v) rounded to nearest even, lo = fp16(v - hi) (v - hi is exact in fp32)
__device__ __forceinline__ void split4(const float4v v, half4& h, half4& l) {
    h = __builtin_convertvector(v, half4);
    l = __builtin_convertvector(v - __builtin_convertvector(h, float4v), half4);
}
// eight consecutive k of one row (v0 | v1) as the fp16 MFMA's operand vectors; `mx` keeps the running maximum of |v| for report_range
__device__ __forceinline__ void split8(const float4v v0, const float4v v1, half8& h, half8& l, float& mx) {
#pragma unroll
    for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fmaxf(__builtin_fabsf(v0[e]), __builtin_fabsf(v1[e])));
    const half4 h0 = __builtin_convertvector(v0, half4), h1 = __builtin_convertvector(v1, half4);
    const half4 l0 = __builtin_convertvector(v0 - __builtin_convertvector(h0, float4v), half4);
    const half4 l1 = __builtin_convertvector(v1 - __builtin_convertvector(h1, float4v), half4);
    h = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    l = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}
// a value beyond the fp16 range is reported, never a silent inf: the model checks the flag at the batch's host synchronisation and
// raises (f32_split = 0 has no such limit)
__device__ __forceinline__ void report_range(int* range_flag, float mx) {
    if (range_flag && mx > kFp16Max) atomicOr(range_flag, 1);
}

// Pass `pass` (0, 1, 2: a compile-time constant after unrolling) of the three-pass product of one 32 x 32 tile.  WEIGHT_IS_A: the
// weights are the MFMA's first operand (D = W A^T) instead of the activations; the term of a pass is the same either way.
template <bool WEIGHT_IS_A>
__device__ __forceinline__ float16v mfma_pass(int pass, const half8 act_hi, const half8 act_lo, const half8 wgt_hi, const half8 wgt_lo, float16v acc) {
    const half8 act = pass == 0 ? act_lo : act_hi;
    const half8 wgt = pass == 1 ? wgt_lo : wgt_hi;
    return WEIGHT_IS_A ? __builtin_amdgcn_mfma_f32_32x32x16_f16(wgt, act, acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_f16(act, wgt, acc, 0, 0, 0);
}
// the three passes of one tile back to back
template <bool WEIGHT_IS_A>
__device__ __forceinline__ float16v mfma_x3(const half8 act_hi, const half8 act_lo, const half8 wgt_hi, const half8 wgt_lo, float16v acc) {
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) acc = mfma_pass<WEIGHT_IS_A>(pass, act_hi, act_lo, wgt_hi, wgt_lo, acc);
    return acc;
}

}  // namespace f32_split
