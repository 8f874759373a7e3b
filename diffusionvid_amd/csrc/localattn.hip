// Local box-level attention: the out-projection of the MultiheadAttention, its bias and the LayerNorm behind it
// (mega_core/modeling/roi_heads/box_head/box_head.py:360-363: attn_ = layer_norm(local_attn(...)[0])) as ONE row kernel.
//
// One wave owns 32 rows of the [rows, 256] attention output and all 256 output channels: eight 32 x 32 accumulator tiles
// (128 fp32 registers per lane).  The weights are the FIRST MFMA operand, so the accumulator layout is D[channel][row]: lane l
// holds row (l & 31) and 128 of its 256 channels, lane l ^ 32 the other 128 -- the LayerNorm statistics of a row are a sum over a
// lane's own registers plus ONE shuffle, and the pre-LayerNorm rows never leave the registers (the layer-by-layer form writes
// them to HBM as fp32 and reads them back).  Two-pass statistics (mean, then centred squares), eps 1e-5.
//
// MODE 0 (DTYPE float16): fp16 rows, fp16 weights in fragment order (weights.hip: make_frags), v_mfma_f32_32x32x16_f16, fp32 sums.
// MODE 1 (DTYPE float32, option f32_split = 1): fp32 rows split in the kernel into (hi, lo) fp16 parts, the scaled weight rows as
//         (hi, lo) fragment planes, the three MFMA passes of csrc/f32_split.h with the weights as the first operand, the two small ones in the opposite order; a row value beyond the fp16 range
//         sets `range_flag`.
// MODE 2 (DTYPE float32, f32_split = 0): exact fp32 products on v_mfma_f32_32x32x2f32, the scaled fp32 rows [256][256] read in place.
// MODE 1 / 2 multiply channel n's sum by wscale[n] (the power of two the packed row was divided by, weights.hip: make_conv).
#include "f32_split.h"
#include "kernels.h"

namespace {

constexpr int LD = 256;          // hidden size = row length = K

template <int MODE>
__global__ __launch_bounds__(256) void outproj_ln_kernel(const void* __restrict__ xin, const half_t* __restrict__ wf_hi,
                                                          const half_t* __restrict__ wf_lo, const float* __restrict__ w32,
                                                          const float* __restrict__ wscale, const float* __restrict__ bias,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ out, int rows, int* __restrict__ range_flag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (r0 >= rows) return;                                   // (no barrier in this kernel: whole waves leave)
    const int c = lane & 31, h = lane >> 5;
    const long row = r0 + c;
    const long rrow = row < rows ? row : rows - 1;            // ragged last tile: read a valid row, store nothing
    float16v acc[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[nt][j] = 0.f;

    if constexpr (MODE == 0) {
        const half_t* x = reinterpret_cast<const half_t*>(xin) + rrow * LD + h * 8;
#pragma unroll 2
        for (int ks = 0; ks < LD / 16; ++ks) {
            const half8 xb = *reinterpret_cast<const half8*>(x + ks * 16);
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                const half8 wa = *reinterpret_cast<const half8*>(wf_hi + (((long)nt * (LD / 16) + ks) * 64 + lane) * 8);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, xb, acc[nt], 0, 0, 0);
            }
        }
    } else if constexpr (MODE == 1) {
        const float* x = reinterpret_cast<const float*>(xin) + rrow * LD + h * 8;
        float mx = 0.f;
#pragma unroll 2
        for (int ks = 0; ks < LD / 16; ++ks) {
            const float4v a = *reinterpret_cast<const float4v*>(x + ks * 16);
            const float4v b = *reinterpret_cast<const float4v*>(x + ks * 16 + 4);
            half8 xh, xl;
            f32_split::split8(a, b, xh, xl, mx);
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                const long o = (((long)nt * (LD / 16) + ks) * 64 + lane) * 8;
                const half8 wh = *reinterpret_cast<const half8*>(wf_hi + o);
                const half8 wl = *reinterpret_cast<const half8*>(wf_lo + o);
                // (this kernel has run the two small terms the other way round since it was written -- weight lo x row hi first; kept, so
                // that its results stay what they were bit for bit)
                acc[nt] = f32_split::mfma_pass<true>(1, xh, xl, wh, wl, acc[nt]);
                acc[nt] = f32_split::mfma_pass<true>(0, xh, xl, wh, wl, acc[nt]);
                acc[nt] = f32_split::mfma_pass<true>(2, xh, xl, wh, wl, acc[nt]);
            }
        }
        f32_split::report_range(range_flag, mx);
    } else {
        // eight k per step: half h of the wave takes k = 8 kc + 4 h .. + 4 of both operands, MFMA e multiplies element e of each
        // (any pairing of k between the operands gives the same sum of products)
        const float* x = reinterpret_cast<const float*>(xin) + rrow * LD + h * 4;
        const float* w = w32 + (long)c * LD + h * 4;
        for (int kc = 0; kc < LD / 8; ++kc) {
            const float4v xv = *reinterpret_cast<const float4v*>(x + kc * 8);
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                const float4v wv = *reinterpret_cast<const float4v*>(w + (long)nt * 32 * LD + kc * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], xv[e], acc[nt], 0, 0, 0);
            }
        }
    }

    // accumulator register j of tile nt = channel 32 nt + 8 (j >> 2) + 4 h + (j & 3) of row c
    float sum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n0 = nt * 32 + q * 8 + h * 4;
            const float4v bv = *reinterpret_cast<const float4v*>(bias + n0);
            float4v sv = {1.f, 1.f, 1.f, 1.f};
            if constexpr (MODE != 0) sv = *reinterpret_cast<const float4v*>(wscale + n0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = MODE != 0 ? __builtin_fmaf(acc[nt][q * 4 + e], sv[e], bv[e]) : acc[nt][q * 4 + e] + bv[e];
                acc[nt][q * 4 + e] = v;
                sum += v;
            }
        }
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.f / LD);
    float sq = 0.f;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float dlt = acc[nt][j] - mean;
            sq = __builtin_fmaf(dlt, dlt, sq);
        }
    sq += __shfl_xor(sq, 32, 64);
    const float rstd = 1.f / sqrtf(sq * (1.f / LD) + 1e-5f);
    if (row >= rows) return;
    float* o = out + row * LD;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n0 = nt * 32 + q * 8 + h * 4;
            const float4v gv = *reinterpret_cast<const float4v*>(gamma + n0);
            const float4v bt = *reinterpret_cast<const float4v*>(beta + n0);
            float4v y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = __builtin_fmaf((acc[nt][q * 4 + e] - mean) * rstd, gv[e], bt[e]);
            *reinterpret_cast<float4v*>(o + n0) = y;
        }
}

}  // namespace

int dvid_outproj_ln_launch(const OutProjLnParams& p, hipStream_t s) {
    if (p.rows <= 0) return DVID_OK;
    if (p.d != LD) return DVID_ERR_UNSUPPORTED;
    if (!p.x || !p.bias || !p.gamma || !p.beta || !p.out) return DVID_ERR_ARG;
    const dim3 grid((unsigned)ceil_div((long)p.rows, 128L)), block(256);
    if (p.mode == 0) {
        if (!p.wf_hi) return DVID_ERR_ARG;
        hipLaunchKernelGGL(outproj_ln_kernel<0>, grid, block, 0, s, p.x, p.wf_hi, nullptr, nullptr, nullptr, p.bias, p.gamma, p.beta, p.out, p.rows,
                           nullptr);
    } else if (p.mode == 1) {
        if (!p.wf_hi || !p.wf_lo || !p.wscale) return DVID_ERR_ARG;
        hipLaunchKernelGGL(outproj_ln_kernel<1>, grid, block, 0, s, p.x, p.wf_hi, p.wf_lo, nullptr, p.wscale, p.bias, p.gamma, p.beta, p.out, p.rows,
                           p.range_flag);
    } else if (p.mode == 2) {
        if (!p.w32 || !p.wscale) return DVID_ERR_ARG;
        hipLaunchKernelGGL(outproj_ln_kernel<2>, grid, block, 0, s, p.x, nullptr, nullptr, p.w32, p.wscale, p.bias, p.gamma, p.beta, p.out, p.rows,
                           nullptr);
    } else {
        return DVID_ERR_ARG;
    }
    LAUNCH_CHECK();
    return DVID_OK;
}
