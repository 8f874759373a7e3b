// Fused DynamicConv instance interaction (box_head.py:692-704), one workgroup per box:
//
//   F1 = relu(LN64 (roi[49x256] . P1[256x64]))      bmm #1 + norm1 + ReLU
//   F2 = relu(LN256(F1 [49x64]  . P2[64x256]))      bmm #2 + norm2 + ReLU     -> out[49][256] fp16
//
// `params` is the dynamic_layer output for this box in the REPACKED order produced by the
// runtime's weight repack: P1T[j][c] (64x256) then P2T[c][j] (256x64), i.e. both are
// "[N][K], K contiguous" MFMA B operands that each wave pulls straight from global memory
// (every parameter is read exactly once per box).  The 49x256 RoI tile (zero-padded to 64 rows)
// is staged once in LDS (528-byte pitch: conflict-free ds_read_b128 fragments); the N
// dimension of both products is split over the 4 waves, so LayerNorm row statistics are
// combined across waves through a tiny LDS buffer (mean first, then centred variance, fp32).
//
// FUSED_ROI (round 6): the RoI tile is not read from memory but GATHERED here -- the per-box walk of multi-level RoIAlignV2
// (csrc/roi_taps.h, the arithmetic of csrc/roialign.hip bit for bit) writes its 49 bins straight into the LDS image the first product
// reads.  The separate launches move the fp16 tile through HBM twice (25 KB out, 25 KB in per box) and run an L1-bound gather and an
// HBM-bound stream one after the other; here the first product's 32 KB of parameters are requested BEFORE the gather, and with three
// workgroups per CU one box's taps (L1 path) overlap another's parameter stream (HBM).  The unfused pair stays for the passes that need
// the tile's mean over the bins before the self-attention (box_head.py:509-510: a head without incoming proposal features).
#include "common.h"
#include "f32_split.h"
#include "igemm_epilogue.h"
#include "kernels.h"
#include "options.h"
#include "roi_taps.h"

namespace {

constexpr int NP = 49;          // 7x7 bins
constexpr int D = 256;          // hidden dim
constexpr int DD = 64;          // dynamic dim
constexpr int A_PITCH = D + 8;  // halves
constexpr int H_PITCH = DD + 8;

// sum over the four 16-lane groups of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48)
__device__ __forceinline__ float groups4_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Both products are computed TRANSPOSED (the per-box parameters are the MFMA's first operand): a lane then holds 4 consecutive
// channels of ONE tile row instead of 4 rows of one channel, so a LayerNorm statistic is 3-15 in-lane adds + 2 shuffles per row tile
// (it was 4 shuffles per accumulator register: 64 per pass), and the fp16 results leave as 8-byte LDS writes (they were 2-byte ones).
// Same products, same K order; only the order of the fp32 sums inside the LayerNorm statistics differs from the row-major form.
template <bool FUSED_ROI>
__global__ __launch_bounds__(256, 3) void dynconv_kernel(const half_t* __restrict__ roi, const half_t* __restrict__ params,
                                                       const float* __restrict__ g1, const float* __restrict__ b1,
                                                       const float* __restrict__ g2, const float* __restrict__ b2,
                                                       half_t* __restrict__ out, RoiLevels lv, const float* __restrict__ boxes,
                                                       int boxes_per_img, int nbox) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* As = reinterpret_cast<half_t*>(smem);                     // [64][A_PITCH]; later the output tile
    half_t* Hs = As + 64 * A_PITCH;                                   // [64][H_PITCH]
    float* red = reinterpret_cast<float*>(Hs + 64 * H_PITCH);         // [64 rows][4 waves]

    // (fused: an XCD takes one contiguous run of boxes, i.e. whole images, as csrc/roialign.hip -- the boxes that gather from one image's
    // pyramid meet in one L2)
    const int box = FUSED_ROI ? igemm_xcd_remap((int)blockIdx.x, nbox) : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const half_t* p1t = params + (long)box * (2 * D * DD);
    const half_t* p2t = p1t + D * DD;
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 bf[8];          // parameter fragments of bmm #1: this wave owns output channels [wave*16, +16)
    half8 b2f[4][2];      // ... of bmm #2: channels [wave*64, +64)

    if (FUSED_ROI) {
        // both products' parameters (64 KB per box) are requested first: they stream in from HBM under the gather, which runs on the L1 path
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            bf[ks] = *reinterpret_cast<const half8*>(p1t + (wave * 16 + l15) * D + ks * 32 + l4 * 8);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                b2f[nt][ks] = *reinterpret_cast<const half8*>(p2t + (wave * 64 + nt * 16 + l15) * DD + ks * 32 + l4 * 8);
        // ---- gather the RoI tile into its LDS image (rows 49..63 zero) ------------------
        float macc[8];
        roi_taps::gather_box(lv, boxes, boxes_per_img, box, tid >> 5, tid & 31, macc,
                             [&](int p, half8 o) { *reinterpret_cast<half8*>(As + p * A_PITCH + (tid & 31) * 8) = o; });
        for (int i = tid; i < (64 - NP) * 32; i += 256) *reinterpret_cast<half8*>(As + (NP + (i >> 5)) * A_PITCH + (i & 31) * 8) = zero8;
    } else {
        // ---- stage the RoI tile (rows 49..63 zero) ----------------------------------------
        const half_t* roi_b = roi + (long)box * NP * D;
        for (int i = tid; i < 64 * 32; i += 256) {
            const int r = i >> 5, cv = i & 31;
            const half8 v = *reinterpret_cast<const half8*>(roi_b + (long)(r < NP ? r : 0) * D + cv * 8);
            *reinterpret_cast<half8*>(As + r * A_PITCH + cv * 8) = (r < NP) ? v : zero8;
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            bf[ks] = *reinterpret_cast<const half8*>(p1t + (wave * 16 + l15) * D + ks * 32 + l4 * 8);
    }
    __syncthreads();

    // ---- bmm #1 (transposed): acc1[mt][r] = F1[row mt*16 + l15][channel wave*16 + 4*l4 + r] -----------------------------
    float4v acc1[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc1[mt] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const half8 af = *reinterpret_cast<const half8*>(As + (mt * 16 + l15) * A_PITCH + ks * 32 + l4 * 8);
            acc1[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[ks], af, acc1[mt], 0, 0, 0);
        }
    }
    // prefetch this wave's bmm #2 parameter fragments (channels [wave*64, +64)); fused: they were requested ahead of the gather
    if (!FUSED_ROI) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                b2f[nt][ks] = *reinterpret_cast<const half8*>(p2t + (wave * 64 + nt * 16 + l15) * DD + ks * 32 + l4 * 8);
    }

    // ---- LayerNorm(64) + ReLU over rows ------------------------------------------------------------------------------------
    float mean[4], rstd[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float s = groups4_sum((acc1[mt][0] + acc1[mt][1]) + (acc1[mt][2] + acc1[mt][3]));
        if (l4 == 0) red[(mt * 16 + l15) * 4 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float4v t = *reinterpret_cast<const float4v*>(red + (mt * 16 + l15) * 4);
        mean[mt] = (t[0] + t[1] + t[2] + t[3]) * (1.f / DD);
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float c = acc1[mt][r] - mean[mt];
            s += c * c;
        }
        s = groups4_sum(s);
        if (l4 == 0) red[(mt * 16 + l15) * 4 + wave] = s;
    }
    __syncthreads();
    {
        const float4v gg = *reinterpret_cast<const float4v*>(g1 + wave * 16 + l4 * 4), bb = *reinterpret_cast<const float4v*>(b1 + wave * 16 + l4 * 4);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float4v t = *reinterpret_cast<const float4v*>(red + (mt * 16 + l15) * 4);
            rstd[mt] = rsqrtf((t[0] + t[1] + t[2] + t[3]) * (1.f / DD) + 1e-5f);
            half4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = (half_t)fmaxf((acc1[mt][r] - mean[mt]) * rstd[mt] * gg[r] + bb[r], 0.f);
            *reinterpret_cast<half4*>(Hs + (mt * 16 + l15) * H_PITCH + wave * 16 + l4 * 4) = y;
        }
    }
    __syncthreads();   // Hs complete; As (RoI) is dead from here on; red reusable

    // ---- bmm #2 (transposed): acc2[mt][nt][r] = F2[row mt*16 + l15][channel wave*64 + nt*16 + 4*l4 + r] -------------------
    float4v acc2[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc2[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const half8 af = *reinterpret_cast<const half8*>(Hs + (mt * 16 + l15) * H_PITCH + ks * 32 + l4 * 8);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc2[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b2f[nt][ks], af, acc2[mt][nt], 0, 0, 0);
        }
    }
    // ---- LayerNorm(256) + ReLU ----------------------------------------------------------------------------------------------
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) s += (acc2[mt][nt][0] + acc2[mt][nt][1]) + (acc2[mt][nt][2] + acc2[mt][nt][3]);
        s = groups4_sum(s);
        if (l4 == 0) red[(mt * 16 + l15) * 4 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float4v t = *reinterpret_cast<const float4v*>(red + (mt * 16 + l15) * 4);
        mean[mt] = (t[0] + t[1] + t[2] + t[3]) * (1.f / D);
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float c = acc2[mt][nt][r] - mean[mt];
                s += c * c;
            }
        s = groups4_sum(s);
        if (l4 == 0) red[(mt * 16 + l15) * 4 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float4v t = *reinterpret_cast<const float4v*>(red + (mt * 16 + l15) * 4);
        rstd[mt] = rsqrtf((t[0] + t[1] + t[2] + t[3]) * (1.f / D) + 1e-5f);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int col = wave * 64 + nt * 16 + l4 * 4;
        const float4v gg = *reinterpret_cast<const float4v*>(g2 + col), bb = *reinterpret_cast<const float4v*>(b2 + col);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            half4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = (half_t)fmaxf((acc2[mt][nt][r] - mean[mt]) * rstd[mt] * gg[r] + bb[r], 0.f);
            *reinterpret_cast<half4*>(As + (mt * 16 + l15) * A_PITCH + col) = y;
        }
    }
    __syncthreads();
    // ---- coalesced 16-byte stores of the 49 valid rows ---------------------------------
    half_t* out_b = out + (long)box * NP * D;
    for (int i = tid; i < NP * 32; i += 256) {
        const int r = i >> 5, cv = i & 31;
        *reinterpret_cast<half8*>(out_b + (long)r * D + cv * 8) = *reinterpret_cast<const half8*>(As + r * A_PITCH + cv * 8);
    }
}

constexpr int kSmem = 64 * A_PITCH * 2 + 64 * H_PITCH * 2 + 64 * 4 * 4;

}  // namespace

int dvid_dynconv_launch(const half_t* roi, const half_t* params, const float* g1, const float* b1, const float* g2,
                        const float* b2, half_t* out, int rows, hipStream_t s) {
    if (rows == 0) return DVID_OK;
    hipLaunchKernelGGL(dynconv_kernel<false>, dim3(rows), dim3(256), kSmem, s, roi, params, g1, b1, g2, b2, out, RoiLevels{}, nullptr, 1, rows);
    LAUNCH_CHECK();
    return DVID_OK;
}

// RoIAlign + DynamicConv as one launch: the tile of box b of image b / boxes_per_img is gathered from the pyramid `lv` (see the header)
int dvid_dynconv_roi_launch(const RoiLevels& lv, int channels, const float* boxes, int n_img, int boxes_per_img, const half_t* params,
                            const float* g1, const float* b1, const float* g2, const float* b2, half_t* out, hipStream_t s) {
    if (channels != 256) return DVID_ERR_UNSUPPORTED;
    const int rows = n_img * boxes_per_img;
    if (rows == 0) return DVID_OK;
    hipLaunchKernelGGL(dynconv_kernel<true>, dim3(rows), dim3(256), kSmem, s, nullptr, params, g1, b1, g2, b2, out, lv, boxes, boxes_per_img, rows);
    LAUNCH_CHECK();
    return DVID_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// DTYPE float32
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// DynamicConv (box_head.py:687-711), one workgroup per box: F1 = roi[49 x 256] . param1[256 x 64] -> LayerNorm(64) + ReLU ->
// F2 = F1 . param2[64 x 256] -> LayerNorm(256) + ReLU -> out[49 x 256].  The per-box parameters arrive as P1T[64][256] | P2T[256][64]
// ([N][K] rows, the row order csrc/weights.hip gives dynamic_layer), so both MFMA operands are K-contiguous rows read straight from
// global as float4 fragments; F1 / F2 cross LDS for the row statistics.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int DC_P1 = 68, DC_P2 = 260;
// (two workgroups per CU: left to itself the compiler takes 200 VGPRs + 64 AGPRs, over the 256 a wave may have at two waves per SIMD, and
// a box's loads, products and LayerNorms then run strictly one after the other on the CU)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void f32_dynconv_kernel(const float* __restrict__ roi, const float* __restrict__ params,
                                                           const float* __restrict__ g1, const float* __restrict__ b1,
                                                           const float* __restrict__ g2, const float* __restrict__ b2, float* __restrict__ out,
                                                           int nbox) {
#pragma clang fp contract(off)
    __shared__ float F1[64 * DC_P1];
    __shared__ float F2[49 * DC_P2];
    const int box = igemm_xcd_remap((int)blockIdx.x, nbox);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fk = (lane >> 5) * 4;
    const float* x = roi + (long)box * 49 * 256;
    const float* p1 = params + (long)box * 32768;
    const float* p2 = p1 + 64 * 256;

    // the second product's parameter fragments are requested first: they land under the first product
    float4v w2[2][8];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int j = 0; j < 8; ++j) w2[nb][j] = *reinterpret_cast<const float4v*>(p2 + (long)((wave * 2 + nb) * 32 + fr) * 64 + j * 8 + fk);

    // ---- product 1: wave = (row block mb, column block nb) of the 64 x 64 result, K = 256 in four chunks of 64
    {
        const int mb = wave >> 1, nb = wave & 1;
        const int prow = mb * 32 + fr;
        const bool pok = prow < 49;
        const float* ap = x + (long)(pok ? prow : 0) * 256 + fk;
        const float* bp = p1 + (long)(nb * 32 + fr) * 256 + fk;
        float16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float4v a[2][8], b[2][8];
        auto fetch = [&](int c, int buf) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a[buf][j] = pok ? *reinterpret_cast<const float4v*>(ap + c * 64 + j * 8) : (float4v){0.f, 0.f, 0.f, 0.f};
                b[buf][j] = *reinterpret_cast<const float4v*>(bp + c * 64 + j * 8);
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c + 1 < 4) fetch(c + 1, (c + 1) & 1);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = mfma_f32(a[c & 1][j][e], b[c & 1][j][e], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) F1[(mb * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3)) * DC_P1 + nb * 32 + fr] = acc[r];
    }
    __syncthreads();
    // ---- LayerNorm(64) + ReLU on rows 0..48: four lanes per row, 16 values each
    if (tid < 49 * 4) {
        const int row = tid >> 2, part = tid & 3;
        float* rp = &F1[row * DC_P1 + part * 16];
        float vals[16], sum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            vals[e] = rp[e];
            sum += vals[e];
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        const float mean = sum / 64.f;
        float sq = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float t = vals[e] - mean;
            sq += t * t;
        }
        sq += __shfl_xor(sq, 1, 64);
        sq += __shfl_xor(sq, 2, 64);
        const float rstd = rsqrtf(sq / 64.f + 1e-5f);
#pragma unroll
        for (int e = 0; e < 16; ++e) rp[e] = fmaxf((vals[e] - mean) * rstd * g1[part * 16 + e] + b1[part * 16 + e], 0.f);
    }
    __syncthreads();
    // ---- product 2: wave w owns columns [64 w, 64 w + 64) of the 64 x 256 result, K = 64
    {
        float16v acc[2][2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float4v a[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) a[mb] = *reinterpret_cast<const float4v*>(&F1[(mb * 32 + fr) * DC_P1 + j * 8 + fk]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = mfma_f32(a[mb][e], w2[nb][j][e], acc[mb][nb]);
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mb * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
                    if (row < 49) F2[row * DC_P2 + (wave * 2 + nb) * 32 + fr] = acc[mb][nb][r];
                }
    }
    __syncthreads();
    // ---- LayerNorm(256) + ReLU, one wave per row, 4 values per lane; rows go straight to global
    const float4v gg = *reinterpret_cast<const float4v*>(g2 + lane * 4);
    const float4v bb = *reinterpret_cast<const float4v*>(b2 + lane * 4);
    for (int row = wave; row < 49; row += 4) {
        const float4v t = *reinterpret_cast<const float4v*>(&F2[row * DC_P2 + lane * 4]);
        const float mean = wave_sum(t[0] + t[1] + t[2] + t[3]) / 256.f;
        float sq = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = t[e] - mean;
            sq += u * u;
        }
        const float rstd = rsqrtf(wave_sum(sq) / 256.f + 1e-5f);
        float4v o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf((t[e] - mean) * rstd * gg[e] + bb[e], 0.f);
        *reinterpret_cast<float4v*>(out + ((long)box * 49 + row) * 256 + lane * 4) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same per-box pipeline with SPLIT operands (library option f32_split = 1, the default): both products run as three passes of the
// fp16 MFMA on (hi, lo) halves of the fp32 values -- the arithmetic of csrc/f32_split.h, as f32x3_igemm_kernel: lo_a hi_b + hi_a lo_b + hi_a hi_b, fp32
// accumulation -- instead of 256 fp32-MFMA instructions of 64 cycles per wave and box.  Each wave splits the fragments it multiplies, in
// registers, straight from the global loads; product 1 is split over K across the four waves (see the kernel), its partial sums and
// F1 cross LDS as fp32 for the LayerNorm statistics, and F1 comes back as two fp16 planes (rows of 64 halves at a pitch of 72:
// conflict-free ds_read_b128 fragments) over the same bytes.
// LayerNorm / ReLU arithmetic is the fp32 kernel's.  |value| > 65504 in the RoI tile or the parameters sets `range_flag`.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int DX_PH = 72;          // halves per F1 plane row

__global__ __launch_bounds__(256) void f32x3_dynconv_kernel(const float* __restrict__ roi, const float* __restrict__ params,
                                                             const float* __restrict__ g1, const float* __restrict__ b1,
                                                             const float* __restrict__ g2, const float* __restrict__ b2, float* __restrict__ out,
                                                             int nbox, int* __restrict__ range_flag) {
#pragma clang fp contract(off)
    // LDS: product 1's four K-quarter partial sums [4][64][68] fp32 (69632 bytes); afterwards the same bytes hold F1 as two fp16 planes
    // (18432) and, behind them, F2 [49][260] fp32
    constexpr int PART = 64 * DC_P1;                      // floats per partial
    constexpr int F1_BYTES = 2 * 64 * DX_PH * 2;
    constexpr int LDS_BYTES = 4 * PART * 4 > F1_BYTES + 49 * DC_P2 * 4 ? 4 * PART * 4 : F1_BYTES + 49 * DC_P2 * 4;
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
    float* const P = reinterpret_cast<float*>(lds);
    half_t* const F1h = reinterpret_cast<half_t*>(lds);
    half_t* const F1l = F1h + 64 * DX_PH;
    float* const F2 = reinterpret_cast<float*>(lds + F1_BYTES);
    const int box = igemm_xcd_remap((int)blockIdx.x, nbox);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fk = (lane >> 5) * 8;          // fp16 MFMA operand map: lane l = row l & 31, k = 8 (l >> 5) .. + 8 of a 16-deep step
    const float* x = roi + (long)box * 49 * 256;
    const float* p1 = params + (long)box * 32768;
    const float* p2 = p1 + 64 * 256;
    float mx = 0.f;

    // ---- product 1, split over K: wave w multiplies k in [64 w, 64 w + 64) for the whole 64 x 64 result.  Every RoI / parameter value is
    // loaded by exactly one lane, and ALL of a box's 114 KB of first-product operands are requested before the first one is used (the
    // (row block, column block) split of the fp32 kernel double-buffers 64-deep chunks: ~32 KB in flight per workgroup, which is what
    // paced it -- 2.4-2.6 TB/s with either MFMA).
    float16v acc[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
    {
        float4v a[2][4][2], b[2][4][2];
        const bool pok = 32 + fr < 49;          // row block 1 holds rows 32..48
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = 64 * wave + 16 * ks + fk + 4 * h;
                a[0][ks][h] = *reinterpret_cast<const float4v*>(x + (long)fr * 256 + k);
                a[1][ks][h] = pok ? *reinterpret_cast<const float4v*>(x + (long)(32 + fr) * 256 + k) : (float4v){0.f, 0.f, 0.f, 0.f};
                b[0][ks][h] = *reinterpret_cast<const float4v*>(p1 + (long)fr * 256 + k);
                b[1][ks][h] = *reinterpret_cast<const float4v*>(p1 + (long)(32 + fr) * 256 + k);
            }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32_split::split8(a[i][ks][0], a[i][ks][1], ah[i], al[i], mx);
                f32_split::split8(b[i][ks][0], b[i][ks][1], bh[i], bl[i], mx);
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = f32_split::mfma_x3<false>(ah[mb], al[mb], bh[nb], bl[nb], acc[mb][nb]);
        }
    }
    // the second product's parameter fragments (raw fp32; wave w owns columns [64 w, 64 w + 64)): requested now, they land under the
    // reduction and the LayerNorm below
    float4v w2[2][4][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float* q = p2 + (long)((wave * 2 + nb) * 32 + fr) * 64 + ks * 16 + fk;
            w2[nb][ks][0] = *reinterpret_cast<const float4v*>(q);
            w2[nb][ks][1] = *reinterpret_cast<const float4v*>(q + 4);
        }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                P[wave * PART + (mb * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3)) * DC_P1 + nb * 32 + fr] = acc[mb][nb][r];
    __syncthreads();
    // ---- the four partial sums in a fixed order, LayerNorm(64) + ReLU on rows 0..48: four lanes per row, 16 values each; the result goes
    // back as (hi, lo) planes, rows 49..63 zero
    {
        const int row = tid >> 2, part = tid & 3;
        float vals[16];
        if (row < 49) {
            const float* rp = &P[row * DC_P1 + part * 16];
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                vals[e] = (rp[e] + rp[PART + e]) + (rp[2 * PART + e] + rp[3 * PART + e]);
                sum += vals[e];
            }
            sum += __shfl_xor(sum, 1, 64);
            sum += __shfl_xor(sum, 2, 64);
            const float mean = sum / 64.f;
            float sq = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float t = vals[e] - mean;
                sq += t * t;
            }
            sq += __shfl_xor(sq, 1, 64);
            sq += __shfl_xor(sq, 2, 64);
            const float rstd = rsqrtf(sq / 64.f + 1e-5f);
#pragma unroll
            for (int e = 0; e < 16; ++e) vals[e] = fmaxf((vals[e] - mean) * rstd * g1[part * 16 + e] + b1[part * 16 + e], 0.f);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) vals[e] = 0.f;
        }
        __syncthreads();          // every partial sum has been read
        float unused = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            half8 vh, vl;
            f32_split::split8((float4v){vals[8 * h], vals[8 * h + 1], vals[8 * h + 2], vals[8 * h + 3]},
                   (float4v){vals[8 * h + 4], vals[8 * h + 5], vals[8 * h + 6], vals[8 * h + 7]}, vh, vl, unused);
            *reinterpret_cast<half8*>(F1h + row * DX_PH + part * 16 + 8 * h) = vh;
            *reinterpret_cast<half8*>(F1l + row * DX_PH + part * 16 + 8 * h) = vl;
        }
    }
    __syncthreads();
    // ---- product 2: wave w owns columns [64 w, 64 w + 64) of the 64 x 256 result, K = 64
    {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                ah[mb] = *reinterpret_cast<const half8*>(F1h + (mb * 32 + fr) * DX_PH + ks * 16 + fk);
                al[mb] = *reinterpret_cast<const half8*>(F1l + (mb * 32 + fr) * DX_PH + ks * 16 + fk);
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) f32_split::split8(w2[nb][ks][0], w2[nb][ks][1], bh[nb], bl[nb], mx);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = f32_split::mfma_x3<false>(ah[mb], al[mb], bh[nb], bl[nb], acc[mb][nb]);
        }
        // (F2 lies behind the planes: no wave's fragment reads are disturbed by another wave's results)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mb * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
                    if (row < 49) F2[row * DC_P2 + (wave * 2 + nb) * 32 + fr] = acc[mb][nb][r];
                }
    }
    f32_split::report_range(range_flag, mx);
    __syncthreads();
    // ---- LayerNorm(256) + ReLU, one wave per row, 4 values per lane; rows go straight to global
    const float4v gg = *reinterpret_cast<const float4v*>(g2 + lane * 4);
    const float4v bb = *reinterpret_cast<const float4v*>(b2 + lane * 4);
    for (int row = wave; row < 49; row += 4) {
        const float4v t = *reinterpret_cast<const float4v*>(&F2[row * DC_P2 + lane * 4]);
        const float mean = wave_sum(t[0] + t[1] + t[2] + t[3]) / 256.f;
        float sq = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = t[e] - mean;
            sq += u * u;
        }
        const float rstd = rsqrtf(wave_sum(sq) / 256.f + 1e-5f);
        float4v o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf((t[e] - mean) * rstd * gg[e] + bb[e], 0.f);
        *reinterpret_cast<float4v*>(out + ((long)box * 49 + row) * 256 + lane * 4) = o;
    }
}

}  // namespace

int dvid_f32_dynconv_launch(const float* roi, const float* params, const float* g1, const float* b1, const float* g2, const float* b2,
                            float* out, int rows, int* range_flag, hipStream_t s) {
    if (rows <= 0) return DVID_OK;
    if (g_opt.f32_split != 0) hipLaunchKernelGGL(f32x3_dynconv_kernel, dim3(rows), dim3(256), 0, s, roi, params, g1, b1, g2, b2, out, rows, range_flag);
    else hipLaunchKernelGGL(f32_dynconv_kernel, dim3(rows), dim3(256), 0, s, roi, params, g1, b1, g2, b2, out, rows);
    LAUNCH_CHECK();
    return DVID_OK;
}
