// The backward of an RCNNHead's instance interaction with its residual and norm2 (box_head.py:666-711 and :521-524; the forward of
// inference is csrc/dynconv.hip and csrc/head.hip), the link in front of the tail (csrc/headtail_bwd.hip):
//   params = dynamic_layer(p)                        [R][32768]   param1 = [:16384] as [256][64], param2 = [16384:] as [64][256]
//   F1 = ReLU(LN64 (roi . param1))                   [R][49][64]
//   F2 = ReLU(LN256(F1  . param2))                   [R][49][256]
//   o  = ReLU(LN256(out_layer(F2 flattened bin * 256 + c)))
//   y  = norm2(p + o)                                [R][256]
// dvid_inst_interact_backward recomputes that forward in fp32 into scratch and walks it back.  The arithmetic is the tail's (its header
// says why): fp32 products on v_mfma_f32_32x32x2_f32, fp32 accumulation, sums over rows in fixed chunks added in ascending order, no
// atomics, two runs give the same bits.  The Linear layers, the 256-wide LayerNorms and the sums over rows run on the kernels of
// csrc/bwd_kernels.h; the per-box part -- both bmm's, their LayerNorms and the four products of their backward -- is inst_box_kernel here.
//
// Bounded scratch: params and d_params are 128 KiB per row each, so rows are processed in slabs of DVID_INST_BWD_ROW_SLAB; the weight and
// bias gradients of dynamic_layer (and out_layer's weight gradient) are accumulated slab by slab: the running sum is partial 0 of the next
// slab's reduction, which adds its chunks behind it in ascending order -- the same chain of additions as one reduction over all chunks.
// Only the kept F2 and its cotangent (R x 49 x 256 each) and a few R x 256 rows grow with R.
#include <math.h>

#include "../../include/dvid_hip.h"
#include "common.h"
#include "kernels.h"
#include "bwd_kernels.h"

namespace {

constexpr int BINS = 49, DD = 64, TILE = BINS * D, NP = 2 * D * DD;          // bins of a 7 x 7 pooler, dim_dynamic, floats of a tile, of params
constexpr int SLAB = DVID_INST_BWD_ROW_SLAB;
static_assert(SLAB % 256 == 0 && SLAB >= 256 && SLAB <= 1024, "the slab is whole row chunks and bounds the scratch");
static_assert(SLAB % CHUNK == 0, "a slab is whole chunks, so slab-wise accumulation is the one chain over all chunks");
constexpr int LN_PART = 2 * (DD + D);          // a box's partial sums: d gamma1 [64], d beta1 [64], d gamma2 [256], d beta2 [256]
constexpr int KSPLIT = 2048;                   // the K = 32768 of dynamic_layer's data gradient, in fixed chunks
constexpr int OSPLIT = 1792;                   // the K = 12544 of out_layer's forward likewise: one chain of 12544 fp32 additions costs y three bits
static_assert(NP % KSPLIT == 0 && TILE % OSPLIT == 0 && OSPLIT % BK == 0 && TILE / OSPLIT <= 1 + NP / KSPLIT, "whole chunks, and the split buffer holds either");

// The live LDS set of inst_box_kernel, in floats.  Tiles have 49 live rows and one more, row 49, of zeros: a 64-row MFMA shape reads its
// rows 49 .. 63 from it (row index clamped to 49), and the products over rows run K to 50.  Odd pitches keep both the row-major and the
// transposed fragment reads on 32 distinct banks.
//   R   the RoI tile              50 x 257 (50,176 B live)      B   roi . param1 . param2 -> xhat2's source -> dF2pre   50 x 257
//   F1  F1pre -> F1 -> dF1 -> dF1pre      50 x 65 (12,544 B live)        X1  xhat of LN64                                50 x 65
//   RS  rstd of LN64 [64]                 PT  the four waves' gamma / beta partial sums  4 x 640
constexpr int RP = D + 1, FP = DD + 1, TROWS = BINS + 1;
constexpr int OFF_R = 0, OFF_B = OFF_R + TROWS * RP, OFF_F1 = OFF_B + TROWS * RP, OFF_X1 = OFF_F1 + TROWS * FP, OFF_RS = OFF_X1 + TROWS * FP,
              OFF_PT = OFF_RS + 64, LDS_FLOATS = OFF_PT + 4 * LN_PART;
constexpr int LDS_BYTES = LDS_FLOATS * 4;
static_assert(LDS_BYTES <= 160 * 1024, "the live set of a box fits the 160 KiB of LDS of a CU");

__device__ __forceinline__ int out_row(int r, int lane) { return (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3); }          // of accumulator register r

// One workgroup per box of a slab.  BWD false: the forward up to F2, written to f2.  BWD true: the same recompute, then back from the
// cotangent df2 of F2 (masked by the kept f2) to d_params (every one of its 32768 elements, one writer each), d_roi (when given) and the
// box's own gamma / beta partial sums lnpart[box][640].  roi, f2, df2, d_roi, lnpart point at the slab's first box; params / d_params are the slab's.
template <bool BWD>
__global__ __launch_bounds__(256) void inst_box_kernel(const float* __restrict__ roi, const float* __restrict__ params, const float* __restrict__ g1,
                                                       const float* __restrict__ b1, const float* __restrict__ g2, const float* __restrict__ b2,
                                                       float* __restrict__ f2, const float* __restrict__ df2, float* __restrict__ d_params,
                                                       float* __restrict__ d_roi, float* __restrict__ lnpart) {
    extern __shared__ float lds[];
    float *sR = lds + OFF_R, *sB = lds + OFF_B, *sF1 = lds + OFF_F1, *sX1 = lds + OFF_X1, *sRs = lds + OFF_RS, *sPt = lds + OFF_PT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lk = lane >> 5;
    const long box = blockIdx.x;
    const float* prm = params + box * NP;
    const float* tile = roi + box * TILE;
    for (int i = tid; i < TILE; i += 256) sR[(i >> 8) * RP + (i & 255)] = tile[i];
    for (int i = tid; i < RP; i += 256) sR[BINS * RP + i] = 0.f, sB[BINS * RP + i] = 0.f;
    if (tid < FP) sF1[BINS * FP + tid] = 0.f, sX1[BINS * FP + tid] = 0.f;
    __syncthreads();
    // MFMA operand maps (cdna_hip_programming.md): A lane l = A[i = l & 31][k = l >> 5], B lane l = B[k = l >> 5][j = l & 31]
    const int mi = wave >> 1, nj = wave & 1;          // the 32 x 32 block of a wave in a 64 x 64 product
    const int rowA[2] = {min(l31, BINS), min(32 + l31, BINS)};          // a tile row as the MFMA's i, rows 49 .. 63 read the zero row

    // ---- F1pre = roi . param1 (K = 256)
    {
        float16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* a = sR + rowA[mi] * RP + lk;
        const float* b = prm + lk * DD + nj * 32 + l31;
#pragma unroll 8
        for (int k = 0; k < D; k += 2) acc = mfma_f32(a[k], b[k * DD], acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mi * 32 + out_row(r, lane);
            if (row < BINS) sF1[row * FP + nj * 32 + l31] = acc[r];
        }
    }
    __syncthreads();
    // ---- LN64 + ReLU, one wave per row, a lane per column (two-pass fp32 statistics, as ln_fwd_kernel)
    for (int row = wave; row < BINS; row += 4) {
        const float v = sF1[row * FP + lane];
        const float t = v - wave_sum(v) / DD;
        const float rs = 1.f / sqrtf(wave_sum(t * t) / DD + 1e-5f);
        const float xh = t * rs;
        sX1[row * FP + lane] = xh;
        sF1[row * FP + lane] = fmaxf(xh * g1[lane] + b1[lane], 0.f);
        if (lane == 0) sRs[row] = rs;
    }
    __syncthreads();
    // ---- F2pre = F1 . param2 (K = 64): a wave takes 64 columns
    {
        float16v acc[2][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q >> 1][q & 1][r] = 0.f;
        const float* b = prm + D * DD + lk * D + wave * 64 + l31;
#pragma unroll 4
        for (int k = 0; k < DD; k += 2) {
            const float a0 = sF1[rowA[0] * FP + k + lk], a1 = sF1[rowA[1] * FP + k + lk];
            const float b0 = b[k * D], b1v = b[k * D + 32];
            acc[0][0] = mfma_f32(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f32(a0, b1v, acc[0][1]);
            acc[1][0] = mfma_f32(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f32(a1, b1v, acc[1][1]);
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mb * 32 + out_row(r, lane);
                    if (row < BINS) sB[row * RP + wave * 64 + nb * 32 + l31] = acc[mb][nb][r];
                }
    }
    __syncthreads();
    // ---- LN256 + ReLU per row (a lane holds columns lane + 64 e); backward: ReLU and LN256 backward in place, B becomes dF2pre
    float ag2[4] = {0.f, 0.f, 0.f, 0.f}, ab2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int row = wave; row < BINS; row += 4) {
        float v[4], xh[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = sB[row * RP + lane + 64 * e];
        const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) / D;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] -= mean;
        const float rs = 1.f / sqrtf(wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) / D + 1e-5f);
#pragma unroll
        for (int e = 0; e < 4; ++e) xh[e] = v[e] * rs;
        const long o = box * TILE + row * D + lane;
        if (!BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) f2[o + 64 * e] = fmaxf(xh[e] * g2[lane + 64 * e] + b2[lane + 64 * e], 0.f);
        } else {
            float dx[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = f2[o + 64 * e] > 0.f ? df2[o + 64 * e] : 0.f;          // nothing passes at a pre-activation of exactly 0
                ag2[e] += d * xh[e];
                ab2[e] += d;
                dx[e] = d * g2[lane + 64 * e];
            }
            const float m1 = wave_sum((dx[0] + dx[1]) + (dx[2] + dx[3])) / D;
            const float m2 = wave_sum((dx[0] * xh[0] + dx[1] * xh[1]) + (dx[2] * xh[2] + dx[3] * xh[3])) / D;
#pragma unroll
            for (int e = 0; e < 4; ++e) sB[row * RP + lane + 64 * e] = (dx[e] - m1 - xh[e] * m2) * rs;
        }
    }
    if (!BWD) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sPt[wave * LN_PART + 2 * DD + lane + 64 * e] = ag2[e];
        sPt[wave * LN_PART + 2 * DD + D + lane + 64 * e] = ab2[e];
    }
    __syncthreads();
    float* dprm = d_params + box * NP;
    // ---- dparam2 = F1^T . dF2pre (64 x 256, K = the 49 rows and the zero row): a wave takes 64 columns
    {
        float16v acc[2][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q >> 1][q & 1][r] = 0.f;
#pragma unroll 5
        for (int k = 0; k < TROWS; k += 2) {
            const float a0 = sF1[(k + lk) * FP + l31], a1 = sF1[(k + lk) * FP + 32 + l31];
            const float b0 = sB[(k + lk) * RP + wave * 64 + l31], b1v = sB[(k + lk) * RP + wave * 64 + 32 + l31];
            acc[0][0] = mfma_f32(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f32(a0, b1v, acc[0][1]);
            acc[1][0] = mfma_f32(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f32(a1, b1v, acc[1][1]);
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) dprm[D * DD + (mb * 32 + out_row(r, lane)) * D + wave * 64 + nb * 32 + l31] = acc[mb][nb][r];
    }
    __syncthreads();          // F1 has been read by every wave: it becomes dF1
    // ---- dF1 = dF2pre . param2^T (K = 256), masked by F1 in place
    {
        float16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* a = sB + rowA[mi] * RP + lk;
        const float* b = prm + D * DD + (nj * 32 + l31) * D + lk;
#pragma unroll 8
        for (int k = 0; k < D; k += 2) acc = mfma_f32(a[k], b[k], acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mi * 32 + out_row(r, lane);
            if (row < BINS) {
                float* q = sF1 + row * FP + nj * 32 + l31;
                *q = *q > 0.f ? acc[r] : 0.f;
            }
        }
    }
    __syncthreads();
    // ---- LN64 backward per row, in place: F1 becomes dF1pre
    {
        float ag1 = 0.f, ab1 = 0.f;
        for (int row = wave; row < BINS; row += 4) {
            const float d = sF1[row * FP + lane], xh = sX1[row * FP + lane];
            ag1 += d * xh;
            ab1 += d;
            const float dx = d * g1[lane];
            const float m1 = wave_sum(dx) / DD, m2 = wave_sum(dx * xh) / DD;
            sF1[row * FP + lane] = (dx - m1 - xh * m2) * sRs[row];
        }
        sPt[wave * LN_PART + lane] = ag1;
        sPt[wave * LN_PART + DD + lane] = ab1;
    }
    __syncthreads();
    // the box's partial sums: the four waves' in order (wave w holds rows w, w + 4, ... ascending)
    for (int i = tid; i < LN_PART; i += 256)
        lnpart[box * LN_PART + i] = ((sPt[i] + sPt[LN_PART + i]) + sPt[2 * LN_PART + i]) + sPt[3 * LN_PART + i];
    // ---- dparam1 = roi^T . dF1pre (256 x 64, K = the 49 rows and the zero row): a wave takes 64 of the 256 rows
    {
        float16v acc[2][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q >> 1][q & 1][r] = 0.f;
#pragma unroll 5
        for (int k = 0; k < TROWS; k += 2) {
            const float a0 = sR[(k + lk) * RP + wave * 64 + l31], a1 = sR[(k + lk) * RP + wave * 64 + 32 + l31];
            const float b0 = sF1[(k + lk) * FP + l31], b1v = sF1[(k + lk) * FP + 32 + l31];
            acc[0][0] = mfma_f32(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f32(a0, b1v, acc[0][1]);
            acc[1][0] = mfma_f32(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f32(a1, b1v, acc[1][1]);
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) dprm[(wave * 64 + mb * 32 + out_row(r, lane)) * DD + nb * 32 + l31] = acc[mb][nb][r];
    }
    if (!d_roi) return;
    // ---- d_roi = dF1pre . param1^T (49 x 256, K = 64): a wave takes 64 columns
    {
        float16v acc[2][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q >> 1][q & 1][r] = 0.f;
        const float* b = prm + (wave * 64 + l31) * DD + lk;
#pragma unroll 4
        for (int k = 0; k < DD; k += 2) {
            const float a0 = sF1[rowA[0] * FP + k + lk], a1 = sF1[rowA[1] * FP + k + lk];
            const float b0 = b[k], b1v = b[32 * DD + k];
            acc[0][0] = mfma_f32(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f32(a0, b1v, acc[0][1]);
            acc[1][0] = mfma_f32(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f32(a1, b1v, acc[1][1]);
        }
        float* out = d_roi + box * TILE;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mb * 32 + out_row(r, lane);
                    if (row < BINS) out[row * D + wave * 64 + nb * 32 + l31] = acc[mb][nb][r];
                }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

struct Layout {
    float *params, *dparams, *f2, *df2, *t, *o, *xhat3, *rstd3, *y, *xhaty, *rstdy, *dy, *gsum, *dmask, *dt, *lnpart, *lnsum, *accw, *accb, *acco, *split, *part;
    long long bytes;
};

Layout lay_out(void* scratch, long R) {
    const long slab = R < SLAB ? R : SLAB, slots = 1 + ceil_div(slab, (long)CHUNK);
    Layout L;
    Bump b{static_cast<char*>(scratch)};
    L.params = b.take(slab * NP);
    L.dparams = b.take(slab * NP);
    L.f2 = b.take(R * TILE);
    L.df2 = b.take(R * TILE);
    L.t = b.take(R * D);
    L.o = b.take(R * D);
    L.xhat3 = b.take(R * D);
    L.rstd3 = b.take(R);
    L.y = b.take(R * D);
    L.xhaty = b.take(R * D);
    L.rstdy = b.take(R);
    L.dy = b.take(R * D);
    L.gsum = b.take(R * D);
    L.dmask = b.take(R * D);
    L.dt = b.take(R * D);
    L.lnpart = b.take(R * LN_PART);
    L.lnsum = b.take(LN_PART);
    // the running sum and one slab's chunks of dynamic_layer's weight and bias gradients and of out_layer's weight gradient
    L.accw = b.take(slots * NP * D);
    L.accb = b.take(slots * NP);
    L.acco = b.take(slots * D * TILE);
    L.split = b.take((1 + NP / KSPLIT) * slab * D);          // the skip term and the K chunks of dynamic_layer's data gradient; out_layer's K chunks
    L.part = b.take(ceil_div(R, (long)CHUNK) * LN_PART);      // column sums over all rows: at most LN_PART columns
    L.bytes = b.off;
    return L;
}

// A sum over rows that is continued slab by slab: acc holds the running sum (slot 0) and room for one slab's chunks behind it
struct SlabSum {
    hipStream_t s;
    bool first, last;
    int* rc;
    void reduce(float* acc, int nz, long count, float* out) {
        if (*rc != DVID_OK) return;
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)ceil_div(count, 256L), 1), dim3(256), 0, s, acc, first ? nz : nz + 1, count, last ? out : acc, 0L);
        if (hipGetLastError() != hipSuccess) *rc = DVID_ERR_HIP;
    }
    // dW[J][K] (+)= dY[rows][J]^T X[rows][K]
    void wgrad(const float* dY, const float* X, int rows, int J, int K, float* acc, float* dW) {
        if (*rc != DVID_OK) return;
        const int nz = ceil_div(rows, CHUNK);
        GemmP p{dY, 1, J, X, 1, K, acc + (first ? 0 : (long)J * K), K, J, K, rows, CHUNK, nullptr, nullptr, nullptr, 0};
        hipLaunchKernelGGL(gemm_kernel, dim3(ceil_div(K, BT), ceil_div(J, BT), nz), dim3(256), 0, s, p);
        reduce(acc, nz, (long)J * K, dW);
    }
    // out[cols] (+)= the column sums of A[rows][cols]
    void colsum(const float* A, int cols, int rows, float* acc, float* out) {
        if (*rc != DVID_OK) return;
        const int nchunk = ceil_div(rows, CHUNK);
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(ceil_div(cols, 64), nchunk, 1), dim3(256), 0, s, A, (const float*)nullptr, cols, rows, nchunk,
                           acc + (first ? 0 : cols));
        reduce(acc, nchunk, cols, out);
    }
};

std::atomic<unsigned long long> g_lds_fwd{0}, g_lds_bwd{0};

}  // namespace

long long dvid_inst_interact_backward_scratch_bytes_host(long long rows) {
    if (rows < 1 || rows > DVID_HEAD_TAIL_BWD_MAX_ROWS) return -1;
    return lay_out(nullptr, (long)rows).bytes;
}

int dvid_inst_interact_backward_launch(const InstInteractBwdArgs& a, hipStream_t s) {
    const long R = a.rows;
    const Layout L = lay_out(a.scratch, R);
    Run run{s, L.part};
    const float* const* P = a.params;
    const float *Wd = P[0], *bd = P[1], *Wo = P[2], *bo = P[3], *g1 = P[4], *b1 = P[5], *g2 = P[6], *b2 = P[7], *g3 = P[8], *b3 = P[9], *gy = P[10], *by = P[11];
    const dim3 rows4((unsigned)ceil_div(R, 4L));
    if (int rc = allow_dynamic_lds(inst_box_kernel<false>, LDS_BYTES, g_lds_fwd); rc != DVID_OK) return rc;
    if (int rc = allow_dynamic_lds(inst_box_kernel<true>, LDS_BYTES, g_lds_bwd); rc != DVID_OK) return rc;

    // ---- forward, recomputed in fp32; F2 is kept for all rows, params live for one slab
    for (long r0 = 0; r0 < R; r0 += SLAB) {
        const int rows = (int)(R - r0 < SLAB ? R - r0 : SLAB);
        run.fwd(a.p + r0 * D, Wd, bd, 0, rows, NP, D, L.params);
        hipLaunchKernelGGL(inst_box_kernel<false>, dim3(rows), dim3(256), LDS_BYTES, s, a.roi + r0 * TILE, L.params, g1, b1, g2, b2, L.f2 + r0 * TILE,
                           (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
        // out_layer: the first K chunk with the bias, the others behind it as partials, added in ascending order
        const float* f2s = L.f2 + r0 * TILE;
        run.gemm({f2s, TILE, 1, Wo, TILE, 1, L.split, D, rows, D, OSPLIT, 0, bo, nullptr, nullptr, 0});
        if (run.rc != DVID_OK) return run.rc;
        GemmP q{f2s + OSPLIT, TILE, 1, Wo + OSPLIT, TILE, 1, L.split + (long)rows * D, D, rows, D, TILE - OSPLIT, OSPLIT, nullptr, nullptr, nullptr, 0};
        hipLaunchKernelGGL(gemm_kernel, dim3(ceil_div(D, BT), ceil_div(rows, BT), TILE / OSPLIT - 1), dim3(256), 0, s, q);
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)ceil_div((long)rows * D, 256L), 1), dim3(256), 0, s, L.split, TILE / OSPLIT, (long)rows * D,
                           L.t + r0 * D, 0L);
    }
    float* y = a.y_out ? a.y_out : L.y;
    hipLaunchKernelGGL(ln_fwd_kernel, rows4, dim3(256), 0, s, L.t, (const float*)nullptr, g3, b3, 1, R, L.o, L.xhat3, L.rstd3);
    hipLaunchKernelGGL(ln_fwd_kernel, rows4, dim3(256), 0, s, L.o, a.p, gy, by, 0, R, y, L.xhaty, L.rstdy);
    if (run.rc != DVID_OK) return run.rc;
    LAUNCH_CHECK();
    if (!a.grads) return DVID_OK;          // forward only

    // ---- backward
    float* const* G = a.grads;
    const float* dy = a.d_y;
    if (!dy) {
        HIP_TRY(hipMemsetAsync(L.dy, 0, (size_t)R * D * 4, s));
        dy = L.dy;
    }
    // norm2 and the residual: gsum is the cotangent of p + o, the skip's share of d_p
    hipLaunchKernelGGL(ln_bwd_kernel, rows4, dim3(256), 0, s, dy, (const float*)nullptr, L.xhaty, L.rstdy, gy, R, (float*)nullptr, L.gsum);
    run.colsum(dy, L.xhaty, D, (int)R, 1, G[10], 0);
    run.colsum(dy, nullptr, D, (int)R, 1, G[11], 0);
    // inst_interact.norm3 + ReLU, out_layer
    hipLaunchKernelGGL(ln_bwd_kernel, rows4, dim3(256), 0, s, L.gsum, L.o, L.xhat3, L.rstd3, g3, R, L.dmask, L.dt);
    run.colsum(L.dmask, L.xhat3, D, (int)R, 1, G[8], 0);
    run.colsum(L.dmask, nullptr, D, (int)R, 1, G[9], 0);
    run.colsum(L.dt, nullptr, D, (int)R, 1, G[3], 0);
    run.dgrad(L.dt, Wo, R, D, TILE, L.df2);
    // the boxes, slab by slab in ascending order
    for (long r0 = 0; r0 < R; r0 += SLAB) {
        const int rows = (int)(R - r0 < SLAB ? R - r0 : SLAB);
        SlabSum sum{s, r0 == 0, r0 + rows == R, &run.rc};
        run.fwd(a.p + r0 * D, Wd, bd, 0, rows, NP, D, L.params);
        if (run.rc != DVID_OK) return run.rc;
        hipLaunchKernelGGL(inst_box_kernel<true>, dim3(rows), dim3(256), LDS_BYTES, s, a.roi + r0 * TILE, L.params, g1, b1, g2, b2, L.f2 + r0 * TILE,
                           L.df2 + r0 * TILE, L.dparams, a.d_roi ? a.d_roi + r0 * TILE : nullptr, L.lnpart + r0 * LN_PART);
        sum.wgrad(L.dt + r0 * D, L.f2 + r0 * TILE, rows, D, TILE, L.acco, G[2]);
        sum.wgrad(L.dparams, a.p + r0 * D, rows, NP, D, L.accw, G[0]);
        sum.colsum(L.dparams, NP, rows, L.accb, G[1]);
        // d_p = the skip + d_params . W, K = 32768 in KSPLIT chunks added in ascending order behind the skip
        HIP_TRY(hipMemcpyAsync(L.split, L.gsum + r0 * D, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, s));
        GemmP q{L.dparams, NP, 1, Wd, 1, D, L.split + (long)rows * D, D, rows, D, NP, KSPLIT, nullptr, nullptr, nullptr, 0};
        hipLaunchKernelGGL(gemm_kernel, dim3(ceil_div(D, BT), ceil_div(rows, BT), NP / KSPLIT), dim3(256), 0, s, q);
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)ceil_div((long)rows * D, 256L), 1), dim3(256), 0, s, L.split, 1 + NP / KSPLIT, (long)rows * D,
                           a.d_p + r0 * D, 0L);
    }
    // the gamma / beta gradients of inst_interact.norm1 / norm2: the boxes' partial sums, added over boxes in ascending order
    run.colsum(L.lnpart, nullptr, LN_PART, (int)R, 1, L.lnsum, 0);
    if (run.rc != DVID_OK) return run.rc;
    const int off[4] = {0, DD, 2 * DD, 2 * DD + D}, len[4] = {DD, DD, D, D};
    for (int i = 0; i < 4; ++i) HIP_TRY(hipMemcpyAsync(G[4 + i], L.lnsum + off[i], (size_t)len[i] * 4, hipMemcpyDeviceToDevice, s));
    LAUNCH_CHECK();
    return DVID_OK;
}
