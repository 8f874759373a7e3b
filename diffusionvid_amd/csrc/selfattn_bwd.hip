// The backward of an RCNNHead's self-attention with its residual and norm1 (box_head.py:514-518; the forward of inference is
// csrc/attention.hip), the link in front of the instance interaction (csrc/interact_bwd.hip):
//   x [n * m][256], rows image-major; an image's m rows attend to each other, 8 heads of 32
//   qkv = in_proj(x)      O = softmax(q k^T / sqrt 32) v  per (image, head)      y = norm1(x + out_proj(O))
// dvid_self_attn_backward recomputes that forward in fp32 into scratch and walks it back.  The arithmetic is the tail's (its header says
// why): fp32 products on v_mfma_f32_32x32x2_f32, fp32 accumulation, sums over rows in fixed chunks added in ascending order, no atomics,
// two runs give the same bits.  The projections, norm1 and the sums over rows run on the kernels of csrc/bwd_kernels.h; the attention
// itself is here: the forward with its statistics and the backward by recompute.  The [m][m] probabilities are never stored: the forward
// keeps the rows' log-sum-exp L [n][8][m], and the backward forms P = exp(S - L) again tile by tile,
//   delta[i] = sum_d dO[i][d] O[i][d]      dP = dO . V^T      dS = P (dP - delta)      dQ = dS . K / sqrt 32      dK = dS^T . Q / sqrt 32      dV = P^T . dO
// once by query tiles (dQ) and once by key tiles (dK, dV), so every output element has one writer and one fixed order of addition.
// Tiles are 32 x 32, the shape of the MFMA; a workgroup is one wave on one (image, head, tile).  q is scaled by 1 / sqrt 32 as it is
// staged (the reference scales q, not the scores), so S leaves the MFMA final and S - L holds no product that could be contracted.
// Rows past an image's last row are staged as zeros and their P and dS are set to an exact 0: the next image's rows lie directly behind.
#include <math.h>

#include "../../include/dvid_hip.h"
#include "common.h"
#include "kernels.h"
#include "bwd_kernels.h"

namespace {

constexpr int NH = 8, HD = 32, T = 32, TP = T + 1, QKV = 3 * D;          // heads, their width, the tile, its LDS pitch (odd: rows on distinct banks)
static_assert(NH * HD == D && T == 32 && HD == 32, "a tile is one 32 x 32 x 2 MFMA shape, a head is one tile wide");
constexpr int TILE_FLOATS = T * TP;
constexpr int LDS_BYTES = 6 * TILE_FLOATS * 4;          // the largest live set: K, V, Q, dO, P^T, dS^T of the backward by keys
static_assert(LDS_BYTES <= 160 * 1024 && LDS_BYTES <= 64 * 1024, "the live set fits the 160 KiB of LDS of a CU, and a static allocation");
#define ATTN_SCALE 0.17677669529663687f          // 1 / sqrt 32

__device__ __forceinline__ int out_row(int r, int lane) { return (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3); }          // of accumulator register r

// over the 32 lanes that hold one accumulator row (a half wave), in a fixed butterfly
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// dst[r][c] = scale * src[(row0 + r) * ld + c] for the 32 x 32 tile at image row row0; rows at or past m (the image's rows) are zeros
__device__ __forceinline__ void load_tile(float* dst, const float* __restrict__ src, int ld, int row0, int m, int lane, float scale = 1.f) {
#pragma unroll 4
    for (int i = lane; i < T * T; i += 64) {
        const int r = i >> 5, c = i & 31;
        dst[r * TP + c] = row0 + r < m ? scale * src[(long)(row0 + r) * ld + c] : 0.f;
    }
}

// MFMA operand maps (cdna_hip_programming.md): A lane l = A[i = l & 31][k = l >> 5], B lane l = B[k = l >> 5][j = l & 31]
// C[i][j] = sum_d a[i][d] b[j][d]
__device__ __forceinline__ float16v tile_abt(const float* a, const float* b, int lane) {
    float16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* pa = a + (lane & 31) * TP + (lane >> 5);
    const float* pb = b + (lane & 31) * TP + (lane >> 5);
#pragma unroll
    for (int k = 0; k < T; k += 2) acc = mfma_f32(pa[k], pb[k], acc);
    return acc;
}
// C[i][j] += sum_k a[i][k] b[k][j]
__device__ __forceinline__ float16v tile_ab(const float* a, const float* b, float16v acc, int lane) {
    const float* pa = a + (lane & 31) * TP + (lane >> 5);
    const float* pb = b + (lane >> 5) * TP + (lane & 31);
#pragma unroll
    for (int k = 0; k < T; k += 2) acc = mfma_f32(pa[k], pb[k * TP], acc);
    return acc;
}

// One wave per (query tile, head, image): L = log sum_j exp S over the image's keys, tiles in ascending order (a running maximum), then
// O = sum_j exp(S - L) V with the same S.  O [n * m][256], L [n][8][m].
__global__ __launch_bounds__(64) void attn_fwd_kernel(const float* __restrict__ qkv, int m, float* __restrict__ O, float* __restrict__ L) {
    __shared__ float sQ[TILE_FLOATS], sK[TILE_FLOATS], sV[TILE_FLOATS], sP[TILE_FLOATS];
    const int lane = threadIdx.x, col = lane & 31, q0 = blockIdx.x * T, h = blockIdx.y;
    const long img = blockIdx.z;
    const float* base = qkv + img * m * QKV + h * HD;
    load_tile(sQ, base, QKV, q0, m, lane, ATTN_SCALE);
    float mx[16], sm[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[r] = -INFINITY, sm[r] = 0.f;
    for (int j0 = 0; j0 < m; j0 += T) {
        __syncthreads();
        load_tile(sK, base + D, QKV, j0, m, lane);
        __syncthreads();
        const float16v s = tile_abt(sQ, sK, lane);
        const bool live = j0 + col < m;          // a tile's first key always is: the maximum is finite
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = live ? s[r] : -INFINITY;
            const float nm = fmaxf(mx[r], half_max(v));
            sm[r] = sm[r] * expf(mx[r] - nm) + half_sum(live ? expf(v - nm) : 0.f);
            mx[r] = nm;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[r] += logf(sm[r]);          // now L
    float16v o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    for (int j0 = 0; j0 < m; j0 += T) {
        __syncthreads();
        load_tile(sK, base + D, QKV, j0, m, lane);
        load_tile(sV, base + 2 * D, QKV, j0, m, lane);
        __syncthreads();
        const float16v s = tile_abt(sQ, sK, lane);
        const bool live = j0 + col < m;
#pragma unroll
        for (int r = 0; r < 16; ++r) sP[out_row(r, lane) * TP + col] = live ? expf(s[r] - mx[r]) : 0.f;
        __syncthreads();
        o = tile_ab(sP, sV, o, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = q0 + out_row(r, lane);
        if (row < m) {
            O[(img * m + row) * D + h * HD + col] = o[r];
            if (col == 0) L[(img * NH + h) * m + row] = mx[r];
        }
    }
}

// delta [n][8][m]: delta[i] = sum_d dO[i][d] O[i][d], as the diagonal of the tile dO . O^T -- the very MFMA chain that forms dP = dO . V^T,
// so where a row attends to one key alone (O = V) dP - delta is an exact 0
__global__ __launch_bounds__(64) void attn_delta_kernel(const float* __restrict__ dO, const float* __restrict__ O, int m, float* __restrict__ delta) {
    __shared__ float sA[TILE_FLOATS], sB[TILE_FLOATS];
    const int lane = threadIdx.x, col = lane & 31, q0 = blockIdx.x * T, h = blockIdx.y;
    const long img = blockIdx.z;
    load_tile(sA, dO + img * m * D + h * HD, D, q0, m, lane);
    load_tile(sB, O + img * m * D + h * HD, D, q0, m, lane);
    __syncthreads();
    const float16v acc = tile_abt(sA, sB, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (out_row(r, lane) == col && q0 + col < m) delta[(img * NH + h) * m + q0 + col] = acc[r];
}

// One wave per (query tile, head, image), the key tiles in ascending order: dQ = sum_j dS K / sqrt 32 -> dqkv[.][0 .. 255]
__global__ __launch_bounds__(64) void attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ L,
                                                        const float* __restrict__ delta, int m, float* __restrict__ dqkv) {
    __shared__ float sQ[TILE_FLOATS], sD[TILE_FLOATS], sK[TILE_FLOATS], sV[TILE_FLOATS], sS[TILE_FLOATS];
    const int lane = threadIdx.x, col = lane & 31, q0 = blockIdx.x * T, h = blockIdx.y;
    const long img = blockIdx.z;
    const float* base = qkv + img * m * QKV + h * HD;
    load_tile(sQ, base, QKV, q0, m, lane, ATTN_SCALE);
    load_tile(sD, dO + img * m * D + h * HD, D, q0, m, lane);
    float lr[16], dr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = q0 + out_row(r, lane);
        lr[r] = row < m ? L[(img * NH + h) * m + row] : 0.f;
        dr[r] = row < m ? delta[(img * NH + h) * m + row] : 0.f;
    }
    float16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int j0 = 0; j0 < m; j0 += T) {
        __syncthreads();
        load_tile(sK, base + D, QKV, j0, m, lane);
        load_tile(sV, base + 2 * D, QKV, j0, m, lane);
        __syncthreads();
        const float16v s = tile_abt(sQ, sK, lane), dp = tile_abt(sD, sV, lane);
        const bool live = j0 + col < m;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = live ? expf(s[r] - lr[r]) : 0.f;
            sS[out_row(r, lane) * TP + col] = p * (dp[r] - dr[r]);
        }
        __syncthreads();
        acc = tile_ab(sS, sK, acc, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = q0 + out_row(r, lane);
        if (row < m) dqkv[(img * m + row) * QKV + h * HD + col] = acc[r] * ATTN_SCALE;
    }
}

// One wave per (key tile, head, image), the query tiles in ascending order, on the transposed tiles S^T = K . q^T (the same products in
// the same order as S, so the same bits): dV = sum_i P^T dO -> dqkv[.][512 ..], dK = sum_i dS^T q (q scaled) -> dqkv[.][256 ..]
__global__ __launch_bounds__(64) void attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dO, const float* __restrict__ L,
                                                         const float* __restrict__ delta, int m, float* __restrict__ dqkv) {
    __shared__ float sK[TILE_FLOATS], sV[TILE_FLOATS], sQ[TILE_FLOATS], sD[TILE_FLOATS], sP[TILE_FLOATS], sS[TILE_FLOATS];
    const int lane = threadIdx.x, col = lane & 31, j0 = blockIdx.x * T, h = blockIdx.y;
    const long img = blockIdx.z;
    const float* base = qkv + img * m * QKV + h * HD;
    load_tile(sK, base + D, QKV, j0, m, lane);
    load_tile(sV, base + 2 * D, QKV, j0, m, lane);
    float16v dk, dv;
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] = 0.f, dv[r] = 0.f;
    for (int i0 = 0; i0 < m; i0 += T) {
        __syncthreads();
        load_tile(sQ, base, QKV, i0, m, lane, ATTN_SCALE);
        load_tile(sD, dO + img * m * D + h * HD, D, i0, m, lane);
        const bool qlive = i0 + col < m;          // the query of this lane's column
        const float lc = qlive ? L[(img * NH + h) * m + i0 + col] : 0.f, dc = qlive ? delta[(img * NH + h) * m + i0 + col] : 0.f;
        __syncthreads();
        const float16v st = tile_abt(sK, sQ, lane), dpt = tile_abt(sV, sD, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = out_row(r, lane);
            const float p = qlive && j0 + row < m ? expf(st[r] - lc) : 0.f;
            sP[row * TP + col] = p;
            sS[row * TP + col] = p * (dpt[r] - dc);
        }
        __syncthreads();
        dv = tile_ab(sP, sD, dv, lane);
        dk = tile_ab(sS, sQ, dk, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = j0 + out_row(r, lane);
        if (row < m) {
            dqkv[(img * m + row) * QKV + D + h * HD + col] = dk[r];
            dqkv[(img * m + row) * QKV + 2 * D + h * HD + col] = dv[r];
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

struct Layout {
    float *qkv, *o, *lse, *t, *y, *xhat, *rstd, *dy, *ds, *d_o, *delta, *dqkv, *part;
    long long bytes;
};

Layout lay_out(void* scratch, long R) {
    Layout L;
    Bump b{static_cast<char*>(scratch)};
    L.qkv = b.take(R * QKV);
    L.o = b.take(R * D);
    L.lse = b.take(R * NH);
    L.t = b.take(R * D);
    L.y = b.take(R * D);
    L.xhat = b.take(R * D);
    L.rstd = b.take(R);
    L.dy = b.take(R * D);
    L.ds = b.take(R * D);
    L.d_o = b.take(R * D);
    L.delta = b.take(R * NH);
    L.dqkv = b.take(R * QKV);
    L.part = b.take(ceil_div(R, (long)CHUNK) * QKV * D);          // in_proj's weight gradient, one partial per row chunk, is the largest
    L.bytes = b.off;
    return L;
}

}  // namespace

long long dvid_self_attn_backward_scratch_bytes_host(long long n, long long m) {
    if (n < 1 || m < 1 || n > 65535 || m > DVID_CRITERION_MAX_ROWS || n * m > DVID_HEAD_TAIL_BWD_MAX_ROWS) return -1;
    return lay_out(nullptr, (long)(n * m)).bytes;
}

int dvid_self_attn_backward_launch(const SelfAttnBwdArgs& a, hipStream_t s) {
    const int n = a.n, m = a.m;
    const long R = (long)n * m;
    const Layout L = lay_out(a.scratch, R);
    Run run{s, L.part};
    const float* const* P = a.params;
    const float *Wi = P[0], *bi = P[1], *Wo = P[2], *bo = P[3], *g = P[4], *b = P[5];
    const dim3 rows4((unsigned)ceil_div(R, 4L)), tiles(ceil_div(m, T), NH, n);

    // ---- forward, recomputed in fp32
    run.fwd(a.x, Wi, bi, 0, R, QKV, D, L.qkv);
    if (run.rc != DVID_OK) return run.rc;
    hipLaunchKernelGGL(attn_fwd_kernel, tiles, dim3(64), 0, s, L.qkv, m, L.o, L.lse);
    run.fwd(L.o, Wo, bo, 0, R, D, D, L.t);
    if (run.rc != DVID_OK) return run.rc;
    float* y = a.y_out ? a.y_out : L.y;
    hipLaunchKernelGGL(ln_fwd_kernel, rows4, dim3(256), 0, s, L.t, a.x, g, b, 0, R, y, L.xhat, L.rstd);
    LAUNCH_CHECK();
    if (!a.grads) return DVID_OK;          // forward only

    // ---- backward
    float* const* G = a.grads;
    const float* dy = a.d_y;
    if (!dy) {
        HIP_TRY(hipMemsetAsync(L.dy, 0, (size_t)R * D * 4, s));
        dy = L.dy;
    }
    // norm1 and the residual: ds is the cotangent of x + out_proj(O), the skip's share of d_x
    hipLaunchKernelGGL(ln_bwd_kernel, rows4, dim3(256), 0, s, dy, (const float*)nullptr, L.xhat, L.rstd, g, R, (float*)nullptr, L.ds);
    run.colsum(dy, L.xhat, D, (int)R, 1, G[4], 0);
    run.colsum(dy, nullptr, D, (int)R, 1, G[5], 0);
    // out_proj
    run.wgrad(L.ds, L.o, R, D, D, G[2]);
    run.colsum(L.ds, nullptr, D, (int)R, 1, G[3], 0);
    run.dgrad(L.ds, Wo, R, D, D, L.d_o);
    if (run.rc != DVID_OK) return run.rc;
    // the attention: every element of dqkv has one writer
    hipLaunchKernelGGL(attn_delta_kernel, tiles, dim3(64), 0, s, L.d_o, L.o, m, L.delta);
    hipLaunchKernelGGL(attn_bwd_q_kernel, tiles, dim3(64), 0, s, L.qkv, L.d_o, L.lse, L.delta, m, L.dqkv);
    hipLaunchKernelGGL(attn_bwd_kv_kernel, tiles, dim3(64), 0, s, L.qkv, L.d_o, L.lse, L.delta, m, L.dqkv);
    // in_proj; d_x = the skip + dqkv . W_in
    run.wgrad(L.dqkv, a.x, R, QKV, D, G[0]);
    run.colsum(L.dqkv, nullptr, QKV, (int)R, 1, G[1], 0);
    run.dgrad(L.dqkv, Wi, R, QKV, D, a.d_x, L.ds);
    if (run.rc != DVID_OK) return run.rc;
    LAUNCH_CHECK();
    return DVID_OK;
}
