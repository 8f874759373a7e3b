// What the fp32 backward passes share (csrc/headtail_bwd.hip, csrc/interact_bwd.hip): the strided fp32-MFMA product with its fixed-order
// split reduction, the column sums over rows, LayerNorm forward / backward per row, and the host helpers that launch them and walk a
// scratch layout.  headtail_bwd.hip's header states the arithmetic; each including file gets its own copy in its unnamed namespace.
#pragma once
#include "../../include/dvid_hip.h"
#include "common.h"

namespace {

constexpr int D = 256;
constexpr int CHUNK = DVID_HEAD_TAIL_BWD_ROW_CHUNK;          // rows of one partial of a reduction over rows
constexpr int BT = 64, BK = 16, LDP = 96;                    // tile, K step, LDS pitch (a 32-lane half reads one bank half)
static_assert(CHUNK % BK == 0 && CHUNK % 4 == 0, "the row chunk is whole K steps");

struct GemmP {
    const float* A;
    long sai, sar;          // A(i, r) = A[i * sai + r * sar]
    const float* B;
    long sbj, sbr;          // B(j, r) = B[j * sbj + r * sbr]
    float* C;
    long ldc;
    int I, J, K;
    int kchunk;             // blockIdx.z reduces r in [z kchunk, min(K, (z + 1) kchunk)) into the tile at C + z * I * ldc
    const float* bias;      // + bias[j]
    const float* addend;    // + addend[i * ldc + j]
    const float* mask;      // then 0 where mask[i * ldc + j] <= 0 (ReLU backward on the kept post-activation)
    int relu;
};

__global__ __launch_bounds__(256) void gemm_kernel(GemmP p) {
    __shared__ float As[2][BK * LDP], Bs[2][BK * LDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wi = wave >> 1, wj = wave & 1;
    const int i0 = blockIdx.y * BT, j0 = blockIdx.x * BT, z = blockIdx.z;
    const int kbeg = z * p.kchunk, kend = min(p.K, kbeg + p.kchunk);
    // a thread stages 4 elements of each operand per K step; the lanes of a wave run along whichever index is contiguous in memory
    const bool a_km = p.sar == 1, b_km = p.sbr == 1;
    const int ai = a_km ? tid >> 2 : tid & 63, ar = a_km ? (tid & 3) * 4 : (tid >> 6) * 4;
    const int bj = b_km ? tid >> 2 : tid & 63, br = b_km ? (tid & 3) * 4 : (tid >> 6) * 4;
    const bool aok = i0 + ai < p.I, bok = j0 + bj < p.J;
    const float* ap = p.A + (long)(aok ? i0 + ai : 0) * p.sai;
    const float* bp = p.B + (long)(bok ? j0 + bj : 0) * p.sbj;
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r1 = k0 + ar + e, r2 = k0 + br + e;
            ra[e] = (aok && r1 < kend) ? ap[(long)r1 * p.sar] : 0.f;
            rb[e] = (bok && r2 < kend) ? bp[(long)r2 * p.sbr] : 0.f;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            As[buf][(ar + e) * LDP + ai] = ra[e];
            Bs[buf][(br + e) * LDP + bj] = rb[e];
        }
    };
    float16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nk = (kend - kbeg + BK - 1) / BK;
    fetch(kbeg);
    stage(0);
    __syncthreads();
    // MFMA operand maps (cdna_hip_programming.md): A lane l = A[i = l & 31][k = l >> 5], B lane l = B[k = l >> 5][j = l & 31]
    const int fa = (lane >> 5) * LDP + wi * 32 + (lane & 31), fb = (lane >> 5) * LDP + wj * 32 + (lane & 31);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) fetch(kbeg + (kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) acc = mfma_f32(As[buf][2 * kk * LDP + fa], Bs[buf][2 * kk * LDP + fb], acc);
        if (kt + 1 < nk) stage(buf ^ 1);
        __syncthreads();
    }
    // register r = row (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3), column lane & 31
    float* c = p.C + (long)z * p.I * p.ldc;
    const int col = j0 + wj * 32 + (lane & 31);
    if (col < p.J) {
        const float bb = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + wi * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
            if (row < p.I) {
                const long o = (long)row * p.ldc + col;
                float v = acc[r] + bb;
                if (p.addend) v += p.addend[o];
                if (p.relu) v = fmaxf(v, 0.f);
                if (p.mask && !(p.mask[o] > 0.f)) v = 0.f;
                c[o] = v;
            }
        }
    }
}

// out[s * ldo + i] = sum over z ascending of part[(s * nz + z) * count + i]
__global__ void reduce_partials_kernel(const float* __restrict__ part, int nz, long count, float* __restrict__ out, long ldo) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const long s = blockIdx.y;
    const float* q = part + s * nz * count + i;
    float v = q[0];
    for (int zz = 1; zz < nz; ++zz) v += q[(long)zz * count];
    out[s * ldo + i] = v;
}

// part[(seg * nchunk + chunk) * cols + c] = sum over the chunk's rows, ascending within each quarter and the quarters in order, of
// A[r][c] * (B ? B[r][c] : 1).  Segment seg = rows [seg * seg_len, (seg + 1) * seg_len); chunks are counted from the segment's first row.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ A, const float* __restrict__ B, int cols, int seg_len, int nchunk,
                                                             float* __restrict__ part) {
    __shared__ float sh[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const int chunk = blockIdx.y, seg = blockIdx.z;
    const int rbeg = chunk * CHUNK + q * (CHUNK / 4), rend = min(seg_len, min((chunk + 1) * CHUNK, rbeg + CHUNK / 4));
    float v = 0.f;
    if (c < cols) {
        const long base = (long)seg * seg_len;
        for (int r = rbeg; r < rend; ++r) {
            const long o = (base + r) * cols + c;
            v += B ? A[o] * B[o] : A[o];
        }
    }
    sh[q][threadIdx.x & 63] = v;
    __syncthreads();
    if (q == 0 && c < cols) part[((long)seg * nchunk + chunk) * cols + c] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

__device__ __forceinline__ float row_sum(float4v v) { return wave_sum((v[0] + v[1]) + (v[2] + v[3])); }

// out = [ReLU] LayerNorm(in + res) * g + b per row, one wave per row of 256; keeps xhat and rstd (two-pass fp32 statistics)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ in, const float* __restrict__ res, const float* __restrict__ g,
                                                     const float* __restrict__ b, int relu, long R, float* __restrict__ out, float* __restrict__ xhat,
                                                     float* __restrict__ rstd) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int col = (threadIdx.x & 63) * 4;
    float4v v = *reinterpret_cast<const float4v*>(in + row * D + col);
    if (res) v += *reinterpret_cast<const float4v*>(res + row * D + col);
    const float mean = row_sum(v) / D;
    const float4v t = v - mean;
    const float rs = 1.f / sqrtf(row_sum(t * t) / D + 1e-5f);
    const float4v xh = t * rs;
    float4v o = xh * *reinterpret_cast<const float4v*>(g + col) + *reinterpret_cast<const float4v*>(b + col);
    if (relu)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
    *reinterpret_cast<float4v*>(out + row * D + col) = o;
    *reinterpret_cast<float4v*>(xhat + row * D + col) = xh;
    if ((threadIdx.x & 63) == 0) rstd[row] = rs;
}

// dy = dout where act > 0 (act: the kept ReLU output; null = no ReLU), written to `dy` when act is given;
// dz = rstd * (dy g - mean(dy g) - xhat mean(dy g xhat))
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ act, const float* __restrict__ xhat,
                                                     const float* __restrict__ rstd, const float* __restrict__ g, long R, float* __restrict__ dy,
                                                     float* __restrict__ dz) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int col = (threadIdx.x & 63) * 4;
    float4v d = *reinterpret_cast<const float4v*>(dout + row * D + col);
    if (act) {
        const float4v a = *reinterpret_cast<const float4v*>(act + row * D + col);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!(a[e] > 0.f)) d[e] = 0.f;
        *reinterpret_cast<float4v*>(dy + row * D + col) = d;
    }
    const float4v xh = *reinterpret_cast<const float4v*>(xhat + row * D + col);
    const float4v dx = d * *reinterpret_cast<const float4v*>(g + col);
    const float m1 = row_sum(dx) / D, m2 = row_sum(dx * xh) / D;
    *reinterpret_cast<float4v*>(dz + row * D + col) = (dx - m1 - xh * m2) * rstd[row];
}

struct Bump {          // the scratch layout, walked alike by the size query (base null) and the launch
    char* base;
    long long off = 0;
    float* take(long long floats) {
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += (floats * 4 + 255) / 256 * 256;
        return p;
    }
};

struct Run {
    hipStream_t s;
    float* part;
    int rc = DVID_OK;
    void gemm(GemmP p, int nz = 1) {
        if (rc != DVID_OK) return;
        p.kchunk = nz > 1 ? CHUNK : p.K;
        hipLaunchKernelGGL(gemm_kernel, dim3(ceil_div(p.J, BT), ceil_div(p.I, BT), nz), dim3(256), 0, s, p);
        if (hipGetLastError() != hipSuccess) rc = DVID_ERR_HIP;
    }
    // Y[rows][J] = X[rows][K] . W[J][K]^T (+ bias) (ReLU)
    void fwd(const float* X, const float* W, const float* bias, int relu, long rows, int J, int K, float* Y) {
        gemm({X, K, 1, W, K, 1, Y, J, (int)rows, J, K, 0, bias, nullptr, nullptr, relu});
    }
    // dX[rows][K] = dY[rows][J] . W[J][K] (+ addend) (masked)
    void dgrad(const float* dY, const float* W, long rows, int J, int K, float* dX, const float* addend = nullptr, const float* mask = nullptr) {
        gemm({dY, J, 1, W, 1, K, dX, K, (int)rows, K, J, 0, nullptr, addend, mask, 0});
    }
    // dW[J][K] = sum over rows of dY[r][J]^T X[r][K]: partial tiles per row chunk, added in chunk order
    void wgrad(const float* dY, const float* X, long rows, int J, int K, float* dW) {
        const int nz = (int)ceil_div(rows, (long)CHUNK);
        GemmP p{dY, 1, J, X, 1, K, part, K, J, K, (int)rows, 0, nullptr, nullptr, nullptr, 0};
        p.kchunk = CHUNK;
        if (rc != DVID_OK) return;
        hipLaunchKernelGGL(gemm_kernel, dim3(ceil_div(K, BT), ceil_div(J, BT), nz), dim3(256), 0, s, p);
        reduce(nz, (long)J * K, 1, dW, 0);
    }
    void reduce(int nz, long count, int segs, float* out, long ldo) {
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)ceil_div(count, 256L), segs), dim3(256), 0, s, part, nz, count, out, ldo);
        if (hipGetLastError() != hipSuccess) rc = DVID_ERR_HIP;
    }
    // out[seg * ldo + c] = sum over the rows of segment seg of A[r][c] (* B[r][c])
    void colsum(const float* A, const float* B, int cols, int seg_len, int segs, float* out, long ldo) {
        if (rc != DVID_OK) return;
        const int nchunk = ceil_div(seg_len, CHUNK);
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(ceil_div(cols, 64), nchunk, segs), dim3(256), 0, s, A, B, cols, seg_len, nchunk, part);
        reduce(nchunk, cols, segs, out, ldo);
    }
};

}  // namespace
