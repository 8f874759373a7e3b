// Multi-head attention on MFMA (fp16 operands, fp32 softmax / accumulate), head_dim 32.
//
// Used for the 300x300 per-frame self-attention of RCNNHead (box_head.py:514-518), the 2400x900 global-memory
// cross-attention of DynamicHead (box_head.py:366-380) and Swin's 7x7 / 12x12 window attention (swintransformer.py:98-176); the
// in/out projections are igemm launches.  (The round-1 fp32 VALU kernel is in this file's history.)
#include <stdlib.h>

#include "common.h"
#include "igemm_epilogue.h"
#include "kernels.h"

// =============================================================================================
// MFMA attention (fp16 operands, fp32 softmax/accumulate), head_dim 32.
//
// One wave = 16 queries, one workgroup = 4 waves = 64 queries of one (batch, head).  Per 32 keys:
//   S^T[key][q] = K[16 keys x 32 dims] . Q^T            two v_mfma_f32_16x16x32_f16 (swapped product, so a
//                                                        lane holds scores of ONE query: (lane & 15))
//   online softmax in registers: lane-local max/sum over its 8 keys, 2 xor-shuffles across the four
//   16-lane groups for the running max; the row sum is reduced across groups once at the end
//   O^T[d][q] += V^T[16 dims x 32 keys] . P^T           two MFMAs; P^T is built from the S^T accumulators
//                                                        in registers: MFMA k-slot (group g, j) <-> key
//                                                        (j < 4 ? 4g + j : 16 + 4g + j - 4), the same slot
//                                                        map is used for the V^T operand, so no LDS / no
//                                                        cross-lane traffic is needed for P.
// K rows and the pre-transposed V^T ([batch][head][32][lk_pad], attn_vt_kernel) are read straight from
// global memory (L1/L2 resident: 19 KB per (frame, head)).
// =============================================================================================
namespace {

constexpr int DH = 32;      // head dimension

// v16 [batch][lk][v_ld] (head h at column h*32) -> vt [batch][nheads][32][lk_pad] (zero padded keys)
__global__ void attn_vt_kernel(const half_t* __restrict__ v, half_t* __restrict__ vt, int lk, int lk_pad, int v_ld, long v_bs,
                               int nheads) {
    __shared__ half_t tile[32][33];
    const int k0 = blockIdx.x * 32, h = blockIdx.y, b = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 256 threads
    for (int r = ty; r < 32; r += 8) {
        const int key = k0 + r;
        tile[r][tx] = key < lk ? v[b * v_bs + (long)key * v_ld + h * 32 + tx] : (half_t)0.f;
    }
    __syncthreads();
    half_t* dst = vt + ((long)(b * nheads + h) * 32) * lk_pad;
    for (int r = ty; r < 32; r += 8) {
        const int key = k0 + tx;
        if (key < lk_pad) dst[(long)r * lk_pad + key] = tile[tx][r];
    }
}

__global__ __launch_bounds__(256) void mha_mfma_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k,
                                                        const half_t* __restrict__ vt, half_t* __restrict__ out, int lq, int lk,
                                                        int lk_pad, int q_ld, int k_ld, int out_ld, long q_bs, long k_bs,
                                                        long out_bs, int nheads, float scaling) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * 64 + wave * 16;
    if (q0 >= lq) return;                                          // whole wave out of range (no barriers below)
    const int qrow = min(q0 + qi, lq - 1);
    const half8 qf = *reinterpret_cast<const half8*>(q + b * q_bs + (long)qrow * q_ld + h * 32 + g * 8);   // B operand of S^T
    const half_t* kb = k + b * k_bs + h * 32 + g * 8;
    const half_t* vb = vt + ((long)(b * nheads + h) * 32) * lk_pad;

    float4v o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};   // O^T rows d = 4g + r (o0) and 16 + 4g + r (o1), column = query
    float m = -1e30f, l = 0.f;
    for (int k0 = 0; k0 < lk; k0 += 32) {
        // ---- scores for keys k0 .. k0+31 (two 16-key tiles) ----
        const int ka = min(k0 + qi, lk - 1), kbi = min(k0 + 16 + qi, lk - 1);       // A operand rows (clamped; masked below)
        const half8 kf0 = *reinterpret_cast<const half8*>(kb + (long)ka * k_ld);
        const half8 kf1 = *reinterpret_cast<const half8*>(kb + (long)kbi * k_ld);
        float4v s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf0, qf, s0, 0, 0, 0);          // rows = keys k0 + 4g + r
        s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf1, qf, s1, 0, 0, 0);          // rows = keys k0 + 16 + 4g + r
        float sc[8];
        float cmax = -1e30f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[r] = (k0 + 4 * g + r < lk) ? s0[r] * scaling : -1e30f;
            sc[4 + r] = (k0 + 16 + 4 * g + r < lk) ? s1[r] * scaling : -1e30f;
            cmax = fmaxf(cmax, fmaxf(sc[r], sc[4 + r]));
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
        const float mn = fmaxf(m, cmax);
        const float f = __expf(m - mn);
        float psum = 0.f;
        half8 pf;                                                   // B operand of O^T: k-slot j <-> sc[j]
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float pj = (sc[j] > -1e29f) ? __expf(sc[j] - mn) : 0.f;
            psum += pj;
            pf[j] = (half_t)pj;
        }
        l = l * f + psum;
        m = mn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0[r] *= f;
            o1[r] *= f;
        }
        // ---- V^T operand: row d = (lane & 15) (+16), k-slots = keys k0+4g..+3 and k0+16+4g..+3 ----
        const half_t* v0 = vb + (long)qi * lk_pad + k0 + 4 * g;
        const half_t* v1 = v0 + 16L * lk_pad;
        const half4 a00 = *reinterpret_cast<const half4*>(v0), a01 = *reinterpret_cast<const half4*>(v0 + 16);
        const half4 a10 = *reinterpret_cast<const half4*>(v1), a11 = *reinterpret_cast<const half4*>(v1 + 16);
        const half8 vf0 = {a00[0], a00[1], a00[2], a00[3], a01[0], a01[1], a01[2], a01[3]};
        const half8 vf1 = {a10[0], a10[1], a10[2], a10[3], a11[0], a11[1], a11[2], a11[3]};
        o0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf0, pf, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf1, pf, o1, 0, 0, 0);
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (q0 + qi >= lq) return;
    const float inv = 1.f / l;
    half_t* op = out + b * out_bs + (long)(q0 + qi) * out_ld + h * 32 + 4 * g;
    const half4 w0 = {(half_t)(o0[0] * inv), (half_t)(o0[1] * inv), (half_t)(o0[2] * inv), (half_t)(o0[3] * inv)};
    const half4 w1 = {(half_t)(o1[0] * inv), (half_t)(o1[1] * inv), (half_t)(o1[2] * inv), (half_t)(o1[3] * inv)};
    *reinterpret_cast<half4*>(op) = w0;
    *reinterpret_cast<half4*>(op + 16) = w1;
}

}  // namespace

// q16/k16/v16: fp16, head h at columns [h*32, h*32+32) of each row; vt_scratch: >= batch*nheads*32*lk_pad halves,
// lk_pad = round_up(lk, 32) + 32.
int dvid_mha_mfma_launch(const half_t* q, const half_t* k, const half_t* v, half_t* out, half_t* vt_scratch, int batch, int lq,
                         int lk, int nheads, int q_ld, int kv_ld, int out_ld, long q_bs, long kv_bs, long out_bs, hipStream_t s) {
    if (lq == 0 || batch == 0) return DVID_OK;
    if (lk <= 0 || (q_ld & 7) || (kv_ld & 7) || (out_ld & 3)) return DVID_ERR_ARG;
    const int lk_pad = (lk + 31) / 32 * 32 + 32;
    hipLaunchKernelGGL(attn_vt_kernel, dim3(lk_pad / 32, nheads, batch), dim3(256), 0, s, v, vt_scratch, lk, lk_pad, kv_ld, kv_bs, nheads);
    LAUNCH_CHECK();
    const float scaling = 1.0f / sqrtf((float)DH);
    hipLaunchKernelGGL(mha_mfma_kernel, dim3(ceil_div(lq, 64), nheads, batch), dim3(256), 0, s, q, k, vt_scratch, out, lq, lk, lk_pad,
                       q_ld, kv_ld, out_ld, q_bs, kv_bs, out_bs, nheads, scaling);
    LAUNCH_CHECK();
    return DVID_OK;
}

// =============================================================================================
// Swin (shifted-)window attention, window 7x7 (49 tokens), head_dim 32, MFMA.
// Replaces WindowAttention.forward + the pad / roll / window_partition / window_reverse plumbing of
// SwinTransformerBlock.forward (mega_core/modeling/backbone/swintransformer.py:135-176, :236-270):
// the window <-> token mapping (padding to multiples of 7, cyclic shift by 3) is resolved in the gather
// addresses, padded positions behave as tokens whose q/k/v equal the qkv bias (the reference pads the
// normalised activations with zeros BEFORE the qkv Linear), the relative-position bias comes from a
// per-layer [heads][49][49] fp32 table, and the SW-MSA mask (-100 between different shift regions,
// swintransformer.py:387-406) is recomputed from the positions' region ids.
// One workgroup = one (window, head): K and V^T of the 49 keys (padded to 64) are staged in LDS,
// each of the 4 waves owns 16 queries; same swapped-product / register-resident P scheme as mha_mfma.
// =============================================================================================
namespace {

// Position `pos` (< WS * WS) of window (wx, wy) of image b -> `tok`, the token row it gathers from (-1: a padded position), and `region`,
// its region of the shifted map's attention mask (swintransformer.py:226-254; 0 without a shift).  Hp / Wp: the map padded to whole
// windows.  The gather address resolves padding and roll.  Integer arithmetic, shared by the fp16 kernels of both window sizes; the fp32
// kernels further down keep the same statements inline (through this helper the compiler allocates them one SGPR less, and this
// file holds every kernel to the register table it had).
template <int WS>
__device__ __forceinline__ void swin_window_pos(int pos, int wx, int wy, int b, int H, int W, int Hp, int Wp, int shift, int& tok, int& region) {
    const int py = pos / WS, px = pos - py * WS;
    const int ys = wy * WS + py, xs = wx * WS + px;          // coordinates in the shifted, padded map
    int y = ys + shift, x = xs + shift;                      // source coordinates before the roll
    if (y >= Hp) y -= Hp;
    if (x >= Wp) x -= Wp;
    region = 0;
    if (shift > 0) {
        const int hr = ys < Hp - WS ? 0 : (ys < Hp - shift ? 1 : 2);
        const int wr = xs < Wp - WS ? 0 : (xs < Wp - shift ? 1 : 2);
        region = hr * 3 + wr;
    }
    tok = (y < H && x < W) ? (b * H + y) * W + x : -1;
}

template <int WPB>
__global__ __launch_bounds__(256) void swin_window_attn_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ qkv_bias16,
                                                                const float* __restrict__ relbias, half_t* __restrict__ out, int H,
                                                                int W, int C, int nheads, int shift, float scaling, int nwin,
                                                                int head_major) {
    constexpr int WS = 7, NT = 49, RB_PITCH = SWIN_RELBIAS_PITCH;
    __shared__ __attribute__((aligned(16))) half_t Ks[64 * 32];      // [key][32 dims]
    __shared__ __attribute__((aligned(16))) half_t Vt[32 * 72];      // [dim][key], pitch 72 halves
    __shared__ int tok[64];                                          // token row or -1 (padded position)
    __shared__ int region[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Launch order.  The heads of a window read neighbouring 64-byte pieces of the same qkv rows (two heads per 128-byte line) and
    // write neighbouring pieces of the same output rows: with the head innermost AND the workgroups of an XCD taking one contiguous
    // run of (window, head) pairs, those pieces meet in that XCD's L2 while the line is there; window-major order per head (the
    // former 2-D grid) fetched every line once per head that touches it.  head_major = 0 keeps the old order for A/B runs.
    // A workgroup takes WPB consecutive windows of ONE head: a lane's relative-position bias depends on its query position and the
    // head only, so it is fetched once per workgroup instead of once per window (16 of the 36 load / store instructions a
    // (window, head) pair costs the CU's L1 path otherwise).
    const int ngrp = (nwin + WPB - 1) / WPB;
    int h, grp;
    if (head_major) {
        const int lid = igemm_xcd_remap((int)blockIdx.x, ngrp * nheads);
        grp = lid / nheads;
        h = lid - grp * nheads;
    } else {
        h = (int)blockIdx.x / ngrp;
        grp = (int)blockIdx.x - h * ngrp;
    }
    const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
    const int nwx = Wp / WS, nwy = Hp / WS;
    const int qi = lane & 15, g = lane >> 4;
    const int qpos = wave * 16 + qi;                                   // query position inside the window (>= 49: idle)
    const int qp = min(qpos, NT - 1);
    const float* brow = relbias + ((long)h * NT + qp) * RB_PITCH + 4 * g;
    float4v bias4[4];                                                  // keys 4g.., 16 + 4g.., 32 + 4g.., 48 + 4g.. of the query's row
#pragma unroll
    for (int i = 0; i < 4; ++i) bias4[i] = *reinterpret_cast<const float4v*>(brow + 16 * i);

    for (int w = 0; w < WPB; ++w) {
    int wid = grp * WPB + w;
    if (wid >= nwin) break;                                            // (uniform over the workgroup)
    if (w) __syncthreads();                                            // the previous window's LDS reads are done
    const int wx = wid % nwx;
    wid /= nwx;
    const int wy = wid % nwy;
    const int b = wid / nwy;

    if (tid < 64) {
        int t = -1, reg = 0;
        if (tid < NT) swin_window_pos<WS>(tid, wx, wy, b, H, W, Hp, Wp, shift, t, reg);
        tok[tid] = t;
        region[tid] = reg;
    }
    __syncthreads();
    // ---- every global read of the window goes out here, ahead of the LDS staging and its barrier: K / V of the thread's
    // (key, 16-byte chunk) and the lane's query fragment (its bias, 4 x 16 bytes of the query's 64-float row, is loaded above)
    const int tq = tok[qp];
    const int qreg = region[qp];
    const int key_s = tid >> 2, ch = tid & 3;
    half8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (key_s < NT) {
        const int t = tok[key_s];
        const half_t* src = t >= 0 ? qkv + (long)t * 3 * C : qkv_bias16;
        kv = *reinterpret_cast<const half8*>(src + C + h * 32 + ch * 8);
        vv = *reinterpret_cast<const half8*>(src + 2 * C + h * 32 + ch * 8);
    }
    const half_t* qsrc = tq >= 0 ? qkv + (long)tq * 3 * C : qkv_bias16;
    const half8 qf = *reinterpret_cast<const half8*>(qsrc + h * 32 + g * 8);
    // ---- stage K rows and V^T ----
    *reinterpret_cast<half8*>(Ks + key_s * 32 + ch * 8) = kv;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * 72 + key_s] = vv[e];
    __syncthreads();

    float4v o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;
#pragma unroll
    for (int k0 = 0; k0 < 64; k0 += 32) {
        const half8 kf0 = *reinterpret_cast<const half8*>(Ks + (k0 + qi) * 32 + g * 8);
        const half8 kf1 = *reinterpret_cast<const half8*>(Ks + (k0 + 16 + qi) * 32 + g * 8);
        float4v s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf0, qf, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf1, qf, s1, 0, 0, 0);
        float sc[8];
        float cmax = -1e30f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int key = k0 + (r < 4 ? 4 * g + r : 16 + 4 * g + (r - 4));
            float v = -1e30f;
            if (key < NT) {
                v = (r < 4 ? s0[r] * scaling + bias4[k0 / 16][r] : s1[r - 4] * scaling + bias4[k0 / 16 + 1][r - 4]);
                if (shift > 0 && region[key] != qreg) v += -100.0f;
            }
            sc[r] = v;
            cmax = fmaxf(cmax, v);
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
        const float mn = fmaxf(m, cmax);
        const float f = __expf(m - mn);
        float psum = 0.f;
        half8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float pj = (sc[j] > -1e29f) ? __expf(sc[j] - mn) : 0.f;
            psum += pj;
            pf[j] = (half_t)pj;
        }
        l = l * f + psum;
        m = mn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0[r] *= f;
            o1[r] *= f;
        }
        const half_t* v0 = Vt + qi * 72 + k0 + 4 * g;
        const half_t* v1 = v0 + 16 * 72;
        const half4 a00 = *reinterpret_cast<const half4*>(v0), a01 = *reinterpret_cast<const half4*>(v0 + 16);
        const half4 a10 = *reinterpret_cast<const half4*>(v1), a11 = *reinterpret_cast<const half4*>(v1 + 16);
        const half8 vf0 = {a00[0], a00[1], a00[2], a00[3], a01[0], a01[1], a01[2], a01[3]};
        const half8 vf1 = {a10[0], a10[1], a10[2], a10[3], a11[0], a11[1], a11[2], a11[3]};
        o0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf0, pf, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf1, pf, o1, 0, 0, 0);
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qpos < NT && tq >= 0) {                                        // padded positions produce no output
        const float inv = 1.f / l;
        half_t* op = out + (long)tq * C + h * 32 + 4 * g;
        const half4 w0 = {(half_t)(o0[0] * inv), (half_t)(o0[1] * inv), (half_t)(o0[2] * inv), (half_t)(o0[3] * inv)};
        const half4 w1 = {(half_t)(o1[0] * inv), (half_t)(o1[1] * inv), (half_t)(o1[2] * inv), (half_t)(o1[3] * inv)};
        *reinterpret_cast<half4*>(op) = w0;
        *reinterpret_cast<half4*>(op + 16) = w1;
    }
    }      // windows of the workgroup
}

}  // namespace

// qkv fp16 [B*H*W, 3C] (q | k | v, head h at columns 32h..), relbias fp32 [nheads][49][SWIN_RELBIAS_PITCH] (rows padded to 64 keys), out fp16 [B*H*W, C]
int dvid_swin_window_attn_launch(const half_t* qkv, const half_t* qkv_bias16, const float* relbias, half_t* out, int batch, int H,
                                 int W, int C, int nheads, int shift, hipStream_t s) {
    if (C != nheads * 32) return DVID_ERR_UNSUPPORTED;
    const int nwy = (H + 6) / 7, nwx = (W + 6) / 7;
    const long nwin = (long)batch * nwy * nwx;
    if (nwin * nheads > 0x7fffffffL) return DVID_ERR_UNSUPPORTED;
    // four windows per workgroup, head-major order (one window per workgroup and window-major order were measured slower: profiles/r02e_*)
    hipLaunchKernelGGL(swin_window_attn_kernel<4>, dim3((unsigned)((nwin + 3) / 4 * nheads)), dim3(256), 0, s, qkv, qkv_bias16, relbias, out,
                       H, W, C, nheads, shift, 1.0f / sqrtf(32.f), (int)nwin, 1);
    LAUNCH_CHECK();
    return DVID_OK;
}

// =============================================================================================
// Swin (shifted-)window attention, window 12x12 (144 tokens), shift 0 or 6, head_dim 32, MFMA: the 384-pretrained sizes
// (B-22k-384, L-22k-384).  Same conventions as the 7x7 kernel above -- gather addresses resolve padding and roll, a padded position
// holds the qkv bias and writes nothing, region ids from Hp / Wp / shift, -100 between regions, online fp32 softmax, P rounded to fp16
// in registers -- on a different decomposition:
//   144 queries are nine 16-row tiles exactly, so a workgroup is NINE waves (576 threads), one tile each, and no lane idles; the 576
//   (key, 16-byte chunk) pairs of K and of V are one pair per thread.
//   144 keys are 4.5 k-steps of 32: K rows and V^T columns 144..159 are zeroed once per workgroup (P is 0 there, but 0 x stale LDS
//   bits could be 0 x NaN), scores of keys >= 144 are masked as the 7x7 kernel masks keys >= 49.
//   LDS: K [160][32] 10 KB + V^T [32][168] 10.5 KB + token / region ids 1.1 KB = 21.8 KB.  (Registers, not LDS, set the occupancy:
//   120 VGPRs with the bias row resident = 4 waves per SIMD = one nine-wave workgroup per CU at a time.)
//   V^T pitch 168 halves = 84 dwords: the 16 rows a ds_read_b64 group touches start 20 banks apart (mod 64), conflict-free.
//   A lane's bias (its query's 160-float row, 40 floats per lane) is the largest read of a (window, head) pair: 92 KB against 27 KB
//   of q / k / v.  WPB consecutive windows of ONE head share it in registers, as above.
// =============================================================================================
namespace {

template <int WPB>
__global__ __launch_bounds__(576) void swin_window12_attn_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ qkv_bias16,
                                                                  const float* __restrict__ relbias, half_t* __restrict__ out, int H,
                                                                  int W, int C, int nheads, int shift, float scaling, int nwin) {
    constexpr int WS = 12, NT = 144, NK = 160, RB_PITCH = SWIN12_RELBIAS_PITCH, VP = 168;
    static_assert(RB_PITCH == NK, "one bias float per padded key");
    __shared__ __attribute__((aligned(16))) half_t Ks[NK * 32];      // [key][32 dims], rows 144.. zero
    __shared__ __attribute__((aligned(16))) half_t Vt[32 * VP];      // [dim][key], columns 144..159 zero
    __shared__ int tok[NT];                                          // token row or -1 (padded position)
    __shared__ int region[NT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // head innermost, one contiguous run of (window group, head) pairs per XCD: see the 7x7 kernel
    const int ngrp = (nwin + WPB - 1) / WPB;
    const int lid = igemm_xcd_remap((int)blockIdx.x, ngrp * nheads);
    const int grp = lid / nheads;
    const int h = lid - grp * nheads;
    const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
    const int nwx = Wp / WS, nwy = Hp / WS;
    const int qi = lane & 15, g = lane >> 4;
    const int qpos = wave * 16 + qi;                                   // query position inside the window, < 144
    const float* brow = relbias + ((long)h * NT + qpos) * RB_PITCH + 4 * g;
    float4v bias4[NK / 16];                                            // keys 16 i + 4g .. + 3 of the query's row
#pragma unroll
    for (int i = 0; i < NK / 16; ++i) bias4[i] = *reinterpret_cast<const float4v*>(brow + 16 * i);
    // the padded keys, once: no window writes them
    if (tid < 64) *reinterpret_cast<half8*>(Ks + NT * 32 + tid * 8) = (half8){0, 0, 0, 0, 0, 0, 0, 0};
    else if (tid < 192) *reinterpret_cast<half4*>(Vt + ((tid - 64) >> 2) * VP + NT + ((tid - 64) & 3) * 4) = (half4){0, 0, 0, 0};

    for (int w = 0; w < WPB; ++w) {
    int wid = grp * WPB + w;
    if (wid >= nwin) break;                                            // (uniform over the workgroup)
    if (w) __syncthreads();                                            // the previous window's LDS reads are done
    const int wx = wid % nwx;
    wid /= nwx;
    const int wy = wid % nwy;
    const int b = wid / nwy;

    if (tid < NT) {
        int t, reg;
        swin_window_pos<WS>(tid, wx, wy, b, H, W, Hp, Wp, shift, t, reg);
        tok[tid] = t;
        region[tid] = reg;
    }
    __syncthreads();
    // ---- the window's global reads, ahead of the LDS staging and its barrier: K / V of the thread's (key, 16-byte chunk) and the
    // lane's query fragment
    const int tq = tok[qpos];
    const int qreg = region[qpos];
    const int key_s = tid >> 2, ch = tid & 3;                          // 576 threads = 144 keys x 4 chunks
    const int tk = tok[key_s];
    const half_t* src = tk >= 0 ? qkv + (long)tk * 3 * C : qkv_bias16;
    const half8 kv = *reinterpret_cast<const half8*>(src + C + h * 32 + ch * 8);
    const half8 vv = *reinterpret_cast<const half8*>(src + 2 * C + h * 32 + ch * 8);
    const half_t* qsrc = tq >= 0 ? qkv + (long)tq * 3 * C : qkv_bias16;
    const half8 qf = *reinterpret_cast<const half8*>(qsrc + h * 32 + g * 8);
    // ---- stage K rows and V^T ----
    *reinterpret_cast<half8*>(Ks + key_s * 32 + ch * 8) = kv;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * VP + key_s] = vv[e];
    __syncthreads();

    float4v o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;
#pragma unroll
    for (int k0 = 0; k0 < NK; k0 += 32) {
        const half8 kf0 = *reinterpret_cast<const half8*>(Ks + (k0 + qi) * 32 + g * 8);
        const half8 kf1 = *reinterpret_cast<const half8*>(Ks + (k0 + 16 + qi) * 32 + g * 8);
        float4v s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf0, qf, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf1, qf, s1, 0, 0, 0);
        float sc[8];
        float cmax = -1e30f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int key = k0 + (r < 4 ? 4 * g + r : 16 + 4 * g + (r - 4));
            float v = -1e30f;
            if (key < NT) {
                v = (r < 4 ? s0[r] * scaling + bias4[k0 / 16][r] : s1[r - 4] * scaling + bias4[k0 / 16 + 1][r - 4]);
                if (shift > 0 && region[key] != qreg) v += -100.0f;
            }
            sc[r] = v;
            cmax = fmaxf(cmax, v);
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
        const float mn = fmaxf(m, cmax);
        const float f = __expf(m - mn);
        float psum = 0.f;
        half8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float pj = (sc[j] > -1e29f) ? __expf(sc[j] - mn) : 0.f;
            psum += pj;
            pf[j] = (half_t)pj;
        }
        l = l * f + psum;
        m = mn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0[r] *= f;
            o1[r] *= f;
        }
        const half_t* v0 = Vt + qi * VP + k0 + 4 * g;
        const half_t* v1 = v0 + 16 * VP;
        const half4 a00 = *reinterpret_cast<const half4*>(v0), a01 = *reinterpret_cast<const half4*>(v0 + 16);
        const half4 a10 = *reinterpret_cast<const half4*>(v1), a11 = *reinterpret_cast<const half4*>(v1 + 16);
        const half8 vf0 = {a00[0], a00[1], a00[2], a00[3], a01[0], a01[1], a01[2], a01[3]};
        const half8 vf1 = {a10[0], a10[1], a10[2], a10[3], a11[0], a11[1], a11[2], a11[3]};
        o0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf0, pf, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf1, pf, o1, 0, 0, 0);
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (tq >= 0) {                                                     // padded positions produce no output
        const float inv = 1.f / l;
        half_t* op = out + (long)tq * C + h * 32 + 4 * g;
        const half4 w0 = {(half_t)(o0[0] * inv), (half_t)(o0[1] * inv), (half_t)(o0[2] * inv), (half_t)(o0[3] * inv)};
        const half4 w1 = {(half_t)(o1[0] * inv), (half_t)(o1[1] * inv), (half_t)(o1[2] * inv), (half_t)(o1[3] * inv)};
        *reinterpret_cast<half4*>(op) = w0;
        *reinterpret_cast<half4*>(op + 16) = w1;
    }
    }      // windows of the workgroup
}

}  // namespace

// the 12x12 form of dvid_swin_window_attn_launch: relbias fp32 [nheads][144][SWIN12_RELBIAS_PITCH] (rows padded to 160 keys), shift 0 or 6
int dvid_swin_window12_attn_launch(const half_t* qkv, const half_t* qkv_bias16, const float* relbias, half_t* out, int batch, int H,
                                   int W, int C, int nheads, int shift, hipStream_t s) {
    if (C != nheads * 32) return DVID_ERR_UNSUPPORTED;
    const int nwy = (H + 11) / 12, nwx = (W + 11) / 12;
    const long nwin = (long)batch * nwy * nwx;
    if (nwin * nheads > 0x7fffffffL) return DVID_ERR_UNSUPPORTED;
    if (nwin == 0) return DVID_OK;
    // two windows per workgroup: halves the bias traffic and still leaves the deeper stages (6 windows x 32 heads per frame in the last)
    // more workgroups than four would
    hipLaunchKernelGGL(swin_window12_attn_kernel<2>, dim3((unsigned)((nwin + 1) / 2 * nheads)), dim3(576), 0, s, qkv, qkv_bias16, relbias, out,
                       H, W, C, nheads, shift, 1.0f / sqrtf(32.f), (int)nwin);
    LAUNCH_CHECK();
    return DVID_OK;
}

// =============================================================================================
// DTYPE float32: the same three attentions on fp32 storage, on the VALU (one query per lane, or four lanes per query; exact fp32
// products and softmax) -- other algorithms than the MFMA kernels above, not their templates.
// =============================================================================================
namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// attention, head dim 32: out[b][q][h*32 ..] = softmax_k(q . k / sqrt(32)) v.  One query per lane (its 32 q values and 32 output
// accumulators in registers), keys and values in chunks of 64 through LDS (every lane reads the same key: broadcast reads), the
// running maximum / sum of the streaming softmax updated once per 16 keys.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void f32_mha_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                     float* __restrict__ out, int lq, int lk, int q_ld, int kv_ld, int out_ld, long q_bs,
                                                     long kv_bs, long out_bs, float scale) {
    __shared__ float Ks[64 * 32];
    __shared__ float Vs[64 * 32];
    const int tid = threadIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int qi = blockIdx.x * 64 + tid;
    const bool live = qi < lq;
    float qv[32], acc[32];
    {
        const float* qp = q + b * q_bs + (long)(live ? qi : 0) * q_ld + head * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(qp + j * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) qv[j * 4 + e] = t[e] * scale;
        }
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) acc[e] = 0.f;
    float mx = -INFINITY, den = 0.f;
    const float* kb = k + b * kv_bs + head * 32;
    const float* vb = v + b * kv_bs + head * 32;
    for (int k0 = 0; k0 < lk; k0 += 64) {
        const int nk = lk - k0 < 64 ? lk - k0 : 64;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {          // 64 keys x 8 float4: lane -> (key = (i * 64 + tid) / 8, quarter = .. % 8)
            const int idx = i * 64 + tid, kr = idx >> 3, c4 = (idx & 7) * 4;
            float4v kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (kr < nk) {
                kk = *reinterpret_cast<const float4v*>(kb + (long)(k0 + kr) * kv_ld + c4);
                vv = *reinterpret_cast<const float4v*>(vb + (long)(k0 + kr) * kv_ld + c4);
            }
            *reinterpret_cast<float4v*>(&Ks[kr * 32 + c4]) = kk;
            *reinterpret_cast<float4v*>(&Vs[kr * 32 + c4]) = vv;
        }
        __syncthreads();
        // sub-chunks of 16 keys: scores into registers, one maximum / rescale per sub-chunk, then the weighted values
#pragma unroll 1
        for (int c0 = 0; c0 < nk; c0 += 16) {
            float sc16[16];
            float cmx = -INFINITY;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                float d = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float4v t = *reinterpret_cast<const float4v*>(&Ks[(c0 + kk) * 32 + j * 4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) d = __builtin_fmaf(qv[j * 4 + e], t[e], d);
                }
                sc16[kk] = c0 + kk < nk ? d : -INFINITY;
                cmx = fmaxf(cmx, sc16[kk]);
            }
            const float nmx = fmaxf(mx, cmx);
            const float rescale = expf(mx - nmx);          // first sub-chunk: exp(-inf) = 0 on zero accumulators
            den *= rescale;
#pragma unroll
            for (int e = 0; e < 32; ++e) acc[e] *= rescale;
            mx = nmx;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float pr = expf(sc16[kk] - mx);          // masked keys: exp(-inf) = 0
                den += pr;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float4v t = *reinterpret_cast<const float4v*>(&Vs[(c0 + kk) * 32 + j * 4]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j * 4 + e] = __builtin_fmaf(pr, t[e], acc[j * 4 + e]);
                }
            }
        }
    }
    if (live) {
        const float inv = 1.f / den;
        float* op = out + b * out_bs + (long)qi * out_ld + head * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            *reinterpret_cast<float4v*>(op + j * 4) = (float4v){acc[j * 4] * inv, acc[j * 4 + 1] * inv, acc[j * 4 + 2] * inv, acc[j * 4 + 3] * inv};
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Swin window attention (swintransformer.py:68-176, :226-254), fp32: one workgroup (one wave) per (window, head), lane = query position of
// the 7 x 7 window, keys and values through LDS.  A padded window position holds the qkv BIAS (the reference pads the normalised tokens
// with zeros before the qkv Linear); the shifted map's region mask adds -100 between positions of different regions.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void f32_swin_window_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                                  const float* __restrict__ relbias, float* __restrict__ out, int H, int W, int C,
                                                                  int nheads, int shift, float scaling, int nwin) {
    constexpr int WS = 7, NT = 49;
    __shared__ float Ks[NT * 32];
    __shared__ float Vs[NT * 32];
    __shared__ int tok[64];
    __shared__ int region[64];
    const int tid = threadIdx.x;
    const int lid = igemm_xcd_remap((int)blockIdx.x, nwin * nheads);
    int wid = lid / nheads;
    const int h = lid - wid * nheads;
    const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
    const int nwx = Wp / WS, nwy = Hp / WS;
    const int wx = wid % nwx;
    wid /= nwx;
    const int wy = wid % nwy;
    const int b = wid / nwy;
    {
        int t = -1, reg = 0;
        if (tid < NT) {
            const int py = tid / WS, px = tid - py * WS;
            const int ys = wy * WS + py, xs = wx * WS + px;          // coordinates in the shifted, padded map
            int y = ys + shift, x = xs + shift;                      // source coordinates before the roll
            if (y >= Hp) y -= Hp;
            if (x >= Wp) x -= Wp;
            if (y < H && x < W) t = (b * H + y) * W + x;
            if (shift > 0) {
                const int hr = ys < Hp - WS ? 0 : (ys < Hp - shift ? 1 : 2);
                const int wr = xs < Wp - WS ? 0 : (xs < Wp - shift ? 1 : 2);
                reg = hr * 3 + wr;
            }
        }
        tok[tid] = t;
        region[tid] = reg;
    }
    __syncthreads();
    for (int idx = tid; idx < NT * 8; idx += 64) {
        const int key = idx >> 3, c4 = (idx & 7) * 4;
        const int t = tok[key];
        const float* src = t >= 0 ? qkv + (long)t * 3 * C : qkv_bias;
        *reinterpret_cast<float4v*>(&Ks[key * 32 + c4]) = *reinterpret_cast<const float4v*>(src + C + h * 32 + c4);
        *reinterpret_cast<float4v*>(&Vs[key * 32 + c4]) = *reinterpret_cast<const float4v*>(src + 2 * C + h * 32 + c4);
    }
    const int qp = tid < NT ? tid : NT - 1;
    const int tq = tok[qp], qreg = region[qp];
    float qv[32];
    {
        const float* qsrc = (tq >= 0 ? qkv + (long)tq * 3 * C : qkv_bias) + h * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(qsrc + j * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) qv[j * 4 + e] = t[e] * scaling;
        }
    }
    __syncthreads();
    const float* brow = relbias + ((long)h * NT + qp) * SWIN_RELBIAS_PITCH;
    float sc[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int key = 0; key < NT; ++key) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(&Ks[key * 32 + j * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) d = __builtin_fmaf(qv[j * 4 + e], t[e], d);
        }
        d += brow[key];
        if (shift > 0 && region[key] != qreg) d += -100.0f;
        sc[key] = d;
        mx = fmaxf(mx, d);
    }
    float acc[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) acc[e] = 0.f;
    float den = 0.f;
#pragma unroll
    for (int key = 0; key < NT; ++key) {
        const float pr = expf(sc[key] - mx);
        den += pr;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(&Vs[key * 32 + j * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j * 4 + e] = __builtin_fmaf(pr, t[e], acc[j * 4 + e]);
        }
    }
    if (tid < NT && tq >= 0) {          // padded positions produce no output
        const float inv = 1.f / den;
        float* op = out + (long)tq * C + h * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            *reinterpret_cast<float4v*>(op + j * 4) = (float4v){acc[j * 4] * inv, acc[j * 4 + 1] * inv, acc[j * 4 + 2] * inv, acc[j * 4 + 3] * inv};
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same with 12 x 12 windows (144 tokens, shift 0 or 6).  One query per lane of one wave no longer covers a window, and 144 scores
// per lane would not stay in registers: a workgroup is nine waves (576 threads) for one (window, head), FOUR lanes per query, lane
// `part` of a query taking keys part, part + 4, ... (36 scores per lane).  The four partial maxima, sums and 32-float accumulators meet
// in two xor-shuffles inside the quad; lane 0 of the quad writes the row.  K and V rows have a pitch of 36 floats (2 x 20.25 KB of
// LDS): the four rows a quad reads in one ds_read_b128 start 36 banks apart, conflict-free.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(576) void f32_swin_window12_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                                     const float* __restrict__ relbias, float* __restrict__ out, int H, int W, int C,
                                                                     int nheads, int shift, float scaling, int nwin) {
    constexpr int WS = 12, NT = 144, KP = 36, NPART = 4, NS = NT / NPART;
    __shared__ __attribute__((aligned(16))) float Ks[NT * KP];
    __shared__ __attribute__((aligned(16))) float Vs[NT * KP];
    __shared__ int tok[NT];
    __shared__ int region[NT];
    const int tid = threadIdx.x;
    const int lid = igemm_xcd_remap((int)blockIdx.x, nwin * nheads);
    int wid = lid / nheads;
    const int h = lid - wid * nheads;
    const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
    const int nwx = Wp / WS, nwy = Hp / WS;
    const int wx = wid % nwx;
    wid /= nwx;
    const int wy = wid % nwy;
    const int b = wid / nwy;
    if (tid < NT) {
        const int py = tid / WS, px = tid - py * WS;
        const int ys = wy * WS + py, xs = wx * WS + px;          // coordinates in the shifted, padded map
        int y = ys + shift, x = xs + shift;                      // source coordinates before the roll
        if (y >= Hp) y -= Hp;
        if (x >= Wp) x -= Wp;
        int reg = 0;
        if (shift > 0) {
            const int hr = ys < Hp - WS ? 0 : (ys < Hp - shift ? 1 : 2);
            const int wr = xs < Wp - WS ? 0 : (xs < Wp - shift ? 1 : 2);
            reg = hr * 3 + wr;
        }
        tok[tid] = (y < H && x < W) ? (b * H + y) * W + x : -1;
        region[tid] = reg;
    }
    __syncthreads();
    for (int idx = tid; idx < NT * 8; idx += 576) {
        const int key = idx >> 3, c4 = (idx & 7) * 4;
        const int t = tok[key];
        const float* src = t >= 0 ? qkv + (long)t * 3 * C : qkv_bias;
        *reinterpret_cast<float4v*>(&Ks[key * KP + c4]) = *reinterpret_cast<const float4v*>(src + C + h * 32 + c4);
        *reinterpret_cast<float4v*>(&Vs[key * KP + c4]) = *reinterpret_cast<const float4v*>(src + 2 * C + h * 32 + c4);
    }
    const int qp = tid >> 2, part = tid & 3;                     // query position (< 144) and which quarter of its keys
    const int tq = tok[qp], qreg = region[qp];
    float qv[32];
    {
        const float* qsrc = (tq >= 0 ? qkv + (long)tq * 3 * C : qkv_bias) + h * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(qsrc + j * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) qv[j * 4 + e] = t[e] * scaling;
        }
    }
    __syncthreads();
    const float* brow = relbias + ((long)h * NT + qp) * SWIN12_RELBIAS_PITCH + part;
    float sc[NS];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int key = i * NPART + part;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(&Ks[key * KP + j * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) d = __builtin_fmaf(qv[j * 4 + e], t[e], d);
        }
        d += brow[i * NPART];
        if (shift > 0 && region[key] != qreg) d += -100.0f;
        sc[i] = d;
        mx = fmaxf(mx, d);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float acc[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) acc[e] = 0.f;
    float den = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int key = i * NPART + part;
        const float pr = expf(sc[i] - mx);
        den += pr;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4v t = *reinterpret_cast<const float4v*>(&Vs[key * KP + j * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j * 4 + e] = __builtin_fmaf(pr, t[e], acc[j * 4 + e]);
        }
    }
    den += __shfl_xor(den, 1, 64);
    den += __shfl_xor(den, 2, 64);
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        acc[e] += __shfl_xor(acc[e], 1, 64);
        acc[e] += __shfl_xor(acc[e], 2, 64);
    }
    if (part == 0 && tq >= 0) {         // padded positions produce no output
        const float inv = 1.f / den;
        float* op = out + (long)tq * C + h * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            *reinterpret_cast<float4v*>(op + j * 4) = (float4v){acc[j * 4] * inv, acc[j * 4 + 1] * inv, acc[j * 4 + 2] * inv, acc[j * 4 + 3] * inv};
    }
}

}  // namespace

int dvid_f32_mha_launch(const float* q, const float* k, const float* v, float* out, int batch, int lq, int lk, int nheads, int q_ld, int kv_ld,
                        int out_ld, long q_bs, long kv_bs, long out_bs, hipStream_t s) {
    if (batch <= 0 || lq <= 0) return DVID_OK;
    if (lk <= 0 || nheads <= 0 || (q_ld | kv_ld | out_ld) % 4) return DVID_ERR_ARG;
    hipLaunchKernelGGL(f32_mha_kernel, dim3(ceil_div(lq, 64), nheads, batch), dim3(64), 0, s, q, k, v, out, lq, lk, q_ld, kv_ld, out_ld, q_bs, kv_bs,
                       out_bs, 0.17677669529663688110f);          // 1 / sqrt(32)
    LAUNCH_CHECK();
    return DVID_OK;
}

int dvid_f32_swin_window_attn_launch(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                                     int nheads, int shift, hipStream_t s) {
    if (C != nheads * 32) return DVID_ERR_UNSUPPORTED;
    const long nwin = (long)batch * ((H + 6) / 7) * ((W + 6) / 7);
    if (nwin * nheads > 0x7fffffffL) return DVID_ERR_UNSUPPORTED;
    if (nwin == 0) return DVID_OK;
    hipLaunchKernelGGL(f32_swin_window_attn_kernel, dim3((unsigned)(nwin * nheads)), dim3(64), 0, s, qkv, qkv_bias, relbias, out, H, W, C, nheads, shift,
                       0.17677669529663688110f, (int)nwin);
    LAUNCH_CHECK();
    return DVID_OK;
}

int dvid_f32_swin_window12_attn_launch(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                                       int nheads, int shift, hipStream_t s) {
    if (C != nheads * 32) return DVID_ERR_UNSUPPORTED;
    const long nwin = (long)batch * ((H + 11) / 12) * ((W + 11) / 12);
    if (nwin * nheads > 0x7fffffffL) return DVID_ERR_UNSUPPORTED;
    if (nwin == 0) return DVID_OK;
    hipLaunchKernelGGL(f32_swin_window12_attn_kernel, dim3((unsigned)(nwin * nheads)), dim3(576), 0, s, qkv, qkv_bias, relbias, out, H, W, C, nheads,
                       shift, 0.17677669529663688110f, (int)nwin);
    LAUNCH_CHECK();
    return DVID_OK;
}
