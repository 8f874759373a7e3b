// The device half of the split JPEG decode (include/dvid_hip.h: dvid_jpeg_reconstruct_u8): what libjpeg does behind its Huffman decoder,
// bit for bit -- dequantisation, the ISLOW 8x8 inverse DCT (jidctint: CONST_BITS 13, PASS1_BITS 2), "fancy" triangle upsampling of 2x1 /
// 2x2 chroma (jdsample: h2v1 / h2v2, plain replication when the chroma row has at most two samples) and the 16-bit fixed-point
// YCbCr -> RGB of jdcolor.  Pure int32 arithmetic, so equal to Pillow's decode, not close.  n frames of different sizes and samplings
// per call, two launches however many: one plan row per frame (blockIdx.y / .z picks it), the rows validated on the host.
//
// Launch 1, jpeg_idct_kernel: 8 lanes per 8x8 block, 32 blocks per workgroup.  Lane j loads row j of the block's int16 coefficients and of
// its quantisation table (16 bytes each, so a wave reads 1 KiB of contiguous coefficients per instruction), multiplies, and parks the
// products in LDS; pass 1 takes column j, pass 2 row j (the rounding between the passes is libjpeg's, which fixes this order), and the
// eight samples of a row leave as one 8-byte store into the component's uint8 plane.  A block's LDS tile is 72 words, not 64: the column
// accesses of the 4 blocks in a 32-lane group then fall on 32 different banks.
// Launch 2, jpeg_colour_kernel: one thread per output pixel: the luma sample, the two upsampled chroma samples (up to four plane reads
// each, neighbours served by the cache), colour, three bytes out.  The planes cost 1.5 bytes per pixel of traffic beside the frame's 3.
// No address depends on a coefficient: only on the plan.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kPlanCols = 10;          // DVID_JPEG_PLAN_COLS
constexpr int kTile = 72;              // LDS words per block: 64 + 8 of padding

struct Geom {
    int w, h, nc, hs, vs, mw, mh;
    __device__ __forceinline__ explicit Geom(const long long* d) {
        w = (int)d[0], h = (int)d[1], nc = (int)d[2], hs = (int)d[3], vs = (int)d[4];
        mw = (w + 8 * hs - 1) / (8 * hs), mh = (h + 8 * vs - 1) / (8 * vs);
    }
};

// one 1-D ISLOW pass over eight values; wrapping (unsigned) arithmetic, so corrupt coefficients cannot overflow a signed int
template <int SHIFT>
__device__ __forceinline__ void idct8(const int* in, int* out) {
    typedef unsigned int u32;
    const u32 i0 = in[0], i1 = in[1], i2 = in[2], i3 = in[3], i4 = in[4], i5 = in[5], i6 = in[6], i7 = in[7];
    u32 z1 = (i2 + i6) * 4433u;
    const u32 t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const u32 t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const u32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u32 a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    u32 z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u32 z5 = (z3 + z4) * 9633u;
    a0 *= 2446u, a1 *= 16819u, a2 *= 25172u, a3 *= 12299u;
    z1 *= (u32)-7373, z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5, z4 = z4 * (u32)-3196 + z5;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    constexpr u32 half = 1u << (SHIFT - 1);
    out[0] = (int)(t10 + a3 + half) >> SHIFT;
    out[7] = (int)(t10 - a3 + half) >> SHIFT;
    out[1] = (int)(t11 + a2 + half) >> SHIFT;
    out[6] = (int)(t11 - a2 + half) >> SHIFT;
    out[2] = (int)(t12 + a1 + half) >> SHIFT;
    out[5] = (int)(t12 - a1 + half) >> SHIFT;
    out[3] = (int)(t13 + a0 + half) >> SHIFT;
    out[4] = (int)(t13 - a0 + half) >> SHIFT;
}

// libjpeg's range_limit table: the low 10 bits as a signed value, + 128, clamped
__device__ __forceinline__ unsigned int sample(int x) {
    const int v = (((x & 1023) ^ 512) - 512) + 128;
    return (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

typedef short short8v __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8v __attribute__((ext_vector_type(8)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, const unsigned short* __restrict__ quant,
                                                         const long long* __restrict__ plan, unsigned char* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) int ws[32 * kTile];
    const long long* d = plan + (long)blockIdx.y * kPlanCols;
    const Geom g(d);
    const int nb0 = g.mw * g.hs * g.mh * g.vs, nb1 = g.nc == 3 ? g.mw * g.mh : 0;
    const int first = blockIdx.x * 32;
    if (first >= nb0 + 2 * nb1) return;          // the whole workgroup leaves: frames smaller than the largest of the call
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int b = first + lb;
    const bool live = b < nb0 + 2 * nb1;
    const int c = b < nb0 ? 0 : (b < nb0 + nb1 ? 1 : 2);
    const int k = b - (c == 0 ? 0 : (c == 1 ? nb0 : nb0 + nb1));          // the block inside its component
    const int bw = c == 0 ? g.mw * g.hs : g.mw;
    const int base = (int)d[5 + c];
    int* tile = ws + lb * kTile;
    int v[8], o[8];
    if (live) {
        const short8v cf = *reinterpret_cast<const short8v*>(coef + base + k * 64 + j * 8);
        const ushort8v q = *reinterpret_cast<const ushort8v*>(quant + (int)d[8] + c * 64 + j * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[j * 8 + i] = (int)cf[i] * (int)q[i];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = tile[r * 8 + j];
        idct8<11>(v, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) tile[r * 8 + j] = o[r];          // column j is this lane's alone
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[j * 8 + i];
        idct8<18>(v, o);
        uint2v px;
        px[0] = sample(o[0]) | (sample(o[1]) << 8) | (sample(o[2]) << 16) | (sample(o[3]) << 24);
        px[1] = sample(o[4]) | (sample(o[5]) << 8) | (sample(o[6]) << 16) | (sample(o[7]) << 24);
        const int by = k / bw, bx = k - by * bw;
        *reinterpret_cast<uint2v*>(planes + base + ((by * 8 + j) * bw + bx) * 8) = px;
    }
}

// the chroma sample at output pixel (x, y) of a plane [..][pitch] whose image part is dh x dw
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
    if (hs == 1) return p[y * pitch + x];
    const int i = x >> 1;
    if (vs == 1) {          // h2v1
        const unsigned char* row = p + y * pitch;
        const int c = row[i];
        if (dw <= 2) return c;
        if (x & 1) return i == dw - 1 ? c : (3 * c + row[i + 1] + 2) >> 2;
        return i == 0 ? c : (3 * c + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;          // h2v2
    const unsigned char* row0 = p + r * pitch;
    if (dw <= 2) return row0[i];
    const int rn = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    const unsigned char* row1 = p + rn * pitch;
    const int cs = 3 * row0[i] + row1[i];
    if (x & 1) {
        const int nb = i == dw - 1 ? cs : 3 * row0[i + 1] + row1[i + 1];
        return (3 * cs + nb + 7) >> 4;
    }
    const int nb = i == 0 ? cs : 3 * row0[i - 1] + row1[i - 1];
    return (3 * cs + nb + 8) >> 4;
}

__device__ __forceinline__ unsigned char clamp8(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const unsigned char* __restrict__ planes, const long long* __restrict__ plan,
                                                           unsigned char* __restrict__ out) {
    const long long* d = plan + (long)blockIdx.z * kPlanCols;
    const Geom g(d);
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= g.w || y >= g.h) return;
    const int yy = planes[(int)d[5] + y * (g.mw * g.hs * 8) + x];
    int r = yy, gr = yy, bl = yy;
    if (g.nc == 3) {
        const int pitch = g.mw * 8, dw = (g.w + g.hs - 1) / g.hs, dh = (g.h + g.vs - 1) / g.vs;
        const int cb = chroma_at(planes + (int)d[6], pitch, dw, dh, g.hs, g.vs, x, y) - 128;
        const int cr = chroma_at(planes + (int)d[7], pitch, dw, dh, g.hs, g.vs, x, y) - 128;
        r = yy + ((91881 * cr + 32768) >> 16);
        gr = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        bl = yy + ((116130 * cb + 32768) >> 16);
    }
    unsigned char* o = out + d[9] + ((long)y * g.w + x) * 3;
    o[0] = clamp8(r);
    o[1] = clamp8(gr);
    o[2] = clamp8(bl);
}

}  // namespace

int dvid_jpeg_reconstruct_launch(const short* coef, const unsigned short* quant, const long long* plan, int n, int max_blocks, int max_w, int max_h,
                                 unsigned char* planes, unsigned char* out, hipStream_t s) {
    if (n <= 0 || n > 65535 || max_blocks <= 0 || max_w <= 0 || max_h <= 0 || max_h > 65535) return DVID_ERR_ARG;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(ceil_div(max_blocks, 32), n), dim3(256), 0, s, coef, quant, plan, planes);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(ceil_div(max_w, 256), max_h, n), dim3(256), 0, s, planes, plan, out);
    LAUNCH_CHECK();
    return DVID_OK;
}
