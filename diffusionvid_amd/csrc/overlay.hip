// The demo surface: detections painted onto uint8 RGB frames where they lie (the reference's demo/predictor.py: select_top_predictions,
// compute_colors_for_labels, overlay_boxes, overlay_class_names).  What is drawn -- which rows, in which order, where, in which colour, with
// which text -- is the reference's; the rasterisation (rings of whole pixels, a bitmap-font plate) is this project's.
//
// in   frames: device table of n pointers to uint8 [h_f][w_f][3], row pitch w_f * 3 bytes, no alignment; sizes int32 [n][2] = (h, w)
//      dets fp32 [n][cap][6] = x1, y1, x2, y2, score, label in the model's frame (engine.inference.pack_predictions), counts int32 [n];
//      ratios fp32 [n][2] = (rw, rh), native / model size; names uint8 [num_classes + 1][24]; atlas uint8 [95][gh][gw] of 0 / 1
// Two launches:
//   overlay_prepare_kernel  one workgroup per frame: the rows that pass (finite corners and score, score > threshold in fp32) get a key
//                           (score as ordered bits, row) in LDS, a bitonic sort puts them in draw order (ascending score, then row), the
//                           last 256 are kept; one thread per kept row then forms its corners (one fp32 multiply, truncation, int32 clamp),
//                           its colour (64-bit product mod 255), its text (name + ": " + the score correctly rounded to hundredths, in
//                           integers) and writes a 96-byte entry of the frame's draw list.
//   overlay_draw_kernel     one workgroup per 64 x 16 pixel tile and frame: the draw list is culled against the tile into LDS, in order
//                           (ballots); a tile nothing touches ends there, so the cost follows the drawn area.  Otherwise every thread
//                           resolves its four pixels by the layer rule -- the latest plate that covers it, else the latest ring -- and
//                           stores only those.  A gather per pixel: overlapping detections cannot race, and no pixel is read.
#include <climits>

#include "common.h"
#include "kernels.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxDrawn = 256;                  // DVID_OVERLAY_MAX_DRAWN
constexpr int kNameMax = 24;                    // DVID_OVERLAY_NAME_MAX
constexpr int kMaxRows = DVID_NMS_MAX_CANDIDATES;
constexpr int kEntryInts = 24;                  // one draw-list entry, 96 bytes
constexpr int kHeaderInts = 16;                 // per frame: the number of entries, padded to 64 bytes
constexpr int kFrameInts = kHeaderInts + kMaxDrawn * kEntryInts;
constexpr int kTileW = 64, kTileH = 16;         // 256 threads x 4 pixels of one row
constexpr int kFar = 1 << 30;                   // beyond any frame: rectangle bounds are clamped to +-kFar, which no pixel of a frame meets
constexpr int kTextInts = 8;                    // up to 32 text bytes: 24 of the name, ": ", "-d.dd"

// entry: 0..3 the ring's outer rectangle, 4..7 its inner one (x1, y1, x2, y2, inclusive; x2 < x1: nothing), 8..11 the plate, 12 the colour
// (r | g << 8 | b << 16), 13 the number of characters, 14 live (0: a row the truncation emptied), 15 spare, 16..23 the text
enum { E_OUT = 0, E_IN = 4, E_PLATE = 8, E_COLOUR = 12, E_NCHAR = 13, E_LIVE = 14, E_TEXT = 16 };

__device__ __forceinline__ int trunc_i32(float v) {          // toward zero, clamped to the int32 range; v is finite or NaN (-> 0)
    if (!(v == v)) return 0;
    if (v >= 2147483648.f) return INT_MAX;
    if (v <= -2147483648.f) return INT_MIN;
    return (int)v;
}
__device__ __forceinline__ int clamp_far(long long v) { return v < -kFar ? -kFar : (v > kFar ? kFar : (int)v); }
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// |score| correctly rounded to hundredths, ties to even, clamped to 999: the 24-bit significand times 100, shifted by the exponent
__device__ __forceinline__ int hundredths(float score) {
    const unsigned bits = __float_as_uint(score) & 0x7fffffffu;
    int e = (int)(bits >> 23);
    unsigned m = bits & 0x7fffffu;
    if (e == 0) e = 1; else m |= 0x800000u;          // value = m * 2^(e - 150)
    const u64 v = (u64)m * 100u;                     // < 2^31
    const int shift = 150 - e;
    if (shift <= 0) return 999;
    if (shift >= 40) return 0;                       // v * 2^-40 < 1/2
    u64 q = v >> shift;
    const u64 rem = v & (((u64)1 << shift) - 1), half = (u64)1 << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return q > 999 ? 999 : (int)q;
}

__global__ __launch_bounds__(256) void overlay_prepare_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int cap,
                                                              const float* __restrict__ ratios, const unsigned char* __restrict__ names,
                                                              int num_classes, int gh, int gw, float threshold, int thickness, int scale,
                                                              int* __restrict__ lists) {
    __shared__ u64 keys[kMaxRows];
    __shared__ int s_m;
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* d = dets + (size_t)f * cap * 6;
    int cnt = counts[f];
    cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
    if (tid == 0) s_m = 0;
    __syncthreads();
    for (int r = tid; r < cnt; r += 256) {
        const float* row = d + (size_t)r * 6;
        const float sc = row[4];
        if (finite_f(row[0]) && finite_f(row[1]) && finite_f(row[2]) && finite_f(row[3]) && finite_f(sc) && sc > threshold) {
            unsigned u = sc == 0.f ? 0u : __float_as_uint(sc);          // -0 and +0 are one score
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // unsigned order = numeric order
            keys[atomicAdd(&s_m, 1)] = ((u64)u << 32) | (unsigned)r;   // distinct keys: the sort decides the order, not the arrival
        }
    }
    __syncthreads();
    const int m = s_m;
    int P = 1;
    while (P < m) P <<= 1;
    for (int i = m + tid; i < P; i += 256) keys[i] = ~(u64)0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int o = i ^ j;
                if (o > i) {
                    const u64 a = keys[i], b = keys[o];
                    if (((i & k) == 0) == (a > b)) keys[i] = b, keys[o] = a;
                }
            }
            __syncthreads();
        }
    const int nd = m < kMaxDrawn ? m : kMaxDrawn;
    int* list = lists + (size_t)f * kFrameInts;
    if (tid == 0) list[0] = nd;
    if (tid >= nd) return;
    const int r = (int)(unsigned)(keys[m - nd + tid] & 0xffffffffu);
    const float* row = d + (size_t)r * 6;
    const float rw = ratios[2 * f], rh = ratios[2 * f + 1];
    const int x1 = trunc_i32(__fmul_rn(row[0], rw)), y1 = trunc_i32(__fmul_rn(row[1], rh));
    const int x2 = trunc_i32(__fmul_rn(row[2], rw)), y2 = trunc_i32(__fmul_rn(row[3], rh));
    int* e = list + kHeaderInts + tid * kEntryInts;
    if (x2 < x1 || y2 < y1) {
        e[E_LIVE] = 0;
        return;
    }
    const int o = thickness / 2, in = thickness - o;
    e[E_OUT + 0] = clamp_far((long long)x1 - o);
    e[E_OUT + 1] = clamp_far((long long)y1 - o);
    e[E_OUT + 2] = clamp_far((long long)x2 + o);
    e[E_OUT + 3] = clamp_far((long long)y2 + o);
    const long long ix1 = (long long)x1 + in, iy1 = (long long)y1 + in, ix2 = (long long)x2 - in, iy2 = (long long)y2 - in;
    const bool hollow = ix1 <= ix2 && iy1 <= iy2;
    e[E_IN + 0] = hollow ? clamp_far(ix1) : 1;
    e[E_IN + 1] = hollow ? clamp_far(iy1) : 1;
    e[E_IN + 2] = hollow ? clamp_far(ix2) : 0;
    e[E_IN + 3] = hollow ? clamp_far(iy2) : 0;
    // colour: (L * palette) % 255 with the sign of Python's %, the reference's BGR triple shown as it looks: B = c0, G = c1, R = c2
    const long long L = trunc_i32(row[5]);
    const long long pal[3] = {(1ll << 25) - 1, (1ll << 15) - 1, (1ll << 21) - 1};
    unsigned c[3];
    for (int k = 0; k < 3; ++k) c[k] = (unsigned)(((L * pal[k]) % 255 + 255) % 255);
    e[E_COLOUR] = (int)(c[2] | (c[1] << 8) | (c[0] << 16));
    // text
    unsigned char text[kTextInts * 4];
    int n = 0;
    if (L >= 0 && L <= num_classes) {
        const unsigned char* nm = names + (size_t)L * kNameMax;
        while (n < kNameMax && nm[n]) text[n] = nm[n], ++n;
    }
    if (n) text[n++] = ':', text[n++] = ' ';
    const float sc = row[4];
    const int q = hundredths(sc);
    if (__float_as_uint(sc) & 0x80000000u) text[n++] = '-';
    text[n++] = (unsigned char)('0' + q / 100);
    text[n++] = '.';
    text[n++] = (unsigned char)('0' + (q / 10) % 10);
    text[n++] = (unsigned char)('0' + q % 10);
    for (int k = n; k < kTextInts * 4; ++k) text[k] = 0;
    for (int k = 0; k < kTextInts; ++k)
        e[E_TEXT + k] = (int)((unsigned)text[4 * k] | ((unsigned)text[4 * k + 1] << 8) | ((unsigned)text[4 * k + 2] << 16) | ((unsigned)text[4 * k + 3] << 24));
    e[E_NCHAR] = n;
    const int pad = scale;
    e[E_PLATE + 0] = clamp_far(x1);
    e[E_PLATE + 1] = clamp_far(y1);
    e[E_PLATE + 2] = clamp_far((long long)x1 + (long long)n * gw * scale + 2 * pad - 1);
    e[E_PLATE + 3] = clamp_far((long long)y1 + (long long)gh * scale + 2 * pad - 1);
    e[E_LIVE] = 1;
    e[15] = 0;
}

__device__ __forceinline__ bool inside(const int* r, int x, int y) { return x >= r[0] && x <= r[2] && y >= r[1] && y <= r[3]; }

__global__ __launch_bounds__(256) void overlay_draw_kernel(unsigned char* const* __restrict__ frames, const int* __restrict__ sizes,
                                                           const int* __restrict__ lists, const unsigned char* __restrict__ atlas, int gh,
                                                           int gw, int scale) {
    __shared__ int ent[kMaxDrawn * kEntryInts];
    __shared__ int wave_kept[4];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int h = sizes[2 * f], w = sizes[2 * f + 1];
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    if (tx0 >= w || ty0 >= h) return;                                   // the grid covers the largest frame of the launch
    const int tx1 = min(tx0 + kTileW, w) - 1, ty1 = min(ty0 + kTileH, h) - 1;
    const int* list = lists + (size_t)f * kFrameInts;
    int nd = list[0];
    nd = nd < 0 ? 0 : (nd > kMaxDrawn ? kMaxDrawn : nd);
    // cull: entry `tid` against the tile, its extent the outer rectangle united with the plate; kept entries keep their order
    const int* mine = list + kHeaderInts + tid * kEntryInts;
    bool keep = false;
    if (tid < nd && mine[E_LIVE]) {
        const int ex1 = min(mine[E_OUT + 0], mine[E_PLATE + 0]), ey1 = min(mine[E_OUT + 1], mine[E_PLATE + 1]);
        const int ex2 = max(mine[E_OUT + 2], mine[E_PLATE + 2]), ey2 = max(mine[E_OUT + 3], mine[E_PLATE + 3]);
        keep = ex1 <= tx1 && ex2 >= tx0 && ey1 <= ty1 && ey2 >= ty0;
    }
    const u64 mask = __ballot(keep);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wave_kept[wv] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < wv) base += wave_kept[k];
        total += wave_kept[k];
    }
    if (total == 0) return;
    if (keep) {
        int* dst = ent + (base + __popcll(mask & (((u64)1 << lane) - 1))) * kEntryInts;
        for (int k = 0; k < kEntryInts; ++k) dst[k] = mine[k];
    }
    __syncthreads();
    // resolve: four pixels of one row per thread
    const int y = ty0 + (tid >> 4), x0 = tx0 + (tid & 15) * 4;
    if (y >= h || x0 >= w) return;
    const int cell = gw * scale, pad = scale;
    unsigned colour[4];
    unsigned owned = 0;
    for (int p = 0; p < 4; ++p) {
        const int x = x0 + p;
        if (x >= w) break;
        int ring = -1, plate = -1;
        for (int k = total - 1; k >= 0; --k) {
            const int* e = ent + k * kEntryInts;
            if (inside(e + E_PLATE, x, y)) {
                plate = k;
                break;
            }
            if (ring < 0 && inside(e + E_OUT, x, y) && !inside(e + E_IN, x, y)) ring = k;
        }
        if (plate >= 0) {
            const int* e = ent + plate * kEntryInts;
            unsigned c = (unsigned)e[E_COLOUR];
            const int tx = x - e[E_PLATE + 0] - pad, ty = y - e[E_PLATE + 1] - pad;
            if (tx >= 0 && ty >= 0 && ty < gh * scale && tx < e[E_NCHAR] * cell) {
                const int k = tx / cell;
                unsigned ch = (((unsigned)e[E_TEXT + (k >> 2)] >> ((k & 3) * 8)) & 0xffu) - 32u;
                if (ch >= 95u) ch = '?' - 32;                           // the host keeps names inside 32 .. 126; never index outside the atlas
                if (atlas[((size_t)ch * gh + ty / scale) * gw + (tx - k * cell) / scale]) c = 0xffffffu;
            }
            colour[p] = c;
            owned |= 1u << p;
        } else if (ring >= 0) {
            colour[p] = (unsigned)ent[ring * kEntryInts + E_COLOUR];
            owned |= 1u << p;
        }
    }
    if (!owned) return;
    unsigned char* px = frames[f] + ((size_t)y * w + x0) * 3;
    if (owned == 0xfu && (reinterpret_cast<uintptr_t>(px) & 3) == 0) {  // 12 bytes of one owner set: three dwords where the row lets them
        unsigned* q = reinterpret_cast<unsigned*>(px);
        q[0] = (colour[0] & 0xffffffu) | (colour[1] << 24);
        q[1] = ((colour[1] >> 8) & 0xffffu) | (colour[2] << 16);
        q[2] = ((colour[2] >> 16) & 0xffu) | (colour[3] << 8);
        return;
    }
    for (int p = 0; p < 4; ++p)
        if (owned & (1u << p)) {
            px[3 * p + 0] = (unsigned char)(colour[p] & 0xff);
            px[3 * p + 1] = (unsigned char)((colour[p] >> 8) & 0xff);
            px[3 * p + 2] = (unsigned char)((colour[p] >> 16) & 0xff);
        }
}

}  // namespace

long long dvid_overlay_scratch_bytes_for(int n) { return (long long)n * kFrameInts * (long long)sizeof(int); }

void dvid_overlay_tile_size(int* tw, int* th) {
    *tw = kTileW;
    *th = kTileH;
}

int dvid_overlay_launch(unsigned char* const* frames, const int* sizes, int n, int max_h, int max_w, const float* dets, const int* counts, int cap,
                        const float* ratios, const unsigned char* names, int num_classes, const unsigned char* atlas, int gh, int gw,
                        float threshold, int thickness, int text_scale, int* lists, hipStream_t s) {
    if (n < 1 || n > 65535 || cap < 1 || cap > kMaxRows || max_h < 1 || max_w < 1 || max_h > 65535 || max_w > 65535) return DVID_ERR_ARG;
    hipLaunchKernelGGL(overlay_prepare_kernel, dim3(n), dim3(256), 0, s, dets, counts, cap, ratios, names, num_classes, gh, gw, threshold,
                       thickness, text_scale, lists);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(overlay_draw_kernel, dim3(ceil_div(max_w, kTileW), ceil_div(max_h, kTileH), n), dim3(256), 0, s, frames, sizes, lists, atlas,
                       gh, gw, text_scale);
    LAUNCH_CHECK();
    return DVID_OK;
}
