// Detection post-processing on device (diffusion_det.py:754-839 `inference`, :607-627 ensemble):
//
//   kernel A  topk_candidates: per (frame, candidate set) sigmoid over [M, C] logits and the
//             top-M of the M*C scores, ordered by (score desc, flat index asc)
//   kernel B  nms_frame: per frame, merge the sets (stable: score desc, position asc), class-aware
//             NMS with torchvision's coordinate trick (boxes + label * (max_coord + 1), IoU
//             without +1, `>` threshold, fp32, same operation order as torchvision's kernels),
//             clip_to_image (bounding_box.py:214-224), compacted outputs + count.
//
//   kernels C  nms_tiled_{sort,mask,sweep}: kernel B for the frames whose candidates do not fit its LDS (more than 997), up to
//             DVID_NMS_MAX_CANDIDATES = 4096: the suppression bit matrix lives in global scratch and is built by many workgroups per
//             frame.  Same inputs, outputs and bits as kernel B.
//
// Integer work (ordering, suppression) is exact given the scores/boxes; no D2H copies.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace {

typedef unsigned long long u64;

// ascending bitonic sort of n (power of two) keys in LDS by all threads of the block
__device__ void bitonic_sort_u64(u64* keys, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // index with bit j clear
                const int p = i | j;
                const bool up = (i & k) == 0;
                const u64 a = keys[i], b = keys[p];
                if ((a > b) == up) {
                    keys[i] = b;
                    keys[p] = a;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ unsigned f2u(float f) { return __float_as_uint(f); }

// grid (frames, sets); logits/boxes for set s of frame f at ((s * n_img + f) * m) rows.
__global__ __launch_bounds__(1024) void topk_candidates_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                                int n_img, int m, int c, int npad, float* __restrict__ cand_boxes,
                                                                float* __restrict__ cand_scores, int* __restrict__ cand_labels) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    const int f = blockIdx.x, set = blockIdx.y;
    const int nsets = gridDim.y;
    const long base = ((long)set * n_img + f) * m;
    const int total = m * c;
    for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        u64 key = ~0ull;
        if (i < total) {
            const float x = logits[base * c + i];
            const float sc = 1.f / (1.f + expf(-x));                 // torch.sigmoid
            key = ((u64)(~f2u(sc)) << 32) | (unsigned)i;             // score desc, index asc (scores > 0)
        }
        keys[i] = key;
    }
    __syncthreads();
    bitonic_sort_u64(keys, npad);
    const long obase = ((long)f * nsets + set) * m;
    for (int r = threadIdx.x; r < m; r += blockDim.x) {
        const u64 key = keys[r];
        const unsigned idx = (unsigned)key;
        const float sc = __uint_as_float(~(unsigned)(key >> 32));
        cand_scores[obase + r] = sc;
        cand_labels[obase + r] = (int)(idx % c) + 1;
        const float4v b = *reinterpret_cast<const float4v*>(boxes + (base + idx / c) * 4);
        *reinterpret_cast<float4v*>(cand_boxes + (obase + r) * 4) = b;
    }
}

// The same selection without sorting all M*C keys: a three-pass radix select (11 + 11 + 10 bits, LDS histograms) finds the M-th
// smallest 32-bit key (= bit pattern of the M-th largest score), the keys below it and -- in index order, by a block-wide prefix sum
// over per-thread contiguous ranges -- as many keys equal to it as complete the M are compacted, and only those M keys are sorted
// (512 instead of 16384 keys for 300 x 30: 45 compare-exchange rounds instead of 105 over 32x fewer keys).  Exactly the set and
// order of the full sort: (score desc, flat index asc).  One workgroup of 1024 threads per (frame, set).
__global__ __launch_bounds__(1024) void topk_select_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, int n_img,
                                                            int m, int c, int mpad, float* __restrict__ cand_boxes,
                                                            float* __restrict__ cand_scores, int* __restrict__ cand_labels) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int total = m * c;
    u64* sel = reinterpret_cast<u64*>(smem);                              // [mpad] selected keys
    unsigned* k32 = reinterpret_cast<unsigned*>(sel + mpad);             // [total] ~bits(score)
    int* hist = reinterpret_cast<int*>(k32 + total);                     // [2048]
    __shared__ int s_bin, s_need, s_cnt, s_wave[16];
    const int f = blockIdx.x, set = blockIdx.y, nsets = gridDim.y, tid = threadIdx.x;
    const long base = ((long)set * n_img + f) * m;
    for (int i = tid; i < total; i += 1024) {
        const float x = logits[base * c + i];
        k32[i] = ~f2u(1.f / (1.f + expf(-x)));                           // torch.sigmoid; smaller key = larger score (scores > 0)
    }
    for (int i = tid; i < mpad; i += 1024) sel[i] = ~0ull;
    if (tid == 0) {
        s_need = m;
        s_cnt = 0;
    }
    unsigned prefix = 0;
    int decided = 0;                                                     // leading bits of the threshold known so far
    const int bits_of[3] = {11, 11, 10};
    for (int pass = 0; pass < 3; ++pass) {
        const int bits = bits_of[pass], shift = 32 - decided - bits;
        for (int i = tid; i < 2048; i += 1024) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < total; i += 1024) {
            const unsigned k = k32[i];
            if (decided == 0 || (k >> (32 - decided)) == prefix) atomicAdd(&hist[(k >> shift) & ((1u << bits) - 1)], 1);
        }
        __syncthreads();
        if (tid < 64) {                                                  // first wave: the bin that holds the s_need-th key
            const int nb = 1 << bits, per = nb / 64;
            int sum = 0;
            for (int b = 0; b < per; ++b) sum += hist[tid * per + b];
            int inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(inc, o, 64);
                if (tid >= o) inc += v;
            }
            const int need = s_need, exc = inc - sum;
            if (exc < need && need <= inc) {
                int run = exc;
                for (int b = 0; b < per; ++b) {
                    const int h = hist[tid * per + b];
                    if (need <= run + h) {
                        s_bin = tid * per + b;
                        s_need = need - run;
                        break;
                    }
                    run += h;
                }
            }
        }
        __syncthreads();
        prefix = (prefix << bits) | (unsigned)s_bin;
        decided += bits;
        __syncthreads();
    }
    const unsigned thr = prefix;                                         // the m-th smallest key; s_need of the keys equal to it belong to the top-m
    const int need_eq = s_need;
    // keys below the threshold: any order (they are sorted afterwards)
    for (int i = tid; i < total; i += 1024) {
        const unsigned k = k32[i];
        if (k < thr) sel[atomicAdd(&s_cnt, 1)] = ((u64)k << 32) | (unsigned)i;
    }
    // keys equal to it: the first need_eq in index order (per-thread contiguous ranges + block-wide exclusive prefix sum)
    const int per = (total + 1023) / 1024, i0 = tid * per, i1 = min(total, i0 + per);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += k32[i] == thr;
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += v;
    }
    if ((tid & 63) == 63) s_wave[tid >> 6] = inc;
    __syncthreads();
    int rank = inc - mine;
    for (int w = 0; w < (tid >> 6); ++w) rank += s_wave[w];
    const int below = s_cnt;                                             // final: every k < thr has been counted before the barrier above
    for (int i = i0; i < i1; ++i)
        if (k32[i] == thr) {
            if (rank < need_eq) sel[below + rank] = ((u64)thr << 32) | (unsigned)i;
            ++rank;
        }
    __syncthreads();
    bitonic_sort_u64(sel, mpad);
    const long obase = ((long)f * nsets + set) * m;
    for (int r = tid; r < m; r += 1024) {
        const u64 key = sel[r];
        const unsigned idx = (unsigned)key;
        cand_scores[obase + r] = __uint_as_float(~(unsigned)(key >> 32));
        cand_labels[obase + r] = (int)(idx % c) + 1;
        *reinterpret_cast<float4v*>(cand_boxes + (obase + r) * 4) = *reinterpret_cast<const float4v*>(boxes + (base + idx / c) * 4);
    }
}

// The same selection for the shapes whose M*C keys no LDS holds (wide class vocabularies: 300 x 1203 = 1.4 MB of keys per frame): the
// keys are never stored.  Every pass recomputes ~bits(sigmoid(x)) from the logits in global memory -- the expression of the two kernels
// above, so the same bits -- with lanes striding the flat index (coalesced; after the first pass the frame's logits come from L2).  LDS
// holds sel[mpad], the histogram and the scan scratch: 8.2 KiB + 8 mpad bytes.
//   passes 1-3  radix histograms over all keys (11 / 11 / 10 bits) -> thr, the M-th smallest key, and need_eq, how many keys equal to it
//               belong to the top M
//   pass 4      wave w walks its own contiguous range [w per_w, (w + 1) per_w): keys below thr go to sel in any order (sorted afterwards),
//               keys equal to thr are counted per wave
//   pass 5      the first need_eq keys equal to thr in flat-index order: rank = equal keys of the waves before + of this wave's earlier
//               iterations + of the lower lanes of this iteration (a ballot); a wave stops once its rank reaches need_eq, so without ties
//               beyond the M-th key only the waves up to the last taken key read anything
// Exactly the set and order of the full sort: (score desc, flat index asc).  One workgroup of 1024 threads per (frame, set).
__global__ __launch_bounds__(1024) void topk_stream_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, int n_img,
                                                            int m, int c, int mpad, float* __restrict__ cand_boxes,
                                                            float* __restrict__ cand_scores, int* __restrict__ cand_labels) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* sel = reinterpret_cast<u64*>(smem);                              // [mpad] selected keys
    __shared__ int hist[2048];
    __shared__ int s_bin, s_need, s_cnt, s_wave[16];
    const int total = m * c;
    const int f = blockIdx.x, set = blockIdx.y, nsets = gridDim.y, tid = threadIdx.x;
    const long base = ((long)set * n_img + f) * m;
    const float* lg = logits + base * c;
    auto key_of = [&](int i) { return ~f2u(1.f / (1.f + expf(-lg[i]))); };          // torch.sigmoid; smaller key = larger score (scores > 0)
    for (int i = tid; i < mpad; i += 1024) sel[i] = ~0ull;
    if (tid == 0) {
        s_need = m;
        s_cnt = 0;
    }
    unsigned prefix = 0;
    int decided = 0;                                                     // leading bits of the threshold known so far
    const int bits_of[3] = {11, 11, 10};
    for (int pass = 0; pass < 3; ++pass) {
        const int bits = bits_of[pass], shift = 32 - decided - bits;
        for (int i = tid; i < 2048; i += 1024) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < total; i += 1024) {
            const unsigned k = key_of(i);
            if (decided == 0 || (k >> (32 - decided)) == prefix) atomicAdd(&hist[(k >> shift) & ((1u << bits) - 1)], 1);
        }
        __syncthreads();
        if (tid < 64) {                                                  // first wave: the bin that holds the s_need-th key
            const int nb = 1 << bits, per = nb / 64;
            int sum = 0;
            for (int b = 0; b < per; ++b) sum += hist[tid * per + b];
            int inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(inc, o, 64);
                if (tid >= o) inc += v;
            }
            const int need = s_need, exc = inc - sum;
            if (exc < need && need <= inc) {
                int run = exc;
                for (int b = 0; b < per; ++b) {
                    const int h = hist[tid * per + b];
                    if (need <= run + h) {
                        s_bin = tid * per + b;
                        s_need = need - run;
                        break;
                    }
                    run += h;
                }
            }
        }
        __syncthreads();
        prefix = (prefix << bits) | (unsigned)s_bin;
        decided += bits;
        __syncthreads();
    }
    const unsigned thr = prefix;                                         // the m-th smallest key; s_need of the keys equal to it belong to the top-m
    const int need_eq = s_need;
    const int lane = tid & 63, wave = tid >> 6;
    const int per_w = (total + 15) / 16, i0 = wave * per_w, i1 = min(total, i0 + per_w);          // this wave's range (empty when i0 >= total)
    // slots are bounded by m on every write: m - need_eq keys are below thr and need_eq equal ones are taken as long as all passes see
    // the same logits, and a caller that overwrites them meanwhile must not make this kernel write outside sel
    int eq = 0;                                                          // wave-uniform: keys equal to thr in this wave's range
    for (int i = i0 + lane; i - lane < i1; i += 64) {
        const unsigned k = i < i1 ? key_of(i) : ~0u;
        if (i < i1 && k < thr) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < m) sel[slot] = ((u64)k << 32) | (unsigned)i;
        }
        eq += __popcll(__ballot(i < i1 && k == thr));
    }
    if (lane == 0) s_wave[wave] = eq;
    __syncthreads();
    const int below = s_cnt;                                             // final: every k < thr has been counted before the barrier above
    int rank = 0;                                                        // wave-uniform: equal keys in front of this wave's next iteration
    for (int w = 0; w < wave; ++w) rank += s_wave[w];
    if (eq > 0) {
        for (int i = i0 + lane; i - lane < i1 && rank < need_eq; i += 64) {
            const bool hit = i < i1 && key_of(i) == thr;
            const unsigned long long mask = __ballot(hit);
            const int r = rank + __popcll(mask & ((1ull << lane) - 1ull));
            if (hit && r < need_eq && below + r < m) sel[below + r] = ((u64)thr << 32) | (unsigned)i;
            rank += __popcll(mask);
        }
    }
    __syncthreads();
    bitonic_sort_u64(sel, mpad);
    const long obase = ((long)f * nsets + set) * m;
    for (int r = tid; r < m; r += 1024) {
        const u64 key = sel[r];
        const unsigned idx = min((unsigned)key, (unsigned)(total - 1));          // (an unfilled slot, see above, reads inside the frame)
        cand_scores[obase + r] = __uint_as_float(~(unsigned)(key >> 32));
        cand_labels[obase + r] = (int)(idx % c) + 1;
        *reinterpret_cast<float4v*>(cand_boxes + (obase + r) * 4) = *reinterpret_cast<const float4v*>(boxes + (base + idx / c) * 4);
    }
}

// one workgroup (1024 threads) per frame; n = nsets * m candidates (<= 1024).  SIZE (common.h): the frame's (w, h) -- one for all frames or
// the frame's row of a table -- read by the final clip alone: max_coord, the class offsets and the IoU never see it.
template <typename SIZE>
__global__ __launch_bounds__(1024) void nms_frame_kernel(const float* __restrict__ cand_boxes, const float* __restrict__ cand_scores,
                                                          const int* __restrict__ cand_labels, int n, int npad, SIZE size, float iou_thr, int use_nms, int out_cap,
                                                          float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                          int* __restrict__ out_labels, int* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int words = (n + 63) >> 6;
    u64* keys = reinterpret_cast<u64*>(smem);                          // [npad]
    float* bx = reinterpret_cast<float*>(keys + npad);                 // [n][4] offset boxes, sorted order
    float* area = bx + 4 * n;                                          // [n]
    int* order = reinterpret_cast<int*>(area + n);                     // [n]
    float* redf = reinterpret_cast<float*>(order + n);                 // [16]
    int* keep_slot = reinterpret_cast<int*>(redf + 16);                // [n]
    u64* mask = reinterpret_cast<u64*>(keep_slot + ((n + 1) & ~1));    // [n][words]
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* cb = cand_boxes + (long)f * n * 4;
    const float* cs = cand_scores + (long)f * n;
    const int* cl = cand_labels + (long)f * n;

    float mx = -INFINITY;
    for (int i = tid; i < npad; i += blockDim.x) {
        u64 key = ~0ull;
        if (i < n) {
            key = ((u64)(~f2u(cs[i])) << 32) | (unsigned)i;
            const float4v b = *reinterpret_cast<const float4v*>(cb + i * 4);
            mx = fmaxf(mx, fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3])));
        }
        keys[i] = key;
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) redf[tid >> 6] = mx;
    __syncthreads();
    bitonic_sort_u64(keys, npad);
    float max_coord = redf[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) max_coord = fmaxf(max_coord, redf[w]);
    const float off_unit = max_coord + 1.0f;
    for (int r = tid; r < n; r += blockDim.x) {
        const int i = (int)(unsigned)keys[r];
        order[r] = i;
        const float4v b = *reinterpret_cast<const float4v*>(cb + i * 4);
        const float off = (float)cl[i] * off_unit;
        const float x1 = b[0] + off, y1 = b[1] + off, x2 = b[2] + off, y2 = b[3] + off;
        bx[r * 4 + 0] = x1;
        bx[r * 4 + 1] = y1;
        bx[r * 4 + 2] = x2;
        bx[r * 4 + 3] = y2;
        area[r] = (x2 - x1) * (y2 - y1);
    }
    __syncthreads();
    if (use_nms) {
        // suppression bit matrix: mask[i][w] bit j = IoU(i, 64w + j) > thr for 64w + j > i
        for (int t = tid; t < n * words; t += blockDim.x) {
            const int i = t / words, w = t - i * words;
            const float ix1 = bx[i * 4], iy1 = bx[i * 4 + 1], ix2 = bx[i * 4 + 2], iy2 = bx[i * 4 + 3];
            const float ia = area[i];
            u64 bits = 0;
            const int j0 = w << 6;
            const int jend = min(64, n - j0);
            for (int jj = 0; jj < jend; ++jj) {
                const int j = j0 + jj;
                if (j <= i) continue;
                const float xx1 = fmaxf(ix1, bx[j * 4]), yy1 = fmaxf(iy1, bx[j * 4 + 1]);
                const float xx2 = fminf(ix2, bx[j * 4 + 2]), yy2 = fminf(iy2, bx[j * 4 + 3]);
                const float ww = fmaxf(0.f, xx2 - xx1), hh = fmaxf(0.f, yy2 - yy1);
                const float inter = ww * hh;
                const float ovr = inter / (ia + area[j] - inter);
                if (ovr > iou_thr) bits |= 1ull << jj;
            }
            mask[(long)i * words + w] = bits;
        }
    }
    __syncthreads();
    // greedy sweep by wave 0: lane w owns word w of the removed set
    if (tid < 64) {
        u64 removed = 0;
        int nkeep = 0;
        for (int i = 0; i < n; ++i) {
            const u64 wrd = __shfl(removed, i >> 6, 64);
            const bool alive = !((wrd >> (i & 63)) & 1ull);
            if (alive) {
                if (tid == 0) keep_slot[nkeep] = i;
                ++nkeep;
                if (use_nms && tid < words) removed |= mask[(long)i * words + tid];
            }
        }
        if (tid == 0) out_counts[f] = nkeep;
        redf[0] = __int_as_float(nkeep);
    }
    __syncthreads();
    const int nkeep = __float_as_int(redf[0]);
    const float img_w = size.width(f), img_h = size.height(f);
    for (int s = tid; s < out_cap; s += blockDim.x) {
        float4v b = {0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;
        int lb = 0;
        if (s < nkeep) {
            const int i = order[keep_slot[s]];
            b = *reinterpret_cast<const float4v*>(cb + i * 4);
            b[0] = fminf(fmaxf(b[0], 0.f), img_w - 1.f);
            b[1] = fminf(fmaxf(b[1], 0.f), img_h - 1.f);
            b[2] = fminf(fmaxf(b[2], 0.f), img_w - 1.f);
            b[3] = fminf(fmaxf(b[3], 0.f), img_h - 1.f);
            sc = cs[i];
            lb = cl[i];
        }
        *reinterpret_cast<float4v*>(out_boxes + ((long)f * out_cap + s) * 4) = b;
        out_scores[(long)f * out_cap + s] = sc;
        out_labels[(long)f * out_cap + s] = lb;
    }
}

// ---- the tiled form -------------------------------------------------------------------------------------------------------------------
// Three launches per chunk of frames, all on the caller's stream:
//   sort   one workgroup per frame: the stable order (score desc, position asc), max_coord, the offset boxes and their areas -> scratch
//   mask   grid (frame, 64-row tile, 4-word tile): the upper-triangular bit words mask[i][w]; tiles wholly below the diagonal return
//          at once and their words stay unwritten -- the sweep reads word w of row i only for w >= i / 64
//   sweep  one workgroup per frame: wave 0 sweeps (lane w owns word w of the removed set: at most 4096 candidates = 64 words) while all
//          four waves stage the next block of mask rows from global memory into the other half of an LDS double buffer; then the
//          outputs as kernel B writes them.
// Every pair is tested, cross-class pairs included: the boxes are unclipped, so with negative coordinates the offset boxes of
// neighbouring classes can overlap, and torchvision's batched_nms suppresses across classes then.
//
// Arithmetic: the operations of nms_frame_kernel as the compiler builds them (-ffp-contract=fast, hipcc's default): there the union
// ia + area[j] - inter is one fused multiply-add, fma(-ww, hh, ia + area[j]), and nothing else contracts.  Written out here under
// contract(off), so both kernels give the same bits whatever the optimiser sees around the expression.
constexpr int NMS_TILE_ROWS = 64;        // mask: rows per workgroup
constexpr int NMS_TILE_WORDS = 4;        // mask: 64-bit words per workgroup (256 columns)
constexpr int NMS_SWEEP_ROWS = 32;       // sweep: mask rows per staged block
constexpr int NMS_SWEEP_THREADS = 256;

__global__ __launch_bounds__(1024) void nms_tiled_sort_kernel(const float* __restrict__ cand_boxes, const float* __restrict__ cand_scores,
                                                               const int* __restrict__ cand_labels, int n, int npad,
                                                               float* __restrict__ sbox, float* __restrict__ sarea, int* __restrict__ sorder) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                          // [npad]
    __shared__ float redf[16];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* cb = cand_boxes + (long)f * n * 4;
    const float* cs = cand_scores + (long)f * n;
    const int* cl = cand_labels + (long)f * n;
    float mx = -INFINITY;
    for (int i = tid; i < npad; i += blockDim.x) {
        u64 key = ~0ull;
        if (i < n) {
            key = ((u64)(~f2u(cs[i])) << 32) | (unsigned)i;
            const float4v b = *reinterpret_cast<const float4v*>(cb + i * 4);
            mx = fmaxf(mx, fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3])));
        }
        keys[i] = key;
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) redf[tid >> 6] = mx;
    __syncthreads();
    bitonic_sort_u64(keys, npad);
    float max_coord = redf[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) max_coord = fmaxf(max_coord, redf[w]);
    const float off_unit = max_coord + 1.0f;
    for (int r = tid; r < n; r += blockDim.x) {
        const int i = (int)(unsigned)keys[r];
        sorder[(long)f * n + r] = i;
        const float4v b = *reinterpret_cast<const float4v*>(cb + i * 4);
        const float off = (float)cl[i] * off_unit;
        const float4v o = {b[0] + off, b[1] + off, b[2] + off, b[3] + off};
        *reinterpret_cast<float4v*>(sbox + ((long)f * n + r) * 4) = o;
        sarea[(long)f * n + r] = (o[2] - o[0]) * (o[3] - o[1]);           // from the OFFSET coordinates, as kernel B
    }
}

// grid (frames, row tiles, word tiles), 256 threads: thread t computes word (t / 64) of row (t % 64) of its tile, so a wave reads one
// column box at a time from LDS (a broadcast); the 64 x 4 words go through LDS once more so that a row's 4 words leave as 32 bytes.
__global__ __launch_bounds__(256) void nms_tiled_mask_kernel(const float* __restrict__ sbox, const float* __restrict__ sarea, int n, int words,
                                                              float iou_thr, u64* __restrict__ mask) {
#pragma clang fp contract(off)
    const int f = blockIdx.x, row0 = blockIdx.y * NMS_TILE_ROWS, word0 = blockIdx.z * NMS_TILE_WORDS, col0 = word0 * 64;
    if (col0 + NMS_TILE_WORDS * 64 - 1 <= row0) return;                // every column j of the tile is <= every row i: no bit can be set
    __shared__ float4v cbx[NMS_TILE_WORDS * 64];
    __shared__ float car[NMS_TILE_WORDS * 64];
    __shared__ u64 tile[NMS_TILE_ROWS * NMS_TILE_WORDS];
    const int tid = threadIdx.x;
    const float* bx = sbox + (long)f * n * 4;
    const float* area = sarea + (long)f * n;
    {
        const int j = col0 + tid;
        float4v b = {0.f, 0.f, 0.f, 0.f};
        float a = 0.f;
        if (j < n) {
            b = *reinterpret_cast<const float4v*>(bx + (long)j * 4);
            a = area[j];
        }
        cbx[tid] = b;
        car[tid] = a;
    }
    __syncthreads();
    const int r = tid & 63, wl = tid >> 6, i = row0 + r;
    u64 bits = 0;
    if (i < n) {
        const float4v ib = *reinterpret_cast<const float4v*>(bx + (long)i * 4);
        const float ia = area[i];
        const int j0 = col0 + wl * 64;
        const int jend = min(64, n - j0);
        for (int jj = 0; jj < jend; ++jj) {
            if (j0 + jj <= i) continue;
            const float4v jb = cbx[wl * 64 + jj];
            const float xx1 = fmaxf(ib[0], jb[0]), yy1 = fmaxf(ib[1], jb[1]);
            const float xx2 = fminf(ib[2], jb[2]), yy2 = fminf(ib[3], jb[3]);
            const float ww = fmaxf(0.f, xx2 - xx1), hh = fmaxf(0.f, yy2 - yy1);
            const float inter = ww * hh;
            const float ovr = inter / __builtin_fmaf(-ww, hh, ia + car[wl * 64 + jj]);      // inter / (ia + area[j] - inter), see above
            if (ovr > iou_thr) bits |= 1ull << jj;
        }
    }
    tile[r * NMS_TILE_WORDS + wl] = bits;
    __syncthreads();
    const int orow = row0 + (tid >> 2), ow = word0 + (tid & 3);
    if (orow < n && ow < words) mask[((long)f * n + orow) * words + ow] = tile[tid];
}

// one workgroup (256 threads) per frame; dynamic LDS: two blocks of NMS_SWEEP_ROWS x words mask words, then keep_slot[n]
template <typename SIZE>
__global__ __launch_bounds__(NMS_SWEEP_THREADS) void nms_tiled_sweep_kernel(
    const float* __restrict__ cand_boxes, const float* __restrict__ cand_scores, const int* __restrict__ cand_labels,
    const int* __restrict__ sorder, const u64* __restrict__ mask, int n, int words, SIZE size, int use_nms, int out_cap,
    float* __restrict__ out_boxes, float* __restrict__ out_scores, int* __restrict__ out_labels, int* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PER = NMS_SWEEP_ROWS * 64 / NMS_SWEEP_THREADS;       // staged words per thread at the widest matrix (64 words)
    const int blk = NMS_SWEEP_ROWS * words;
    u64* stage = reinterpret_cast<u64*>(smem);                         // [2][blk]
    int* keep_slot = reinterpret_cast<int*>(stage + 2 * blk);          // [n]
    __shared__ int s_nkeep;
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* cb = cand_boxes + (long)f * n * 4;
    const float* cs = cand_scores + (long)f * n;
    const int* cl = cand_labels + (long)f * n;
    const int* order = sorder + (long)f * n;
    const u64* mrow = mask + (long)f * n * words;
    if (!use_nms) {
        for (int i = tid; i < n; i += NMS_SWEEP_THREADS) keep_slot[i] = i;
        if (tid == 0) s_nkeep = n;
    } else {
        u64 regs[PER];
        // block b of the matrix -> registers; words below the diagonal (never written by the mask kernel) and rows past n read as 0
        auto fetch = [&](int b) {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int idx = tid + k * NMS_SWEEP_THREADS;
                const int r = idx / words, w = idx - r * words, i = b * NMS_SWEEP_ROWS + r;
                regs[k] = (idx < blk && i < n && w >= (i >> 6)) ? mrow[(long)i * words + w] : 0ull;
            }
        };
        auto put = [&](u64* dst) {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int idx = tid + k * NMS_SWEEP_THREADS;
                if (idx < blk) dst[idx] = regs[k];
            }
        };
        const int nblk = (n + NMS_SWEEP_ROWS - 1) / NMS_SWEEP_ROWS;
        fetch(0);
        put(stage);
        __syncthreads();
        u64 removed = 0;                                               // wave 0: lane w owns word w of the removed set
        int nkeep = 0;
        for (int b = 0; b < nblk; ++b) {
            const bool more = b + 1 < nblk;
            if (more) fetch(b + 1);                                    // in flight while wave 0 sweeps block b
            if (tid < 64) {
                const u64* cur_blk = stage + (b & 1) * blk;
                const int i0 = b * NMS_SWEEP_ROWS, rows = min(NMS_SWEEP_ROWS, n - i0);
                u64 cur = tid < words ? cur_blk[tid] : 0ull;
                for (int r = 0; r < rows; ++r) {
                    const u64 nxt = (r + 1 < rows && tid < words) ? cur_blk[(r + 1) * words + tid] : 0ull;      // ahead of the keep decision
                    const int i = i0 + r;
                    const unsigned half = (i & 32) ? (unsigned)(removed >> 32) : (unsigned)removed;
                    const unsigned wrd = __builtin_amdgcn_readlane(half, i >> 6);
                    if (!((wrd >> (i & 31)) & 1u)) {
                        if (tid == 0) keep_slot[nkeep] = i;
                        ++nkeep;
                        removed |= cur;
                    }
                    cur = nxt;
                }
            }
            if (more) put(stage + ((b + 1) & 1) * blk);                // that half was last read while block b - 1 was swept
            __syncthreads();
        }
        if (tid == 0) s_nkeep = nkeep;
    }
    __syncthreads();
    const int nkeep = s_nkeep;
    if (tid == 0) out_counts[f] = nkeep;
    const float img_w = size.width(f), img_h = size.height(f);
    for (int s = tid; s < out_cap; s += NMS_SWEEP_THREADS) {
        float4v b = {0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;
        int lb = 0;
        if (s < nkeep) {
            const int i = order[keep_slot[s]];
            b = *reinterpret_cast<const float4v*>(cb + i * 4);
            b[0] = fminf(fmaxf(b[0], 0.f), img_w - 1.f);
            b[1] = fminf(fmaxf(b[1], 0.f), img_h - 1.f);
            b[2] = fminf(fmaxf(b[2], 0.f), img_w - 1.f);
            b[3] = fminf(fmaxf(b[3], 0.f), img_h - 1.f);
            sc = cs[i];
            lb = cl[i];
        }
        *reinterpret_cast<float4v*>(out_boxes + ((long)f * out_cap + s) * 4) = b;
        out_scores[(long)f * out_cap + s] = sc;
        out_labels[(long)f * out_cap + s] = lb;
    }
}

int next_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace

// topk_stream_kernel at any shape it takes: 1 <= m <= DVID_NMS_MAX_CANDIDATES (sel[mpad] is at most 32 KiB), 1 <= c <= DVID_MAX_CLASSES
// (m * c stays far inside 32 bits)
int dvid_topk_stream_launch(const float* logits, const float* boxes, int n_img, int nsets, int m, int c, float* cand_boxes,
                            float* cand_scores, int* cand_labels, hipStream_t s) {
    if (m < 1 || m > DVID_NMS_MAX_CANDIDATES || c < 1 || c > DVID_MAX_CLASSES || nsets < 1 || nsets > 65535) return DVID_ERR_UNSUPPORTED;
    if (n_img == 0) return DVID_OK;
    const int mpad = next_pow2(m);
    hipLaunchKernelGGL(topk_stream_kernel, dim3(n_img, nsets), dim3(1024), (size_t)mpad * 8, s, logits, boxes, n_img, m, c, mpad, cand_boxes,
                       cand_scores, cand_labels);
    LAUNCH_CHECK();
    return DVID_OK;
}

// THE dispatch rule of the three selection forms: topk_select_kernel runs every shape whose keys fit its LDS (mpad * 8 + m * c * 4 + 8 KiB
// <= 150 KiB: 300 x 30, 300 x 80), topk_candidates_kernel (the full sort) the others up to 16384 padded keys, topk_stream_kernel the rest
// (500 x 80, 1000 x 80, anything x 1203).  All three give the same bits.
int dvid_topk_candidates_launch(const float* logits, const float* boxes, int n_img, int nsets, int m, int c, float* cand_boxes,
                                float* cand_scores, int* cand_labels, hipStream_t s) {
    if (n_img == 0) return DVID_OK;
    {
        // radix select + sort of the M selected keys (topk_select_kernel); shapes whose keys do not fit its LDS take the full sort below
        const int mpad = next_pow2(m);
        const size_t smem2 = (size_t)mpad * 8 + (size_t)m * c * 4 + 2048 * 4;
        if (m * c > m && smem2 <= 150 * 1024) {
            static std::atomic<unsigned long long> attr2{0};          // one bit per device: the attribute belongs to (function, device)
            if (const int rc = allow_dynamic_lds(&topk_select_kernel, 150 * 1024, attr2); rc != DVID_OK) return rc;
            hipLaunchKernelGGL(topk_select_kernel, dim3(n_img, nsets), dim3(1024), smem2, s, logits, boxes, n_img, m, c, mpad, cand_boxes,
                               cand_scores, cand_labels);
            LAUNCH_CHECK();
            return DVID_OK;
        }
    }
    const int npad = next_pow2(m * c);
    const size_t smem = (size_t)npad * 8;
    if (smem > 160 * 1024) return dvid_topk_stream_launch(logits, boxes, n_img, nsets, m, c, cand_boxes, cand_scores, cand_labels, s);
    static std::atomic<unsigned long long> attr{0};          // one bit per device: the attribute belongs to (function, device)
    if (const int rc = allow_dynamic_lds(&topk_candidates_kernel, 160 * 1024, attr); rc != DVID_OK) return rc;
    hipLaunchKernelGGL(topk_candidates_kernel, dim3(n_img, nsets), dim3(1024), smem, s, logits, boxes, n_img, m, c, npad, cand_boxes,
                       cand_scores, cand_labels);
    LAUNCH_CHECK();
    return DVID_OK;
}

// LDS of nms_frame_kernel for n candidates: the keys, the boxes and the whole bit matrix
static size_t nms_frame_lds_bytes(int n) {
    const int npad = next_pow2(n), words = (n + 63) / 64;
    return (size_t)npad * 8 + (size_t)n * (16 + 4 + 4) + 64 + (size_t)((n + 1) & ~1) * 4 + (size_t)n * words * 8;
}

// THE dispatch rule of the two NMS forms: nms_frame_kernel runs every shape it holds in LDS, the tiled form the others
bool dvid_nms_frames_fits_lds(int n) { return n <= 1024 && nms_frame_lds_bytes(n) <= 160 * 1024; }

template <typename SIZE>
static int nms_frames_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, SIZE size, float iou,
                             int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels, int* out_counts, hipStream_t s) {
    if (n_img == 0) return DVID_OK;
    if (!dvid_nms_frames_fits_lds(n) || out_cap < n) return DVID_ERR_UNSUPPORTED;
    const int npad = next_pow2(n);
    const size_t smem = nms_frame_lds_bytes(n);
    static std::atomic<unsigned long long> attr{0};          // one bit per device: the attribute belongs to (function, device); one per SIZE
    if (const int rc = allow_dynamic_lds(&nms_frame_kernel<SIZE>, 160 * 1024, attr); rc != DVID_OK) return rc;
    hipLaunchKernelGGL(nms_frame_kernel<SIZE>, dim3(n_img), dim3(1024), smem, s, cand_boxes, cand_scores, cand_labels, n, npad, size,
                       iou, use_nms, out_cap, out_boxes, out_scores, out_labels, out_counts);
    LAUNCH_CHECK();
    return DVID_OK;
}

int dvid_nms_frames_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, float img_w,
                           float img_h, float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels,
                           int* out_counts, hipStream_t s) {
    return nms_frames_launch(cand_boxes, cand_scores, cand_labels, n_img, n, FrameSizeAll{img_w, img_h}, iou, use_nms, out_cap, out_boxes, out_scores,
                             out_labels, out_counts, s);
}

int dvid_nms_frames_sizes_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, const float* sizes,
                                 float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels, int* out_counts,
                                 hipStream_t s) {
    if (n_img > 0 && !sizes) return DVID_ERR_ARG;
    return nms_frames_launch(cand_boxes, cand_scores, cand_labels, n_img, n, FrameSizeTable{sizes}, iou, use_nms, out_cap, out_boxes, out_scores,
                             out_labels, out_counts, s);
}

// Frames per chunk of the tiled form: as many as keep the chunk's bit matrices within NMS_TILED_MATRIX_CEILING (2 MiB per frame at
// 4096 candidates, 0.53 MiB at 2100: a 304-frame group would need 160 MiB at once), at least one.
static const size_t NMS_TILED_MATRIX_CEILING = (size_t)64 << 20;
static int nms_tiled_chunk_frames(int n_img, int n) {
    const size_t per = (size_t)n * ((n + 63) / 64) * 8;
    const size_t fit = NMS_TILED_MATRIX_CEILING / per;
    return (int)(fit < 1 ? 1 : fit > (size_t)n_img ? (size_t)n_img : fit);
}

size_t dvid_nms_tiled_scratch_size(int n_img, int n) {
    if (n_img <= 0 || n <= 0 || n > DVID_NMS_MAX_CANDIDATES) return 0;
    const size_t fc = (size_t)nms_tiled_chunk_frames(n_img, n);
    return 256 + fc * n * (16 + 4 + 4 + (size_t)((n + 63) / 64) * 8);          // 256: the launcher aligns its base
}

// size_of(f0): the SIZE of the chunk of frames that starts at frame f0 (the kernels index it by the frame inside the chunk)
template <typename SIZE_OF>
static int nms_frames_tiled_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, SIZE_OF size_of,
                                   float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels, int* out_counts,
                                   void* scratch, hipStream_t s) {
    if (n_img == 0) return DVID_OK;
    if (n < 1 || n > DVID_NMS_MAX_CANDIDATES || out_cap < n || !scratch) return DVID_ERR_UNSUPPORTED;
    const int npad = next_pow2(n), words = (n + 63) / 64;
    const int fc = nms_tiled_chunk_frames(n_img, n);
    char* base = reinterpret_cast<char*>(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
    float* sbox = reinterpret_cast<float*>(base);                                  // [fc][n][4]
    float* sarea = sbox + (size_t)fc * n * 4;                                      // [fc][n]
    int* sorder = reinterpret_cast<int*>(sarea + (size_t)fc * n);                  // [fc][n]
    u64* mask = reinterpret_cast<u64*>(sorder + (size_t)fc * n);                   // [fc][n][words]; fc * n * 24 bytes in: 8-byte aligned
    const size_t sweep_lds = (size_t)2 * NMS_SWEEP_ROWS * words * 8 + (size_t)n * 4;          // <= 48 KiB
    for (int f0 = 0; f0 < n_img; f0 += fc) {
        const int nf = n_img - f0 < fc ? n_img - f0 : fc;
        const float* cb = cand_boxes + (size_t)f0 * n * 4;
        const float* cs = cand_scores + (size_t)f0 * n;
        const int* cl = cand_labels + (size_t)f0 * n;
        hipLaunchKernelGGL(nms_tiled_sort_kernel, dim3(nf), dim3(1024), (size_t)npad * 8, s, cb, cs, cl, n, npad, sbox, sarea, sorder);
        LAUNCH_CHECK();
        if (use_nms) {
            hipLaunchKernelGGL(nms_tiled_mask_kernel, dim3(nf, ceil_div(n, NMS_TILE_ROWS), ceil_div(words, NMS_TILE_WORDS)), dim3(256), 0, s, sbox,
                               sarea, n, words, iou, mask);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(nms_tiled_sweep_kernel<decltype(size_of(f0))>, dim3(nf), dim3(NMS_SWEEP_THREADS), sweep_lds, s, cb, cs, cl, sorder, mask, n, words,
                           size_of(f0), use_nms, out_cap, out_boxes + (size_t)f0 * out_cap * 4, out_scores + (size_t)f0 * out_cap,
                           out_labels + (size_t)f0 * out_cap, out_counts + f0);
        LAUNCH_CHECK();
    }
    return DVID_OK;
}

int dvid_nms_frames_tiled_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, float img_w,
                                 float img_h, float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels,
                                 int* out_counts, void* scratch, hipStream_t s) {
    return nms_frames_tiled_launch(cand_boxes, cand_scores, cand_labels, n_img, n, [=](int) { return FrameSizeAll{img_w, img_h}; }, iou, use_nms,
                                   out_cap, out_boxes, out_scores, out_labels, out_counts, scratch, s);
}

int dvid_nms_frames_tiled_sizes_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n,
                                       const float* sizes, float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores,
                                       int* out_labels, int* out_counts, void* scratch, hipStream_t s) {
    if (n_img > 0 && !sizes) return DVID_ERR_ARG;
    return nms_frames_tiled_launch(cand_boxes, cand_scores, cand_labels, n_img, n, [=](int f0) { return FrameSizeTable{sizes + (size_t)f0 * 2}; }, iou,
                                   use_nms, out_cap, out_boxes, out_scores, out_labels, out_counts, scratch, s);
}
