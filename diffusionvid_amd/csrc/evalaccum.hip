// The accumulation of the COCO and the LVIS bbox evaluators on the device (data/evaluation/coco_eval.py: accumulate_arrays), from what
// dvid_coco_eval_match / dvid_lvis_eval_match leave there: precision [T, R, K, A, M] and recall [T, K, A, M] float64 with numpy's bits.
//
// The order.  accumulate_arrays orders the live rows with lexsort((rank, image, label)) and then sorts every (category, maxDet) block
// with a STABLE argsort(-score) on float32, so its order is (label ascending, score descending with -0 == +0, image ascending, rank
// ascending, and the row where a table repeats a rank).  Here the rows are laid out beforehand in (image, rank, row) order -- a workgroup
// per image sorts its rows in LDS -- and a STABLE radix sort of the (label, score) bits follows: rows of one (label, score) keep the
// layout's order, which is (image, rank, row).  That is numpy's order, so nothing is left for the sort to decide.  The other choice,
// a key widened by the image and the rank, sorts 32 + 11 + 31 + 12 bits where this one sorts 32 + bits(K): eleven digit passes
// against five (COCO) or six (LVIS).
//
// Stages, each its own launch; workgroups exchange data only across launch boundaries:
//   1  ea_count_kernel      a workgroup per image counts its live rows (row < counts[image], rank >= 0, 1 <= label <= K)
//      ea_scan_kernel       ONE workgroup turns the counts into offsets (tiles in sequence with a carry); the total is n_live
//      ea_emit_kernel       a workgroup per image sorts its live rows by (rank, row) (bitonic, LDS) and writes per row the 64-bit key
//                           (label << 32 | ce_score_desc(score)) and two masks: bit a * T + t of `tp` is match != 0 && ignore == 0, of
//                           `fp` match == 0 && ignore == 0; the rank rides in bits 40 .. 55 of `tp`
//   2  per 8-bit digit, least significant first: ea_hist_kernel (a 256-bin histogram per tile of EA_TILE rows), ea_scan_kernel (over the
//      digit-major table, so an entry becomes the first output place of its (digit, tile)), ea_scatter_kernel (stable: a wave owns a
//      contiguous quarter of the tile and walks it 64 rows at a time; lanes of one digit find each other with ballots, so a row's place
//      is the count of equal digits in front of it).  The sort moves (key, index into the layout); the masks are gathered once at the end
//   3  ea_bounds_kernel     bounds[l] = the first sorted row with label >= l (searchsorted(lab, arange(K + 2))), and the gather
//   4  ea_sample_kernel     a workgroup per (category, area range, maxDet) walks its block twice in tiles of 256 rows: forward for the
//                           totals, then backward with the running maximum of the precision.  tp and fp are int32 counts; recall is
//                           __ddiv_rn(tp, n_gt), precision __ddiv_rn(tp, (fp + tp) + 2^-52).  searchsorted(rc, thr, "left") lands on the
//                           first selected row or on a row that adds a true positive, so such a row writes the thresholds in
//                           (rc of the row before, its own rc]; no two rows share one.  Every entry of the outputs is written here
//                           (-1 for an uncounted range, 0 where nothing reaches a threshold), so no launch in front of it touches them
//
// Every count that a table supplies is clamped again where it indexes memory.
#include "../../include/dvid_hip.h"
#include "kernels.h"
#include "evalmatch.h"          // em_sort; evalkey.h: u64, ce_score_desc

#define EA_THREADS 256
#define EA_WAVES (EA_THREADS / 64)
#define EA_ITEMS 16                                    // rows per lane in a sort tile
#define EA_TILE (EA_THREADS * EA_ITEMS)                // 4096 rows
#define EA_T DVID_COCO_EVAL_THRESHOLDS
#define EA_A DVID_COCO_EVAL_AREAS
#define EA_R DVID_EVAL_ACCUMULATE_RECALLS
#define EA_M DVID_EVAL_ACCUMULATE_MAX_LIMITS
#define EA_PAD 0xffffffffu
#define EA_RANK_SHIFT 40
#define EA_RANK_MAX 0xffff
#define EA_MASK40 ((u64(1) << 40) - 1)

struct EaSampleParams {
    double thr[EA_R];
    int max_dets[EA_M];
};

__device__ __forceinline__ int ea_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the label of a live row (1 .. K), 0 for any other row
__device__ __forceinline__ int ea_live_label(const float* __restrict__ d, const int* __restrict__ rank_row, int row, int n, int K) {
    if (row >= n || rank_row[row] < 0) return 0;
    const float lf = d[(size_t)row * 6 + 5];
    return (lf >= 1.f && lf < (float)(K + 1)) ? (int)lf : 0;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EA_THREADS) void ea_count_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                              const int* __restrict__ rank, int cap, int K, int* __restrict__ img_off) {
    __shared__ int s_n;
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int n = ea_clampi(counts[f], 0, cap);
    int mine = 0;
    for (int i = tid; i < n; i += EA_THREADS) mine += ea_live_label(dets + (size_t)f * cap * 6, rank + (size_t)f * cap, i, n, K) != 0;
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0) img_off[f] = s_n;
}

// exclusive scan of data[0 .. n) in place by ONE workgroup, four entries per lane and tile; *total (when given) gets the sum
__global__ __launch_bounds__(EA_THREADS) void ea_scan_kernel(int* __restrict__ data, int n, int* __restrict__ total) {
    __shared__ int s_wave[EA_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += EA_THREADS * 4) {
        const int at = base + tid * 4;
        int v[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = at + j < n ? data[at + j] : 0, sum += v[j];
        int inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < EA_WAVES; ++w) {
            if (w < wave) before += s_wave[w];
            all += s_wave[w];
        }
        int run = before + inc - sum;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (at + j < n) data[at + j] = run;
            run += v[j];
        }
        carry += all;
        __syncthreads();
    }
    if (total && tid == 0) *total = carry;
}

__global__ __launch_bounds__(EA_THREADS) void ea_emit_kernel(const float* __restrict__ dets, const int* __restrict__ counts, const int* __restrict__ rank,
                                                             const signed char* __restrict__ match, const signed char* __restrict__ ignore, int N,
                                                             int cap, int K, int rows, const int* __restrict__ img_off, u64* __restrict__ key,
                                                             u64* __restrict__ tpk, u64* __restrict__ fpm) {
    __shared__ unsigned s_key[DVID_NMS_MAX_CANDIDATES];          // rank << 12 | row
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = ea_clampi(counts[f], 0, cap);
    if (n == 0) return;
    const float* d = dets + (size_t)f * cap * 6;
    const int* rk = rank + (size_t)f * cap;
    int Pf = 64;
    while (Pf < n) Pf <<= 1;          // <= DVID_NMS_MAX_CANDIDATES: the host checked cap
    for (int i = tid; i < Pf; i += EA_THREADS)
        s_key[i] = ea_live_label(d, rk, i, n, K) ? ((unsigned)min(rk[i], EA_RANK_MAX) << 12) | (unsigned)i : EA_PAD;
    __syncthreads();
    em_sort<EA_THREADS>(s_key, Pf, tid);
    const size_t plane = (size_t)N * cap, image = (size_t)f * cap;
    const int off = img_off[f];
    for (int j = tid; j < n; j += EA_THREADS) {
        const unsigned sk = s_key[j];
        if (sk == EA_PAD) break;          // the live rows come first
        const int row = (int)(sk & 0xfff), at = off + j;
        if (at < 0 || at >= rows) break;
        const int label = ea_live_label(d, rk, row, n, K);
        u64 tp = 0, fp = 0;
        for (int q = 0; q < EA_A * EA_T; ++q) {
            const bool m = match[q * plane + image + row] != 0, ig = ignore[q * plane + image + row] != 0;
            tp |= (u64)(m && !ig) << q;
            fp |= (u64)(!m && !ig) << q;
        }
        key[at] = ((u64)label << 32) | ce_score_desc(d[(size_t)row * 6 + 4]);
        tpk[at] = tp | ((u64)(sk >> 12) << EA_RANK_SHIFT);
        fpm[at] = fp;
    }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EA_THREADS) void ea_hist_kernel(const u64* __restrict__ key, const int* __restrict__ n_live_p, int rows, int shift,
                                                             int nblocks, int* __restrict__ hist) {
    __shared__ int s_bin[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n_live = ea_clampi(*n_live_p, 0, rows);
    s_bin[tid] = 0;
    __syncthreads();
    const int base = b * EA_TILE;
    for (int j = 0; j < EA_ITEMS; ++j) {
        const int i = base + j * EA_THREADS + tid;
        if (i < n_live) atomicAdd(&s_bin[(int)((key[i] >> shift) & 255)], 1);
    }
    __syncthreads();
    hist[tid * nblocks + b] = s_bin[tid];
}

__global__ __launch_bounds__(EA_THREADS) void ea_scatter_kernel(const u64* __restrict__ key_in, const unsigned* __restrict__ idx_in,
                                                                const int* __restrict__ n_live_p, int rows, int shift, int nblocks,
                                                                const int* __restrict__ hist, int first, u64* __restrict__ key_out,
                                                                unsigned* __restrict__ idx_out) {
    __shared__ int s_cnt[EA_WAVES][256];          // rows of the digit met so far by the wave; then the first place of (wave, digit)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int n_live = ea_clampi(*n_live_p, 0, rows);
    if (b * EA_TILE >= n_live) return;          // the whole workgroup
    for (int w = 0; w < EA_WAVES; ++w) s_cnt[w][tid] = 0;
    __syncthreads();
    const int base = b * EA_TILE + wave * (EA_TILE / EA_WAVES);
    const u64 lt = ((u64)1 << lane) - 1;
    u64 k[EA_ITEMS];
    unsigned ix[EA_ITEMS];
    int place[EA_ITEMS];          // among the wave's rows of the same digit
#pragma unroll
    for (int s = 0; s < EA_ITEMS; ++s) {
        const int i = base + s * 64 + lane;
        const bool valid = i < n_live;
        k[s] = valid ? key_in[i] : 0;
        ix[s] = valid ? (first ? (unsigned)i : idx_in[i]) : 0;
        const int dg = (int)((k[s] >> shift) & 255);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (dg >> bit) & 1;
            const u64 m = __ballot(valid && on);
            peers &= on ? m : ~m;
        }
        const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
        int old = 0;
        if (valid && lane == leader) old = atomicAdd(&s_cnt[wave][dg], __popcll(peers));
        old = __shfl(old, leader);
        place[s] = old + __popcll(peers & lt);
    }
    __syncthreads();
    {
        int run = hist[tid * nblocks + b];          // digit `tid`
        for (int w = 0; w < EA_WAVES; ++w) {
            const int c = s_cnt[w][tid];
            s_cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < EA_ITEMS; ++s) {
        const int i = base + s * 64 + lane;
        if (i >= n_live) continue;
        const int at = s_cnt[wave][(int)((k[s] >> shift) & 255)] + place[s];
        if (at < 0 || at >= rows) continue;
        key_out[at] = k[s];
        idx_out[at] = ix[s];
    }
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EA_THREADS) void ea_bounds_kernel(const u64* __restrict__ key, const unsigned* __restrict__ idx,
                                                               const int* __restrict__ n_live_p, int rows, int K, const u64* __restrict__ tpk,
                                                               const u64* __restrict__ fpm, int* __restrict__ bounds, u64* __restrict__ s_tpk,
                                                               u64* __restrict__ s_fpm) {
    const int n_live = ea_clampi(*n_live_p, 0, rows);
    const int i = blockIdx.x * EA_THREADS + threadIdx.x;
    if (i >= n_live) return;          // no live row: the launcher zeroed bounds
    const int lab = ea_clampi((int)(key[i] >> 32), 0, K + 1);
    const int prev = i ? ea_clampi((int)(key[i - 1] >> 32), 0, K + 1) : 0;
    for (int l = prev + 1; l <= lab; ++l) bounds[l] = i;
    if (i == n_live - 1)
        for (int l = lab + 1; l <= K + 1; ++l) bounds[l] = n_live;
    const unsigned src = min(idx[i], (unsigned)(rows - 1));
    s_tpk[i] = tpk[src];
    s_fpm[i] = fpm[src];
}

// ---- stage 4 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EA_THREADS) void ea_sample_kernel(const u64* __restrict__ s_tpk, const u64* __restrict__ s_fpm, const int* __restrict__ bounds,
                                                               const int* __restrict__ n_live_p, int rows, const int* __restrict__ npig, int K, int M,
                                                               EaSampleParams prm, double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ double s_prec[EA_T][EA_R], s_thr[EA_R];
    __shared__ double s_max[EA_T][EA_WAVES];
    __shared__ int s_sum[EA_T][EA_WAVES];
    __shared__ int s_tp[EA_T], s_fp[EA_T], s_nd, s_first;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % EA_A, k = blockIdx.x / (M * EA_A);
    const size_t col = ((size_t)k * EA_A + a) * M + m, col_stride = (size_t)K * EA_A * M;          // precision[t, r] is at (t * R + r) * col_stride + col
    const int npg = npig[a * (K + 1) + k + 1];
    if (npg <= 0) {
        for (int q = tid; q < EA_T * EA_R; q += EA_THREADS) precision[q * col_stride + col] = -1.0;
        if (tid < EA_T) recall[tid * col_stride + col] = -1.0;
        return;
    }
    const int n_live = ea_clampi(*n_live_p, 0, rows);
    const int b0 = ea_clampi(bounds[k + 1], 0, n_live), b1 = ea_clampi(bounds[k + 2], b0, n_live);
    const int max_det = prm.max_dets[m], sh = a * EA_T;
    const double n_gt = (double)npg, eps = 2.220446049250313e-16;          // 2^-52

    for (int q = tid; q < EA_T * EA_R; q += EA_THREADS) (&s_prec[0][0])[q] = 0.0;
    if (tid < EA_R) s_thr[tid] = prm.thr[tid];
    if (tid < EA_T) s_tp[tid] = 0, s_fp[tid] = 0;
    if (tid == 0) s_nd = 0, s_first = b1;
    __syncthreads();

    // ---- forward: the totals, the count of selected rows and the first of them ----
    {
        int tp[EA_T], fp[EA_T], nd = 0, first = b1;
#pragma unroll
        for (int t = 0; t < EA_T; ++t) tp[t] = 0, fp[t] = 0;
        for (int i = b0 + tid; i < b1; i += EA_THREADS) {
            const u64 x = s_tpk[i];
            if ((int)(x >> EA_RANK_SHIFT) >= max_det) continue;
            const unsigned bt = (unsigned)(x >> sh) & 0x3ff, bf = (unsigned)(s_fpm[i] >> sh) & 0x3ff;
#pragma unroll
            for (int t = 0; t < EA_T; ++t) tp[t] += (bt >> t) & 1, fp[t] += (bf >> t) & 1;
            first = min(first, i);
            ++nd;
        }
        if (nd) {
#pragma unroll
            for (int t = 0; t < EA_T; ++t) {
                if (tp[t]) atomicAdd(&s_tp[t], tp[t]);
                if (fp[t]) atomicAdd(&s_fp[t], fp[t]);
            }
            atomicAdd(&s_nd, nd);
            atomicMin(&s_first, first);
        }
    }
    __syncthreads();
    const int nd = s_nd, first = s_first;
    if (nd > 0) {
        int before_tp[EA_T], before_fp[EA_T];          // the counts in front of the tile at hand; start: in front of the end
        double later_max[EA_T];                        // the greatest precision behind the tile at hand
#pragma unroll
        for (int t = 0; t < EA_T; ++t) before_tp[t] = s_tp[t], before_fp[t] = s_fp[t], later_max[t] = -1.0;
        const int ntiles = (b1 - b0 + EA_THREADS - 1) / EA_THREADS;
        for (int tile = ntiles - 1; tile >= 0; --tile) {
            const int i = b0 + tile * EA_THREADS + tid;
            bool sel = false;
            unsigned bt = 0, bf = 0;
            if (i < b1) {
                const u64 x = s_tpk[i];
                sel = (int)(x >> EA_RANK_SHIFT) < max_det;
                if (sel) bt = (unsigned)(x >> sh) & 0x3ff, bf = (unsigned)(s_fpm[i] >> sh) & 0x3ff;
            }
            int inc[EA_T];          // tp << 16 | fp up to and with this row, within the wave
#pragma unroll
            for (int t = 0; t < EA_T; ++t) {
                int v = (int)(((bt >> t) & 1) << 16 | ((bf >> t) & 1));
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(v, off);
                    if (lane >= off) v += o;
                }
                inc[t] = v;
                if (lane == 63) s_sum[t][wave] = v;
            }
            __syncthreads();
            double pr[EA_T];
            int tp_here[EA_T];
#pragma unroll
            for (int t = 0; t < EA_T; ++t) {
                int in_front = 0, all = 0;
#pragma unroll
                for (int w = 0; w < EA_WAVES; ++w) {
                    if (w < wave) in_front += s_sum[t][w];
                    all += s_sum[t][w];
                }
                before_tp[t] -= all >> 16, before_fp[t] -= all & 0xffff;
                const int v = in_front + inc[t];
                const int tp = before_tp[t] + (v >> 16), fp = before_fp[t] + (v & 0xffff);
                tp_here[t] = tp;
                double p = -1.0;
                if (sel) {
#pragma clang fp contract(off)
                    p = __ddiv_rn((double)tp, (double)(fp + tp) + eps);
                }
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const double o = __shfl_down(p, off);
                    if (lane + off < 64) p = fmax(p, o);
                }
                pr[t] = p;
                if (lane == 0) s_max[t][wave] = p;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < EA_T; ++t) {
                double p = fmax(pr[t], later_max[t]), all = later_max[t];
#pragma unroll
                for (int w = 0; w < EA_WAVES; ++w) {
                    if (w > wave) p = fmax(p, s_max[t][w]);
                    all = fmax(all, s_max[t][w]);
                }
                later_max[t] = all;
                if (sel && (i == first || ((bt >> t) & 1))) {
                    const double rc = __ddiv_rn((double)tp_here[t], n_gt);
                    int r = 0;          // the first selected row takes every threshold up to its own recall
                    if (i != first) {
                        const double rc_prev = __ddiv_rn((double)(tp_here[t] - 1), n_gt);
                        int hi = EA_R;          // the first threshold > rc_prev (the thresholds ascend: the host checked)
                        while (r < hi) {
                            const int mid = (r + hi) >> 1;
                            if (s_thr[mid] > rc_prev) hi = mid; else r = mid + 1;
                        }
                    }
                    for (; r < EA_R && s_thr[r] <= rc; ++r) s_prec[t][r] = p;
                }
            }
            __syncthreads();          // s_sum and s_max are free again
        }
    }
    __syncthreads();
    for (int q = tid; q < EA_T * EA_R; q += EA_THREADS) precision[q * col_stride + col] = (&s_prec[0][0])[q];
    if (tid < EA_T) recall[tid * col_stride + col] = nd > 0 ? __ddiv_rn((double)s_tp[tid], n_gt) : 0.0;
}

// ---- the launcher ----------------------------------------------------------------------------------------------------------------------
namespace {
struct EaLayout {
    size_t head, img, hist, key_a, key_b, idx_a, idx_b, tpk, fpm, s_tpk, s_fpm, total;
    int nblocks;
};
constexpr size_t EA_HEAD_INTS = 4 + DVID_MAX_CLASSES + 2;          // n_live and three spare words, then bounds[0 .. K + 1]

size_t ea_up(size_t v) { return (v + 255) & ~(size_t)255; }

EaLayout ea_layout(long long n_images, long long cap) {
    const size_t rows = (size_t)(n_images * cap);
    EaLayout l;
    l.nblocks = (int)((rows + EA_TILE - 1) / EA_TILE);
    size_t at = 0;
    l.head = at, at += ea_up(EA_HEAD_INTS * sizeof(int));
    l.img = at, at += ea_up((size_t)(n_images + 1) * sizeof(int));
    l.hist = at, at += ea_up((size_t)l.nblocks * 256 * sizeof(int));
    l.key_a = at, at += ea_up(rows * 8);
    l.key_b = at, at += ea_up(rows * 8);
    l.idx_a = at, at += ea_up(rows * 4);
    l.idx_b = at, at += ea_up(rows * 4);
    l.tpk = at, at += ea_up(rows * 8);
    l.fpm = at, at += ea_up(rows * 8);
    l.s_tpk = at, at += ea_up(rows * 8);
    l.s_fpm = at, at += ea_up(rows * 8);
    l.total = at;
    return l;
}
}          // namespace

long long dvid_eval_accumulate_scratch_size(int n_images, int cap, int max_dets_count) {
    if (n_images < 0 || cap < 1 || max_dets_count < 1 || max_dets_count > EA_M) return -1;
    return (long long)ea_layout(n_images, cap).total;
}

int dvid_eval_accumulate_launch(const float* dets, const int* counts, const int* rank, const signed char* match, const signed char* ignore,
                                const int* npig, int n_images, int cap, int num_classes, const int* max_dets, int max_dets_count,
                                const double* rec_thrs, double* precision, double* recall, void* scratch, hipStream_t s) {
    if (cap < 1 || cap > DVID_NMS_MAX_CANDIDATES || num_classes < 1 || num_classes > DVID_MAX_CLASSES || n_images < 0 || max_dets_count < 1 ||
        max_dets_count > EA_M || (long long)n_images * cap >= (1ll << 31))
        return DVID_ERR_ARG;
    const EaLayout l = ea_layout(n_images, cap);
    char* base = reinterpret_cast<char*>(scratch);
    int* head = reinterpret_cast<int*>(base + l.head);
    int* n_live = head;
    int* bounds = head + 4;
    int* img_off = reinterpret_cast<int*>(base + l.img);
    int* hist = reinterpret_cast<int*>(base + l.hist);
    u64* key[2] = {reinterpret_cast<u64*>(base + l.key_a), reinterpret_cast<u64*>(base + l.key_b)};
    unsigned* idx[2] = {reinterpret_cast<unsigned*>(base + l.idx_a), reinterpret_cast<unsigned*>(base + l.idx_b)};
    u64* tpk = reinterpret_cast<u64*>(base + l.tpk);
    u64* fpm = reinterpret_cast<u64*>(base + l.fpm);
    u64* s_tpk = reinterpret_cast<u64*>(base + l.s_tpk);
    u64* s_fpm = reinterpret_cast<u64*>(base + l.s_fpm);
    const int rows = n_images * cap, K = num_classes;

    HIP_TRY(hipMemsetAsync(head, 0, ea_up(EA_HEAD_INTS * sizeof(int)), s));
    if (rows > 0) {
        hipLaunchKernelGGL(ea_count_kernel, dim3((unsigned)n_images), dim3(EA_THREADS), 0, s, dets, counts, rank, cap, K, img_off);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(ea_scan_kernel, dim3(1), dim3(EA_THREADS), 0, s, img_off, n_images, n_live);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(ea_emit_kernel, dim3((unsigned)n_images), dim3(EA_THREADS), 0, s, dets, counts, rank, match, ignore, n_images, cap, K, rows,
                           img_off, key[0], tpk, fpm);
        LAUNCH_CHECK();
        int label_bits = 1;
        while ((1 << label_bits) <= K) ++label_bits;
        const int passes = (32 + label_bits + 7) / 8;
        int cur = 0;
        for (int p = 0; p < passes; ++p, cur ^= 1) {
            hipLaunchKernelGGL(ea_hist_kernel, dim3((unsigned)l.nblocks), dim3(EA_THREADS), 0, s, key[cur], n_live, rows, 8 * p, l.nblocks, hist);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(ea_scan_kernel, dim3(1), dim3(EA_THREADS), 0, s, hist, l.nblocks * 256, (int*)nullptr);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(ea_scatter_kernel, dim3((unsigned)l.nblocks), dim3(EA_THREADS), 0, s, key[cur], idx[cur], n_live, rows, 8 * p, l.nblocks, hist,
                               p == 0 ? 1 : 0, key[cur ^ 1], idx[cur ^ 1]);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(ea_bounds_kernel, dim3((unsigned)((rows + EA_THREADS - 1) / EA_THREADS)), dim3(EA_THREADS), 0, s, key[cur], idx[cur], n_live, rows, K,
                           tpk, fpm, bounds, s_tpk, s_fpm);
        LAUNCH_CHECK();
    }
    EaSampleParams prm = {};
    for (int r = 0; r < EA_R; ++r) prm.thr[r] = rec_thrs[r];
    for (int m = 0; m < max_dets_count; ++m) prm.max_dets[m] = max_dets[m];
    hipLaunchKernelGGL(ea_sample_kernel, dim3((unsigned)(K * EA_A * max_dets_count)), dim3(EA_THREADS), 0, s, s_tpk, s_fpm, bounds, n_live, rows, npig, K,
                       max_dets_count, prm, precision, recall);
    LAUNCH_CHECK();
    return DVID_OK;
}
