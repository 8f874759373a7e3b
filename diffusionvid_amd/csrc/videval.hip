// The greedy matching of the ImageNet-VID AP50 evaluator (data/evaluation/vid_eval.py: calc_prec_rec's loop over frames, classes and
// ground-truth boxes) and the CorLoc test of the frame's top detection, one workgroup per frame.
//
//   per frame   the ground truth (boxes with the evaluator's first + 1 on x2, y2, labels, the ignored flag per motion range) goes to LDS;
//               the frame's rows are sorted by (label, score descending, row) as 64-bit keys in LDS (bitonic, padded to a power of
//               two); a row that starts a label is the head of a segment
//   per task    one lane per (segment, motion range) walks the segment's rows in order and, per row, the frame's boxes of that label:
//               the best box not yet taken with IoU >= threshold (on an exact tie the earlier box stays unless it is ignored), top_ig /
//               top_cnt over all of them, then the weight rules of calc_prec_rec.  `taken` is one byte per (range, box): a box belongs
//               to one label, so two tasks of a range never share one
//   n_pos       1.0 per counted box, added to n_pos[range][label]: sums of small integers in float64, exact in any order
//
// Arithmetic: _iou_vid computes in float32, one operation at a time, and divides once; so does vid_iou (contraction off, __fdiv_rn).
// The comparisons with the threshold are float32 ones (numpy compares a float32 with a Python float as float32), the motion
// comparisons and ig.sum() / len float64.  The comparisons are written as calc_prec_rec writes them, so a NaN takes the same branch.
#include "../../include/dvid_hip.h"
#include "kernels.h"
#include "evalmatch.h"          // the key, the sort and the segment heads

#define VE_THREADS 256
#define VE_MAX_SEGS (DVID_MAX_CLASSES + 1)          // labels 0 .. DVID_MAX_CLASSES

struct VidEvalRanges {
    double lo[DVID_VID_EVAL_MAX_RANGES], hi[DVID_VID_EVAL_MAX_RANGES], empty_w[DVID_VID_EVAL_MAX_RANGES];
};

// `g` already has + 1 on x2, y2; `p` gets it here
__device__ __forceinline__ float vid_iou(const float* __restrict__ d, const float4v g, const float ga) {
#pragma clang fp contract(off)
    const float px1 = d[0], py1 = d[1], px2 = d[2] + 1.f, py2 = d[3] + 1.f;
    const float pa = ((px2 - px1) + 1.f) * ((py2 - py1) + 1.f);
    const float ltx = fmaxf(px1, g[0]), lty = fmaxf(py1, g[1]), rbx = fminf(px2, g[2]), rby = fminf(py2, g[3]);
    const float w = fmaxf((rbx - ltx) + 1.f, 0.f), h = fmaxf((rby - lty) + 1.f, 0.f);
    const float inter = w * h;
    return __fdiv_rn(inter, (pa + ga) - inter);
}
__device__ __forceinline__ float vid_area(const float4v g) {
#pragma clang fp contract(off)
    return ((g[2] - g[0]) + 1.f) * ((g[3] - g[1]) + 1.f);
}

__global__ __launch_bounds__(VE_THREADS) void vid_eval_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int F, int cap, int P,
                                                                    const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                                    const int* __restrict__ gt_starts, const double* __restrict__ motion,
                                                                    VidEvalRanges rg, int R, float thr, int num_classes, signed char* __restrict__ match,
                                                                    double* __restrict__ weight, int* __restrict__ rank, double* __restrict__ n_pos,
                                                                    int* __restrict__ top_row, signed char* __restrict__ top_hit) {
    extern __shared__ u64 s_key[];          // [P]
    __shared__ float4v s_gbox[DVID_VID_EVAL_MAX_GT];
    __shared__ float s_garea[DVID_VID_EVAL_MAX_GT];
    __shared__ int s_glab[DVID_VID_EVAL_MAX_GT];
    __shared__ unsigned char s_ign[DVID_VID_EVAL_MAX_RANGES][DVID_VID_EVAL_MAX_GT], s_taken[DVID_VID_EVAL_MAX_RANGES][DVID_VID_EVAL_MAX_GT];
    __shared__ unsigned short s_seg[VE_MAX_SEGS];
    __shared__ u64 s_top[VE_THREADS / WAVE];
    __shared__ int s_nseg, s_hit;

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(counts[f], 0), cap);          // cap <= P, a power of two
    const int g0 = gt_starts[f], g = min(max(gt_starts[f + 1] - g0, 0), DVID_VID_EVAL_MAX_GT);
    const float* d = dets + (size_t)f * cap * 6;
    const size_t plane = (size_t)F * cap, frame = (size_t)f * cap;
    if (tid == 0) s_nseg = 0, s_hit = 0;

    // ---- the ground truth; the counted boxes ----
    for (int k = tid; k < g; k += VE_THREADS) {
        const float* b = gt_boxes + (size_t)(g0 + k) * 4;
        float4v q;
        {
#pragma clang fp contract(off)
            q = (float4v){b[0], b[1], b[2] + 1.f, b[3] + 1.f};
        }
        const int l = gt_labels[g0 + k];
        s_gbox[k] = q, s_garea[k] = vid_area(q), s_glab[k] = l;
        const double mi = motion ? motion[g0 + k] : 0.0;
        for (int r = 0; r < R; ++r) {
            const bool ig = motion && (mi < rg.lo[r] || mi > rg.hi[r]);
            s_ign[r][k] = ig, s_taken[r][k] = 0;
            if (!ig && l >= 0 && l <= num_classes) atomicAdd(&n_pos[(size_t)r * (num_classes + 1) + l], 1.0);
        }
    }
    // ---- the keys; the rows that belong to no segment; the top-scoring row (the lowest row of equal scores) ----
    u64 top = 0;
    for (int i = tid; i < P; i += VE_THREADS) {
        u64 key = EM_PAD;
        if (i < n) {
            const float sc = d[(size_t)i * 6 + 4];
            const int l = (int)d[(size_t)i * 6 + 5];
            if (l >= 0 && l <= num_classes) key = em_key(l, ce_score_desc(sc), i);
            const u64 t = ((u64)(~ce_score_desc(sc)) << 32) | (u64)(0xffffffffu - (unsigned)i);
            top = t > top ? t : top;
        }
        s_key[i] = key;
        if (i < cap && key == EM_PAD) {
            rank[frame + i] = -1;
            for (int r = 0; r < R; ++r) match[r * plane + frame + i] = 0, weight[r * plane + frame + i] = 0.0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)top, o, 64), hi = __shfl_xor((unsigned)(top >> 32), o, 64);
        const u64 other = ((u64)hi << 32) | lo;
        top = other > top ? other : top;
    }
    if (lane == 0) s_top[wave] = top;
    __syncthreads();

    // ---- CorLoc: the top row against the boxes of its label, IoU > threshold ----
    {
        for (int w = 0; w < VE_THREADS / WAVE; ++w) top = s_top[w] > top ? s_top[w] : top;
        const int row = n > 0 ? (int)(0xffffffffu - (unsigned)top) : -1;
        if (row >= 0) {
            const int l = (int)d[(size_t)row * 6 + 5];
            bool hit = false;
            for (int k = tid; k < g; k += VE_THREADS)
                if (s_glab[k] == l && vid_iou(d + (size_t)row * 6, s_gbox[k], s_garea[k]) > thr) hit = true;
            if (hit) s_hit = 1;
        }
        __syncthreads();
        if (tid == 0) top_row[f] = row, top_hit[f] = (signed char)s_hit;
    }

    int Pf = 64;          // the frame's own power of two
    while (Pf < n) Pf <<= 1;
    em_sort<VE_THREADS>(s_key, Pf, tid);
    const int nseg = em_segment_heads<VE_THREADS>(s_key, n, tid, &s_nseg, s_seg, VE_MAX_SEGS);

    // ---- the matching: a lane per (segment, range) ----
    for (int t = tid; t < nseg * R; t += VE_THREADS) {
        const int start = s_seg[t / R], r = t - (t / R) * R;
        const int l = em_label(s_key[start]);
        const double empty_w = rg.empty_w[r];
        signed char* m_out = match + r * plane + frame;
        double* w_out = weight + r * plane + frame;
        for (int i = start; i < n; ++i) {
            const u64 key = s_key[i];
            if (key == EM_PAD || em_label(key) != l) break;
            const int row = em_row(key);
            if (r == 0) rank[frame + row] = i - start;
            const float* p = d + (size_t)row * 6;
            float best = thr, top_ig = -1.f, top_cnt = -1.f;
            int arg = -1, len = 0, ig_sum = 0;
            bool arg_ig = false;
            for (int k = 0; k < g; ++k) {
                if (s_glab[k] != l) continue;
                const bool ig = s_ign[r][k];
                ++len, ig_sum += ig;
                const float v = vid_iou(p, s_gbox[k], s_garea[k]);
                if (ig) {
                    if (v > top_ig) top_ig = v;
                } else {
                    if (v > top_cnt) top_cnt = v;
                }
                if (s_taken[r][k] || v < best) continue;
                if (v == best && arg >= 0 && !arg_ig) continue;
                best = v, arg = k, arg_ig = ig;
            }
            if (len == 0) {
                m_out[row] = 0, w_out[row] = empty_w;
            } else if (arg >= 0) {
                s_taken[r][arg] = 1;
                m_out[row] = 1, w_out[row] = arg_ig ? 1.0 : 0.0;
            } else {
                m_out[row] = 0;
                w_out[row] = top_cnt > top_ig ? 0.0 : (top_ig > top_cnt ? 1.0 : (double)ig_sum / (double)len);
            }
        }
    }
}

int dvid_vid_eval_match_launch(const float* dets, const int* counts, int n_frames, int cap, const float* gt_boxes, const int* gt_labels,
                               const int* gt_starts, const double* motion, const double* ranges, const double* empty_w, int n_ranges, float iou_thresh,
                               int num_classes, signed char* match, double* weight, int* rank, double* n_pos, int* top_row, signed char* top_hit,
                               hipStream_t s) {
    if (n_ranges < 1 || n_ranges > DVID_VID_EVAL_MAX_RANGES || cap < 1 || cap > DVID_NMS_MAX_CANDIDATES || num_classes < 1 ||
        num_classes > DVID_MAX_CLASSES || n_frames < 0)
        return DVID_ERR_ARG;
    VidEvalRanges rg = {};
    for (int r = 0; r < n_ranges; ++r) rg.lo[r] = ranges[2 * r], rg.hi[r] = ranges[2 * r + 1], rg.empty_w[r] = empty_w[r];
    HIP_TRY(hipMemsetAsync(n_pos, 0, (size_t)n_ranges * (num_classes + 1) * sizeof(double), s));
    if (n_frames == 0) return DVID_OK;
    int P = 64;
    while (P < cap) P <<= 1;
    hipLaunchKernelGGL(vid_eval_match_kernel, dim3((unsigned)n_frames), dim3(VE_THREADS), (size_t)P * sizeof(u64), s, dets, counts, n_frames, cap, P, gt_boxes,
                       gt_labels, gt_starts, motion, rg, n_ranges, iou_thresh, num_classes, match, weight, rank, n_pos, top_row, top_hit);
    LAUNCH_CHECK();
    return DVID_OK;
}
