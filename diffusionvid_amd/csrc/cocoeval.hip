// The matching of the COCO bbox evaluator (data/evaluation/coco_eval.py: evaluate_numpy's loop over images, categories, area ranges, IoU
// thresholds, detections and ground-truth boxes), one workgroup per image, all ten thresholds and all four area ranges in one launch.
//
//   per image   the ground truth (xywh float64, the annotation's area, the crowd flag, the label, the ignored flag per area range) goes
//               to LDS; the image's rows are sorted by (label, score descending, row) as 64-bit keys in LDS (bitonic, padded to a power
//               of two); a row that starts a label is the head of a segment; a row past position 100 of its segment is out
//   per task    one lane per (segment, area range, threshold) walks the segment's first 100 rows in order and, per row, the image's boxes
//               of that label in two passes, the not ignored ones and then the ignored ones: that is the protocol's order "not ignored
//               first, each group in annotation order", and its rule that a row matched to a counted box does not move on to an ignored
//               one is "no second pass after a hit in the first".  `matched` is one byte per (range, threshold, box): a box belongs to
//               one label, so two tasks never share one
//   npig        1 per counted box, added to npig[range][label]: int32 atomics, exact in any order
//
// Arithmetic: the IoU is float64, one operation at a time (contraction off) and one correctly rounded division; the detection's xyxy
// float32 row becomes xywh with w = x2 - x1 in float64.  The thresholds are the caller's float64 values.  The comparisons are written
// as the protocol writes them (`iou < best` skips), so a NaN takes the same branch.  Precondition: the scores are finite.
#include "../../include/dvid_hip.h"
#include "kernels.h"
#include "evalkey.h"          // u64, ce_score_desc, coco_iou: shared with lviseval.hip

#define CE_THREADS 256
#define CE_PAD (~(u64)0)
#define CE_MAX_SEGS (DVID_MAX_CLASSES + 1)          // labels 0 .. DVID_MAX_CLASSES
#define CE_T DVID_COCO_EVAL_THRESHOLDS
#define CE_A DVID_COCO_EVAL_AREAS
#define CE_TOP DVID_COCO_EVAL_MAX_DETS
#define CE_G DVID_COCO_EVAL_MAX_GT

struct CocoEvalParams {
    double thr[CE_T], lo[CE_A], hi[CE_A];
};

// key: label (bits 44..), the score's bits mapped so that a greater score is a smaller number (bits 12..43), the row (bits 0..11)
__device__ __forceinline__ int ce_label(u64 key) { return (int)(key >> 44); }
__device__ __forceinline__ int ce_row(u64 key) { return (int)(key & 0xfff); }

__global__ __launch_bounds__(CE_THREADS) void coco_eval_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int N, int cap, int P,
                                                                     const double* __restrict__ gt_boxes, const double* __restrict__ gt_areas,
                                                                     const unsigned char* __restrict__ gt_crowd, const int* __restrict__ gt_labels,
                                                                     const int* __restrict__ gt_starts, CocoEvalParams prm, int num_classes,
                                                                     signed char* __restrict__ match, signed char* __restrict__ ignore,
                                                                     int* __restrict__ rank, int* __restrict__ npig) {
    extern __shared__ u64 s_key[];          // [P]
    __shared__ double s_gbox[CE_G][4];
    __shared__ int s_glab[CE_G];
    __shared__ unsigned char s_gcrowd[CE_G], s_gig[CE_A][CE_G], s_matched[CE_A][CE_T][CE_G];
    __shared__ unsigned short s_seg[CE_MAX_SEGS];
    __shared__ int s_nseg;

    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[f], 0), cap);          // cap <= P, a power of two
    const int g0 = gt_starts[f], g = min(max(gt_starts[f + 1] - g0, 0), CE_G);
    const float* d = dets + (size_t)f * cap * 6;
    const size_t plane = (size_t)N * cap, image = (size_t)f * cap;
    if (tid == 0) s_nseg = 0;

    // ---- the ground truth; the counted boxes ----
    for (int k = tid; k < g; k += CE_THREADS) {
        const double* b = gt_boxes + (size_t)(g0 + k) * 4;
        s_gbox[k][0] = b[0], s_gbox[k][1] = b[1], s_gbox[k][2] = b[2], s_gbox[k][3] = b[3];
        const int l = gt_labels[g0 + k];
        const bool crowd = gt_crowd[g0 + k] != 0;
        const double area = gt_areas[g0 + k];
        s_glab[k] = l, s_gcrowd[k] = crowd;
        for (int a = 0; a < CE_A; ++a) {
            const bool ig = crowd || area < prm.lo[a] || area > prm.hi[a];
            s_gig[a][k] = ig;
            for (int t = 0; t < CE_T; ++t) s_matched[a][t][k] = 0;
            if (!ig && l >= 0 && l <= num_classes) atomicAdd(&npig[a * (num_classes + 1) + l], 1);
        }
    }
    // ---- the keys; the rows that belong to no segment ----
    for (int i = tid; i < P; i += CE_THREADS) {
        u64 key = CE_PAD;
        if (i < n) {
            const float sc = d[(size_t)i * 6 + 4];
            const float lf = d[(size_t)i * 6 + 5];
            const int l = (lf >= 0.f && lf <= (float)num_classes) ? (int)lf : -1;
            if (l >= 0) key = ((u64)l << 44) | ((u64)ce_score_desc(sc) << 12) | (u64)i;
        }
        s_key[i] = key;
        if (i < cap && key == CE_PAD) {
            rank[image + i] = -1;
            for (int at = 0; at < CE_A * CE_T; ++at) match[at * plane + image + i] = 0, ignore[at * plane + image + i] = 0;
        }
    }
    __syncthreads();

    // ---- sort ----
    int Pf = 64;          // the image's own power of two
    while (Pf < n) Pf <<= 1;
    for (int k = 2; k <= Pf; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < Pf; i += CE_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const u64 a = s_key[i], b = s_key[x];
                    if ((a > b) == ((i & k) == 0)) s_key[i] = b, s_key[x] = a;
                }
            }
            __syncthreads();
        }
    // ---- segment heads (their order in s_seg does not matter: the segments are independent); the rows past the cut are out ----
    for (int i = tid; i < n; i += CE_THREADS) {
        const u64 key = s_key[i];
        if (key == CE_PAD) continue;
        if (i == 0 || ce_label(s_key[i - 1]) != ce_label(key)) {
            const int at = atomicAdd(&s_nseg, 1);
            if (at < CE_MAX_SEGS) s_seg[at] = (unsigned short)i;
        }
        if (i >= CE_TOP && ce_label(s_key[i - CE_TOP]) == ce_label(key)) {
            const int row = ce_row(key);
            rank[image + row] = -1;
            for (int at = 0; at < CE_A * CE_T; ++at) match[at * plane + image + row] = 0, ignore[at * plane + image + row] = 0;
        }
    }
    __syncthreads();
    const int nseg = min(s_nseg, CE_MAX_SEGS);

    // ---- the matching: a lane per (segment, area range, threshold) ----
    for (int task = tid; task < nseg * (CE_A * CE_T); task += CE_THREADS) {
        const int seg = task / (CE_A * CE_T), at = task - seg * (CE_A * CE_T);
        const int a = at / CE_T, t = at - a * CE_T;
        const int start = s_seg[seg];
        const int l = ce_label(s_key[start]);
        const double lo = prm.lo[a], hi = prm.hi[a], best0 = fmin(prm.thr[t], 1.0 - 1e-10);
        signed char* m_out = match + at * plane + image;
        signed char* i_out = ignore + at * plane + image;
        const int end = min(n, start + CE_TOP);
        for (int i = start; i < end; ++i) {
            const u64 key = s_key[i];
            if (key == CE_PAD || ce_label(key) != l) break;
            const int row = ce_row(key);
            if (at == 0) rank[image + row] = i - start;
            const float* p = d + (size_t)row * 6;
            const double dx = (double)p[0], dy = (double)p[1];
            double dw, dh, da;
            {
#pragma clang fp contract(off)
                dw = (double)p[2] - dx, dh = (double)p[3] - dy;
                da = dw * dh;
            }
            double best = best0;
            int m = -1;
            for (int pass = 0; pass < 2 && m < 0; ++pass)
                for (int k = 0; k < g; ++k) {
                    if (s_glab[k] != l || s_gig[a][k] != pass) continue;
                    const bool crowd = s_gcrowd[k];
                    if (s_matched[a][t][k] && !crowd) continue;
                    const double v = coco_iou(dx, dy, dw, dh, s_gbox[k], crowd);
                    if (v < best) continue;
                    best = v, m = k;
                }
            if (m >= 0) {
                s_matched[a][t][m] = 1;
                m_out[row] = 1, i_out[row] = (signed char)s_gig[a][m];
            } else {
                m_out[row] = 0, i_out[row] = (da < lo || da > hi) ? 1 : 0;
            }
        }
    }
}

int dvid_coco_eval_match_launch(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                                const unsigned char* gt_crowd, const int* gt_labels, const int* gt_starts, const double* iou_thrs,
                                const double* area_ranges, int num_classes, signed char* match, signed char* ignore, int* rank, int* npig,
                                hipStream_t s) {
    if (cap < 1 || cap > DVID_NMS_MAX_CANDIDATES || num_classes < 1 || num_classes > DVID_MAX_CLASSES || n_images < 0) return DVID_ERR_ARG;
    CocoEvalParams prm = {};
    for (int t = 0; t < CE_T; ++t) prm.thr[t] = iou_thrs[t];
    for (int a = 0; a < CE_A; ++a) prm.lo[a] = area_ranges[2 * a], prm.hi[a] = area_ranges[2 * a + 1];
    HIP_TRY(hipMemsetAsync(npig, 0, (size_t)CE_A * (num_classes + 1) * sizeof(int), s));
    if (n_images == 0) return DVID_OK;
    int P = 64;
    while (P < cap) P <<= 1;
    hipLaunchKernelGGL(coco_eval_match_kernel, dim3((unsigned)n_images), dim3(CE_THREADS), (size_t)P * sizeof(u64), s, dets, counts, n_images, cap, P,
                       gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, prm, num_classes, match, ignore, rank, npig);
    LAUNCH_CHECK();
    return DVID_OK;
}
