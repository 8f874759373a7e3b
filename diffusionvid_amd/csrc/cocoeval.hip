// The matching of the COCO bbox evaluator (data/evaluation/coco_eval.py: evaluate_numpy's loop over images, categories, area ranges, IoU
// thresholds, detections and ground-truth boxes), one workgroup per image, all ten thresholds and all four area ranges in one launch.
//
//   per image   the ground truth (xywh float64, the annotation's area, the crowd flag, the label, the ignored flag per area range) goes
//               to LDS; the image's rows are sorted by (label, score descending, row) as 64-bit keys in LDS (bitonic, padded to a power
//               of two); a row that starts a label is the head of a segment; a row past position 100 of its segment is out
//   per task    one lane per (segment, area range, threshold) walks the segment's first 100 rows in order and, per row, the image's boxes
//               of that label (evalmatch.h: em_walk); a crowd box can be taken again
//   npig        1 per counted box, added to npig[range][label]
//
// The steps and the arithmetic that lviseval.hip shares are in evalmatch.h; here is what the COCO protocol adds: the cut of a segment at 100.
#include "../../include/dvid_hip.h"
#include "kernels.h"
#include "evalmatch.h"

#define CE_THREADS 256
#define CE_MAX_SEGS (DVID_MAX_CLASSES + 1)          // labels 0 .. DVID_MAX_CLASSES
#define CE_TOP DVID_COCO_EVAL_MAX_DETS
#define CE_G DVID_COCO_EVAL_MAX_GT

__global__ __launch_bounds__(CE_THREADS) void coco_eval_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int N, int cap, int P,
                                                                     const double* __restrict__ gt_boxes, const double* __restrict__ gt_areas,
                                                                     const unsigned char* __restrict__ gt_crowd, const int* __restrict__ gt_labels,
                                                                     const int* __restrict__ gt_starts, EvalMatchParams prm, int num_classes,
                                                                     signed char* __restrict__ match, signed char* __restrict__ ignore,
                                                                     int* __restrict__ rank, int* __restrict__ npig) {
    extern __shared__ u64 s_key[];          // [P]
    __shared__ double s_gbox[CE_G][4];
    __shared__ int s_glab[CE_G];
    __shared__ unsigned char s_gcrowd[CE_G], s_gig[EM_A][CE_G], s_matched[EM_A][EM_T][CE_G];
    __shared__ unsigned short s_seg[CE_MAX_SEGS];
    __shared__ int s_nseg;

    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[f], 0), cap);          // cap <= P, a power of two
    const int g0 = gt_starts[f], g = min(max(gt_starts[f + 1] - g0, 0), CE_G);
    const float* d = dets + (size_t)f * cap * 6;
    const EvalMatchGt gt = {&s_gbox[0][0], s_glab, s_gcrowd, &s_gig[0][0], &s_matched[0][0][0], CE_G};
    const EvalMatchOut out = {match, ignore, rank, (size_t)N * cap, (size_t)f * cap};
    if (tid == 0) s_nseg = 0;

    em_load_gt<CE_THREADS>(gt, gt_boxes, gt_areas, gt_crowd, gt_labels, g0, g, prm, num_classes, npig, tid);
    // ---- the keys; the rows that belong to no segment ----
    for (int i = tid; i < P; i += CE_THREADS) {
        u64 key = EM_PAD;
        if (i < n) {
            const float sc = d[(size_t)i * 6 + 4];
            const float lf = d[(size_t)i * 6 + 5];
            if (lf >= 0.f && lf <= (float)num_classes) key = em_key((int)lf, ce_score_desc(sc), i);
        }
        s_key[i] = key;
        if (i < cap && key == EM_PAD) em_row_out(out, i);
    }
    __syncthreads();

    int Pf = 64;          // the image's own power of two
    while (Pf < n) Pf <<= 1;
    em_sort<CE_THREADS>(s_key, Pf, tid);
    // ---- the rows past the cut are out ----
    for (int i = CE_TOP + tid; i < n; i += CE_THREADS) {
        const u64 key = s_key[i];
        if (key != EM_PAD && em_label(s_key[i - CE_TOP]) == em_label(key)) em_row_out(out, em_row(key));
    }
    const int nseg = em_segment_heads<CE_THREADS>(s_key, n, tid, &s_nseg, s_seg, CE_MAX_SEGS);

    // ---- the matching: a lane per (segment, area range, threshold) ----
    for (int task = tid; task < nseg * (EM_A * EM_T); task += CE_THREADS) {
        const int seg = task / (EM_A * EM_T), start = s_seg[seg];
        em_walk<true>(s_key, start, min(n, start + CE_TOP), task - seg * (EM_A * EM_T), d, prm, gt, g, false, out);
    }
}

int dvid_coco_eval_match_launch(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                                const unsigned char* gt_crowd, const int* gt_labels, const int* gt_starts, const double* iou_thrs,
                                const double* area_ranges, int num_classes, signed char* match, signed char* ignore, int* rank, int* npig,
                                hipStream_t s) {
    if (cap < 1 || cap > DVID_NMS_MAX_CANDIDATES || num_classes < 1 || num_classes > DVID_MAX_CLASSES || n_images < 0) return DVID_ERR_ARG;
    HIP_TRY(hipMemsetAsync(npig, 0, (size_t)EM_A * (num_classes + 1) * sizeof(int), s));
    if (n_images == 0) return DVID_OK;
    int P = 64;
    while (P < cap) P <<= 1;
    hipLaunchKernelGGL(coco_eval_match_kernel, dim3((unsigned)n_images), dim3(CE_THREADS), (size_t)P * sizeof(u64), s, dets, counts, n_images, cap, P,
                       gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, em_params(iou_thrs, area_ranges), num_classes, match, ignore, rank, npig);
    LAUNCH_CHECK();
    return DVID_OK;
}
