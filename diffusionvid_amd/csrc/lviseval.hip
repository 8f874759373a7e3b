// The matching of the LVIS bbox evaluator (data/evaluation/lvis_eval.py: match_numpy), the federated protocol: one workgroup per image,
// all ten thresholds and all four area ranges in one launch.  The steps it shares with cocoeval.hip are in evalmatch.h; here is what the
// protocol adds: the three label sets, the cut at 300 rows per image, the listed test and the second sort.
//
//   per image   the ground truth (xywh float64, the annotation's area, the `ignore` flag where COCO has the crowd byte, the label, the
//               ignored flag per area range) goes to LDS, and every box sets its label's bit in the image's POSITIVE set; the image's
//               negative and not-exhaustive lists (two CSR tables) set the bits of two more masks.  The rows are sorted ONCE by (score
//               descending, row): the first 300 are the image's detections, the others are out.  Of the 300, a row whose label is in
//               neither the positive nor the negative set is out too.  The survivors are sorted by (label, score descending, row); a row
//               that starts a label is the head of a segment.  There is no cut per segment: it may hold all 300.
//   per task    one lane per (segment, area range, threshold) walks the segment's rows in order and, per row, the image's boxes of that
//               label (evalmatch.h: em_walk).  No crowd case: a taken box is never taken again.  A row that takes no box is ignored
//               when its own area lies outside the range OR its label is in the not-exhaustive set
//   npig        1 per counted box, added to npig[range][label]
//
// LDS, all dynamic, with G the launch's largest box count per image rounded up to 64 and P the power of two >= cap:
//   boxes 32 G + labels 4 G + ignored flags 4 G + matched bytes 40 G = 80 G; keys 8 P; three masks of ceil(1281 / 32) = 41 words and the
//   segment counter 496; segment heads 600.  At the limits G = DVID_LVIS_EVAL_MAX_GT = 1024 and P = 4096:
//   81920 + 32768 + 496 + 600 = 115784 bytes of the CU's 160 KiB (one workgroup per CU); a launch of LVIS' own shape (300 rows: P = 512,
//   G = 256) takes 25672 bytes, so six workgroups fit in a CU's LDS.  2048 boxes would need 197704 bytes: 1024 is the largest power of two.
#include "../../include/dvid_hip.h"
#include "kernels.h"
#include "evalmatch.h"

#define LE_THREADS 256
#define LE_TOP DVID_LVIS_EVAL_MAX_DETS
#define LE_TOP_P2 512                                // the power of two >= LE_TOP: the second sort's size
#define LE_G DVID_LVIS_EVAL_MAX_GT
#define LE_WORDS ((DVID_MAX_CLASSES + 1 + 31) / 32)          // a bit per label 0 .. DVID_MAX_CLASSES
static_assert(LE_TOP <= LE_TOP_P2 && DVID_MAX_CLASSES < (1 << 11) && DVID_NMS_MAX_CANDIDATES <= (1 << 12), "the keys' fields");

static size_t le_lds_bytes(int G, int P) {
    return (size_t)G * 32 + (size_t)P * 8 + (size_t)G * 4 + (3 * LE_WORDS + 1) * 4 + LE_TOP * 2 + (size_t)G * EM_A + (size_t)G * EM_A * EM_T;
}
static_assert(((3 * LE_WORDS + 1) * 4 + LE_TOP * 2) % 4 == 0, "the byte arrays start on a word");

// labels[from + tid, from + tid + LE_THREADS, .. < to) set their bits in `set`; a label outside 0 .. num_classes is in no set
__device__ __forceinline__ void le_set_bits(unsigned* __restrict__ set, const int* __restrict__ labels, const int from, const int to, const int num_classes,
                                            const int tid) {
    for (int k = from + tid; k < to; k += LE_THREADS) {
        const int l = labels[k];
        if (l >= 0 && l <= num_classes) atomicOr(&set[l >> 5], 1u << (l & 31));
    }
}

__global__ __launch_bounds__(LE_THREADS) void lvis_eval_match_kernel(
    const float* __restrict__ dets, const int* __restrict__ counts, int N, int cap, int P, int G, const double* __restrict__ gt_boxes,
    const double* __restrict__ gt_areas, const unsigned char* __restrict__ gt_ignore, const int* __restrict__ gt_labels,
    const int* __restrict__ gt_starts, const int* __restrict__ neg_starts, const int* __restrict__ neg_labels, const int* __restrict__ nex_starts,
    const int* __restrict__ nex_labels, EvalMatchParams prm, int num_classes, signed char* __restrict__ match, signed char* __restrict__ ignore,
    int* __restrict__ rank, int* __restrict__ npig) {
    extern __shared__ double s_lds[];
    double* s_gbox = s_lds;                                              // [G][4]
    u64* s_key = reinterpret_cast<u64*>(s_gbox + (size_t)G * 4);         // [P]
    int* s_glab = reinterpret_cast<int*>(s_key + P);                     // [G]
    unsigned* s_pos = reinterpret_cast<unsigned*>(s_glab + G);           // [LE_WORDS] each: the positive, negative and not-exhaustive sets
    unsigned* s_neg = s_pos + LE_WORDS;
    unsigned* s_nex = s_neg + LE_WORDS;
    int* s_nseg = reinterpret_cast<int*>(s_nex + LE_WORDS);
    unsigned short* s_seg = reinterpret_cast<unsigned short*>(s_nseg + 1);          // [LE_TOP]: a segment holds at least one of the 300
    unsigned char* s_gig = reinterpret_cast<unsigned char*>(s_seg + LE_TOP);        // [EM_A][G]
    unsigned char* s_matched = s_gig + (size_t)EM_A * G;                            // [EM_A][EM_T][G]

    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[f], 0), cap);          // cap <= P, a power of two
    const int g0 = gt_starts[f], g = min(max(gt_starts[f + 1] - g0, 0), G);
    const float* d = dets + (size_t)f * cap * 6;
    const EvalMatchGt gt = {s_gbox, s_glab, nullptr, s_gig, s_matched, G};
    const EvalMatchOut out = {match, ignore, rank, (size_t)N * cap, (size_t)f * cap};
    for (int i = tid; i < 3 * LE_WORDS; i += LE_THREADS) s_pos[i] = 0;
    if (tid == 0) *s_nseg = 0;
    __syncthreads();

    em_load_gt<LE_THREADS>(gt, gt_boxes, gt_areas, gt_ignore, gt_labels, g0, g, prm, num_classes, npig, tid);
    // ---- the positive, the negative and the not-exhaustive set ----
    le_set_bits(s_pos, gt_labels, g0, g0 + g, num_classes, tid);
    le_set_bits(s_neg, neg_labels, neg_starts[f], neg_starts[f + 1], num_classes, tid);
    le_set_bits(s_nex, nex_labels, nex_starts[f], nex_starts[f + 1], num_classes, tid);
    // ---- the first keys: the score (bits 23..54), the row (bits 11..22), the label (bits 0..10), which only rides along: a row occurs
    //      once.  The rows that are no detection of any label ----
    for (int i = tid; i < P; i += LE_THREADS) {
        u64 key = EM_PAD;
        if (i < n) {
            const float sc = d[(size_t)i * 6 + 4];
            const float lf = d[(size_t)i * 6 + 5];
            if (lf >= 0.f && lf <= (float)num_classes) key = ((u64)ce_score_desc(sc) << 23) | ((u64)i << 11) | (u64)(int)lf;
        }
        s_key[i] = key;
        if (i < cap && key == EM_PAD) em_row_out(out, i);
    }
    __syncthreads();

    // ---- the image's 300: by (score descending, row) ----
    int Pf = 64;          // the image's own power of two
    while (Pf < n) Pf <<= 1;
    em_sort<LE_THREADS>(s_key, Pf, tid);
    // ---- past the 300, or of a label in neither set: out.  The others get the segments' key, at their own place ----
    for (int i = tid; i < Pf; i += LE_THREADS) {
        const u64 key = s_key[i];
        if (key == EM_PAD) continue;
        const int l = (int)(key & 0x7ff), row = (int)((key >> 11) & 0xfff);
        const bool listed = (((s_pos[l >> 5] | s_neg[l >> 5]) >> (l & 31)) & 1u) != 0;
        if (i < LE_TOP && listed) {
            s_key[i] = em_key(l, (unsigned)(key >> 23), row);
        } else {
            s_key[i] = EM_PAD;
            em_row_out(out, row);
        }
    }
    __syncthreads();
    // ---- the segments: by (label, score descending, row); every survivor is in front of LE_TOP ----
    const int P2 = min(Pf, LE_TOP_P2);
    em_sort<LE_THREADS>(s_key, P2, tid);
    const int nseg = em_segment_heads<LE_THREADS>(s_key, P2, tid, s_nseg, s_seg, LE_TOP);

    // ---- the matching: a lane per (segment, area range, threshold); no cut per segment ----
    for (int task = tid; task < nseg * (EM_A * EM_T); task += LE_THREADS) {
        const int seg = task / (EM_A * EM_T), start = s_seg[seg];
        const int l = em_label(s_key[start]);
        const bool not_exhaustive = ((s_nex[l >> 5] >> (l & 31)) & 1u) != 0;
        em_walk<false>(s_key, start, P2, task - seg * (EM_A * EM_T), d, prm, gt, g, not_exhaustive, out);
    }
}

// max_gt: the greatest box count of one image (the caller read it from the host's gt_starts); 0 <= max_gt <= DVID_LVIS_EVAL_MAX_GT
int dvid_lvis_eval_match_launch(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                                const unsigned char* gt_ignore, const int* gt_labels, const int* gt_starts, int max_gt, const int* neg_starts,
                                const int* neg_labels, const int* nex_starts, const int* nex_labels, const double* iou_thrs,
                                const double* area_ranges, int num_classes, signed char* match, signed char* ignore, int* rank, int* npig,
                                hipStream_t s) {
    if (cap < 1 || cap > DVID_NMS_MAX_CANDIDATES || num_classes < 1 || num_classes > DVID_MAX_CLASSES || n_images < 0 || max_gt < 0 || max_gt > LE_G)
        return DVID_ERR_ARG;
    HIP_TRY(hipMemsetAsync(npig, 0, (size_t)EM_A * (num_classes + 1) * sizeof(int), s));
    if (n_images == 0) return DVID_OK;
    int P = 64;
    while (P < cap) P <<= 1;
    const int G = max_gt <= 64 ? 64 : (max_gt + 63) / 64 * 64;
    const size_t smem = le_lds_bytes(G, P);
    if (smem > 64 * 1024) {
        static std::atomic<unsigned long long> attr{0};          // one bit per device: the attribute belongs to (function, device)
        if (const int rc = allow_dynamic_lds(&lvis_eval_match_kernel, (int)le_lds_bytes(LE_G, 4096), attr); rc != DVID_OK) return rc;
    }
    hipLaunchKernelGGL(lvis_eval_match_kernel, dim3((unsigned)n_images), dim3(LE_THREADS), smem, s, dets, counts, n_images, cap, P, G, gt_boxes,
                       gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels, em_params(iou_thrs, area_ranges), num_classes,
                       match, ignore, rank, npig);
    LAUNCH_CHECK();
    return DVID_OK;
}
