// The matching of the LVIS bbox evaluator (data/evaluation/lvis_eval.py: match_numpy), the federated protocol: one workgroup per image,
// all ten thresholds and all four area ranges in one launch.  A sibling of cocoeval.hip; what differs is what the protocol changes.
//
//   per image   the ground truth (xywh float64, the annotation's area, the `ignore` flag where COCO has the crowd byte, the label, the
//               ignored flag per area range) goes to LDS, and every box sets its label's bit in the image's POSITIVE set; the image's
//               negative and not-exhaustive lists (two CSR tables) set the bits of two more masks.  The rows are sorted ONCE by (score
//               descending, row): the first 300 are the image's detections, the others are out.  Of the 300, a row whose label is in
//               neither the positive nor the negative set is out too.  The survivors are sorted by (label, score descending, row); a row
//               that starts a label is the head of a segment.  There is no cut per segment: it may hold all 300.
//   per task    one lane per (segment, area range, threshold) walks the segment's rows in order and, per row, the image's boxes of that
//               label in two passes, the not ignored ones and then the ignored ones (cocoeval.hip says why that is the protocol's
//               order and its break rule).  No crowd case: a taken box is never taken again.  A row that takes no box is ignored when
//               its own area lies outside the range OR its label is in the not-exhaustive set
//   npig        1 per counted box, added to npig[range][label]: int32 atomics, exact in any order
//
// LDS, all dynamic, with G the launch's largest box count per image rounded up to 64 and P the power of two >= cap:
//   boxes 32 G + labels 4 G + ignored flags 4 G + matched bytes 40 G = 80 G; keys 8 P; three masks of ceil(1281 / 32) = 41 words and the
//   segment counter 496; segment heads 600.  At the limits G = DVID_LVIS_EVAL_MAX_GT = 1024 and P = 4096:
//   81920 + 32768 + 496 + 600 = 115784 bytes of the CU's 160 KiB (one workgroup per CU); a launch of LVIS' own shape (300 rows: P = 512,
//   G = 256) takes 25672 bytes, so six workgroups fit in a CU's LDS.  2048 boxes would need 197704 bytes: 1024 is the largest power of two.
//
// Arithmetic: as cocoeval.hip (float64 IoU, contraction off, one correctly rounded division; `iou < best` skips, so a NaN takes the same
// branch).  Precondition: the scores are finite.
#include "../../include/dvid_hip.h"
#include "kernels.h"
#include "evalkey.h"

#define LE_THREADS 256
#define LE_PAD (~(u64)0)
#define LE_T DVID_COCO_EVAL_THRESHOLDS
#define LE_A DVID_COCO_EVAL_AREAS
#define LE_TOP DVID_LVIS_EVAL_MAX_DETS
#define LE_TOP_P2 512                                // the power of two >= LE_TOP: the second sort's size
#define LE_G DVID_LVIS_EVAL_MAX_GT
#define LE_WORDS ((DVID_MAX_CLASSES + 1 + 31) / 32)          // a bit per label 0 .. DVID_MAX_CLASSES
static_assert(LE_TOP <= LE_TOP_P2 && DVID_MAX_CLASSES < (1 << 11) && DVID_NMS_MAX_CANDIDATES <= (1 << 12), "the keys' fields");

struct LvisEvalParams {
    double thr[LE_T], lo[LE_A], hi[LE_A];
};

static size_t le_lds_bytes(int G, int P) {
    return (size_t)G * 32 + (size_t)P * 8 + (size_t)G * 4 + (3 * LE_WORDS + 1) * 4 + LE_TOP * 2 + (size_t)G * LE_A + (size_t)G * LE_A * LE_T;
}
static_assert(((3 * LE_WORDS + 1) * 4 + LE_TOP * 2) % 4 == 0, "the byte arrays start on a word");

// first key: the score (bits 23..54), the row (bits 11..22), the label (bits 0..10); the label only rides along: a row occurs once
// second key: as in cocoeval.hip, the label (bits 44..), the score (bits 12..43), the row (bits 0..11)
__device__ __forceinline__ int le_label(u64 key) { return (int)(key >> 44); }
__device__ __forceinline__ int le_row(u64 key) { return (int)(key & 0xfff); }

// bitonic, ascending, n a power of two; ends behind a barrier
__device__ __forceinline__ void le_sort(u64* __restrict__ s_key, const int n, const int tid) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n; i += LE_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const u64 a = s_key[i], b = s_key[x];
                    if ((a > b) == ((i & k) == 0)) s_key[i] = b, s_key[x] = a;
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(LE_THREADS) void lvis_eval_match_kernel(
    const float* __restrict__ dets, const int* __restrict__ counts, int N, int cap, int P, int G, const double* __restrict__ gt_boxes,
    const double* __restrict__ gt_areas, const unsigned char* __restrict__ gt_ignore, const int* __restrict__ gt_labels,
    const int* __restrict__ gt_starts, const int* __restrict__ neg_starts, const int* __restrict__ neg_labels, const int* __restrict__ nex_starts,
    const int* __restrict__ nex_labels, LvisEvalParams prm, int num_classes, signed char* __restrict__ match, signed char* __restrict__ ignore,
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
    unsigned char* s_gig = reinterpret_cast<unsigned char*>(s_seg + LE_TOP);        // [LE_A][G]
    unsigned char* s_matched = s_gig + (size_t)LE_A * G;                            // [LE_A][LE_T][G]

    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[f], 0), cap);          // cap <= P, a power of two
    const int g0 = gt_starts[f], g = min(max(gt_starts[f + 1] - g0, 0), G);
    const float* d = dets + (size_t)f * cap * 6;
    const size_t plane = (size_t)N * cap, image = (size_t)f * cap;
    for (int i = tid; i < 3 * LE_WORDS; i += LE_THREADS) s_pos[i] = 0;
    if (tid == 0) *s_nseg = 0;
    __syncthreads();

    // ---- the ground truth; the counted boxes; the positive set ----
    for (int k = tid; k < g; k += LE_THREADS) {
        const double* b = gt_boxes + (size_t)(g0 + k) * 4;
        s_gbox[k * 4 + 0] = b[0], s_gbox[k * 4 + 1] = b[1], s_gbox[k * 4 + 2] = b[2], s_gbox[k * 4 + 3] = b[3];
        const int l = gt_labels[g0 + k];
        const bool flagged = gt_ignore[g0 + k] != 0, known = l >= 0 && l <= num_classes;
        const double area = gt_areas[g0 + k];
        s_glab[k] = l;
        if (known) atomicOr(&s_pos[l >> 5], 1u << (l & 31));
        for (int a = 0; a < LE_A; ++a) {
            const bool ig = flagged || area < prm.lo[a] || area > prm.hi[a];
            s_gig[a * G + k] = ig;
            for (int t = 0; t < LE_T; ++t) s_matched[(a * LE_T + t) * G + k] = 0;
            if (!ig && known) atomicAdd(&npig[a * (num_classes + 1) + l], 1);
        }
    }
    // ---- the negative and the not-exhaustive set ----
    for (int k = neg_starts[f] + tid; k < neg_starts[f + 1]; k += LE_THREADS) {
        const int l = neg_labels[k];
        if (l >= 0 && l <= num_classes) atomicOr(&s_neg[l >> 5], 1u << (l & 31));
    }
    for (int k = nex_starts[f] + tid; k < nex_starts[f + 1]; k += LE_THREADS) {
        const int l = nex_labels[k];
        if (l >= 0 && l <= num_classes) atomicOr(&s_nex[l >> 5], 1u << (l & 31));
    }
    // ---- the first keys; the rows that are no detection of any label ----
    for (int i = tid; i < P; i += LE_THREADS) {
        u64 key = LE_PAD;
        if (i < n) {
            const float sc = d[(size_t)i * 6 + 4];
            const float lf = d[(size_t)i * 6 + 5];
            const int l = (lf >= 0.f && lf <= (float)num_classes) ? (int)lf : -1;
            if (l >= 0) key = ((u64)ce_score_desc(sc) << 23) | ((u64)i << 11) | (u64)l;
        }
        s_key[i] = key;
        if (i < cap && key == LE_PAD) {
            rank[image + i] = -1;
            for (int at = 0; at < LE_A * LE_T; ++at) match[at * plane + image + i] = 0, ignore[at * plane + image + i] = 0;
        }
    }
    __syncthreads();

    // ---- the image's 300: by (score descending, row) ----
    int Pf = 64;          // the image's own power of two
    while (Pf < n) Pf <<= 1;
    le_sort(s_key, Pf, tid);
    // ---- past the 300, or of a label in neither set: out.  The others get their second key, at their own place ----
    for (int i = tid; i < Pf; i += LE_THREADS) {
        const u64 key = s_key[i];
        if (key == LE_PAD) continue;
        const int l = (int)(key & 0x7ff), row = (int)((key >> 11) & 0xfff);
        const bool listed = (((s_pos[l >> 5] | s_neg[l >> 5]) >> (l & 31)) & 1u) != 0;
        if (i < LE_TOP && listed) {
            s_key[i] = ((u64)l << 44) | (((key >> 23) & 0xffffffffull) << 12) | (u64)row;
        } else {
            s_key[i] = LE_PAD;
            rank[image + row] = -1;
            for (int at = 0; at < LE_A * LE_T; ++at) match[at * plane + image + row] = 0, ignore[at * plane + image + row] = 0;
        }
    }
    __syncthreads();
    // ---- the segments: by (label, score descending, row); every survivor is in front of LE_TOP ----
    const int P2 = min(Pf, LE_TOP_P2);
    le_sort(s_key, P2, tid);
    // ---- segment heads (their order in s_seg does not matter: the segments are independent) ----
    for (int i = tid; i < P2; i += LE_THREADS) {
        const u64 key = s_key[i];
        if (key == LE_PAD) continue;
        if (i == 0 || le_label(s_key[i - 1]) != le_label(key)) {
            const int at = atomicAdd(s_nseg, 1);
            if (at < LE_TOP) s_seg[at] = (unsigned short)i;
        }
    }
    __syncthreads();
    const int nseg = min(*s_nseg, LE_TOP);

    // ---- the matching: a lane per (segment, area range, threshold) ----
    for (int task = tid; task < nseg * (LE_A * LE_T); task += LE_THREADS) {
        const int seg = task / (LE_A * LE_T), at = task - seg * (LE_A * LE_T);
        const int a = at / LE_T, t = at - a * LE_T;
        const int start = s_seg[seg];
        const int l = le_label(s_key[start]);
        const bool not_exhaustive = ((s_nex[l >> 5] >> (l & 31)) & 1u) != 0;
        const double lo = prm.lo[a], hi = prm.hi[a], best0 = fmin(prm.thr[t], 1.0 - 1e-10);
        const unsigned char* gig = s_gig + a * G;
        unsigned char* matched = s_matched + (a * LE_T + t) * G;
        signed char* m_out = match + at * plane + image;
        signed char* i_out = ignore + at * plane + image;
        for (int i = start; i < P2; ++i) {
            const u64 key = s_key[i];
            if (key == LE_PAD || le_label(key) != l) break;
            const int row = le_row(key);
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
                    if (s_glab[k] != l || gig[k] != pass || matched[k]) continue;
                    const double v = coco_iou(dx, dy, dw, dh, s_gbox + k * 4, false);
                    if (v < best) continue;
                    best = v, m = k;
                }
            if (m >= 0) {
                matched[m] = 1;
                m_out[row] = 1, i_out[row] = (signed char)gig[m];
            } else {
                m_out[row] = 0, i_out[row] = (da < lo || da > hi || not_exhaustive) ? 1 : 0;
            }
        }
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
    LvisEvalParams prm = {};
    for (int t = 0; t < LE_T; ++t) prm.thr[t] = iou_thrs[t];
    for (int a = 0; a < LE_A; ++a) prm.lo[a] = area_ranges[2 * a], prm.hi[a] = area_ranges[2 * a + 1];
    HIP_TRY(hipMemsetAsync(npig, 0, (size_t)LE_A * (num_classes + 1) * sizeof(int), s));
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
                       gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels, prm, num_classes, match, ignore,
                       rank, npig);
    LAUNCH_CHECK();
    return DVID_OK;
}
