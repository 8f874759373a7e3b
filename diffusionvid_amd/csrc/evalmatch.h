// The device code the evaluator kernels share, each piece once:
//   all four (cocoeval.hip, lviseval.hip, videval.hip, evalaccum.hip)   the bitonic sort of a power-of-two array in LDS
//   the three match kernels                                            the (label, score descending, row) key and the segment heads
//   COCO and LVIS                                                      the float64 IoU, the ground-truth load, the "row is out" store, the
//                                                                      walk of one (segment, area range, threshold) task and its parameters
// What a protocol adds (COCO's cut at 100 per segment and its crowd boxes; LVIS' cut at 300 per image, its three label sets and its second
// sort; VID's float32 IoU, CorLoc and weight rules) is in that protocol's file.
//
// Arithmetic of the COCO / LVIS matching: the IoU is float64, one operation at a time (contraction off) and one correctly rounded division;
// a detection's xyxy float32 row becomes xywh with w = x2 - x1 in float64.  The thresholds are the caller's float64 values.  The comparisons
// are written as the protocol writes them (`iou < best` skips), so a NaN takes the same branch.  Precondition: the scores are finite.
#pragma once
#include "../../include/dvid_hip.h"
#include "evalkey.h"          // u64, ce_score_desc

#define EM_PAD (~(u64)0)          // sorts behind every key
#define EM_T DVID_COCO_EVAL_THRESHOLDS
#define EM_A DVID_COCO_EVAL_AREAS

// key: label (bits 44..), the score's bits mapped so that a greater score is a smaller number (bits 12..43), the row (bits 0..11)
__device__ __forceinline__ u64 em_key(int label, unsigned score_desc, int row) { return ((u64)label << 44) | ((u64)score_desc << 12) | (u64)row; }
__device__ __forceinline__ int em_label(u64 key) { return (int)(key >> 44); }
__device__ __forceinline__ int em_row(u64 key) { return (int)(key & 0xfff); }

// bitonic, ascending, by a workgroup of THREADS; n a power of two; ends behind a barrier
template <int THREADS, typename K>
__device__ __forceinline__ void em_sort(K* __restrict__ s_key, const int n, const int tid) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n; i += THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const K a = s_key[i], b = s_key[x];
                    if ((a > b) == ((i & k) == 0)) s_key[i] = b, s_key[x] = a;
                }
            }
            __syncthreads();
        }
}

// The heads of the segments of s_key[0 .. n), sorted: a key that is not the pad and whose label differs from the key's in front of it.
// *s_nseg is 0 on entry, behind a barrier.  Their order in s_seg does not matter: the segments are independent.  Ends behind a barrier;
// -> the number of heads in s_seg, at most `capacity`.
template <int THREADS>
__device__ __forceinline__ int em_segment_heads(const u64* __restrict__ s_key, const int n, const int tid, int* __restrict__ s_nseg,
                                                unsigned short* __restrict__ s_seg, const int capacity) {
    for (int i = tid; i < n; i += THREADS) {
        const u64 key = s_key[i];
        if (key != EM_PAD && (i == 0 || em_label(s_key[i - 1]) != em_label(key))) {
            const int at = atomicAdd(s_nseg, 1);
            if (at < capacity) s_seg[at] = (unsigned short)i;
        }
    }
    __syncthreads();
    return min(*s_nseg, capacity);
}

// ---- COCO and LVIS ------------------------------------------------------------------------------------------------------------------------
struct EvalMatchParams {
    double thr[EM_T], lo[EM_A], hi[EM_A];
};
static inline EvalMatchParams em_params(const double* iou_thrs, const double* area_ranges) {
    EvalMatchParams prm = {};
    for (int t = 0; t < EM_T; ++t) prm.thr[t] = iou_thrs[t];
    for (int a = 0; a < EM_A; ++a) prm.lo[a] = area_ranges[2 * a], prm.hi[a] = area_ranges[2 * a + 1];
    return prm;
}

// an image's ground truth in LDS; `pitch` boxes fit
struct EvalMatchGt {
    double* box;                     // [pitch][4] xywh
    int* label;                      // [pitch]
    unsigned char* flag;             // [pitch]: COCO's crowd byte; null where the kernel does not read the flag again
    unsigned char* ignored;          // [EM_A][pitch]: flagged, or the area outside the range
    unsigned char* matched;          // [EM_A][EM_T][pitch]: a box belongs to one label, so two tasks never share a byte
    int pitch;
};
// the outputs, and where the image's rows are in them
struct EvalMatchOut {
    signed char *match, *ignore;          // [EM_A * EM_T] planes of `plane` rows
    int* rank;
    size_t plane, image;
};

// d, g: x, y, w, h
__device__ __forceinline__ double coco_iou(const double dx, const double dy, const double dw, const double dh, const double* __restrict__ g,
                                           const bool crowd) {
#pragma clang fp contract(off)
    const double w = fmin(dx + dw, g[0] + g[2]) - fmax(dx, g[0]);
    if (w <= 0.0) return 0.0;
    const double h = fmin(dy + dh, g[1] + g[3]) - fmax(dy, g[1]);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double da = dw * dh, ga = g[2] * g[3];
    const double u = crowd ? da : (da + ga) - i;
    return __ddiv_rn(i, u);
}

// the row is out: it belongs to no segment, or lies behind the protocol's cut
__device__ __forceinline__ void em_row_out(const EvalMatchOut& out, const int row) {
    out.rank[out.image + row] = -1;
    for (int at = 0; at < EM_A * EM_T; ++at) out.match[at * out.plane + out.image + row] = 0, out.ignore[at * out.plane + out.image + row] = 0;
}

// Boxes g0 .. g0 + g of the ground truth go to LDS with the matched bytes cleared; npig[range][label] += 1 per counted box (int32
// atomics, exact in any order).  No barrier.
template <int THREADS>
__device__ __forceinline__ void em_load_gt(const EvalMatchGt& gt, const double* __restrict__ gt_boxes, const double* __restrict__ gt_areas,
                                           const unsigned char* __restrict__ gt_flag, const int* __restrict__ gt_labels, const int g0, const int g,
                                           const EvalMatchParams& prm, const int num_classes, int* __restrict__ npig, const int tid) {
    for (int k = tid; k < g; k += THREADS) {
        const double* b = gt_boxes + (size_t)(g0 + k) * 4;
        gt.box[k * 4 + 0] = b[0], gt.box[k * 4 + 1] = b[1], gt.box[k * 4 + 2] = b[2], gt.box[k * 4 + 3] = b[3];
        const int l = gt_labels[g0 + k];
        const bool flagged = gt_flag[g0 + k] != 0;
        const double area = gt_areas[g0 + k];
        gt.label[k] = l;
        if (gt.flag) gt.flag[k] = flagged;
        for (int a = 0; a < EM_A; ++a) {
            const bool ig = flagged || area < prm.lo[a] || area > prm.hi[a];
            gt.ignored[a * gt.pitch + k] = ig;
            for (int t = 0; t < EM_T; ++t) gt.matched[(a * EM_T + t) * gt.pitch + k] = 0;
            if (!ig && l >= 0 && l <= num_classes) atomicAdd(&npig[a * (num_classes + 1) + l], 1);
        }
    }
}

// One task: the rows s_key[start .. end) of the label of s_key[start], in order, for area range at / EM_T and threshold at % EM_T.  Per row
// the image's g boxes of that label in two passes, the not ignored ones and then the ignored ones: that is the protocol's order "not
// ignored first, each group in annotation order", and its rule that a row matched to a counted box does not move on to an ignored one is
// "no second pass after a hit in the first".  RETAKE: a flagged box that a row took may be taken again (COCO's crowd boxes).  A row that
// takes no box is ignored when its own area lies outside the range or `unmatched_ignored` is set.  Task 0 writes the rank.
template <bool RETAKE>
__device__ __forceinline__ void em_walk(const u64* __restrict__ s_key, const int start, const int end, const int at, const float* __restrict__ d,
                                        const EvalMatchParams& prm, const EvalMatchGt& gt, const int g, const bool unmatched_ignored,
                                        const EvalMatchOut& out) {
    const int a = at / EM_T, t = at - a * EM_T;
    const int l = em_label(s_key[start]);
    const double lo = prm.lo[a], hi = prm.hi[a], best0 = fmin(prm.thr[t], 1.0 - 1e-10);
    const unsigned char* gig = gt.ignored + a * gt.pitch;
    unsigned char* matched = gt.matched + at * gt.pitch;
    signed char* m_out = out.match + at * out.plane + out.image;
    signed char* i_out = out.ignore + at * out.plane + out.image;
    for (int i = start; i < end; ++i) {
        const u64 key = s_key[i];
        if (key == EM_PAD || em_label(key) != l) break;
        const int row = em_row(key);
        if (at == 0) out.rank[out.image + row] = i - start;
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
                if (gt.label[k] != l || gig[k] != pass) continue;
                const bool again = RETAKE && gt.flag[k];
                if (matched[k] && !again) continue;
                const double v = coco_iou(dx, dy, dw, dh, gt.box + k * 4, again);
                if (v < best) continue;
                best = v, m = k;
            }
        if (m >= 0) {
            matched[m] = 1;
            m_out[row] = 1, i_out[row] = (signed char)gig[m];
        } else {
            m_out[row] = 0, i_out[row] = (da < lo || da > hi || unmatched_ignored) ? 1 : 0;
        }
    }
}
