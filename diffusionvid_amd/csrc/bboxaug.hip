// TEST.BBOX_AUG: the detections of the V views of every still image, mapped into view 0's frame and packed as the candidate lists of the
// tiled NMS (mega_core/engine/bbox_aug.py: im_detect_bbox_aug's add_preds_t + torch.cat; im_detect_bbox_hflip's transpose(0)).
//
// in   boxes [n * V][cap][4], scores, labels [n * V][cap], counts [n * V] as postproc_topk_nms leaves them, slot i * V + v = view v of image i;
//      table fp32 [n * V][5] = (w_v, h_v, flip, rw, rh): the view's size and the fp32 multipliers w0 / w_v, h0 / h_v toward view 0
// out  cand_boxes [n][V * cap][4], cand_scores, cand_labels [n][V * cap]: the live rows in (view, row) order, behind them the padding of
//      engine.inference.seq_nms_boxlists (a zero-area box at the origin, the smallest normal score, label 1: it neither suppresses nor is
//      suppressed, sorts behind every detection and leaves the NMS's class offset alone); live [n] = the image's live rows
// The arithmetic is BoxList's, one fp32 operation at a time: a mirrored view takes x1' = (w_v - x2) - 1, x2' = (w_v - x1) - 1
// (transpose(FLIP_LEFT_RIGHT)), then every corner is multiplied by its axis' ratio (resize; with rw == rh the reference multiplies all
// four numbers by rw, which is the same product).  View 0 is copied.  One workgroup per image; byte work, a few KiB per image.
#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kMaxViews = 64;

__global__ __launch_bounds__(256) void bbox_aug_merge_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int* __restrict__ labels, const int* __restrict__ counts,
                                                             const float* __restrict__ table, int V, int cap, float* __restrict__ cand_boxes,
                                                             float* __restrict__ cand_scores, int* __restrict__ cand_labels, int* __restrict__ live) {
    __shared__ int start[kMaxViews + 1];
    const int img = blockIdx.x, N = V * cap;
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int v = 0; v < V; ++v) {
            start[v] = acc;
            const int c = counts[img * V + v];
            acc += c < 0 ? 0 : (c > cap ? cap : c);          // a count outside [0, cap] cannot move a write out of the image's rows
        }
        start[V] = acc;
        live[img] = acc;
    }
    __syncthreads();
    float4* ob = reinterpret_cast<float4*>(cand_boxes) + (long)img * N;
    float* os = cand_scores + (long)img * N;
    int* ol = cand_labels + (long)img * N;
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        const int v = j / cap, r = j - v * cap;
        if (r >= start[v + 1] - start[v]) continue;
        const long slot = (long)img * V + v;
        float4 b = reinterpret_cast<const float4*>(boxes)[slot * cap + r];
        if (v > 0) {
            const float* t = table + slot * 5;
            if (t[2] != 0.f) {
                const float w = t[0];
                const float x1 = __fsub_rn(__fsub_rn(w, b.z), 1.f), x2 = __fsub_rn(__fsub_rn(w, b.x), 1.f);
                b.x = x1;
                b.z = x2;
            }
            b.x = __fmul_rn(b.x, t[3]);
            b.y = __fmul_rn(b.y, t[4]);
            b.z = __fmul_rn(b.z, t[3]);
            b.w = __fmul_rn(b.w, t[4]);
        }
        const int dst = start[v] + r;
        ob[dst] = b;
        os[dst] = scores[slot * cap + r];
        ol[dst] = labels[slot * cap + r];
    }
    for (int j = start[V] + threadIdx.x; j < N; j += blockDim.x) {
        ob[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        os[j] = FLT_MIN;
        ol[j] = 1;
    }
}

}  // namespace

int dvid_bbox_aug_merge_launch(const float* boxes, const float* scores, const int* labels, const int* counts, const float* table, int n, int V,
                               int cap, float* cand_boxes, float* cand_scores, int* cand_labels, int* live, hipStream_t s) {
    if (n <= 0 || V < 1 || V > kMaxViews || cap < 1) return DVID_ERR_ARG;
    hipLaunchKernelGGL(bbox_aug_merge_kernel, dim3(n), dim3(256), 0, s, boxes, scores, labels, counts, table, V, cap, cand_boxes, cand_scores,
                       cand_labels, live);
    LAUNCH_CHECK();
    return DVID_OK;
}
