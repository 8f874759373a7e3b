// Multi-level RoIAlignV2 (aligned=True, 7x7 bins, 2x2 samples) over NHWC fp16 pyramids.
//
// Replaces detectron2 ROIPooler(ROIAlignV2) as called at box_head.py:507/:617 (restated in
// oracle/roi_align.py).  HBM/L2-bound gather: one workgroup per box; 32 lanes x 8 channels
// (16-byte loads) cover the 256-channel vector of one tap, the 8 lane-groups of the block
// walk the 49 bins.  Output is [box][bin][channel] fp16 -- exactly the A operand of the
// DynamicConv batched matmul -- plus the optional fp32 mean over the 49 bins that RCNNHead
// uses as initial proposal features (box_head.py:509-510).  Coordinate math is fp32.
#include <stdlib.h>

#include "common.h"
#include "igemm_epilogue.h"
#include "kernels.h"
#include "roi_taps.h"

namespace {

using namespace roi_taps;

__global__ __launch_bounds__(256) void roialign_kernel(RoiLevels lv, const float* __restrict__ boxes, int boxes_per_img,
                                                        half_t* __restrict__ roi_out, float* __restrict__ mean_out, int nbox,
                                                        int xcd_major) {
    __shared__ float red[8][256];
    // an XCD takes one contiguous run of boxes, i.e. whole images: the boxes that gather from one image's pyramid meet in one L2
    // instead of pulling that image's lines into all eight (xcd_major = 0: round-robin, for A/B runs)
    const int box = xcd_major ? igemm_xcd_remap((int)blockIdx.x, nbox) : (int)blockIdx.x;
    const int tid = threadIdx.x;
    const int grp = tid >> 5, ln = tid & 31;
    float macc[8];
    gather_box(lv, boxes, boxes_per_img, box, grp, ln, macc,
               [&](int p, half8 o) { *reinterpret_cast<half8*>(roi_out + ((long)box * (P * P) + p) * (CV * 8) + ln * 8) = o; });
    if (mean_out) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[grp][ln * 8 + e] = macc[e];
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) s += red[g][tid];
        mean_out[(long)box * 256 + tid] = s / (P * P);
    }
}

// DTYPE float32: the same walk over fp32 pyramids with fp32 taps (roi_taps' axis taps and level choice; the bin geometry and the tap
// accumulation are written out here under contract(off), they round differently from the fp16 walk's v_fma_mix form)
__global__ __launch_bounds__(256) void f32_roialign_kernel(RoiLevels32 lv, const float* __restrict__ boxes, int boxes_per_img,
                                                            float* __restrict__ roi_out, float* __restrict__ mean_out, int nbox) {
#pragma clang fp contract(off)
    __shared__ float red[8][256];
    const int box = igemm_xcd_remap((int)blockIdx.x, nbox);
    const int img = box / boxes_per_img;
    const int tid = threadIdx.x;
    const int grp = tid >> 5, ln = tid & 31;
    const float bx1 = boxes[box * 4 + 0], by1 = boxes[box * 4 + 1], bx2 = boxes[box * 4 + 2], by2 = boxes[box * 4 + 3];
    bool valid_box;
    const int level = box_level(bx1, by1, bx2, by2, lv.min_level, valid_box);
    const int H = lv.h[level], W = lv.w[level];
    const float sc = lv.scale[level];
    const float* feat = lv.feat[level] + (long)img * H * W * 256;
    const float x1 = bx1 * sc - 0.5f, y1 = by1 * sc - 0.5f;
    const float x2 = bx2 * sc - 0.5f, y2 = by2 * sc - 0.5f;
    const float bin_w = (x2 - x1) / P, bin_h = (y2 - y1) / P;
    float macc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) macc[e] = 0.f;
    for (int pb = grp; pb < P * P; pb += 8) {
        const int ph = pb / P, pw = pb - ph * P;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        if (valid_box) {
#pragma unroll
            for (int iy = 0; iy < G; ++iy) {
                const float y = y1 + ph * bin_h + (iy + 0.5f) * bin_h / G;
                const Tap ty = axis_tap(y, H);
#pragma unroll
                for (int ix = 0; ix < G; ++ix) {
                    const float x = x1 + pw * bin_w + (ix + 0.5f) * bin_w / G;
                    const Tap tx = axis_tap(x, W);
                    if (!(ty.ok && tx.ok)) continue;
                    const float w4[4] = {ty.wl * tx.wl, ty.wl * tx.wh, ty.wh * tx.wl, ty.wh * tx.wh};
                    const long o4[4] = {(long)ty.lo * W + tx.lo, (long)ty.lo * W + tx.hi, (long)ty.hi * W + tx.lo, (long)ty.hi * W + tx.hi};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4v a = *reinterpret_cast<const float4v*>(feat + o4[q] * 256 + ln * 8);
                        const float4v b = *reinterpret_cast<const float4v*>(feat + o4[q] * 256 + ln * 8 + 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc[e] += w4[q] * a[e];
                            acc[4 + e] += w4[q] * b[e];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[e] *= 1.f / (G * G);
            macc[e] += acc[e];
        }
        float* o = roi_out + ((long)box * (P * P) + pb) * 256 + ln * 8;
        *reinterpret_cast<float4v*>(o) = (float4v){acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<float4v*>(o + 4) = (float4v){acc[4], acc[5], acc[6], acc[7]};
    }
    if (mean_out) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[grp][ln * 8 + e] = macc[e];
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) s += red[g][tid];
        mean_out[(long)box * 256 + tid] = s / (P * P);
    }
}

}  // namespace

int dvid_roialign_launch(const RoiLevels& lv, int channels, const float* boxes, int n_img, int boxes_per_img, half_t* roi_out,
                         float* mean_out, hipStream_t s) {
    if (channels != 256) return DVID_ERR_UNSUPPORTED;
    const int nbox = n_img * boxes_per_img;
    if (nbox == 0) return DVID_OK;
    hipLaunchKernelGGL(roialign_kernel, dim3(nbox), dim3(256), 0, s, lv, boxes, boxes_per_img, roi_out, mean_out, nbox, /*xcd_major=*/1);
    LAUNCH_CHECK();
    return DVID_OK;
}

int dvid_f32_roialign_launch(const RoiLevels32& lv, int channels, const float* boxes, int n_img, int boxes_per_img, float* roi_out,
                             float* mean_out, hipStream_t s) {
    if (channels != 256) return DVID_ERR_UNSUPPORTED;
    const int nbox = n_img * boxes_per_img;
    if (nbox == 0) return DVID_OK;
    hipLaunchKernelGGL(f32_roialign_kernel, dim3(nbox), dim3(256), 0, s, lv, boxes, boxes_per_img, roi_out, mean_out, nbox);
    LAUNCH_CHECK();
    return DVID_OK;
}
