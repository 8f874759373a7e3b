// Internal launcher declarations (C++), one per HIP kernel family.  The public C ABI is
// include/dvid_hip.h; these are what the runtime (runtime.h and its files) and the C-ABI op wrappers (ops_abi.hip) call.
#pragma once
#include "common.h"

struct IgemmParams {
    const half_t* in;    // NHWC fp16 [N,H,W,Cin]  (Linear: [M,K] as N=M, H=W=1, Cin=K)
    const half_t* w;     // [Cout][Kpad], k = (ky*KW + kx)*Cin + c
    const float* bias;   // [Cout] or nullptr
    const void* res;     // residual (fp16, or fp32 if res_f32), see res_mode
    void* out;           // [M][ldc] fp16 (or fp32 if out_f32)
    int H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
    int M, Kpad, ntaps, ldc, alg_k;
    int relu, out_f32, res_mode, res_f32;   // relu: 0 none, 1 ReLU, 2 exact GELU; res_mode: 0 none, 1 same shape, 2 nearest-x2 upsample
    int splitk;                             // > 1: K split over `splitk` workgroups per tile, fp32 partials (no bias/relu/residual)
    long split_stride;                      //       written to out + split * split_stride (elements)
    int tiles_m, tiles_n;                   // filled by the launcher
};
int dvid_igemm_launch(const IgemmParams& p, hipStream_t s);   // igemm2.hip: picks the kernel family (wstat / conv3x3 / igemm2) by the layer's shape
int dvid_igemm2_launch(const IgemmParams& p, hipStream_t s);  // igemm2.hip: the igemm2 kernel with its per-shape tuned tile configuration

// conv3x3.hip: 3x3 / stride-1 / pad-1 layers with the input patch + halo staged once per channel chunk (all nine taps read it)
bool dvid_conv3x3_halo_supported(const IgemmParams& p);   // the layer type fits the kernel
bool dvid_conv3x3_halo_preferred(const IgemmParams& p);   // ... and the shape rule (patch grid waste, patches per CU) picks it
int dvid_conv3x3_halo_launch(const IgemmParams& p, hipStream_t s);
// ... the space-to-depth stem + ReLU + 3x3 / stride-2 max pool as one launch (p.out = the pooled map); bit-identical to the two launches
bool dvid_stem_pool_supported(const IgemmParams& p);
int dvid_stem_pool_launch(const IgemmParams& p, hipStream_t s);

// wstat.hip: short-K / wide-N 1x1 layers with the weights stationary in registers (bit-identical to igemm2)
bool dvid_wstat_supported(const IgemmParams& p);
bool dvid_wstat_preferred(const IgemmParams& p);
int dvid_wstat_launch(const IgemmParams& p, hipStream_t s);

// bneck.hip: the tail of a res2 bottleneck block (conv2 3x3 64 -> 64, conv3 64 -> 256 + residual or shortcut convolution, ReLU and the
// next block's conv1 256 -> 64) as one launch; bit-identical to the layer-by-layer launches.  ws == null: the residual is `res`
// [rows][W][256]; else `res` is the 64-channel block input and the residual is its shortcut convolution.  w1n == null: no next conv1.
bool dvid_bneck64_tail_preferred(int H, int W);          // the shape rule (a function of the map size only), for either width
// 128-wide blocks (res3: 128 -> 128 -> 512; weights streamed through an LDS ring).  w2 == null: `t1` is the conv2 output (res3's first
// block, whose 3x3 / stride-2 conv2 runs as its own launch); w1n == null: no next conv1.  Bit-identical to the layer-by-layer launches
// on igemm2 (the chunked 3x3 patch kernel sums in another order).
int dvid_bneck128_tail_launch(const half_t* t1, const half_t* w2, const float* b2, const half_t* w3, const float* b3, const half_t* res,
                              const half_t* w1n, const float* b1n, half_t* out, half_t* t1n, int n, int H, int W, hipStream_t s);
int dvid_bneck64_tail_launch(const half_t* t1, const half_t* w2, const float* b2, const half_t* w3, const float* b3, const half_t* res,
                             const half_t* ws, const float* bs, const half_t* w1n, const float* b1n, int n_next, half_t* out, half_t* t1n,
                             int n, int H, int W, hipStream_t s);      // n_next: rows of w1n (64; 128 without a shortcut)

// elementwise.hip
// per-frame source pointers of one image-prep launch (passed by value as a kernel argument)
struct FrameTable {
    static constexpr int kMax = 32;
    const float* p[kMax];
};
// frames[i]: fp32 CHW [3, h, w] in [0, 1] of frame i (a host array of n device pointers; the frames need not be contiguous)
int dvid_prep_images_launch(const float* const* frames, half_t* nhwc8, int n, int h, int w, const float* mean, const float* inv_std,
                            hipStream_t s);
int dvid_prep_images_s2d_launch(const float* const* frames, half_t* s2d16, int n, int h, int w, const float* mean, const float* inv_std,
                                hipStream_t s);
int dvid_maxpool3x3s2_launch(const half_t* in, half_t* out, int n, int h, int w, int c, hipStream_t s);
int dvid_nchw_from_nhwc_launch(const half_t* in, float* out, int n, int h, int w, int c, hipStream_t s);
int dvid_nhwc_from_nchw_launch(const float* in, half_t* out, int n, int h, int w, int c, hipStream_t s);
// y = LN(x + r) * g + b, rows of D (= 256 or 64-multiple <= 1024); writes fp32 and/or fp16 copies
// x may be `nsplit` split-K partial slabs (x + s * split_stride) plus a per-column bias `xbias` (or nsplit 1, null)
int dvid_add_layernorm_launch(const float* x, const float* r, const float* g, const float* b, float* y32, half_t* y16,
                              int rows, int d, int relu, hipStream_t s, int nsplit = 1, long split_stride = 0,
                              const float* xbias = nullptr);
int dvid_f32_to_f16_launch(const float* x, half_t* y, long n, hipStream_t s);
int dvid_resize_u8_launch(const unsigned char* src, int h, int w, unsigned char* tmp, float* out, int oh, int ow, int ph, int pw,
                          const int* xbounds, const int* xk, int xksize, const int* ybounds, const int* yk, int yksize, hipStream_t s);
// n images, each by its own row of `plan` (resize.hip), -> out [n * (1 + flip)][3][ph][pw]; max_h: the tallest source with an x pass (0: none)
int dvid_resize_views_u8_launch(const unsigned char* const* srcs, int n, const long long* plan, const int* bounds, const int* kk,
                                unsigned char* tmp, float* out, int ph, int pw, int flip, int max_h, int max_ow, hipStream_t s);
// bboxaug.hip
int dvid_bbox_aug_merge_launch(const float* boxes, const float* scores, const int* labels, const int* counts, const float* table, int n, int V,
                               int cap, float* cand_boxes, float* cand_scores, int* cand_labels, int* live, hipStream_t s);
// overlay.hip: overlay_prepare_kernel (one workgroup per frame: select, sort, map, colour, text -> the frame's draw list in `lists`) and
// overlay_draw_kernel (one workgroup per tile and frame: cull, resolve, store); lists holds dvid_overlay_scratch_bytes_for(n) bytes
int dvid_overlay_launch(unsigned char* const* frames, const int* sizes, int n, int max_h, int max_w, const float* dets, const int* counts, int cap,
                        const float* ratios, const unsigned char* names, int num_classes, const unsigned char* atlas, int gh, int gw,
                        float threshold, int thickness, int text_scale, int* lists, hipStream_t s);
long long dvid_overlay_scratch_bytes_for(int n);
void dvid_overlay_tile_size(int* tw, int* th);
// jpeg.hip: jpeg_idct_kernel (8 lanes per 8x8 block -> uint8 component planes) and jpeg_colour_kernel (upsample + YCbCr -> RGB), n frames by
// the rows of `plan`; max_blocks: the most blocks any frame has over its components, max_w / max_h: the widest / tallest frame
int dvid_jpeg_reconstruct_launch(const short* coef, const unsigned short* quant, const long long* plan, int n, int max_blocks, int max_w, int max_h,
                                 unsigned char* planes, unsigned char* out, hipStream_t s);
// fc = x * (scale[frame] + 1) + shift  (shift per frame [B,D] or per row [R,D])
int dvid_modulate_launch(const float* x, const float* scale, int scale_ld, const float* shift, int shift_per_row, int shift_ld,
                         half_t* y16, int rows, int rows_per_frame, int d, hipStream_t s);
int dvid_silu_f16_launch(const float* x, half_t* y, long n, hipStream_t s);

// roialign.hip
template <typename T>          // the pyramid's maps, finest first: fp16 (RoiLevels) or fp32 (RoiLevels32).  Three levels p3..p5
struct RoiLevelsT {            // (min_level 3) or four, p2..p5 (min_level 2): index l is level min_level + l (runtime.h: roi_levels)
    const T* feat[4];
    int h[4], w[4];
    float scale[4];
    int min_level, n_levels;
};
using RoiLevels = RoiLevelsT<half_t>;
using RoiLevels32 = RoiLevelsT<float>;
int dvid_roialign_launch(const RoiLevels& lv, int channels, const float* boxes, int n_img, int boxes_per_img, half_t* roi_out,
                         float* mean_out, hipStream_t s);

// attention.hip: out[b][q][:] = softmax(Q K^T * scale) V per head on MFMA: fp16 q/k/v (head h at columns h*32..), fp16 out; vt_scratch >= batch*nheads*32*(round_up(lk,32)+32) halves
int dvid_mha_mfma_launch(const half_t* q, const half_t* k, const half_t* v, half_t* out, half_t* vt_scratch, int batch, int lq,
                         int lk, int nheads, int q_ld, int kv_ld, int out_ld, long q_bs, long kv_bs, long out_bs, hipStream_t s);

// localattn.hip: out = LayerNorm(x W^T + bias) over rows of d = 256 as one row kernel (the out-projection of the local box-level attention and
// the LayerNorm behind it, box_head.py:362-363); the pre-LayerNorm rows stay in registers.
struct OutProjLnParams {
    const void* x;          // [rows, 256]: fp16 (mode 0) or fp32 (modes 1, 2)
    int mode;               // 0: fp16 MFMA; 1: fp32 rows as split (hi, lo) fp16 operands, three fp16-MFMA passes; 2: fp32 MFMA
    const half_t* wf_hi;    // [256][256] in MFMA fragment order (weights.hip: make_frags): the fp16 weights (mode 0) / the hi plane (mode 1)
    const half_t* wf_lo;    // mode 1: the lo plane, same order
    const float* w32;       // mode 2: the scaled fp32 rows [256][256]
    const float* wscale;    // modes 1, 2: [256], channel n's sum is multiplied by wscale[n]
    const float* bias;      // [256]
    const float* gamma;     // LayerNorm weight / bias [256]
    const float* beta;
    float* out;             // [rows, 256] fp32
    int rows, d;
    int* range_flag;        // mode 1: device int or null, ORed with 1 when a row value exceeds the fp16 range
};
int dvid_outproj_ln_launch(const OutProjLnParams& p, hipStream_t s);

constexpr int SWIN_RELBIAS_PITCH = 64;     // floats per query row of the relative-position bias table [heads][49][64] (keys 49..63 = 0)
int dvid_swin_window_attn_launch(const half_t* qkv, const half_t* qkv_bias16, const float* relbias, half_t* out, int batch, int H,
                                 int W, int C, int nheads, int shift, hipStream_t s);
// 12 x 12 windows (144 tokens, shift 0 or 6): relbias [heads][144][160] (keys 144..159 = 0)
constexpr int SWIN12_RELBIAS_PITCH = 160;
int dvid_swin_window12_attn_launch(const half_t* qkv, const half_t* qkv_bias16, const float* relbias, half_t* out, int batch, int H,
                                   int W, int C, int nheads, int shift, hipStream_t s);
int dvid_patch_merge_ln_launch(const float* x, const float* g, const float* b, half_t* y16, int B, int H, int W, int C, hipStream_t s,
                               float* y32 = nullptr);          // y32: an fp32 copy of the result (DTYPE float32: y16 null)

// dynconv.hip
int dvid_dynconv_launch(const half_t* roi, const half_t* params, const float* g1, const float* b1, const float* g2,
                        const float* b2, half_t* out, int rows, hipStream_t s);
// RoIAlign gathered straight into DynamicConv's LDS tile (csrc/dynconv.hip, FUSED_ROI): bit-identical to dvid_roialign_launch + dvid_dynconv_launch
int dvid_dynconv_roi_launch(const RoiLevels& lv, int channels, const float* boxes, int n_img, int boxes_per_img, const half_t* params,
                            const float* g1, const float* b1, const float* g2, const float* b2, half_t* out, hipStream_t s);

// headtail.hip: FFN + norm3 + modulation + cls / reg towers + class_logits + bboxes_delta + apply_deltas of one RCNNHead pass as one
// row-tile kernel.  Every `*f` weight is in MFMA fragment order (weights.hip: make_frags): [n-tile of 32 rows][K step of 16][lane][8].
struct HeadTailParams {
    const half_t* x16;          // [R, 256] fp16   norm2 output (operand of linear1)
    const float* obj32;         // [R, 256] fp32   the same rows, the FFN's residual
    const half_t* w1f;          // linear1 [dff][256]
    const float* b1;
    const half_t* w2f;          // linear2 [256][dff]
    const float* b2;
    const float* n3g;           // norm3
    const float* n3b;
    const float* scale;         // block_time_mlp rows: scale (and, plain head, shift at + 256) of frame f at scale + f * ss_stride
    int ss_stride, rows_per_frame;
    const float* cond32;        // [R, 256] fp32 or null (RCNNHead_cond: shift = c_mlp(SiLU(cond)))
    const half_t* wcf;          // c_mlp.1 [256][256]
    const float* bc;
    int num_cls, num_reg, num_classes, dff;
    const half_t* clsf[4];
    const float* clsg[4];
    const float* clsb[4];
    const half_t* regf[4];
    const float* regg[4];
    const float* regb[4];
    const half_t* wlogf;        // class_logits, rows zero-padded to a multiple of 32
    const float* blog;
    const half_t* wdelf;        // bboxes_delta, 4 rows zero-padded to 32
    const float* bdel;
    const float* boxes;         // [R, 4] input boxes
    float* obj_out;             // [R, 256] fp32 obj_features
    float* logits;              // [R, num_classes]
    float* boxes_out;           // [R, 4]
    int* bad_flag;
    long R;
    float wx, wy, ww, wh, clamp;
};
bool dvid_head_tail_supported(int hidden, int dff, int num_cls, int num_reg, int num_classes);
int dvid_head_tail_launch(const HeadTailParams& p, hipStream_t s);

// headtail_bwd.hip: the tail's fp32 recompute and its backward (include/dvid_hip.h: dvid_head_tail_backward states the arguments)
struct HeadTailBwdArgs {
    const float *x, *boxes_in, *time_emb, *cond;
    int n, m, dff, num_classes, num_cls, num_reg;
    const float* const* params;
    float wx, wy, ww, wh, scale_clamp;
    const float *d_logits, *d_boxes, *d_obj;
    float *logits_out, *boxes_out, *obj_out;
    float *d_x, *d_time_emb, *d_cond;
    float* const* grads;          // null: the forward only
    void* scratch;
};
long long dvid_head_tail_backward_scratch_bytes_host(int n, int m, int dff, int num_classes, int num_cls, int num_reg, int has_cond);
int dvid_head_tail_backward_launch(const HeadTailBwdArgs& a, hipStream_t s);

// interact_bwd.hip: the fp32 recompute of DynamicConv + norm2 and its backward (include/dvid_hip.h: dvid_inst_interact_backward)
struct InstInteractBwdArgs {
    const float *p, *roi;
    long long rows;
    const float* const* params;
    const float* d_y;
    float *y_out, *d_p, *d_roi;
    float* const* grads;          // null: the forward only
    void* scratch;
};
long long dvid_inst_interact_backward_scratch_bytes_host(long long rows);
int dvid_inst_interact_backward_launch(const InstInteractBwdArgs& a, hipStream_t s);

// selfattn_bwd.hip: the fp32 recompute of self-attention + norm1 and its backward (include/dvid_hip.h: dvid_self_attn_backward)
struct SelfAttnBwdArgs {
    const float* x;
    int n, m;
    const float* const* params;
    const float* d_y;
    float *y_out, *d_x;
    float* const* grads;          // null: the forward only
    void* scratch;
};
long long dvid_self_attn_backward_scratch_bytes_host(long long n, long long m);
int dvid_self_attn_backward_launch(const SelfAttnBwdArgs& a, hipStream_t s);

// boxes.hip
int dvid_apply_deltas_launch(const float* deltas, int delta_ld, const float* boxes, float* out, int n, float wx, float wy, float ww,
                             float wh, float clamp, int* bad_flag, hipStream_t s);
int dvid_counter_normal_launch(float* out, long per_image, int n_images, uint64_t key0, hipStream_t s, uint64_t key_stride = 1);          // image i: key0 + i * key_stride
int dvid_noise_to_boxes_launch(const float* x, float* boxes, int n, float scale, float w, float h, hipStream_t s);
// the per-frame forms (`sizes`: device fp32 [n_frames][2] = (w, h) of each frame, every entry positive and finite) of the size-dependent
// kernels: the same kernels instantiated over FrameSizeTable (common.h).  noise_to_boxes: n boxes, m per frame
int dvid_noise_to_boxes_sizes_launch(const float* x, float* boxes, int n, int m, float scale, const float* sizes, hipStream_t s);
int dvid_ddim_renew_sizes_launch(const float* logits, const float* boxes, const float* xt, const float* noise, const float* fresh,
                                 float* out, int n_img, int m, int c, const float* sizes, float scale, float sra, float srm1, float sqrt_an,
                                 float cc, float sigma, float thr, hipStream_t s);
int dvid_topk_mask_launch(const float* logits, int n_img, int m, int c, int k1, int k2, const float* feats, int d, float* out1,
                          float* out2, hipStream_t s);

int dvid_ddim_renew_launch(const float* logits, const float* boxes, const float* xt, const float* noise, const float* fresh,
                           float* out, int n_img, int m, int c, float w, float h, float scale, float sra, float srm1, float sqrt_an,
                           float cc, float sigma, float thr, hipStream_t s);

// criterion.hip
int dvid_q_sample_boxes_launch(const float* gt, const int* gt_starts, int n, int m, const int* t, const float* sqrt_ac, const float* sqrt_omac,
                               int timesteps, const float* noise, const float* placeholder, float scale, const float* sizes, float* out, hipStream_t s);
long long dvid_set_criterion_scratch_bytes_host(int n_sets, int n, int m, int gmax);
int dvid_set_criterion_launch(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes, const int* gt_labels,
                              const int* gt_starts, const float* sizes, float alpha, float gamma, int ota_k, float cost_class, float cost_bbox,
                              float cost_giou, int* assign, int* matched_query, int gmax, double* sums, int* status, void* scratch, hipStream_t s);
int dvid_set_criterion_backward_launch(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes,
                                       const int* gt_labels, const int* gt_starts, const float* sizes, float alpha, float gamma, const int* assign,
                                       const int* status, const double* coef, float* d_logits, float* d_boxes, hipStream_t s);

// postproc.hip
int dvid_topk_candidates_launch(const float* logits, const float* boxes, int n_img, int nsets, int m, int c, float* cand_boxes,
                                float* cand_scores, int* cand_labels, hipStream_t s);
// the streaming form of the same selection (topk_stream_kernel), forced at any 1 <= m <= DVID_NMS_MAX_CANDIDATES, 1 <= c <= DVID_MAX_CLASSES;
// dvid_topk_candidates_launch takes it for the shapes its two LDS forms do not hold
int dvid_topk_stream_launch(const float* logits, const float* boxes, int n_img, int nsets, int m, int c, float* cand_boxes,
                            float* cand_scores, int* cand_labels, hipStream_t s);
int dvid_nms_frames_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, float img_w,
                           float img_h, float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels,
                           int* out_counts, hipStream_t s);
// the tiled form of the same step (nms_tiled_*_kernel): any 1 <= n <= DVID_NMS_MAX_CANDIDATES; `scratch` holds dvid_nms_tiled_scratch_size bytes
bool dvid_nms_frames_fits_lds(int n);          // nms_frame_kernel holds n candidates in LDS: THE dispatch rule between the two forms
size_t dvid_nms_tiled_scratch_size(int n_img, int n);
int dvid_nms_frames_tiled_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, float img_w,
                                 float img_h, float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels,
                                 int* out_counts, void* scratch, hipStream_t s);
// ... and with the clip of frame f to sizes[f] (see boxes.hip above)
int dvid_nms_frames_sizes_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n, const float* sizes,
                                 float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels, int* out_counts,
                                 hipStream_t s);
int dvid_nms_frames_tiled_sizes_launch(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_img, int n,
                                       const float* sizes, float iou, int use_nms, int out_cap, float* out_boxes, float* out_scores,
                                       int* out_labels, int* out_counts, void* scratch, hipStream_t s);

// seqnms.hip: Seq-NMS over videos, a workgroup per (video, class); class_counts / video_starts are host tables (include/dvid_hip.h)
long long dvid_seq_nms_scratch_size(const int* class_counts, const int* video_starts, int n_videos, int num_classes);
int dvid_seq_nms_launch(const float* dets, const int* counts, const int* class_counts, const int* video_starts, int n_videos, int cap, int num_classes,
                        unsigned char* keep, float* scores, int* status, void* scratch, hipStream_t s);

// The evaluators.  evalmatch.h holds the device code they share (the sort key, the bitonic sort, the segment heads; for COCO and LVIS also the
// IoU, the ground-truth load and the walk of one task), evalkey.h the score's key bits.
// videval.hip: the VID evaluator's greedy matching and CorLoc test, a workgroup per frame; ranges / empty_w are host tables (include/dvid_hip.h)
int dvid_vid_eval_match_launch(const float* dets, const int* counts, int n_frames, int cap, const float* gt_boxes, const int* gt_labels,
                               const int* gt_starts, const double* motion, const double* ranges, const double* empty_w, int n_ranges, float iou_thresh,
                               int num_classes, signed char* match, double* weight, int* rank, double* n_pos, int* top_row, signed char* top_hit,
                               hipStream_t s);

// cocoeval.hip: the COCO bbox evaluator's matching, a workgroup per image; iou_thrs / area_ranges are host tables (include/dvid_hip.h)
int dvid_coco_eval_match_launch(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                                const unsigned char* gt_crowd, const int* gt_labels, const int* gt_starts, const double* iou_thrs,
                                const double* area_ranges, int num_classes, signed char* match, signed char* ignore, int* rank, int* npig,
                                hipStream_t s);

// lviseval.hip: the LVIS (federated) bbox evaluator's matching, a workgroup per image; max_gt is the greatest box count of one image, read
// from the host's gt_starts; iou_thrs / area_ranges are host tables (include/dvid_hip.h)
int dvid_lvis_eval_match_launch(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                                const unsigned char* gt_ignore, const int* gt_labels, const int* gt_starts, int max_gt, const int* neg_starts,
                                const int* neg_labels, const int* nex_starts, const int* nex_labels, const double* iou_thrs,
                                const double* area_ranges, int num_classes, signed char* match, signed char* ignore, int* rank, int* npig,
                                hipStream_t s);

// evalaccum.hip: the COCO / LVIS evaluators' accumulation (precision and recall with numpy's bits); max_dets / rec_thrs are host tables,
// the scratch is dvid_eval_accumulate_scratch_size(...) bytes (-1: bad sizes); every argument is checked by the caller (ops_abi.hip)
long long dvid_eval_accumulate_scratch_size(int n_images, int cap, int max_dets_count);
int dvid_eval_accumulate_launch(const float* dets, const int* counts, const int* rank, const signed char* match, const signed char* ignore,
                                const int* npig, int n_images, int cap, int num_classes, const int* max_dets, int max_dets_count,
                                const double* rec_thrs, double* precision, double* recall, void* scratch, hipStream_t s);

// fps.hip
int dvid_cdist_launch(const float* x, int n, int d, float* dist, hipStream_t s);
int dvid_fps_launch(const float* dist, int n, int m, int bs_emul, int* idx, hipStream_t s);
int dvid_gather_rows_launch(const float* x, const int* idx, float* y, int m, int d, hipStream_t s);
// `groups` problems of one shape per launch, each computed as the single form computes it
int dvid_cdist_groups_launch(const float* x, int groups, int n, int d, float* dist, hipStream_t s);
int dvid_fps_groups_launch(const float* dist, int groups, int n, int m, int bs_emul, int* idx, hipStream_t s);
int dvid_gather_rows_groups_launch(const float* x, const int* idx, float* y, int groups, int n, int m, int d, hipStream_t s);

// DTYPE float32 (fp32 storage, fp32-grade products).  f32.hip: the implicit GEMM of every convolution and linear layer -- exact fp32 products
// on v_mfma_f32_32x32x2_f32, or split (hi, lo) fp16 operands on three passes of the fp16 MFMA (f32_split.h)
struct F32GemmParams {
    const float* in;     // NHWC fp32 [N,H,W,Cin], Cin % 4 == 0  (Linear: [M,K] as N = M, H = W = 1, Cin = K)
    const float* w;      // [Cout][Kpad], k = (ky*KW + kx)*Cin + c, zero beyond K; Kpad % 16 == 0
    const half_t* w_hi;  // the same rows split for the split-operand kernel: w_hi = fp16(w), w_lo = fp16(w - w_hi) (null: the fp32-MFMA kernel runs)
    const half_t* w_lo;
    const float* bias;   // [Cout] or nullptr
    int* range_flag;     // device int or nullptr: the split-operand kernel ORs 1 into it when an activation's magnitude exceeds the fp16 range (65504)
    const float* wscale; // [Cout] or nullptr: the accumulator of channel n is multiplied by wscale[n] (undoes a power-of-two scaling of the packed row)
    const float* res;    // fp32 residual, see res_mode
    float* out;          // [M][ldc]
    int H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
    int M, K, Kpad, ldc;
    int relu, res_mode;  // relu: 0 none, 1 ReLU, 2 exact GELU; res_mode: 0 none, 1 same shape, 2 nearest-x2 upsample
    int tiles_m, tiles_n;   // filled by the launcher
};
int dvid_f32_igemm_launch(const F32GemmParams& p, hipStream_t s);
// csrc/f32_wstat.hip: the weight-stationary form of the split-operand kernel (bit-identical to it)
bool dvid_f32_wstat_supported(const F32GemmParams& p);
bool dvid_f32_wstat_preferred(const F32GemmParams& p);
int dvid_f32_wstat_tile_rows(const F32GemmParams& p);
int dvid_f32_wstat_launch_tiles(const F32GemmParams& p, hipStream_t s);
// csrc/f32_conv3x3.hip: 3x3 / stride-1 layers with the halo staged and split once per channel chunk (another summation order than the tiled kernel)
bool dvid_f32_conv3x3_supported(const F32GemmParams& p);
int dvid_f32_conv3x3_launch(const F32GemmParams& p, hipStream_t s);
// the other float32 kernels stand beside their fp16 siblings.  elementwise.hip:
int dvid_f32_prep_images_launch(const float* const* frames, float* nhwc4, int n, int h, int w, const float* mean, const float* std_, hipStream_t s);
int dvid_f32_maxpool3x3s2_launch(const float* in, float* out, int n, int h, int w, int c, hipStream_t s);
int dvid_f32_silu_launch(const float* x, float* y, long n, hipStream_t s);
int dvid_f32_modulate_launch(const float* x, const float* scale, int scale_ld, const float* shift, int shift_per_row, int shift_ld, float* y,
                             int rows, int rows_per_frame, int d, hipStream_t s);
// roialign.hip
int dvid_f32_roialign_launch(const RoiLevels32& lv, int channels, const float* boxes, int n_img, int boxes_per_img, float* roi_out,
                             float* mean_out, hipStream_t s);
// attention.hip: q / k / v fp32 with head h at columns [32 h, 32 h + 32) of a row (head dim 32)
int dvid_f32_mha_launch(const float* q, const float* k, const float* v, float* out, int batch, int lq, int lk, int nheads, int q_ld, int kv_ld,
                        int out_ld, long q_bs, long kv_bs, long out_bs, hipStream_t s);
// Swin window attention (shift + 7 x 7 windows + relative-position bias + region mask), fp32: qkv [B*H*W][3C], qkv_bias [3C] (q / k / v of a
// padded window position), relbias [nheads][49][SWIN_RELBIAS_PITCH], out [B*H*W][C]
int dvid_f32_swin_window_attn_launch(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                                     int nheads, int shift, hipStream_t s);
// the same with 12 x 12 windows: relbias [nheads][144][SWIN12_RELBIAS_PITCH]
int dvid_f32_swin_window12_attn_launch(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                                       int nheads, int shift, hipStream_t s);
// dynconv.hip: roi [R][49][256], params [R][32768] as P1T[64][256] | P2T[256][64], out [R][49][256]; range_flag (device int or null): the split-operand
// form ORs 1 into it when a RoI / parameter magnitude exceeds the fp16 range
int dvid_f32_dynconv_launch(const float* roi, const float* params, const float* g1, const float* b1, const float* g2, const float* b2,
                            float* out, int rows, int* range_flag, hipStream_t s);
