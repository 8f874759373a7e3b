/* libdvid_hip -- MI355X (gfx950) native DiffusionVID inference hot path, C ABI.
 *
 * Drop-in boundary for the reference's per-batch compute (sdroh1027/DiffusionVID).  Every entry
 * point takes plain device/host pointers and sizes, enqueues work on the HIP stream given
 * (`stream` = hipStream_t, NULL = default stream), performs no hidden synchronisation and returns
 * 0 on success (see DVID_* codes; dvid_last_error() has the text).  The Python host side
 * (diffusionvid_amd/) binds these with ctypes on torch `data_ptr()`s; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Reference interfaces replaced (paths relative to the reference repo root):
 *   dvid_backbone_resnet_fpn   detectron2 build_resnet_fpn_backbone called at
 *                              mega_core/modeling/detector/diffusion_det.py:219,:427 (+ normalizer :301-303,:422)
 *   dvid_backbone_swin_fpn     build_swintransformer_fpn_backbone, mega_core/modeling/backbone/swintransformer.py:464-751
 *   dvid_rcnn_head             RCNNHead.forward / RCNNHead_cond.forward, DynamicConv.forward, apply_deltas
 *                              mega_core/modeling/roi_heads/box_head/box_head.py:495-548, :605-664, :687-711, :550-590
 *   dvid_roialign_v2_multilevel detectron2 ROIPooler(ROIAlignV2) built at box_head.py:250-271, called :507,:617
 *   dvid_global_xattn          nn.MultiheadAttention global stage, box_head.py:366-380
 *   dvid_local_xattn           nn.MultiheadAttention + LayerNorm of the local box-level stage, box_head.py:186-194, :360-363
 *   dvid_select_topk_features  box_head.py:304-317
 *   dvid_noise_to_boxes        diffusion_det.py:657-660
 *   dvid_counter_normal        torch.randn(shape, device=self.device) at diffusion_det.py:449, :542, :587, :595
 *   dvid_ddim_renew_step       box renewal + DDIM update, diffusion_det.py:559-596
 *   dvid_postproc_topk_nms     DiffusionDet.inference + detectron2 batched_nms + BoxList.clip_to_image
 *                              diffusion_det.py:754-839, :607-627; structures/bounding_box.py:214-224
 *   dvid_cdist / dvid_fps_greedy / dvid_gather_rows
 *                              update_erase_memory / select_farthest_k_greedy_cuda, diffusion_det.py:841-896;
 *                              mega_core/csrc/fps.h:15-36 + csrc/cuda/fps.cu:25-185 (`_C.furthest_point_sampling`)
 *   dvid_model_set_tensor      DetectronCheckpointer.load name contract, mega_core/utils/model_serialization.py:12-73
 *
 * Layouts: images fp32 NCHW in [0,1] (what the reference model receives); feature maps fp16 NHWC
 * (channels fastest; fp32 NHWC with DTYPE float32, dvid_model_set_precision); boxes fp32 xyxy absolute pixels; object features
 * fp32 [rows, hidden].
 */
#ifndef DVID_HIP_H
#define DVID_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVID_OK 0
#define DVID_ERR_ARG 1
#define DVID_ERR_HIP 2
#define DVID_ERR_UNSUPPORTED 3
#define DVID_ERR_STATE 4

/* The largest MODEL.DiffusionDet.NUM_CLASSES a model is created with (DVID_ERR_UNSUPPORTED beyond): LVIS's 1203 rounded up to whole
 * 64-row tiles of class_logits; COCO's 80 and Objects365's 365 lie inside.  Up to 64 classes the head's tail runs as one fused kernel
 * (csrc/headtail.hip); above it class_logits and the layers in front of it run layer by layer, in both precisions.  The logits of one
 * head output take n_frames * boxes_per_frame * num_classes * 4 bytes: 0.44 GB for 304 frames of 300 boxes at 1203 classes. */
#define DVID_MAX_CLASSES 1280

typedef struct dvid_model dvid_model;

typedef struct dvid_config {
    int hidden_dim;        /* MODEL.DiffusionDet.HIDDEN_DIM      (256) */
    int nheads;            /* MODEL.DiffusionDet.NHEADS          (8)   */
    int dim_feedforward;   /* MODEL.DiffusionDet.DIM_FEEDFORWARD (2048) */
    int dim_dynamic;       /* MODEL.DiffusionDet.DIM_DYNAMIC     (64)  */
    int num_classes;       /* MODEL.DiffusionDet.NUM_CLASSES     (30)  1 .. DVID_MAX_CLASSES */
    int num_cls;           /* MODEL.DiffusionDet.NUM_CLS         (1)   */
    int num_reg;           /* MODEL.DiffusionDet.NUM_REG         (3)   */
    int num_heads;         /* MODEL.DiffusionDet.NUM_HEADS       (3)   head_series */
    int num_heads_cond;    /* MODEL.DiffusionDet.NUM_HEADS_LOCAL (1)   head_series_cond */
    int pooler_resolution; /* MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION (7) */
    int sampling_ratio;    /* MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO (2) */
    int res_blocks[4];     /* bottleneck blocks per stage, {3,4,23,3} for R-101; all 0 = no backbone */
    float pixel_mean[3];   /* MODEL.PIXEL_MEAN (0..255 scale) */
    float pixel_std[3];
    int backbone_type;     /* 0: ResNet-FPN (res_blocks), 1: Swin-FPN (swin_*), MODEL.BACKBONE.NAME */
    int swin_embed_dim;    /* size2config[MODEL.SWIN.SIZE]: 128 for B */
    int swin_depths[4];    /* {2,2,18,2} */
    int swin_heads[4];     /* {4,8,16,32}; head dim must be 32 */
    int swin_window;       /* 7, or 12 for the 384-pretrained sizes (B-22k-384, L-22k-384) */
} dvid_config;

const char* dvid_last_error(void);
int dvid_version(void);

/* ---- model: weights (host fp32 in, repacked fp16 on device) + workspace ---------------------- */
int dvid_model_create(const dvid_config* cfg, dvid_model** out);
int dvid_model_destroy(dvid_model* m);
/* state_dict entry, reference parameter names ("backbone.bottom_up.res2.0.conv1.weight",
 * "head.head_series.0.inst_interact.dynamic_layer.weight", ...); data is copied. */
int dvid_model_set_tensor(dvid_model* m, const char* name, const float* data, const int64_t* shape, int ndim);
/* The reference's global DTYPE switch (mega_core/config/defaults.py:582, default "float32"; tools/test_net.py:97-98 turns apex amp on for
 * "float16" only): precision 0 = DTYPE float16 -- fp16 weights / stored activations, fp16 MFMA, fp32 accumulation (the apex O1 policy);
 * precision 1 = DTYPE float32 -- every weight and activation fp32, products on the fp32 MFMA (csrc/f32.hip; both backbones).  Feature maps handed to / taken from the stage functions below are fp16 NHWC in mode 0 and fp32 NHWC in
 * mode 1.  Must be called before dvid_model_finalize (the weights are packed for one precision); the default is 0. */
int dvid_model_set_precision(dvid_model* m, int precision);
/* precision 1 with library option f32_split = 1 (default) multiplies (hi, lo) fp16 pairs: an ACTIVATION whose magnitude exceeds the fp16 range
 * (65504) cannot be split, and its products would be inf / NaN where fp32 arithmetic is finite.  Such a launch sets a device flag instead of
 * failing silently; this call copies it to *exceeded (synchronising `stream`) and clears it.  The detector reads it at each batch's host
 * synchronisation and raises, naming f32_split = 0 (the fp32 MFMA, no range limit) as the remedy.  Always 0 for precision 0. */
int dvid_model_take_range_flag(dvid_model* m, int* exceeded, void* stream);
/* fold FrozenBN, repack to MFMA operand layouts, upload.  Fails (DVID_ERR_STATE) naming the first
 * missing tensor. */
int dvid_model_finalize(dvid_model* m);
/* (re)allocate the activation workspace for batches of up to max_frames frames of height x width
 * (multiples of 32) and boxes_per_frame boxes. */
int dvid_workspace_reserve(dvid_model* m, int max_frames, int height, int width, int boxes_per_frame);
/* Counts the MOVES of this model's workspace buffers (dvid_workspace_reserve growing the arena, dvid_global_memory_project /
 * dvid_global_xattn / dvid_local_memory_project / dvid_local_xattn growing the memories' projection buffers; a buffer's first allocation does not count: nothing can hold its address yet).
 * A caller that captured launches into a hipGraph holds addresses inside the workspace; when the counter differs from its value at
 * capture time the graph must be dropped.  Per model: another model's growth leaves this one's graphs alone.
 * (The reference has no counterpart: its workspace is torch's caching allocator, mega_core/modeling/detector/diffusion_det.py:418-476.) */
unsigned long long dvid_workspace_generation(const dvid_model* m);

/* Number of concurrent sub-batch chains (separate HIP streams inside the library, joined back to the caller's
 * stream before returning) used by the backbone and the heads; 1 = strictly sequential kernels (profiling). */
int dvid_set_chains(dvid_model* m, int nchain);

/* ResNet stem: 1 (default) = the 7x7 / stride-2 convolution runs as a 4x4 / stride-1 convolution over the 2x2 space-to-depth image
 * (16 channels per block, K = 256 packed columns); 0 = over the NHWC8 image (K = 448).  Same products, different summation order. */
int dvid_set_stem_layout(dvid_model* m, int space_to_depth);

/* ---- stages -------------------------------------------------------------------------------- */
/* images: fp32 NCHW [n,3,height,width] in [0,1] (zero padded, un-normalised).  Outputs fp16 NHWC
 * p3 [n,h/8,w/8,256], p4 [n,h/16,w/16,256], p5 [n,h/32,w/32,256]. */
int dvid_backbone_resnet_fpn(dvid_model* m, const float* images, int n, int height, int width, void* p3, void* p4, void* p5,
                             void* stream);
/* The same with the frames as a host array of n device pointers, each an fp32 CHW [3, height, width] frame: the reference hands
 * the detector a list of per-frame tensors and concatenates them (diffusion_det.py:418-421); here nothing is copied. */
int dvid_backbone_resnet_fpn_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* p3, void* p4, void* p5,
                                    void* stream);

/* Swin-Transformer + FPN (mega_core/modeling/backbone/swintransformer.py:464-751, out_indices (1,2,3)); same
 * inputs/outputs as dvid_backbone_resnet_fpn. */
int dvid_backbone_swin_fpn(dvid_model* m, const float* images, int n, int height, int width, void* p3, void* p4, void* p5,
                           void* stream);
int dvid_backbone_swin_fpn_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* p3, void* p4, void* p5,
                                  void* stream);

/* The pyramid as an array (detectron2 FPN.forward over MODEL.FPN.IN_FEATURES, bottom level last; the reference's default node,
 * diffusion_det.py:155-159, runs it over res2..res5, its configs/vid_*.yaml over res3..res5).  A model HAS THE p2 LEVEL when the tensor
 * backbone.fpn_lateral2.weight was set before dvid_model_finalize; it then also needs backbone.fpn_lateral2.bias and
 * backbone.fpn_output2.weight / .bias, a Swin model backbone.bottom_up.norm0.weight / .bias (out_indices (0,1,2,3)) as well, and the
 * finalize fails with DVID_ERR_STATE naming the first one missing.  Its workspace holds res2's (Swin: stage 0's) output and a fourth
 * lateral map per frame.
 * levels: host array of n_levels output pointers, levels[0] the finest: 3 = p3, p4, p5 as above; 4 = p2 [n,h/4,w/4,256] in front of
 * them.  n_levels must be the model's count (DVID_ERR_ARG otherwise, nothing is written).  The three-pointer entries above are these
 * with n_levels 3, and a model with the p2 level answers them with DVID_ERR_STATE. */
int dvid_backbone_resnet_fpn_levels_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* const* levels,
                                           int n_levels, void* stream);
int dvid_backbone_swin_fpn_levels_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* const* levels,
                                         int n_levels, void* stream);

/* One RCNNHead (cond == NULL) or RCNNHead_cond pass.  head_index indexes head_series, or
 * head_series_cond when is_cond.  t: host int64 [n_frames] diffusion timesteps.
 * pro_features may be NULL (-> mean of the RoI features).  Outputs: logits [R,num_classes],
 * boxes [R,4], obj_features [R,hidden] (fp32, R = n_frames*boxes_per_frame).
 * bad_box_flag (device int, may be NULL) is OR-ed with 1 if any predicted box has x2<x1 or y2<y1
 * (the reference's AssertionError at box_head.py:588, reported without a host sync). */
int dvid_rcnn_head(dvid_model* m, int head_index, int is_cond, const void* p3, const void* p4, const void* p5, int n_frames,
                   int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                   const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                   int* bad_box_flag, void* stream);
/* The same over a pyramid given as an array (detectron2 ROIPooler as built at box_head.py:250-271: one scale per entry of
 * ROI_HEADS.IN_FEATURES, canonical size 224 at level 4): levels[0] is the finest map, n_levels 3 = p3..p5 (strides 8..32),
 * 4 = p2..p5 (strides 4..32); DVID_ERR_ARG for any other count, a null map, or a count that differs from the model's backbone.  A
 * head-only model takes either.  dvid_rcnn_head is this with n_levels 3; a model with the p2 level answers it with DVID_ERR_STATE. */
int dvid_rcnn_head_levels(dvid_model* m, int head_index, int is_cond, const void* const* levels, int n_levels, int n_frames,
                          int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                          const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                          int* bad_box_flag, void* stream);
/* dvid_rcnn_head_levels_keep (dvid_version >= 14): dvid_rcnn_head_levels, which also writes the tail's input -- the fp32 norm2 output
 * [n_frames * boxes_per_frame][256] that dvid_head_tail_backward takes as x -- to tail_input.  Null: exactly dvid_rcnn_head_levels.  The copy
 * is one device-to-device transfer behind norm2; every kernel of the pass reads and writes what it did, so all other outputs keep their
 * bits.  DTYPE float32 models only: a float16 model is refused (DVID_ERR_UNSUPPORTED), fp16 gradients being out of scope. */
int dvid_rcnn_head_levels_keep(dvid_model* m, int head_index, int is_cond, const void* const* levels, int n_levels, int n_frames,
                               int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                               const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                               int* bad_box_flag, float* tail_input, void* stream);
/* dvid_rcnn_head_levels_keep2 (dvid_version >= 15): dvid_rcnn_head_levels_keep with two more nullable outputs, the inputs of
 * dvid_inst_interact_backward: interact_input [n_frames * boxes_per_frame][256], the fp32 norm1 output, and roi_tiles
 * [n_frames * boxes_per_frame][49][256], the fp32 RoI tiles.  Each is one device-to-device copy; with both null the call is exactly
 * dvid_rcnn_head_levels_keep, and every other output keeps its bits.  A float16 model is refused when any of the three is asked for. */
int dvid_rcnn_head_levels_keep2(dvid_model* m, int head_index, int is_cond, const void* const* levels, int n_levels, int n_frames,
                                int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                                const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                                int* bad_box_flag, float* tail_input, float* interact_input, float* roi_tiles, void* stream);

/* cond[R,hidden] = MHA(query = obj_features[R,hidden], key = value = memory[lk,hidden]).  memory == NULL: use the K/V
 * projections kept by the last dvid_global_memory_project (lk 0 or the same row count). */
int dvid_global_xattn(dvid_model* m, const float* query, int rows, const float* memory, int lk, float* out, void* stream);
/* Project the video's global memory [lk, hidden] to K/V once (box_head.py:366-380 re-projects the same rows on every
 * call); valid until the next call of this function. */
int dvid_global_memory_project(dvid_model* m, const float* memory, int lk, void* stream);
/* The global stage for several live streams that share one model (dvid_version >= 4), after dvid_local_memory_project / dvid_local_xattn:
 * dvid_global_memory_project_groups projects `groups` memories of `lk` rows each, memory fp32 [groups * lk, hidden] (group g = rows
 * [g lk, (g + 1) lk)), with one K/V linear over all rows, into a buffer of ITS OWN: what dvid_global_memory_project holds for a video is
 * neither read nor written, so a video's projection survives any number of stream steps.  Valid until the next call of this function.
 * dvid_global_xattn_groups: out[rows, hidden], rows / groups consecutive query rows per group, group g attending its own lk projected
 * rows -- per group the value dvid_global_xattn gives on that group's memory alone; groups and lk must be what the last
 * dvid_global_memory_project_groups projected (DVID_ERR_STATE otherwise).  DTYPE float16 and float32. */
int dvid_global_memory_project_groups(dvid_model* m, const float* memory, int lk, int groups, void* stream);
int dvid_global_xattn_groups(dvid_model* m, const float* query, int rows, int groups, int lk, float* out, void* stream);

/* Local box-level attention (MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE; box_head.py:186-194, :338, :360-363).  The model has it when the
 * tensors head.local_attention.{i}.0.in_proj_weight / .0.in_proj_bias / .0.out_proj.weight / .0.out_proj.bias / .2.weight / .2.bias were
 * set before dvid_model_finalize, i = 0 .. stages - 1 (stages = the number of consecutive groups present; more than 2 fails the
 * finalize with DVID_ERR_UNSUPPORTED: the reference holds two local memories and indexes past them).  The reference's loop overwrites
 * attn_ on every stage and never updates the query, so ONLY THE LAST STAGE is observable and only it is computed: earlier stages' tensors
 * are accepted and ignored, and `stage` must be stages - 1 (DVID_ERR_ARG otherwise).  A model without the tensors answers DVID_ERR_STATE.
 *
 * dvid_local_memory_project: K/V projection of `groups` local memories of `lk` rows each, memory fp32 [groups * lk, hidden] (group g = rows
 * [g lk, (g + 1) lk): proposal_feats_local[stage] of that group's batch), into a buffer the MODEL owns; it moves only when it grows, and such a
 * move is counted by dvid_workspace_generation.  Valid until the next call of this function.
 * dvid_local_xattn: out[rows, hidden] = LayerNorm(out_proj(MHA(q_proj(query), K, V))), query fp32 [rows, hidden], rows / groups consecutive
 * query rows per group, each group attending its own lk projected memory rows; groups and lk must be what the last
 * dvid_local_memory_project projected (DVID_ERR_STATE otherwise).  The out-projection, its bias and the LayerNorm run as one kernel
 * (csrc/localattn.hip).  DTYPE float32 follows option f32_split and reports the fp16 range like the other fp32 linears. */
int dvid_local_memory_project(dvid_model* m, int stage, const float* memory, int lk, int groups, void* stream);
int dvid_local_xattn(dvid_model* m, int stage, const float* query, int rows, int groups, int lk, float* out, void* stream);

/* ---- stand-alone ops (also used by the parity tests) -------------------------------------- */
int dvid_roialign_v2_multilevel(const void* p3, const void* p4, const void* p5, int n_frames, int height, int width,
                                int channels, const float* boxes, int boxes_per_frame, void* roi_out /* fp16 [R,49,C] */,
                                float* mean_out /* [R,C] or NULL */, void* stream);
/* The same with the pyramid as an array (ROIPooler, box_head.py:250-271): levels[0] the finest map, n_levels 3 (p3..p5, what the entry
 * above forwards) or 4 (p2..p5); a box goes to level clamp(floor(4 + log2(sqrt(area) / 224 + 1e-8)), 6 - n_levels, 5).  DVID_ERR_ARG for
 * another count or a null map.  dvid_roialign_v2_levels_f32: the DTYPE float32 form (fp32 NHWC maps, fp32 tiles). */
int dvid_roialign_v2_levels(const void* const* levels, int n_levels, int n_frames, int height, int width, int channels,
                            const float* boxes, int boxes_per_frame, void* roi_out, float* mean_out, void* stream);
int dvid_roialign_v2_levels_f32(const float* const* levels, int n_levels, int n_frames, int height, int width, int channels,
                                const float* boxes, int boxes_per_frame, float* roi_out, float* mean_out, void* stream);
/* The DTYPE float32 forms of the stand-alone ops (csrc/f32.hip for conv / linear; the others beside their fp16 kernels in csrc/roialign.hip, attention.hip, dynconv.hip): fp32 NHWC pyramids -> fp32 [R,49,C] tiles; fp32 conv / linear with
 * w [cout][kpad] fp32, k = (ky*kw+kx)*cin + c, cin % 4 == 0, kpad = round_up(kh*kw*cin, 16) zero-padded, and row_scale [cout] (may be
 * NULL): out channel n = act(acc_n * row_scale[n] + bias[n] + residual) -- the model packs each row times a power of two that puts its
 * largest magnitude in [0.5, 1) and hands 2^-e here, which keeps the split-operand products at fp32 grade for small weights; w_hi / w_lo
 * (fp16 [cout][kpad], may be NULL): w_hi = fp16(w), w_lo = fp16(w - w_hi) -- given, and with option f32_split = 1 (default), the products run
 * as three fp16-MFMA passes over (hi, lo) operand pairs (the activations are split in the kernel); NULL, or f32_split = 0: fp32 MFMA; fp32 attention (head dim 32, head h at columns [32h, 32h+32)); fp32 DynamicConv (params [R][32768] = P1T[64][256] |
 * P2T[256][64]). */
int dvid_roialign_v2_multilevel_f32(const float* p3, const float* p4, const float* p5, int n_frames, int height, int width, int channels,
                                    const float* boxes, int boxes_per_frame, float* roi_out, float* mean_out, void* stream);
int dvid_conv2d_nhwc_f32(const float* in, const float* w, const void* w_hi, const void* w_lo, const float* bias, const float* row_scale, const float* residual,
                         float* out, int n, int h, int wd, int cin, int cout, int kh, int kw, int stride, int pad, int kpad, int relu, int residual_mode,
                         void* stream);
int dvid_mha_f32(const float* q, const float* k, const float* v, float* out, int batch, int lq, int lk, int nheads, int q_ld, int kv_ld, int out_ld,
                 int64_t q_bs, int64_t kv_bs, int64_t out_bs, void* stream);
/* Swin (shifted-)window attention, fp32 form of dvid_swin_window_attn_f16 below: qkv fp32 [batch*H*W][3C], qkv_bias fp32 [3C], out fp32. */
int dvid_swin_window_attn_f32(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                              int nheads, int shift, void* stream);
/* The same with the window size as an argument: the fp32 form of dvid_swin_window_attn_f16_ws below. */
int dvid_swin_window_attn_f32_ws(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                                 int nheads, int shift, int window, void* stream);
int dvid_dynconv_f32(const float* roi, const float* params, const float* g1, const float* b1, const float* g2, const float* b2, float* out,
                     int rows, void* stream);
int dvid_select_topk_features(const float* logits, int n_frames, int m, int num_classes, int k1, int k2, const float* feats,
                              int hidden, float* out_k1, float* out_k2, void* stream);
/* N(0, 1) draws as a pure function of (key, element index): out[i][e], i < n_images, e < per_image, = element e of the stream
 * keyed key0 + i.  Philox4x32-10 + fp64 Box-Muller rounded to fp32; oracle/noise.py restates it on the CPU (same values). */
int dvid_counter_normal(float* out, int64_t per_image, int n_images, uint64_t key0, void* stream);
/* The same with image i keyed key0 + i * key_stride (key_stride 1 is dvid_counter_normal): one launch for a batch of still images whose
 * draws are keyed by consecutive image ids, which lie a fixed stride apart in key space. */
int dvid_counter_normal_strided(float* out, int64_t per_image, int n_images, uint64_t key0, uint64_t key_stride, void* stream);
int dvid_noise_to_boxes(const float* x, float* boxes, int n, float snr_scale, float img_w, float img_h, void* stream);
/* The `_sizes` entries (dvid_version >= 3): the four size-dependent steps for a batch of still images, each with its own size.  Same
 * arguments as their siblings, with `sizes` where img_w, img_h stood: a DEVICE table of fp32 [n_frames][2], row f = (w, h) of the
 * un-padded frame f.  Precondition: every entry is positive and finite (not checked on the device).  The same kernels and the same
 * expressions: a table whose rows are all (w, h) gives the bits of the sibling called with (w, h).
 * dvid_noise_to_boxes_sizes: n boxes, m per frame (n a multiple of m, the table holds n / m rows): box i is scaled by row i / m. */
int dvid_noise_to_boxes_sizes(const float* x, float* boxes, int n, int m, float snr_scale, const float* sizes, void* stream);
/* Box renewal + DDIM update (eta = 1) of diffusion_det.py:559-596 (+ :649-653, :666-672): per frame, boxes whose
 * sigmoid(max logit) > keep_thr are kept (index order), updated as x0*sqrt_ac_next + coef_c*eps + sigma*noise[j],
 * and the tail is refilled from `fresh`.  All tensors [n_frames, m, 4] (logits [n_frames, m, c]). */
int dvid_ddim_renew_step(const float* logits, const float* boxes, const float* x_t, const float* noise, const float* fresh,
                         float* x_next, int n_frames, int m, int c, float img_w, float img_h, float snr_scale,
                         float sqrt_recip_ac, float sqrt_recipm1_ac, float sqrt_ac_next, float coef_c, float sigma, float keep_thr,
                         void* stream);
/* ... every frame's x_start normalised by its own row of `sizes` (see dvid_noise_to_boxes_sizes) */
int dvid_ddim_renew_step_sizes(const float* logits, const float* boxes, const float* x_t, const float* noise, const float* fresh,
                               float* x_next, int n_frames, int m, int c, const float* sizes, float snr_scale, float sqrt_recip_ac,
                               float sqrt_recipm1_ac, float sqrt_ac_next, float coef_c, float sigma, float keep_thr, void* stream);
/* logits [nsets, n_frames, m, c], boxes [nsets, n_frames, m, 4]; outputs [n_frames, nsets*m, ...] sorted by
 * descending score, first counts[f] entries valid.  scratch: >= dvid_postproc_scratch_bytes(nsets, n_frames, m) bytes, 16-byte aligned.
 * nsets * m candidates per frame, at most DVID_NMS_MAX_CANDIDATES (DVID_ERR_UNSUPPORTED beyond: torchvision's batched_nms itself
 * leaves the coordinate trick this step reproduces for a per-class NMS from 5000 boxes on).  Frames whose candidates fit one
 * workgroup's LDS (up to 997) run one kernel; the others a tiled form whose bit matrix lives in the scratch,
 * in chunks of frames of at most 64 MiB of matrix, every launch on `stream`. */
#define DVID_NMS_MAX_CANDIDATES 4096
int dvid_postproc_topk_nms(const float* logits, const float* boxes, int nsets, int n_frames, int m, int c, float img_w,
                           float img_h, float iou_threshold, int use_nms, float* out_boxes, float* out_scores,
                           int* out_labels, int* out_counts, void* scratch, void* stream);
/* ... frame f's survivors clipped to its own row of `sizes` (see dvid_noise_to_boxes_sizes); the selection and the NMS do not read it */
int dvid_postproc_topk_nms_sizes(const float* logits, const float* boxes, int nsets, int n_frames, int m, int c, const float* sizes,
                                 float iou_threshold, int use_nms, float* out_boxes, float* out_scores, int* out_labels,
                                 int* out_counts, void* scratch, void* stream);
/* Bytes of scratch dvid_postproc_topk_nms (and _sizes) needs for that shape: n_frames*nsets*m*24 where the single-kernel NMS runs, more where the
 * tiled form does (0 for a shape with no work). */
int64_t dvid_postproc_scratch_bytes(int nsets, int n_frames, int m);
/* The candidate selection of dvid_postproc_topk_nms on its own, in its streaming form (csrc/postproc.hip: topk_stream_kernel), forced at
 * any 1 <= m <= DVID_NMS_MAX_CANDIDATES and 1 <= c <= DVID_MAX_CLASSES: logits [nsets, n_frames, m, c], boxes [nsets, n_frames, m, 4] ->
 * per (frame, set) the m largest of the m * c sigmoid scores in (score desc, flat index asc) order: cand_boxes [n_frames, nsets * m, 4]
 * (the box of the score's row, unclipped), cand_scores and cand_labels (int32, class + 1) [n_frames, nsets * m], set s at columns
 * [s m, (s + 1) m).  dvid_postproc_topk_nms selects with one of three kernels that give the same bits: the keys of a (frame, set) held
 * in LDS and radix-selected where m * c * 4 + 8 * next_pow2(m) + 8 KiB <= 150 KiB (300 x 30, 300 x 80), a full sort in LDS up to 16384
 * padded keys, and this form, which recomputes the keys from the logits on every pass and holds none, for every other shape (500 x 80,
 * any m x 1203). */
int dvid_topk_candidates_stream(const float* logits, const float* boxes, int nsets, int n_frames, int m, int c, float* cand_boxes,
                                float* cand_scores, int* cand_labels, void* stream);
/* The tiled NMS on its own, at any 1 <= n <= DVID_NMS_MAX_CANDIDATES: cand_boxes [n_frames, n, 4] (unclipped xyxy), cand_scores
 * [n_frames, n], cand_labels [n_frames, n] (int32, >= 1) -> per frame the survivors of the class-aware NMS in (score desc, position
 * asc) order, clipped to the image: out_boxes [n_frames, out_cap, 4], out_scores, out_labels [n_frames, out_cap] (zero behind
 * out_counts[f]), out_cap >= n.  The same bits as dvid_postproc_topk_nms's NMS wherever both run.
 * scratch: >= dvid_nms_tiled_scratch_bytes(n_frames, n) bytes. */
int dvid_nms_frames_tiled(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_frames, int n, float img_w,
                          float img_h, float iou_threshold, int use_nms, int out_cap, float* out_boxes, float* out_scores,
                          int* out_labels, int* out_counts, void* scratch, void* stream);
int dvid_nms_frames_tiled_sizes(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_frames, int n,
                                const float* sizes, float iou_threshold, int use_nms, int out_cap, float* out_boxes, float* out_scores,
                                int* out_labels, int* out_counts, void* scratch, void* stream);
int64_t dvid_nms_tiled_scratch_bytes(int n_frames, int n);
/* Seq-NMS (TEST.SEQ_NMS; the reference's seq_nms.py, its engine's inference.py:54-62) over the detections of n_videos videos, as one
 * launch with a workgroup per (video, class) (csrc/seqnms.hip).  dets [frames, cap, 6] (device; a row = xyxy box, score, label as a float, labels 1 ..
 * num_classes, the layout of engine.pack_predictions), counts [frames] (device): the rows in front of counts[f] are the frame's detections.
 * video_starts [n_videos + 1] (host): video v is frames [video_starts[v], video_starts[v + 1]); video_starts[n_videos] = frames.
 * class_counts [frames, num_classes] (host): the frame's detections with label c + 1; the scratch is sized and laid out from it, and a
 * table that does not describe `dets` ends as DVID_SEQ_NMS_ERR_COUNTS in the class's status word, with nothing written outside the
 * class's share.  Per class, and independently per class: boxes of adjacent frames link at IoU >= 0.5 (x2 - x1 + 1 extents); the
 * highest-sum path through the links is found by dynamic programming (strictly greater improves, lowest predecessor and first
 * (frame, box) on ties), its boxes are rescored to sum / length, every other box within IoU 0.3 of a path box in its frame is
 * suppressed, and the search repeats until the best sum is below 1e-2 or no link is left.  float32 without contraction and an IEEE
 * division: the reference's bits.  -> keep [frames, cap] (uint8: 0 for a suppressed row and behind counts[f]), scores [frames, cap]
 * (rescored; 0 where keep is 0), status [n_videos, num_classes] (int32: the rounds the class ran, or an error word; the rounds are
 * bounded by the class's box count + 1, DVID_SEQ_NMS_ERR_ROUNDS beyond).  One-frame videos and classes without a link leave the input
 * as it is.  num_classes <= DVID_MAX_CLASSES, cap <= DVID_NMS_MAX_CANDIDATES and dvid_seq_nms_scratch_bytes(...) <=
 * DVID_SEQ_NMS_MAX_SCRATCH_BYTES (DVID_ERR_UNSUPPORTED beyond, before anything is launched).  scratch: >= that many bytes, 16-byte
 * aligned (may be NULL where it is 0).  The call uploads the layout and waits for that copy: it is synchronous with `stream`. */
#define DVID_SEQ_NMS_MAX_SCRATCH_BYTES (1ll << 30)
#define DVID_SEQ_NMS_ERR_ROUNDS (1 << 30)
#define DVID_SEQ_NMS_ERR_COUNTS (1 << 29)
int dvid_seq_nms_video(const float* dets, const int* counts, const int* class_counts, const int* video_starts, int n_videos, int cap,
                       int num_classes, unsigned char* keep, float* scores, int* status, void* scratch, int64_t scratch_bytes, void* stream);
/* Bytes of scratch for those tables (0: no class has a link to look for; -1: bad arguments).  Per (video, class) with at least one pair
 * of boxes in adjacent frames, with F frames, n_f boxes in frame f, N = sum n_f, L = sum over frame pairs of n_f * ceil(n_{f+1} / 64)
 * link words and M = sum ceil(n_f / 64): round16(12 (F + 1)) + round16(8 (L + M) + 36 N + 12 F) bytes, behind round16(40 n_videos
 * num_classes) bytes of headers. */
int64_t dvid_seq_nms_scratch_bytes(const int* class_counts, const int* video_starts, int n_videos, int num_classes);
/* The greedy matching of the VID AP50 evaluator on the device (dvid_version >= 5; csrc/videval.hip; data/evaluation/vid_eval.py:
 * calc_prec_rec's loop and corloc_eval_detection_vid's test), one workgroup per frame, all motion ranges in one launch.  No model handle,
 * independent of DTYPE.
 * in   dets [n_frames, cap, 6] fp32 (xyxy box in annotation pixels, score, label as a float), counts [n_frames] int32 (device), the
 *      layout of engine.pack_predictions; the ragged ground truth gt_boxes [G, 4] fp32, gt_labels [G] int32, gt_starts [n_frames + 1]
 *      int32 (device; frame f owns boxes [gt_starts[f], gt_starts[f + 1])), motion [G] float64 (device; NULL: nothing is ignored) and,
 *      on the HOST, gt_starts_host (the same table), ranges [n_ranges, 2] and empty_w [n_ranges] float64 (a box is ignored in range r
 *      when its motion IoU is < ranges[r][0] or > ranges[r][1]; empty_w[r] is the weight of a row in a frame without a box of its
 *      label), and label_min / label_max: the least and the greatest label among the rows in front of counts[f] and gt_labels, which
 *      the caller reads (ops.vid_eval_match does).
 * out  match [n_ranges, n_frames, cap] int8 and weight [n_ranges, n_frames, cap] float64 as calc_prec_rec appends them, at the row's own
 *      place; rank [n_frames, cap] int32: the row's position in its (frame, label) list in descending score, equal scores lower row
 *      first (-1, match 0 and weight 0 behind counts[f]); n_pos [n_ranges, num_classes + 1] float64: the counted boxes per label;
 *      top_row [n_frames] int32: the frame's highest-scoring row (the lowest of equal ones; -1 without rows) and top_hit [n_frames]
 *      int8: 1 when it overlaps a box of its own label by MORE than iou_thresh.
 * A row takes the best box of its label that no earlier row took and whose IoU is >= iou_thresh; on an exact tie the earlier box stays
 * unless it is ignored.  The IoU is _iou_vid's, bit for bit: float32, + 1 on x2, y2 and + 1 again in the extents, one IEEE division.
 * Before anything is launched: cap <= DVID_NMS_MAX_CANDIDATES, num_classes <= DVID_MAX_CLASSES, 1 <= n_ranges <=
 * DVID_VID_EVAL_MAX_RANGES, 0 <= label_min and label_max <= num_classes, at most DVID_VID_EVAL_MAX_GT boxes per frame
 * (DVID_ERR_UNSUPPORTED beyond, with the limit and the value in the message; nothing is written). */
#define DVID_VID_EVAL_MAX_GT 256
#define DVID_VID_EVAL_MAX_RANGES 4
int dvid_vid_eval_match(const float* dets, const int* counts, int n_frames, int cap, const float* gt_boxes, const int* gt_labels,
                        const int* gt_starts, const int* gt_starts_host, int label_min, int label_max, const double* motion,
                        const double* ranges, const double* empty_w, int n_ranges, float iou_thresh, int num_classes, signed char* match,
                        double* weight, int* rank, double* n_pos, int* top_row, signed char* top_hit, void* stream);
/* The matching of the COCO bbox evaluator on the device (dvid_version >= 6; csrc/cocoeval.hip on csrc/evalmatch.h;
 * data/evaluation/coco_eval.py: evaluate_numpy's loop), one workgroup per image, the ten IoU thresholds and the four area ranges in one launch.  No model handle,
 * independent of DTYPE.
 * in   dets [n_images, cap, 6] fp32 (xyxy box in annotation pixels, score, label as a float), counts [n_images] int32 (device), the
 *      layout of engine.pack_predictions; the ragged ground truth gt_boxes [G, 4] float64 (x, y, w, h), gt_areas [G] float64 (the
 *      annotation's own area), gt_crowd [G] uint8, gt_labels [G] int32, gt_starts [n_images + 1] int32 (device; image f owns boxes
 *      [gt_starts[f], gt_starts[f + 1])) and, on the HOST, gt_starts_host (the same table), iou_thrs [DVID_COCO_EVAL_THRESHOLDS] and
 *      area_ranges [DVID_COCO_EVAL_AREAS, 2] float64 (both ends inclusive).
 * out  match and ignore [DVID_COCO_EVAL_AREAS, DVID_COCO_EVAL_THRESHOLDS, n_images, cap] int8, at the row's own place: 1 when the row took
 *      a box / when it does not count (it took an ignored box, or took none and its own area w * h lies outside the range); rank
 *      [n_images, cap] int32: the row's position in its (image, label) list in descending score, equal scores lower row first; -1, match
 *      0 and ignore 0 behind counts[f], for a label outside 0 .. num_classes and past position DVID_COCO_EVAL_MAX_DETS; npig
 *      [DVID_COCO_EVAL_AREAS, num_classes + 1] int32: the boxes per label that are neither crowd nor outside the range.
 * A box is ignored in a range when it is crowd or its area lies outside.  A row walks the boxes of its label, the not ignored ones and
 * then the ignored ones, each group in annotation order, starting from best = min(threshold, 1 - 1e-10): a box that an earlier row took
 * is skipped unless it is crowd, a box with IoU < best is skipped, any other becomes the match and its IoU the new best (so equal IoU
 * moves to the later box); a row matched to a not ignored box does not go on to the ignored ones.  The IoU is float64, one operation at
 * a time: the overlap per axis min(dx + dw, gx + gw) - max(dx, gx) (<= 0 on either axis: IoU 0), i = w * h, u = dw * dh for a crowd box
 * and (dw * dh + gw * gh) - i otherwise, one IEEE division; a row's w is x2 - x1 of its float32 corners, in float64.  Precondition: the
 * scores are finite.
 * Before anything is launched: cap <= DVID_NMS_MAX_CANDIDATES, num_classes <= DVID_MAX_CLASSES, at most DVID_COCO_EVAL_MAX_GT boxes
 * per image (DVID_ERR_UNSUPPORTED beyond, with the limit and the value in the message; nothing is written). */
#define DVID_COCO_EVAL_MAX_GT 256
#define DVID_COCO_EVAL_THRESHOLDS 10
#define DVID_COCO_EVAL_AREAS 4
#define DVID_COCO_EVAL_MAX_DETS 100
int dvid_coco_eval_match(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                         const unsigned char* gt_crowd, const int* gt_labels, const int* gt_starts, const int* gt_starts_host,
                         const double* iou_thrs, const double* area_ranges, int num_classes, signed char* match, signed char* ignore,
                         int* rank, int* npig, void* stream);
/* The matching of the LVIS bbox evaluator on the device, the federated protocol (dvid_version >= 8; csrc/lviseval.hip on
 * csrc/evalmatch.h; data/evaluation/lvis_eval.py: match_numpy), one workgroup per image, the ten IoU thresholds and the four area ranges in one launch.  No
 * model handle, independent of DTYPE.
 * in   dets, counts, gt_boxes, gt_areas, gt_labels, gt_starts, gt_starts_host, iou_thrs, area_ranges: as dvid_coco_eval_match; gt_ignore
 *      [G] uint8 (the annotation's `ignore`) where that entry has gt_crowd; the image's negative and not-exhaustive label lists as two CSR
 *      tables on the device, neg_starts [n_images + 1] int32 with neg_labels, nex_starts [n_images + 1] int32 with nex_labels (image f owns
 *      neg_labels[neg_starts[f] .. neg_starts[f + 1]); a label outside 0 .. num_classes is skipped), and the two start tables on the HOST.
 * out  match, ignore, rank, npig: the layout of dvid_coco_eval_match.  rank -1, match 0 and ignore 0 also for every row that is not among
 *      the image's DVID_LVIS_EVAL_MAX_DETS rows of highest score (all labels together; equal scores: the lower row first; a row whose
 *      label is outside 0 .. num_classes takes no place) and for every row among them whose label is neither a label of one of the
 *      image's boxes nor in its negative list.  There is no further cut per label.
 * A box is ignored in a range when gt_ignore is set or its area lies outside.  The walk is dvid_coco_eval_match's without the crowd case:
 * a taken box is never taken again.  A row that takes no box does not count when its own area lies outside the range or its label is in
 * the image's not-exhaustive list; a row that takes a box counts as that box does.  Precondition: the scores are finite.
 * Before anything is launched: cap <= DVID_NMS_MAX_CANDIDATES, num_classes <= DVID_MAX_CLASSES, at most DVID_LVIS_EVAL_MAX_GT boxes
 * per image (DVID_ERR_UNSUPPORTED beyond, with the limit and the value in the message; nothing is written); the three start tables begin
 * at 0 and do not decrease (DVID_ERR_ARG).  DVID_LVIS_EVAL_MAX_GT is what the workgroup's LDS holds beside 4096 row keys: 115784 bytes
 * of 160 KiB (csrc/lviseval.hip has the sum). */
#define DVID_LVIS_EVAL_MAX_GT 1024
#define DVID_LVIS_EVAL_MAX_DETS 300
int dvid_lvis_eval_match(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                         const unsigned char* gt_ignore, const int* gt_labels, const int* gt_starts, const int* gt_starts_host,
                         const int* neg_starts, const int* neg_labels, const int* neg_starts_host, const int* nex_starts, const int* nex_labels,
                         const int* nex_starts_host, const double* iou_thrs, const double* area_ranges, int num_classes, signed char* match,
                         signed char* ignore, int* rank, int* npig, void* stream);
/* The accumulation of the COCO and the LVIS bbox evaluators on the device (dvid_version >= 9; csrc/evalaccum.hip;
 * data/evaluation/coco_eval.py: accumulate_arrays), with that function's bits: its order of the rows is total (label, score descending
 * with -0 == +0, image, rank), and everything behind the sort is integer counting, one correctly rounded float64 division, a maximum and
 * a comparison.  No host synchronise.
 * in   on the device, as dvid_coco_eval_match / dvid_lvis_eval_match read and leave them: dets [n_images, cap, 6] float32 (columns 4 and
 *      5 are read), counts [n_images] int32, rank [n_images, cap] int32, match and ignore [n_areas, n_thresholds, n_images, cap] int8, npig
 *      [n_areas, num_classes + 1] int32.  On the HOST: max_dets [max_dets_count] int32, ascending and positive ((1, 10, 100) for COCO,
 *      (300) for LVIS), and rec_thrs [n_rec_thrs] float64, which do not decrease.
 * out  precision [n_thresholds, n_rec_thrs, num_classes, n_areas, max_dets_count] and recall [n_thresholds, num_classes, n_areas,
 *      max_dets_count] float64, every entry: -1 for a (category, range) without counted ground truth, as accumulate_arrays leaves it.
 * A row is live when it lies in front of counts[image], its rank is >= 0 and its label is 1 .. num_classes; the scores must be finite.
 * scratch: >= dvid_eval_accumulate_scratch_bytes(n_images, cap, max_dets_count) bytes, 16-byte aligned: 56 bytes per row of
 * n_images * cap (two 64-bit keys and two 32-bit indices for the sort's two sides, two 64-bit flag masks in the layout's order and two in
 * the sorted order), a 1 KiB histogram per 4096 rows, one int32 per image and 5 KiB of tables.
 * Before anything is launched or written: n_areas == DVID_COCO_EVAL_AREAS, n_thresholds == DVID_COCO_EVAL_THRESHOLDS, n_rec_thrs ==
 * DVID_EVAL_ACCUMULATE_RECALLS, 1 <= max_dets_count <= DVID_EVAL_ACCUMULATE_MAX_LIMITS, max_dets ascending and positive, rec_thrs not
 * decreasing (DVID_ERR_ARG); cap <= DVID_NMS_MAX_CANDIDATES, num_classes <= DVID_MAX_CLASSES, n_images * cap < 2^31 and the scratch at
 * most DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES, that is about 19 million rows (DVID_ERR_UNSUPPORTED, with the limit and the value in
 * the message).  dvid_eval_accumulate_scratch_bytes is -1 for sizes that are no sizes. */
#define DVID_EVAL_ACCUMULATE_RECALLS 101
#define DVID_EVAL_ACCUMULATE_MAX_LIMITS 3
#define DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES (1ll << 30)
int dvid_eval_accumulate(const float* dets, const int* counts, const int* rank, const signed char* match, const signed char* ignore,
                         const int* npig, int n_images, int cap, int num_classes, int n_areas, int n_thresholds, const int* max_dets,
                         int max_dets_count, const double* rec_thrs, int n_rec_thrs, double* precision, double* recall, void* scratch,
                         long long scratch_bytes, void* stream);
long long dvid_eval_accumulate_scratch_bytes(int n_images, int cap, int max_dets_count);
int dvid_cdist(const float* x, int n, int d, float* dist, void* stream);
/* bs_emul: block size of the reference CUDA launch to emulate for tie-breaking (0 = fps.cu's own rule) */
int dvid_fps_greedy(const float* dist, int n, int m, int bs_emul, int* idx, void* stream);
int dvid_gather_rows(const float* x, const int* idx, float* y, int m, int d, void* stream);
/* The grouped forms (dvid_version >= 4): `groups` independent problems of one shape per launch, problem g computed exactly as the entry
 * above computes it alone (the same bits and the same picks, ties included).
 * dvid_cdist_groups: x [groups, n, d] -> dist [groups, n, n].
 * dvid_fps_greedy_groups: dist [groups, n, n] -> idx [groups, m]; one workgroup per problem with the running distances in registers
 * for n <= 4096, so the groups' sweeps of m - 1 dependent steps run side by side; beyond, the single-problem sweep once per group.
 * dvid_gather_rows_groups: y[g, r, :] = x[g, idx[g, r], :], x [groups, n, d], idx [groups, m], y [groups, m, d].
 * dvid_update_memory_groups: the three in a row -- merged [groups, n, d] -> idx [groups, m] and out [groups, m, d], with
 * dist_scratch >= groups * n * n floats.  Every argument is checked before the first launch: 1 <= m <= n, d % 4 == 0, groups >= 1, no
 * null pointer (DVID_ERR_ARG), and groups * n * n * 4 bytes of scratch at most DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES
 * (DVID_ERR_UNSUPPORTED, with the numbers in the message: prune fewer memories per call). */
#define DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES (1ll << 30)
int dvid_cdist_groups(const float* x, int groups, int n, int d, float* dist, void* stream);
int dvid_fps_greedy_groups(const float* dist, int groups, int n, int m, int bs_emul, int* idx, void* stream);
int dvid_gather_rows_groups(const float* x, const int* idx, float* y, int groups, int n, int m, int d, void* stream);
int dvid_update_memory_groups(const float* merged, int groups, int n, int d, int m, float* dist_scratch, int* idx, float* out, void* stream);
/* NHWC fp16 conv / linear (implicit GEMM on MFMA): w is [cout][kpad] fp16 with k = (ky*kw+kx)*cin + c,
 * kpad = round_up(kh*kw*cin, 64).  residual_mode: 0 none, 1 same shape, 2 nearest-x2 upsample.  pad < 0 (stride 1 only): |pad|
 * rows / columns before the image and as many after as keep the output at the input's size (the space-to-depth stem's 4x4 window). */
int dvid_conv2d_nhwc_f16(const void* in, const void* w, const float* bias, const void* residual, void* out, int n, int h,
                         int wd, int cin, int cout, int kh, int kw, int stride, int pad, int kpad, int relu, int out_f32,
                         int residual_mode, void* stream);
/* Everything behind conv1 of a res2 bottleneck block (detectron2 BottleneckBlock, widths 64 -> 64 -> 256, stride 1) as one launch:
 * conv2 3x3 + ReLU, conv3 1x1 + residual + ReLU and -- w1_next != NULL -- the next block's conv1 256 -> next_channels + ReLU
 * (next_channels 64: the next res2 block; 128, without a shortcut in the same launch: res3's first block).  t1 [n,h,wd,64] is the
 * block's conv1 output; w2 [64][576], w3 [256][64], w1_next [next_channels][256] in dvid_conv2d_nhwc_f16's packing (FrozenBN folded,
 * biases fp32).  w_shortcut == NULL: `residual` is the block input [n,h,wd,256]; else `residual` is the 64-channel block input
 * [n,h,wd,64] and the residual is its shortcut convolution w_shortcut [256][64].  out [n,h,wd,256], t1_next [n,h,wd,next_channels]
 * (must not alias t1).  Bit-identical to the same layers run through dvid_conv2d_nhwc_f16 (csrc/bneck.hip). */
int dvid_bottleneck64_tail_f16(const void* t1, const void* w2, const float* b2, const void* w3, const float* b3, const void* residual,
                               const void* w_shortcut, const float* b_shortcut, const void* w1_next, const float* b1_next, int next_channels,
                               void* out, void* t1_next, int n, int h, int wd, void* stream);
/* The same for the 128-wide blocks of res3 (128 -> 128 -> 512; the weights stream through an LDS ring): t1 [n,h,wd,128], w2 [128][1152],
 * w3 [512][128], residual [n,h,wd,512] (the block input, or the first block's shortcut output), w1_next [128][512], out [n,h,wd,512],
 * t1_next [n,h,wd,128].  w2 == NULL: `t1` is already the block's conv2 output (res3's first block: its 3x3 / stride-2 conv2 runs through
 * dvid_conv2d_nhwc_f16).  Bit-identical to the layer-by-layer launches on the igemm2 kernel (dvid_igemm_set_conv3x3(0)); the chunked 3x3
 * patch kernel sums conv2 in another order. */
int dvid_bottleneck128_tail_f16(const void* t1, const void* w2, const float* b2, const void* w3, const float* b3, const void* residual,
                                const void* w1_next, const float* b1_next, void* out, void* t1_next, int n, int h, int wd, void* stream);
/* MFMA attention, head_dim 32: fp16 q/k/v with head h at columns [32h, 32h+32) of each row, fp16 out;
 * vt_scratch: >= batch*nheads*32*(round_up(lk,32)+32) halves (receives V transposed per head). */
int dvid_mha_f16(const void* q, const void* k, const void* v, void* out, void* vt_scratch, int batch, int lq, int lk, int nheads,
                 int q_ld, int kv_ld, int out_ld, int64_t q_bs, int64_t kv_bs, int64_t out_bs, void* stream);
int dvid_dynconv(const void* roi, const void* params, const float* g1, const float* b1, const float* g2, const float* b2,
                 void* out, int rows, void* stream);
int dvid_add_layernorm(const float* x, const float* r, const float* g, const float* b, float* y, int rows, int d, int relu,
                       void* stream);
/* The Swin backbone's own kernels (swintransformer.py:135-176 and :216-270 without the two Linears; :296-319 without the reduction).
 * dvid_swin_pack_relbias (host only): relative_position_bias_table [169][nheads] -> the table the attention kernels read,
 * out [nheads][49][64] floats, out[h][i][j] = table[relative_position_index(i, j)][h], columns 49..63 zero.
 * dvid_swin_window_attn_f16: qkv fp16 [batch*H*W][3C] (q | k | v, head h at columns [32h, 32h+32) of each third; C = 32 * nheads), the
 * token map H x W of each image is padded to multiples of 7 with tokens whose q/k/v equal qkv_bias16 [3C], rolled by -shift on both axes
 * (0 <= shift < 7; shift > 0 adds the -100 mask between shift regions), attended per 7x7 window with the packed bias, and mapped back:
 * out fp16 [batch*H*W][C], padded positions write nothing.
 * dvid_patch_merge_ln: x fp32 [B][H][W][C] -> LayerNorm (eps 1e-5, g / b [4C]) of [x(2i,2j) | x(2i+1,2j) | x(2i,2j+1) | x(2i+1,2j+1)]
 * (zeros beyond an odd H / W), [B][ceil(H/2)][ceil(W/2)][4C] as fp16 (y16) and / or fp32 (y32); either may be NULL, not both.
 * C % 4 == 0 and C <= 512, DVID_ERR_UNSUPPORTED otherwise. */
int dvid_swin_pack_relbias(const float* table, int nheads, float* out);
int dvid_swin_window_attn_f16(const void* qkv, const void* qkv_bias16, const float* relbias, void* out, int batch, int H, int W, int C,
                              int nheads, int shift, void* stream);
/* The two entries above with the window size w as an argument, 7 or 12 (DVID_ERR_UNSUPPORTED otherwise; nothing is written on a refusal).
 * w = 7 forwards to them.  w = 12 (the 384-pretrained Swin sizes): table [(2w-1)^2 = 529][nheads] -> out [nheads][144][160] floats
 * (pitch = w*w rounded up to a multiple of 32), columns 144..159 zero; the token map is padded to multiples of 12 and rolled by -shift,
 * 0 <= shift < w (DVID_ERR_ARG otherwise), attended per 12x12 window (csrc/attention.hip: swin_window12_attn_kernel; fp32:
 * csrc/attention.hip: f32_swin_window12_attn_kernel).  C = 32 * nheads, DVID_ERR_UNSUPPORTED otherwise. */
int dvid_swin_pack_relbias_ws(const float* table, int nheads, int window, float* out);
int dvid_swin_window_attn_f16_ws(const void* qkv, const void* qkv_bias16, const float* relbias, void* out, int batch, int H, int W, int C,
                                 int nheads, int shift, int window, void* stream);
int dvid_patch_merge_ln(const float* x, const float* g, const float* b, void* y16, float* y32, int B, int H, int W, int C, void* stream);
int dvid_nhwc_from_nchw(const float* in, void* out_f16, int n, int h, int w, int c, void* stream);
int dvid_nchw_from_nhwc(const void* in_f16, float* out, int n, int h, int w, int c, void* stream);
int dvid_f32_to_f16(const float* x, void* y, int64_t n, void* stream);

/* Test-time Resize + ToTensor + padding on the device (mega_core/data/transforms/build.py:89-97, transforms.py:31-70:
 * PIL.Image.resize(BILINEAR) through torchvision; structures/image_list.py:54-61): src uint8 [h][w][3] RGB ->
 * out fp32 [3][ph][pw] in [0,1], rows >= oh / columns >= ow zero.  Bit-identical to Pillow: two integer passes with the
 * 22-bit weight tables of diffusionvid_amd/data/transforms.py:resample_tables (bounds int32 [n][2] = first source sample,
 * count; weights int32 [n][ksize]); a table pointer is NULL exactly when that axis keeps its size.  tmp: >= h*ow*3 bytes
 * (unused when ow == w). */
int dvid_resize_u8_to_f32(const void* src_hwc, int h, int w, void* tmp, float* out_chw, int oh, int ow, int ph, int pw,
                          const int* xbounds, const int* xk, int xksize, const int* ybounds, const int* yk, int yksize, void* stream);

/* The views of TEST.BBOX_AUG (dvid_version >= 7; csrc/resize.hip): n uint8 images, each with its own size, resized as
 * dvid_resize_u8_to_f32 resizes one -- the same two integer passes, the same bits -- onto one canvas in two launches however many images.
 * srcs: DEVICE table of n pointers to uint8 [h_i][w_i][3]; plan (device) and plan_host (the same rows on the host, checked before
 * anything is launched): int64 [n][11] = h, w, oh, ow, then for x and for y the first row of the image's tables in `bounds`
 * (-1 exactly when that axis keeps its size), its first entry in `weights` and its ksize, and the byte offset of its h * ow * 3
 * intermediate bytes in `tmp`; bounds int32 [n_bound_rows][2] and weights int32 [n_weights]: the images' resample tables concatenated.
 * -> out fp32 [n * (1 + flip)][3][ph][pw] in [0, 1]: slot i * (1 + flip) holds image i, zero outside [oh_i, ow_i]; with flip the next
 * slot holds its mirror inside its own ow_i columns, out[y][x] = resized[y][ow_i - 1 - x] (Resize, then RandomHorizontalFlip(1.0)). */
int dvid_resize_views_u8(const void* const* srcs, int n, const long long* plan, const long long* plan_host, const int* bounds,
                         int64_t n_bound_rows, const int* weights, int64_t n_weights, void* tmp, int64_t tmp_bytes, float* out, int ph, int pw,
                         int flip, void* stream);
/* The merge of TEST.BBOX_AUG (dvid_version >= 7; csrc/bboxaug.hip; mega_core/engine/bbox_aug.py): the detections of `views` views of
 * each of n images -- boxes [n * views][cap][4], scores, labels (int32) [n * views][cap], counts [n * views], slot i * views + v, as
 * dvid_postproc_topk_nms leaves them -- mapped into view 0's frame and packed as the candidates of dvid_nms_frames_tiled_sizes:
 * cand_* [n][views * cap], live rows first in (view, row) order, behind them padding rows (a zero-area box at the origin, score
 * FLT_MIN, label 1), live [n] the number of live rows.  table fp32 [n * views][5] = w_v, h_v, flip (0 / 1), rw, rh: a mirrored view
 * takes x1' = w_v - x2 - 1, x2' = w_v - x1 - 1, then x is multiplied by rw = fp32(w_0 / w_v) and y by rh, one fp32 operation at a time
 * (BoxList.transpose / resize); view 0 is copied.  views <= DVID_BBOX_AUG_MAX_VIEWS, views * cap <= DVID_NMS_MAX_CANDIDATES
 * (DVID_ERR_UNSUPPORTED beyond); the box arrays 16-byte aligned. */
#define DVID_BBOX_AUG_MAX_VIEWS 64
int dvid_bbox_aug_merge(const float* boxes, const float* scores, const int* labels, const int* counts, const float* table, int n, int views,
                        int cap, float* cand_boxes, float* cand_scores, int* cand_labels, int* live, void* stream);

/* The demo surface (dvid_version >= 10; csrc/overlay.hip; the reference's demo/predictor.py: select_top_predictions, overlay_boxes,
 * overlay_class_names): the detections of n frames painted onto them in place, two launches however many frames.
 * frames: DEVICE table of n pointers to uint8 RGB [h_i][w_i][3] at the image's native size (row pitch w_i * 3 bytes, no alignment asked);
 * sizes (device) and sizes_host (the same rows on the host: the grid, checked before anything is launched): int32 [n][2] = (h, w),
 * each 1 .. 65535.  dets fp32 [n][cap][6] = x1, y1, x2, y2, score, label in the model's frame, counts int32 [n]: rows at and beyond
 * counts[i] are never read for meaning.  ratios fp32 [n][2] = (rw, rh), native / model size.
 * A row is drawn iff its corners and score are finite and score > threshold (fp32, strict); draw order is ascending score, then
 * ascending row; the last DVID_OVERLAY_MAX_DRAWN in that order are kept.  Each corner is one fp32 product with its axis' ratio,
 * truncated toward zero and clamped to int32; corners are inclusive; a kept row with x2 < x1 or y2 < y1 is skipped.  Colour: with L the
 * truncated label, c_k = (L * (2^25 - 1, 2^15 - 1, 2^21 - 1)_k) mod 255 (non-negative), shown as R = c_2, G = c_1, B = c_0.
 * Ring of `thickness` t (1 .. 16), o = t / 2, i = t - o: [x1 - o, x2 + o] x [y1 - o, y2 + o] minus [x1 + i, x2 - i] x [y1 + i, y2 - i].
 * Text: names[L] (uint8 [num_classes + 1][DVID_OVERLAY_NAME_MAX], zero-padded, bytes 32 .. 126; a label outside 0 .. num_classes has
 * none) + ": " + the score as "%.2f" prints it (correctly rounded, ties to even; hundredths clamped to 999), the score alone without a
 * name.  Plate: with n characters, s = text_scale (1 .. 4) and pad = s, [x1, x1 + n * gw * s + 2 * pad - 1] x [y1, y1 + gh * s + 2 * pad - 1]
 * in the colour, white (255) where atlas (uint8 [95][gh][gw] of 0 / 1 for the characters 32 .. 126, gh, gw <= 32) holds 1 at the
 * pixel's cell, each atlas pixel s x s frame pixels.  Layers: a pixel takes the latest plate that covers it, else the latest ring,
 * else it is not written.  Everything is clipped to the frame.
 * DVID_ERR_UNSUPPORTED, with the numbers, before anything is launched: cap > DVID_NMS_MAX_CANDIDATES, num_classes > DVID_MAX_CLASSES,
 * a glyph cell beyond 32, thickness or text_scale out of range, scratch_bytes < dvid_overlay_scratch_bytes(n, cap). */
#define DVID_OVERLAY_MAX_DRAWN 256
#define DVID_OVERLAY_NAME_MAX 24
int dvid_overlay_detections(void* const* frames, const int* sizes, const int* sizes_host, int n, const float* dets, const int* counts, int cap,
                            const float* ratios, const unsigned char* names, int num_classes, const unsigned char* atlas, int gh, int gw,
                            float threshold, int thickness, int text_scale, void* scratch, int64_t scratch_bytes, void* stream);
int64_t dvid_overlay_scratch_bytes(int n, int cap);
/* the pixel tile one workgroup of the draw kernel resolves (the tests place boxes on its edges) */
int dvid_overlay_tile(int* tile_w, int* tile_h);

/* ---- split JPEG decode (dvid_version >= 11) --------------------------------------------------
 * The entropy (Huffman) stage runs on the host (csrc/jpeg_host.cpp, plain C++), everything behind it on the device (csrc/jpeg.hip), and
 * the result equals libjpeg's default decode bit for bit: ISLOW integer IDCT, "fancy" triangle upsampling, 16-bit fixed-point colour.
 *
 * Accepted files: SOF0 (baseline, 8-bit, Huffman), one interleaved scan, one component or three in YCbCr (a JFIF APP0 marker, or Adobe
 * APP14 with transform 1, or neither and component ids 1, 2, 3), luma sampling 1x1, 2x1 or 2x2 with chroma 1x1, 8-bit quantisation
 * tables; any Huffman tables, DRI / RSTn, stuffed FF 00.  DVID_ERR_UNSUPPORTED from dvid_jpeg_parse, the reason in the message:
 * progressive, arithmetic coding, 12-bit, SOF1, several scans, four components, Adobe transform 0 or 2, other sampling factors, 16-bit
 * quantisation tables, DNL or zero height.  Malformed data is DVID_ERR_ARG; no byte outside [data, data + size) is read.
 *
 * The two host entries call no HIP function and initialise no GPU (worker processes call them), keep no state and write their message
 * into the caller's `err` (err_cap bytes, may be NULL): they are re-entrant, and dvid_last_error does not speak for them.
 * dvid_jpeg_info holds no pointers.  Component c has a padded grid of blocks_w[c] x blocks_h[c] 8x8 blocks, blocks_w = ceil(width /
 * (8 * hmax)) * hsamp[c] and likewise down; its coefficients start at element coef_offset[c], blocks in raster order of that grid, 64
 * int16 per block in natural (de-zigzagged) order, NOT dequantised; coef_count is the total.  quant[c] is component c's table in natural
 * order.  A single component always reports sampling 1x1. */
typedef struct dvid_jpeg_info {
    int32_t width, height, ncomp;
    int32_t hsamp[3], vsamp[3];
    int32_t blocks_w[3], blocks_h[3];
    int32_t reserved;
    int64_t coef_offset[3];
    int64_t coef_count;
    uint16_t quant[3][64];
} dvid_jpeg_info;
int dvid_jpeg_parse(const void* data, int64_t size, dvid_jpeg_info* info, char* err, int err_cap);
/* parse + Huffman decode into coef[0 .. coef_count) (coef_cap: elements the buffer holds; zeroed first); info may be NULL */
int dvid_jpeg_entropy_decode(const void* data, int64_t size, int16_t* coef, int64_t coef_cap, dvid_jpeg_info* info, char* err, int err_cap);
/* The device half: n frames, each with its own size and sampling, in two launches however many frames (IDCT into uint8 component planes,
 * then upsample + colour into packed RGB).  coef: int16 [n_coef], the frames' coefficients one after the other; quant: uint16 [n_quant],
 * 192 entries (quant[3][64]) per frame; planes: >= n_coef bytes of scratch, 8-byte aligned (component samples, at the coefficients' own
 * offsets); out: uint8 [out_bytes], frame i as [h_i][w_i][3] RGB at byte out_off_i, a one-component frame with R = G = B.
 * plan (device) and plan_host (the same rows on the host, checked before anything is launched): int64 [n][DVID_JPEG_PLAN_COLS] = width,
 * height, ncomp, luma hsamp, luma vsamp, coef_offset[0..2] (elements into coef), the first entry of its tables in quant, out_off.
 * No address in either kernel depends on a coefficient's value: a corrupt file gives wrong pixels inside its own image.
 * DVID_ERR_ARG, with the numbers: a null pointer, a sampling outside 1x1 / 2x1 / 2x2, offsets that are not 64-element aligned, do not
 * ascend (overlap) or leave their buffers.  DVID_ERR_UNSUPPORTED: n > 65535 or n_coef > DVID_JPEG_MAX_COEFS -- the kernels index
 * coefficients and plane samples with int32, and 2^31 - 1 coefficients are 1.4 gigapixels of 4:2:0 per call; pixel offsets are 64-bit
 * (one 65535 x 65535 frame alone would be 12.9 GB of RGB). */
#define DVID_JPEG_PLAN_COLS 10
#define DVID_JPEG_MAX_COEFS 2147483647LL
int dvid_jpeg_reconstruct_u8(const int16_t* coef, int64_t n_coef, const uint16_t* quant, int64_t n_quant, const long long* plan,
                             const long long* plan_host, int n, void* planes, int64_t planes_bytes, void* out, int64_t out_bytes, void* stream);

/* ---- the training objective (dvid_version >= 12; its gradient >= 13; csrc/criterion.hip) ----
 * The host mirror is modeling/roi_heads/box_head/loss.py (the reference's box_head/loss.py:257-688, diffusion_det.py:681-725).  The first
 * three entries compute values only; dvid_set_criterion_backward is the gradient with respect to the head outputs.
 *
 * dvid_q_sample_boxes: the noisy boxes of a labelled batch, one launch.  Image i: its ground truth gt[gt_starts[i] .. gt_starts[i + 1])
 * as normalised (cx, cy, w, h) -- with none, the box (0.5, 0.5, 1, 1) -- padded to m rows with placeholder / 6 + 0.5 (w, h at least 1e-4;
 * padding row j reads placeholder[i][j - real], the reference's draw of m - real rows), (x * 2 - 1) * snr_scale, sqrt_ac[t[i]] * x +
 * sqrt_omac[t[i]] * noise, clamped to +-snr_scale, back to [0, 1], to xyxy, times the image's (w, h, w, h) from sizes [n][2].  fp32, one
 * operation at a time.  t, noise [n][m][4] and placeholder [n][m][4] are the caller's draws; sqrt_ac / sqrt_omac are the detector's
 * sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod tables of `timesteps` entries.  t_host / gt_starts_host: the same values on the
 * host, checked before the launch.  DVID_ERR_UNSUPPORTED: an image with more than m ground-truth boxes (the reference draws a random
 * subset there, which is not restated), with both numbers in the message; DVID_ERR_ARG: t outside [0, timesteps), null pointers.
 *
 * dvid_set_criterion: the dynamic-k matcher and the loss sums of n_sets head outputs of n images in one call.  logits [n_sets][n][m][c]
 * and boxes [n_sets][n][m][4] (absolute xyxy) fp32; the ragged ground truth gt_boxes [G][4] fp32 absolute xyxy, gt_labels [G] int32
 * 1-based, gt_starts [n + 1] (device) and gt_starts_host; sizes [n][2] = (w, h).  Outputs, all on the device:
 *   assign [n_sets][n][m] int32          the ground-truth index within the image a query is matched to, -1 for none
 *   matched_query [n_sets][n][gmax] int32 per ground-truth box its matched query of least cost (the matcher's second return value), -1 behind
 *                                         the image's boxes; gmax >= the largest box count of the batch
 *   sums [n_sets][n][4] float64          focal sum over the m x c elements, L1 sum and (1 - GIoU) sum over the matched queries, matched count
 *   status [n_sets][n] int32             0, or DVID_CRITERION_ERR_* bits; a set with DEGENERATE, NONFINITE or LABEL is not matched
 * Every term is fp32, summed in float64 by a fixed tree: two runs give the same bits.  The repair loop of the matcher is bounded by
 * box count + DVID_CRITERION_REPAIR_SLACK rounds.  Refused before any launch, with the numbers: ota_k outside
 * 1 .. DVID_CRITERION_MAX_OTA_K, m outside ota_k .. DVID_CRITERION_MAX_ROWS, c outside 1 .. DVID_MAX_CLASSES, an image with more than
 * DVID_CRITERION_MAX_GT boxes or more than gmax (DVID_ERR_UNSUPPORTED); scratch smaller than dvid_set_criterion_scratch_bytes or not
 * 16-byte aligned (DVID_ERR_ARG). */
#define DVID_CRITERION_MAX_GT 256
#define DVID_CRITERION_MAX_ROWS 4096
#define DVID_CRITERION_MAX_OTA_K 64
#define DVID_CRITERION_REPAIR_SLACK 32
#define DVID_CRITERION_ERR_ROUNDS 1
#define DVID_CRITERION_ERR_DEGENERATE 2
#define DVID_CRITERION_ERR_NONFINITE 4
#define DVID_CRITERION_ERR_LABEL 8
int dvid_q_sample_boxes(const float* gt_cxcywh, const int* gt_starts, const int* gt_starts_host, int n, int m, const int* t, const int* t_host,
                        const float* sqrt_ac, const float* sqrt_omac, int timesteps, const float* noise, const float* placeholder, float snr_scale,
                        const float* sizes, float* boxes, void* stream);
int dvid_set_criterion(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes, const int* gt_labels,
                       const int* gt_starts, const int* gt_starts_host, const float* sizes, float alpha, float gamma, int ota_k, float cost_class,
                       float cost_bbox, float cost_giou, int* assign, int* matched_query, int gmax, double* sums, int* status, void* scratch,
                       int64_t scratch_bytes, void* stream);
int64_t dvid_set_criterion_scratch_bytes(int n_sets, int n, int m, int gmax);

/* dvid_set_criterion_backward (dvid_version >= 13): the gradient of  sum_s sum_k coef[s][k] * sum_k(s)  with respect to logits and boxes,
 * where sum_0 .. sum_2 (s) are the focal, L1 and (1 - GIoU) sums dvid_set_criterion reports for head output s, added over the batch.  One
 * launch for all n_sets head outputs of n images.  logits, boxes, the ground truth, sizes, alpha and gamma: dvid_set_criterion's own
 * arguments; assign [n_sets][n][m] and status [n_sets][n] as that call left them; coef [n_sets][3] float64 on the device, formed by the
 * caller (the reference's losses: upstream gradient / denominator, the denominators from sums[..][3], so no host synchronise is needed).
 * Outputs d_logits [n_sets][n][m][c] and d_boxes [n_sets][n][m][4], fp32; EVERY element is written (an uninitialised buffer is fine).
 *   focal  coef0 * d/dx of BCE-with-logits * (1 - p_t)^gamma * alpha_t (alpha < 0: no alpha weight; gamma != 2: powf), fp32, the one-hot
 *          built from assign and the labels as the forward builds it
 *   L1     matched rows: coef1 * sign(q / whwh - target) / whwh, target the forward's normalised, to-cxcywh-and-back value; sign(0) = 0
 *   GIoU   matched rows: coef2 * d(1 - GIoU(q, gt)) / dq
 * At the kinks the gradient is what torch's autograd gives on the host restatement (loss.losses_host), and this is part of the contract:
 * a maximum / minimum of EQUAL operands hands each operand half of the gradient; clamp(min = 0) passes the gradient at exactly 0 (an
 * intersection of zero width still sends its gradient on, a negative one does not).
 * Zeros: unmatched rows have d_boxes exactly 0; a set whose status carries DEGENERATE, NONFINITE or LABEL gets all zeros (the forward did
 * not match it); a coef of 0 gives exact zeros for its term, whatever the inputs hold (never 0 * inf).
 * No atomics and no reduction: every output element has one writer, so two runs give the same bits.
 * Refused before any launch, with the numbers: m outside 1 .. DVID_CRITERION_MAX_ROWS, c outside 1 .. DVID_MAX_CLASSES, an image with
 * more than DVID_CRITERION_MAX_GT boxes, more than 65535 sets (DVID_ERR_UNSUPPORTED); null pointers, a gt_starts that does not start at
 * 0 or decreases (DVID_ERR_ARG). */
int dvid_set_criterion_backward(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes, const int* gt_labels,
                                const int* gt_starts, const int* gt_starts_host, const float* sizes, float alpha, float gamma, const int* assign,
                                const int* status, const double* coef, float* d_logits, float* d_boxes, void* stream);

/* ---- the backward of the head's tail (dvid_version >= 14; csrc/headtail_bwd.hip) ----
 * dvid_head_tail_backward (dvid_version >= 14): the tail of an RCNNHead / RCNNHead_cond pass (box_head.py:524-548 / :636-664) recomputed in
 * fp32, and its gradient.  The host mirror is modeling/roi_heads/box_head/tail.py (head_tail_host).  The function: x [R][256] is the norm2
 * output, R = n * m rows image-major; boxes_in [R][4]; time_emb [n][1024]; cond [R][256] or null (null: RCNNHead; given: RCNNHead_cond,
 * whose shift is c_mlp.1(SiLU(cond)) per row and whose block_time_mlp.1 has 256 rows, the scale alone).
 *   obj    = norm3(x + linear2(ReLU(linear1(x))))                 fc = obj * (scale + 1) + shift, (scale, shift) = block_time_mlp.1(SiLU(time_emb))
 *   logits = class_logits(cls tower(fc))                            boxes = apply_deltas(bboxes_delta(reg tower(fc)), boxes_in)
 * a tower layer being ReLU(LayerNorm(Linear without bias)), dropout the identity.  `params` is a HOST table of n_params = 14 + 3 * (num_cls +
 * num_reg) device pointers, fp32 in the reference's row-major layout, and `grads` a host table of the same length and shapes:
 *   0 linear1.weight [dff][256]   1 linear1.bias   2 linear2.weight [256][dff]   3 linear2.bias   4 norm3.weight   5 norm3.bias
 *   6 block_time_mlp.1.weight [512 or 256][1024]   7 block_time_mlp.1.bias   8 c_mlp.1.weight [256][256]   9 c_mlp.1.bias (8, 9: cond head
 *   only, ignored without cond)   10 class_logits.weight [c][256]   11 class_logits.bias   12 bboxes_delta.weight [4][256]   13 bboxes_delta.bias
 *   14 + 3 l, 15 + 3 l, 16 + 3 l: tower layer l's Linear weight [256][256], LayerNorm weight and bias; the num_cls layers of cls_module first
 *   (cls_module.{3 i, 3 i + 1}), then the num_reg layers of reg_module.
 * Forward outputs logits_out [R][c], boxes_out [R][4], obj_out [R][256]: any of them may be null.  Cotangents d_logits, d_boxes, d_obj: null
 * means zeros.  Gradient outputs d_x [R][256], d_time_emb [n][1024], d_cond [R][256] (with cond) and grads: every element is written.  With
 * grads, d_x, d_time_emb and d_cond ALL null the call is the forward alone.
 * Arithmetic: fp32 storage, fp32 products on v_mfma_f32_32x32x2_f32, fp32 accumulation -- not the split fp16 operands of the DTYPE float32
 * inference path, whose low half is lost on a cotangent below fp16's normal range.  A sum over the R rows (weight, bias and LayerNorm
 * gradients; over an image's m rows for d_time_emb) is formed in chunks of DVID_HEAD_TAIL_BWD_ROW_CHUNK rows whose partial results go to
 * scratch and are added in ascending order: no atomics, two runs give the same bits.
 * At the kinks the gradient is what torch's autograd gives on the host restatement, and this is part of the contract:
 *   ReLU passes nothing at a pre-activation of exactly 0;
 *   clamp(max = scale_clamp) passes the gradient at equality and nothing above it;
 *   a row whose dw is clamped still gets its dx and dy gradients (and dh its own, unless clamped too);
 *   a box of zero width gets exact zeros for the terms that multiply the width (likewise the height).
 * Refused before any launch, with the numbers: hidden other than 256, dff not a positive multiple of DVID_HEAD_TAIL_BWD_TILE, c outside
 * 1 .. DVID_MAX_CLASSES, num_cls / num_reg outside the forward's 0 .. 4, more than 65535 images or DVID_HEAD_TAIL_BWD_MAX_ROWS rows
 * (DVID_ERR_UNSUPPORTED); n < 1 or m < 1, a wrong n_params, null pointers, a scratch smaller than dvid_head_tail_backward_scratch_bytes or
 * not 16-byte aligned (DVID_ERR_ARG). */
#define DVID_HEAD_TAIL_BWD_ROW_CHUNK 256
#define DVID_HEAD_TAIL_BWD_TILE 64
#define DVID_HEAD_TAIL_BWD_MAX_ROWS 1048576
int dvid_head_tail_backward(const float* x, const float* boxes_in, const float* time_emb, const float* cond, int n, int m, int hidden, int dff,
                            int num_classes, int num_cls, int num_reg, const float* const* params, int n_params, float wx, float wy, float ww, float wh,
                            float scale_clamp, const float* d_logits, const float* d_boxes, const float* d_obj, float* logits_out, float* boxes_out,
                            float* obj_out, float* d_x, float* d_time_emb, float* d_cond, float* const* grads, void* scratch, int64_t scratch_bytes,
                            void* stream);
int64_t dvid_head_tail_backward_scratch_bytes(int n, int m, int dff, int num_classes, int num_cls, int num_reg, int has_cond);

/* ---- the backward of the head's instance interaction (dvid_version >= 15; csrc/interact_bwd.hip) ----
 * dvid_inst_interact_backward (dvid_version >= 15): an RCNNHead's DynamicConv (box_head.py:666-711) with its residual and norm2
 * (box_head.py:521-524) recomputed in fp32, and its gradient: the link in front of dvid_head_tail_backward, whose x is this function's y.  The
 * host mirror is modeling/roi_heads/box_head/interact.py (inst_interact_host).  The function: p [rows][256] is the norm1 output, rows image-major;
 * roi [rows][49][256] the fp32 RoI tiles, bin-major as dvid_roialign_v2_levels_f32 writes them;
 *   params = dynamic_layer(p)   [rows][32768], param1 = [:16384] as [256][64], param2 = [16384:] as [64][256]
 *   F1 = ReLU(LN64(roi . param1))   F2 = ReLU(LN256(F1 . param2))   o = ReLU(LN256(out_layer(F2 flattened bin * 256 + c)))   y = norm2(p + o)
 * dropout being the identity.  `params` is a HOST table of n_params = 12 device pointers, fp32 in the reference's names and row-major layouts
 * (NOT the inference runtime's repacked dynamic_layer order), and `grads` a host table of the same length and shapes:
 *   0 inst_interact.dynamic_layer.weight [32768][256]   1 inst_interact.dynamic_layer.bias [32768]
 *   2 inst_interact.out_layer.weight [256][12544]       3 inst_interact.out_layer.bias [256]
 *   4, 5 inst_interact.norm1.weight, .bias [64]         6, 7 inst_interact.norm2.weight, .bias [256]
 *   8, 9 inst_interact.norm3.weight, .bias [256]        10, 11 norm2.weight, .bias [256]
 * Forward output y_out [rows][256] (may be null).  Cotangent d_y [rows][256]: null means zeros.  Gradient outputs d_p [rows][256], d_roi
 * [rows][49][256] (may be null, then it is not written) and grads: every element is written.  With d_p, d_roi and grads ALL null the call is
 * the forward alone.
 * Arithmetic and order of summation as dvid_head_tail_backward: fp32 products on v_mfma_f32_32x32x2_f32, no atomics, sums over rows in chunks
 * of DVID_HEAD_TAIL_BWD_ROW_CHUNK added in ascending order, two runs give the same bits.  A box's dynamic parameters and their gradient (128 KiB
 * each) exist for DVID_INST_BWD_ROW_SLAB rows at a time; of the scratch only the kept F2 and its cotangent ([rows][49][256] each) and a few
 * [rows][256] terms grow with rows.  ReLU passes nothing at a pre-activation of exactly 0.
 * Refused before any launch, with the numbers: hidden other than 256, dim_dynamic other than 64, a pooler other than 7 (7 x 7 bins), rows
 * above DVID_HEAD_TAIL_BWD_MAX_ROWS (DVID_ERR_UNSUPPORTED); rows < 1, n_params other than 12, null pointers, d_roi or a cotangent without
 * d_p and grads, a scratch smaller than dvid_inst_interact_backward_scratch_bytes or not 16-byte aligned (DVID_ERR_ARG). */
#define DVID_INST_BWD_ROW_SLAB 512
int dvid_inst_interact_backward(const float* p, const float* roi, int rows, int hidden, int dim_dynamic, int pooler, const float* const* params,
                                int n_params, const float* d_y, float* y_out, float* d_p, float* d_roi, float* const* grads, void* scratch,
                                int64_t scratch_bytes, void* stream);
/* bytes of scratch for `rows` rows; -1 for a row count the entry refuses */
int64_t dvid_inst_interact_backward_scratch_bytes(int rows);

/* ---- the backward of the head's self-attention (dvid_version >= 16; csrc/selfattn_bwd.hip) ----
 * dvid_self_attn_backward (dvid_version >= 16): an RCNNHead's self-attention with its residual and norm1 (box_head.py:514-518) recomputed in
 * fp32, and its gradient: the link in front of dvid_inst_interact_backward, whose p is this function's y.  A head's x is the previous head's
 * obj_features (the mean over the RoI bins for the first), so this function's d_x is the previous head's d_obj: with it the links compose over
 * all heads.  The host mirror is modeling/roi_heads/box_head/attention.py (self_attention_host).  The function: x [n * m][256], rows
 * image-major; the m rows of an image attend to each other, nheads = 8 heads of 32:
 *   qkv = in_proj(x)   O = softmax(q k^T / sqrt 32) v per (image, head)   y = norm1(x + out_proj(O))
 * dropout being the identity.  `params` is a HOST table of n_params = 6 device pointers, fp32 in the reference's names and row-major layouts,
 * and `grads` a host table of the same length and shapes:
 *   0 self_attn.in_proj_weight [768][256] (q, k, v rows in this order)   1 self_attn.in_proj_bias [768]
 *   2 self_attn.out_proj.weight [256][256]                               3 self_attn.out_proj.bias [256]
 *   4 norm1.weight [256]                                                 5 norm1.bias [256]
 * Forward output y_out [n * m][256] (may be null).  Cotangent d_y [n * m][256]: null means zeros.  Gradient outputs d_x [n * m][256] and
 * grads: every element is written.  With d_x and grads BOTH null the call is the forward alone.
 * Arithmetic and order of summation as dvid_head_tail_backward: fp32 products on v_mfma_f32_32x32x2_f32, no atomics, sums over rows in chunks
 * of DVID_HEAD_TAIL_BWD_ROW_CHUNK added in ascending order, two runs give the same bits.  The [m][m] probabilities are never stored: the
 * forward keeps the log-sum-exp of every (row, head) and the backward forms P = exp(S - L) again in 32 x 32 tiles, once by query tiles (dQ,
 * the key tiles in ascending order) and once by key tiles (dK and dV, the query tiles in ascending order); every element has one writer.
 * Padded keys: rows past an image's last row in its last tile are staged as zeros and their probabilities are set to an exact 0, never
 * exp(S - L) of what lies behind -- the next image's rows.  The scratch grows linearly with n * m.
 * Refused before any launch, with the numbers: hidden other than 256, nheads other than 8, m above DVID_CRITERION_MAX_ROWS, n * m above
 * DVID_HEAD_TAIL_BWD_MAX_ROWS, more than 65535 images (DVID_ERR_UNSUPPORTED); n < 1 or m < 1, n_params other than 6, null pointers, a
 * cotangent without d_x and grads, a scratch smaller than dvid_self_attn_backward_scratch_bytes or not 16-byte aligned (DVID_ERR_ARG). */
int dvid_self_attn_backward(const float* x, int n, int m, int hidden, int nheads, const float* const* params, int n_params, const float* d_y,
                            float* y_out, float* d_x, float* const* grads, void* scratch, int64_t scratch_bytes, void* stream);
/* bytes of scratch for n images of m rows; -1 for sizes the entry refuses */
int64_t dvid_self_attn_backward_scratch_bytes(int n, int m);

/* ---- options ------------------------------------------------------------------------------
 * The library's behaviour switches are ONE table set through this ABI, never through the environment (csrc/options.h; the defaults
 * are the benchmarked configuration).  Names: conv3x3, wstat, bneck_fuse (0 off / 1 by the layer's shape rule / 2 wherever the layer
 * type fits), stem_pool, head_tail, ln_rows (0 / 1), igemm_cfg (-1 = tuner, >= 0 forced tile configuration), igemm_tune (-1 / 0 / 1, see
 * dvid_igemm_set_tuning), igemm_generic (0 / 1), f32_split (DTYPE float32 products: 1 = split fp16 operands on the fp16 MFMA, 0 = the fp32
 * MFMA), bneck_lds (diagnostics).  Every choice gives the same values up to fp32 summation
 * order (most are bit-identical; the tests say which).  dvid_effective_config writes "name=value ..." of all options followed by the
 * environment variables the library still reads (DVID_IGEMM_TUNE, DVID_IGEMM_TUNE_CACHE, DVID_CHAINS, DVID_POISON_WORKSPACE) as they
 * are set; bench.py echoes it.  The dvid_igemm_set_* / dvid_set_stem_pool entry points below write the same table (-1 = the default). */
int dvid_set_option(const char* name, int value);
int dvid_get_option(const char* name, int* value);
int dvid_reset_options(void);
int dvid_effective_config(char* buf, int cap);

/* ---- measurement -------------------------------------------------------------------------- */
/* Tile configurations of the implicit-GEMM kernel (all bit-identical in their results): the per-shape tuner picks one;
 * dvid_igemm_set_config(k) forces table entry k wherever it is valid (k = -1: back to the tuner). */
int dvid_igemm_num_configs(void);
int dvid_igemm_set_config(int cfg);
/* Per-shape tile tuning: 1 = the first launch of a new (row bucket, N, K, ...) key times every valid configuration on the
 * launch's own stream (stream sync + ~80 launches once per key; keys bucket the row count 8 steps per octave, so ragged
 * video tails do not create new ones); 0 = never time on the calling path: cached winners (DVID_IGEMM_TUNE_CACHE, earlier
 * launches) or the hand rule; -1 = follow the environment: DVID_IGEMM_TUNE if set, else 0 when DVID_IGEMM_TUNE_CACHE names a
 * non-empty winners file (a deployment that ships one is in serving mode by default), else 1. */
int dvid_igemm_set_tuning(int mode);
/* Shape buckets timed on the calling path in this process so far (each = one stream synchronisation + 4 .. ~40 launches per valid
 * configuration): a serving process wants this to stop growing after warm-up -- ragged video tails whose launches are under two rounds of
 * the CUs inherit a tuned bucket only within a quarter octave and may add passes mid-stream (bench.py reports the count per run). */
long long dvid_igemm_tuning_passes(void);
/* 3x3 / stride-1 / pad-1 convolutions with Cin % 32 == 0 and Cout % 128 == 0 (the bottleneck conv2 layers of res3-res5, the FPN
 * output convolutions) on the halo-staged kernel (csrc/conv3x3.hip: the 8 x 32 output patch's input pixels are staged once per
 * 32-channel chunk and serve all nine taps): 1 = on where the shape rule prefers it (W within 1/8 of a multiple of 32, maps of at least
 * 512 pixels -- a function of the layer and the image size, not of the number of frames in the launch), 2 = on wherever the layer type fits (tests), 0 = off (the igemm2 kernel), -1 = the default
 * (1).  The choice depends on the layer's shape only; the two kernels differ in fp32 summation order. */
int dvid_igemm_set_conv3x3(int mode);
/* 1x1 convolutions / linear layers with K in {128, 256} (512 without a residual) and N a multiple of 256 (bottleneck conv3 + residual, the decoder's
 * dynamic_layer and linear1) on the weight-stationary kernel (csrc/wstat.hip: a workgroup keeps the weights of 256 output channels in
 * registers and streams its rows through a DMA ring; epilogue straight from the accumulator layout): 1 = on for launches large
 * enough for 256 persistent workgroups, 2 = wherever the layer type fits (tests), 0 = off (igemm2), -1 = the default (1).
 * Bit-identical to igemm2. */
int dvid_igemm_set_wstat(int mode);

/* res2 / res3 bottleneck blocks behind their conv1 as one launch each (csrc/bneck.hip: dvid_bottleneck64_tail_f16 /
 * dvid_bottleneck128_tail_f16 inside the ResNet backbone): 1 = where the shape rule of the 3x3 patch kernels holds for the stage's map
 * (a function of the image size only), 2 = whenever the stage is made of such bottlenecks (tests), 0 = off (layer-by-layer launches),
 * -1 = the default (1).  res2: bit-identical to the layer-by-layer launches; res3: to those on igemm2 (see above). */
int dvid_igemm_set_bottleneck_fusion(int mode);

/* The ResNet stem (7x7 / stride 2 as a 4x4 convolution over the space-to-depth image, + FrozenBN + ReLU) and the 3x3 / stride-2 max pool
 * behind it (detectron2 BasicStem, reached from mega_core/modeling/detector/diffusion_det.py:427) as ONE launch: 1 = on, 0 = two launches,
 * -1 = the default (1).  Bit-identical either way (csrc/conv3x3.hip: stem_pool_kernel). */
int dvid_set_stem_pool(int mode);

/* When enabled, every igemm launch is bracketed by HIP events on its stream; dvid_profile_read
 * synchronises those events and returns totals since the last reset. */
int dvid_profile_enable(int on);
int dvid_profile_reset(void);
int dvid_profile_read(double* igemm_ms, double* igemm_flop, int64_t* igemm_launches);
/* sum over the recorded launches of the algorithmic HBM bytes (input + weights + output + residual, each touched once) */
int dvid_profile_read_bytes(double* igemm_alg_bytes);
/* CSV (kernel,family,M,N,K,taps,stride,res_mode,ms,tflops,alg_mbytes,alg_gbs), one line per recorded launch: the implicit-GEMM family
 * (family = 1: what dvid_profile_read sums) and the heads' / backbone's other kernels (RoIAlign, DynamicConv, attention, head tail, max pool) */
int dvid_profile_dump(const char* path);

#ifdef __cplusplus
}
#endif
#endif
