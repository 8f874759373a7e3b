// The stand-alone ops of the C ABI (include/dvid_hip.h): one thin wrapper per kernel launcher, for the tests and for callers that
// run a single layer -- argument checks, pointer casts, the error message.  No model state.
#include "runtime.h"

extern "C" {
int dvid_roialign_v2_multilevel(const void* p3, const void* p4, const void* p5, int n_frames, int height, int width, int channels,
                                const float* boxes, int boxes_per_frame, void* roi_out, float* mean_out, void* stream) {
    const void* levels[3] = {p3, p4, p5};
    return dvid_roialign_v2_levels(levels, 3, n_frames, height, width, channels, boxes, boxes_per_frame, roi_out, mean_out, stream);
}

int dvid_roialign_v2_levels(const void* const* levels, int n_levels, int n_frames, int height, int width, int channels, const float* boxes,
                            int boxes_per_frame, void* roi_out, float* mean_out, void* stream) {
    g_err[0] = 0;
    if (!pyramid_ok(levels, n_levels)) FAIL(DVID_ERR_ARG, "the pyramid is 3 maps (p3..p5) or 4 (p2..p5), none of them null (got n_levels %d)", n_levels);
    if (height % 32 || width % 32) FAIL(DVID_ERR_ARG, "height/width must be multiples of 32");
    TRY(dvid_roialign_launch(roi_levels<half_t>(levels, n_levels, height, width, 0, channels), channels, boxes, n_frames, boxes_per_frame,
                             reinterpret_cast<half_t*>(roi_out), mean_out, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_roialign_v2_multilevel_f32(const float* p3, const float* p4, const float* p5, int n_frames, int height, int width, int channels,
                                    const float* boxes, int boxes_per_frame, float* roi_out, float* mean_out, void* stream) {
    const float* levels[3] = {p3, p4, p5};
    return dvid_roialign_v2_levels_f32(levels, 3, n_frames, height, width, channels, boxes, boxes_per_frame, roi_out, mean_out, stream);
}

int dvid_roialign_v2_levels_f32(const float* const* levels, int n_levels, int n_frames, int height, int width, int channels, const float* boxes,
                                int boxes_per_frame, float* roi_out, float* mean_out, void* stream) {
    g_err[0] = 0;
    const void* const* lp = reinterpret_cast<const void* const*>(levels);
    if (!pyramid_ok(lp, n_levels)) FAIL(DVID_ERR_ARG, "the pyramid is 3 maps (p3..p5) or 4 (p2..p5), none of them null (got n_levels %d)", n_levels);
    if (height % 32 || width % 32) FAIL(DVID_ERR_ARG, "height/width must be multiples of 32");
    TRY(dvid_f32_roialign_launch(roi_levels<float>(lp, n_levels, height, width, 0, channels), channels, boxes, n_frames, boxes_per_frame, roi_out, mean_out,
                                 reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_conv2d_nhwc_f32(const float* in, const float* w, const void* w_hi, const void* w_lo, const float* bias, const float* row_scale, const float* residual,
                         float* out, int n, int h, int wd, int cin, int cout, int kh, int kw, int stride, int pad, int kpad, int relu, int residual_mode,
                         void* stream) {
    g_err[0] = 0;
    if (cin % 4 || kpad % 16 || kpad < kh * kw * cin || pad < 0) FAIL(DVID_ERR_ARG, "fp32 conv: cin %% 4 == 0, kpad %% 16 == 0, kpad >= kh*kw*cin, pad >= 0");
    ConvW cw;
    cw.w32 = const_cast<float*>(w);
    cw.w16hi = reinterpret_cast<half_t*>(const_cast<void*>(w_hi));
    cw.w16lo = reinterpret_cast<half_t*>(const_cast<void*>(w_lo));
    cw.bias = const_cast<float*>(bias);
    cw.wscale32 = const_cast<float*>(row_scale);
    cw.cin32 = cin;
    cw.cin_real = cin;
    cw.cout = cout;
    cw.kh = kh;
    cw.kw = kw;
    cw.stride = stride;
    cw.pad = pad;
    cw.kpad32 = kpad;
    TRY(conv_run32(cw, in, n, h, wd, out, reinterpret_cast<hipStream_t>(stream), {.relu = relu, .res = residual, .res_mode = residual_mode}));
    return DVID_OK;
}

int dvid_mha_f32(const float* q, const float* k, const float* v, float* out, int batch, int lq, int lk, int nheads, int q_ld, int kv_ld, int out_ld,
                 int64_t q_bs, int64_t kv_bs, int64_t out_bs, void* stream) {
    g_err[0] = 0;
    TRY(dvid_f32_mha_launch(q, k, v, out, batch, lq, lk, nheads, q_ld, kv_ld, out_ld, (long)q_bs, (long)kv_bs, (long)out_bs,
                            reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_swin_window_attn_f32(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                              int nheads, int shift, void* stream) {
    g_err[0] = 0;
    if (!qkv || !qkv_bias || !relbias || !out) FAIL(DVID_ERR_ARG, "swin window attention: null pointer");
    if (batch <= 0 || H <= 0 || W <= 0 || nheads <= 0 || shift < 0 || shift >= 7)
        FAIL(DVID_ERR_ARG, "swin window attention: bad sizes (batch %d, %d x %d tokens, %d heads, shift %d)", batch, H, W, nheads, shift);
    const int rc = dvid_f32_swin_window_attn_launch(qkv, qkv_bias, relbias, out, batch, H, W, C, nheads, shift, reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "swin window attention (fp32): C %d with %d heads on %d x %d x %d tokens is not supported", C, nheads, batch, H, W);
    return DVID_OK;
}

int dvid_swin_window_attn_f32_ws(const float* qkv, const float* qkv_bias, const float* relbias, float* out, int batch, int H, int W, int C,
                                 int nheads, int shift, int window, void* stream) {
    if (window == 7) return dvid_swin_window_attn_f32(qkv, qkv_bias, relbias, out, batch, H, W, C, nheads, shift, stream);
    g_err[0] = 0;
    if (window != 12) FAIL(DVID_ERR_UNSUPPORTED, "swin window attention: window size %d (7 and 12 are built)", window);
    if (!qkv || !qkv_bias || !relbias || !out) FAIL(DVID_ERR_ARG, "swin window attention: null pointer");
    if (batch <= 0 || H <= 0 || W <= 0 || nheads <= 0 || shift < 0 || shift >= window)
        FAIL(DVID_ERR_ARG, "swin window attention: bad sizes (batch %d, %d x %d tokens, %d heads, shift %d, window %d)", batch, H, W, nheads, shift, window);
    const int rc = dvid_f32_swin_window12_attn_launch(qkv, qkv_bias, relbias, out, batch, H, W, C, nheads, shift, reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "swin window attention (fp32, window 12): C %d with %d heads on %d x %d x %d tokens is not supported", C, nheads, batch, H, W);
    return DVID_OK;
}

int dvid_dynconv_f32(const float* roi, const float* params, const float* g1, const float* b1, const float* g2, const float* b2, float* out,
                     int rows, void* stream) {
    g_err[0] = 0;
    TRY(dvid_f32_dynconv_launch(roi, params, g1, b1, g2, b2, out, rows, nullptr, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_select_topk_features(const float* logits, int n_frames, int mm, int num_classes, int k1, int k2, const float* feats,
                              int hidden, float* out_k1, float* out_k2, void* stream) {
    g_err[0] = 0;
    TRY(dvid_topk_mask_launch(logits, n_frames, mm, num_classes, k1, k2, feats, hidden, out_k1, out_k2,
                              reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_counter_normal(float* out, int64_t per_image, int n_images, uint64_t key0, void* stream) {
    g_err[0] = 0;
    if (!out || per_image < 0 || n_images < 0 || n_images > 65535) FAIL(DVID_ERR_ARG, "dvid_counter_normal: bad arguments");
    TRY(dvid_counter_normal_launch(out, (long)per_image, n_images, key0, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_counter_normal_strided(float* out, int64_t per_image, int n_images, uint64_t key0, uint64_t key_stride, void* stream) {
    g_err[0] = 0;
    if (!out || per_image < 0 || n_images < 0 || n_images > 65535) FAIL(DVID_ERR_ARG, "dvid_counter_normal_strided: bad arguments");
    TRY(dvid_counter_normal_launch(out, (long)per_image, n_images, key0, reinterpret_cast<hipStream_t>(stream), key_stride));
    return DVID_OK;
}

int dvid_noise_to_boxes(const float* x, float* boxes, int n, float snr_scale, float img_w, float img_h, void* stream) {
    g_err[0] = 0;
    TRY(dvid_noise_to_boxes_launch(x, boxes, n, snr_scale, img_w, img_h, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_noise_to_boxes_sizes(const float* x, float* boxes, int n, int mm, float snr_scale, const float* sizes, void* stream) {
    g_err[0] = 0;
    if (n < 0 || mm < 1 || n % mm) FAIL(DVID_ERR_ARG, "noise_to_boxes: %d boxes are not whole frames of %d", n, mm);
    if (n > 0 && (!x || !boxes || !sizes)) FAIL(DVID_ERR_ARG, "noise_to_boxes: null pointer");
    TRY(dvid_noise_to_boxes_sizes_launch(x, boxes, n, mm, snr_scale, sizes, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_ddim_renew_step(const float* logits, const float* boxes, const float* x_t, const float* noise, const float* fresh,
                         float* x_next, int n_frames, int mm, int c, float img_w, float img_h, float snr_scale,
                         float sqrt_recip_ac, float sqrt_recipm1_ac, float sqrt_ac_next, float coef_c, float sigma, float keep_thr,
                         void* stream) {
    g_err[0] = 0;
    TRY(dvid_ddim_renew_launch(logits, boxes, x_t, noise, fresh, x_next, n_frames, mm, c, img_w, img_h, snr_scale, sqrt_recip_ac,
                               sqrt_recipm1_ac, sqrt_ac_next, coef_c, sigma, keep_thr, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_ddim_renew_step_sizes(const float* logits, const float* boxes, const float* x_t, const float* noise, const float* fresh,
                               float* x_next, int n_frames, int mm, int c, const float* sizes, float snr_scale, float sqrt_recip_ac,
                               float sqrt_recipm1_ac, float sqrt_ac_next, float coef_c, float sigma, float keep_thr, void* stream) {
    g_err[0] = 0;
    if (n_frames > 0 && !sizes) FAIL(DVID_ERR_ARG, "ddim_renew_step: null size table");
    TRY(dvid_ddim_renew_sizes_launch(logits, boxes, x_t, noise, fresh, x_next, n_frames, mm, c, sizes, snr_scale, sqrt_recip_ac, sqrt_recipm1_ac,
                                     sqrt_ac_next, coef_c, sigma, keep_thr, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

// bytes of the candidate lists (boxes, scores, labels) at the head of dvid_postproc_topk_nms's scratch
static size_t postproc_cand_bytes(int nsets, int n_frames, int mm) { return (size_t)n_frames * nsets * mm * 6 * 4; }

int64_t dvid_postproc_scratch_bytes(int nsets, int n_frames, int mm) {
    if (nsets <= 0 || n_frames <= 0 || mm <= 0) return 0;
    const size_t cand = postproc_cand_bytes(nsets, n_frames, mm);
    const long n = (long)nsets * mm;
    if (n > DVID_NMS_MAX_CANDIDATES || dvid_nms_frames_fits_lds((int)n)) return (int64_t)cand;
    return (int64_t)(cand + dvid_nms_tiled_scratch_size(n_frames, (int)n));
}

int64_t dvid_nms_tiled_scratch_bytes(int n_frames, int n) { return (int64_t)dvid_nms_tiled_scratch_size(n_frames, n); }

// dvid_postproc_topk_nms / _sizes: nms(cb, cs, cl, tiled scratch or null, stream) launches the NMS form the shape takes with the caller's sizes
extern "C++" template <typename NMS>
static int postproc_topk_nms(const float* logits, const float* boxes, int nsets, int n_frames, int mm, int c, void* scratch, void* stream, NMS nms) {
    g_err[0] = 0;
    if (!scratch) FAIL(DVID_ERR_ARG, "scratch required");
    if (nsets <= 0 || n_frames < 0 || mm <= 0) FAIL(DVID_ERR_ARG, "postproc: bad sizes (%d sets, %d frames, %d boxes)", nsets, n_frames, mm);
    const long n = (long)nsets * mm;
    if (n > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED,
             "postproc: %ld candidates per frame (%d sets x %d boxes) exceed the limit of %d: (SAMPLE_STEP - 1) * NUM_PROPOSALS, or NUM_PROPOSALS "
             "at SAMPLE_STEP 1, must stay within %d",
             n, nsets, mm, DVID_NMS_MAX_CANDIDATES, DVID_NMS_MAX_CANDIDATES);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t ncand = (size_t)n_frames * nsets * mm;
    float* cb = reinterpret_cast<float*>(scratch);
    float* cs = cb + ncand * 4;
    int* cl = reinterpret_cast<int*>(cs + ncand);
    TRY(dvid_topk_candidates_launch(logits, boxes, n_frames, nsets, mm, c, cb, cs, cl, s));
    // the shapes nms_frame_kernel cannot hold in LDS take the tiled form, its scratch behind the candidate lists
    TRY(nms(cb, cs, cl, dvid_nms_frames_fits_lds((int)n) ? nullptr : reinterpret_cast<char*>(scratch) + postproc_cand_bytes(nsets, n_frames, mm), s));
    return DVID_OK;
}

int dvid_postproc_topk_nms(const float* logits, const float* boxes, int nsets, int n_frames, int mm, int c, float img_w, float img_h,
                           float iou_threshold, int use_nms, float* out_boxes, float* out_scores, int* out_labels, int* out_counts,
                           void* scratch, void* stream) {
    return postproc_topk_nms(logits, boxes, nsets, n_frames, mm, c, scratch, stream, [=](const float* cb, const float* cs, const int* cl, void* tiled, hipStream_t s) {
        return tiled ? dvid_nms_frames_tiled_launch(cb, cs, cl, n_frames, nsets * mm, img_w, img_h, iou_threshold, use_nms, nsets * mm, out_boxes, out_scores,
                                                    out_labels, out_counts, tiled, s)
                     : dvid_nms_frames_launch(cb, cs, cl, n_frames, nsets * mm, img_w, img_h, iou_threshold, use_nms, nsets * mm, out_boxes, out_scores, out_labels,
                                              out_counts, s);
    });
}

int dvid_postproc_topk_nms_sizes(const float* logits, const float* boxes, int nsets, int n_frames, int mm, int c, const float* sizes,
                                 float iou_threshold, int use_nms, float* out_boxes, float* out_scores, int* out_labels, int* out_counts,
                                 void* scratch, void* stream) {
    if (n_frames > 0 && !sizes) {
        g_err[0] = 0;
        FAIL(DVID_ERR_ARG, "postproc: null size table");
    }
    return postproc_topk_nms(logits, boxes, nsets, n_frames, mm, c, scratch, stream, [=](const float* cb, const float* cs, const int* cl, void* tiled, hipStream_t s) {
        return tiled ? dvid_nms_frames_tiled_sizes_launch(cb, cs, cl, n_frames, nsets * mm, sizes, iou_threshold, use_nms, nsets * mm, out_boxes, out_scores,
                                                          out_labels, out_counts, tiled, s)
                     : dvid_nms_frames_sizes_launch(cb, cs, cl, n_frames, nsets * mm, sizes, iou_threshold, use_nms, nsets * mm, out_boxes, out_scores, out_labels,
                                                    out_counts, s);
    });
}

int dvid_topk_candidates_stream(const float* logits, const float* boxes, int nsets, int n_frames, int mm, int c, float* cand_boxes,
                                float* cand_scores, int* cand_labels, void* stream) {
    g_err[0] = 0;
    if (!logits || !boxes || !cand_boxes || !cand_scores || !cand_labels) FAIL(DVID_ERR_ARG, "streaming top-k: null pointer");
    if (nsets <= 0 || n_frames < 0 || mm <= 0 || c <= 0)
        FAIL(DVID_ERR_ARG, "streaming top-k: bad sizes (%d sets, %d frames, %d boxes, %d classes)", nsets, n_frames, mm, c);
    if (mm > DVID_NMS_MAX_CANDIDATES || c > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "streaming top-k: %d boxes x %d classes exceed the limits of %d boxes (DVID_NMS_MAX_CANDIDATES) and %d classes (DVID_MAX_CLASSES)",
             mm, c, DVID_NMS_MAX_CANDIDATES, DVID_MAX_CLASSES);
    TRY(dvid_topk_stream_launch(logits, boxes, n_frames, nsets, mm, c, cand_boxes, cand_scores, cand_labels, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_nms_frames_tiled(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_frames, int n, float img_w,
                          float img_h, float iou_threshold, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels,
                          int* out_counts, void* scratch, void* stream) {
    g_err[0] = 0;
    if (!cand_boxes || !cand_scores || !cand_labels || !out_boxes || !out_scores || !out_labels || !out_counts || !scratch)
        FAIL(DVID_ERR_ARG, "tiled NMS: null pointer");
    if (n_frames < 0 || n < 1 || out_cap < n) FAIL(DVID_ERR_ARG, "tiled NMS: bad sizes (%d frames, %d candidates, out_cap %d)", n_frames, n, out_cap);
    if (n > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "tiled NMS: %d candidates per frame exceed the limit of %d ((SAMPLE_STEP - 1) * NUM_PROPOSALS)", n, DVID_NMS_MAX_CANDIDATES);
    TRY(dvid_nms_frames_tiled_launch(cand_boxes, cand_scores, cand_labels, n_frames, n, img_w, img_h, iou_threshold, use_nms, out_cap, out_boxes,
                                     out_scores, out_labels, out_counts, scratch, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_nms_frames_tiled_sizes(const float* cand_boxes, const float* cand_scores, const int* cand_labels, int n_frames, int n, const float* sizes,
                                float iou_threshold, int use_nms, int out_cap, float* out_boxes, float* out_scores, int* out_labels,
                                int* out_counts, void* scratch, void* stream) {
    g_err[0] = 0;
    if (!cand_boxes || !cand_scores || !cand_labels || !out_boxes || !out_scores || !out_labels || !out_counts || !scratch || !sizes)
        FAIL(DVID_ERR_ARG, "tiled NMS: null pointer");
    if (n_frames < 0 || n < 1 || out_cap < n) FAIL(DVID_ERR_ARG, "tiled NMS: bad sizes (%d frames, %d candidates, out_cap %d)", n_frames, n, out_cap);
    if (n > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "tiled NMS: %d candidates per frame exceed the limit of %d ((SAMPLE_STEP - 1) * NUM_PROPOSALS)", n, DVID_NMS_MAX_CANDIDATES);
    TRY(dvid_nms_frames_tiled_sizes_launch(cand_boxes, cand_scores, cand_labels, n_frames, n, sizes, iou_threshold, use_nms, out_cap, out_boxes,
                                           out_scores, out_labels, out_counts, scratch, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

// A host CSR start table of n units ("frame", "image", "video"): [0] is 0 and it never decreases; with a limit (LIMIT(macro)) no unit holds
// more ground-truth boxes than that.  *most, when given, gets the greatest count of one unit.
#define LIMIT(macro) macro, #macro
static int csr_starts_ok(const char* entry, const char* table, const char* unit, const int* starts, int n, int* most = nullptr, int limit = 0,
                         const char* limit_name = nullptr) {
    if (starts[0] != 0) FAIL(DVID_ERR_ARG, "%s: %s[0] is %d, not 0", entry, table, starts[0]);
    int top = 0;
    for (int i = 0; i < n; ++i) {
        const int g = starts[i + 1] - starts[i];
        if (g < 0) FAIL(DVID_ERR_ARG, "%s: %s decreases at %s %d", entry, table, unit, i);
        if (limit_name && g > limit)
            FAIL(DVID_ERR_UNSUPPORTED, "%s: %s %d holds %d ground-truth boxes, the limit is %d (%s)", entry, unit, i, g, limit, limit_name);
        top = g > top ? g : top;
    }
    if (most) *most = top;
    return DVID_OK;
}

static int scratch_ok(const char* entry, const void* scratch, long long scratch_bytes, long long need) {
    if (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 15))
        FAIL(DVID_ERR_ARG, "%s: the scratch holds %lld bytes, %lld are needed (16-byte aligned)", entry, scratch_bytes, need);
    return DVID_OK;
}

int64_t dvid_seq_nms_scratch_bytes(const int* class_counts, const int* video_starts, int n_videos, int num_classes) {
    return (int64_t)dvid_seq_nms_scratch_size(class_counts, video_starts, n_videos, num_classes);
}

int dvid_seq_nms_video(const float* dets, const int* counts, const int* class_counts, const int* video_starts, int n_videos, int cap,
                       int num_classes, unsigned char* keep, float* scores, int* status, void* scratch, int64_t scratch_bytes, void* stream) {
    g_err[0] = 0;
    if (!dets || !counts || !class_counts || !video_starts || !keep || !scores || !status) FAIL(DVID_ERR_ARG, "Seq-NMS: null pointer");
    if (n_videos < 1 || cap < 1 || num_classes < 1) FAIL(DVID_ERR_ARG, "Seq-NMS: bad sizes (%d videos, %d rows per frame, %d classes)", n_videos, cap, num_classes);
    TRY(csr_starts_ok("Seq-NMS", "video_starts", "video", video_starts, n_videos));
    if (cap > DVID_NMS_MAX_CANDIDATES || num_classes > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "Seq-NMS: %d rows per frame x %d classes exceed the limits of %d rows (DVID_NMS_MAX_CANDIDATES) and %d classes (DVID_MAX_CLASSES)",
             cap, num_classes, DVID_NMS_MAX_CANDIDATES, DVID_MAX_CLASSES);
    const long long need = dvid_seq_nms_scratch_size(class_counts, video_starts, n_videos, num_classes);
    if (need < 0) FAIL(DVID_ERR_ARG, "Seq-NMS: a negative entry in class_counts");
    if (need > DVID_SEQ_NMS_MAX_SCRATCH_BYTES)
        FAIL(DVID_ERR_UNSUPPORTED, "Seq-NMS: %lld bytes of link rows and tables for %d frames x %d classes exceed the limit of %lld (DVID_SEQ_NMS_MAX_SCRATCH_BYTES): "
             "run fewer videos per call", need, video_starts[n_videos], num_classes, (long long)DVID_SEQ_NMS_MAX_SCRATCH_BYTES);
    if (need > 0) TRY(scratch_ok("Seq-NMS", scratch, scratch_bytes, need));
    TRY(dvid_seq_nms_launch(dets, counts, class_counts, video_starts, n_videos, cap, num_classes, keep, scores, status, scratch,
                            reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_vid_eval_match(const float* dets, const int* counts, int n_frames, int cap, const float* gt_boxes, const int* gt_labels,
                        const int* gt_starts, const int* gt_starts_host, int label_min, int label_max, const double* motion,
                        const double* ranges, const double* empty_w, int n_ranges, float iou_thresh, int num_classes, signed char* match,
                        double* weight, int* rank, double* n_pos, int* top_row, signed char* top_hit, void* stream) {
    g_err[0] = 0;
    if (!dets || !counts || !gt_starts || !gt_starts_host || !ranges || !empty_w || !match || !weight || !rank || !n_pos || !top_row || !top_hit)
        FAIL(DVID_ERR_ARG, "VID evaluation: null pointer");
    if (n_frames < 0 || cap < 1 || num_classes < 1) FAIL(DVID_ERR_ARG, "VID evaluation: bad sizes (%d frames, %d rows per frame, %d classes)", n_frames, cap, num_classes);
    if (cap > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "VID evaluation: %d rows per frame exceed the limit of %d (DVID_NMS_MAX_CANDIDATES)", cap, DVID_NMS_MAX_CANDIDATES);
    if (num_classes > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "VID evaluation: %d classes exceed the limit of %d (DVID_MAX_CLASSES)", num_classes, DVID_MAX_CLASSES);
    if (n_ranges < 1 || n_ranges > DVID_VID_EVAL_MAX_RANGES)
        FAIL(DVID_ERR_UNSUPPORTED, "VID evaluation: %d motion ranges, the limit is 1 .. %d (DVID_VID_EVAL_MAX_RANGES)", n_ranges, DVID_VID_EVAL_MAX_RANGES);
    if (label_min < 0 || label_max > num_classes)
        FAIL(DVID_ERR_UNSUPPORTED, "VID evaluation: labels %d .. %d leave the range 0 .. %d (num_classes)", label_min, label_max, num_classes);
    TRY(csr_starts_ok("VID evaluation", "gt_starts", "frame", gt_starts_host, n_frames, nullptr, LIMIT(DVID_VID_EVAL_MAX_GT)));
    if (gt_starts_host[n_frames] > 0 && (!gt_boxes || !gt_labels)) FAIL(DVID_ERR_ARG, "VID evaluation: null ground truth");
    TRY(dvid_vid_eval_match_launch(dets, counts, n_frames, cap, gt_boxes, gt_labels, gt_starts, motion, ranges, empty_w, n_ranges, iou_thresh, num_classes,
                                   match, weight, rank, n_pos, top_row, top_hit, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_q_sample_boxes(const float* gt_cxcywh, const int* gt_starts, const int* gt_starts_host, int n, int m, const int* t, const int* t_host,
                        const float* sqrt_ac, const float* sqrt_omac, int timesteps, const float* noise, const float* placeholder, float snr_scale,
                        const float* sizes, float* boxes, void* stream) {
    g_err[0] = 0;
    if (n < 0 || m < 1 || timesteps < 1) FAIL(DVID_ERR_ARG, "q_sample_boxes: bad sizes (%d images, %d proposals, %d time steps)", n, m, timesteps);
    if (n == 0) return DVID_OK;
    if (!gt_starts || !gt_starts_host || !t || !t_host || !sqrt_ac || !sqrt_omac || !noise || !placeholder || !sizes || !boxes)
        FAIL(DVID_ERR_ARG, "q_sample_boxes: null pointer");
    TRY(csr_starts_ok("q_sample_boxes", "gt_starts", "image", gt_starts_host, n));
    for (int i = 0; i < n; ++i) {
        if (const int g = gt_starts_host[i + 1] - gt_starts_host[i]; g > m)
            FAIL(DVID_ERR_UNSUPPORTED, "q_sample_boxes: image %d holds %d ground-truth boxes, NUM_PROPOSALS is %d (the reference's random subset is not built)",
                 i, g, m);
        if (t_host[i] < 0 || t_host[i] >= timesteps) FAIL(DVID_ERR_ARG, "q_sample_boxes: t[%d] is %d, outside 0 .. %d", i, t_host[i], timesteps - 1);
    }
    if (gt_starts_host[n] > 0 && !gt_cxcywh) FAIL(DVID_ERR_ARG, "q_sample_boxes: null ground truth");
    TRY(dvid_q_sample_boxes_launch(gt_cxcywh, gt_starts, n, m, t, sqrt_ac, sqrt_omac, timesteps, noise, placeholder, snr_scale, sizes, boxes,
                                   reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int64_t dvid_set_criterion_scratch_bytes(int n_sets, int n, int m, int gmax) { return dvid_set_criterion_scratch_bytes_host(n_sets, n, m, gmax); }

int dvid_set_criterion(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes, const int* gt_labels,
                       const int* gt_starts, const int* gt_starts_host, const float* sizes, float alpha, float gamma, int ota_k, float cost_class,
                       float cost_bbox, float cost_giou, int* assign, int* matched_query, int gmax, double* sums, int* status, void* scratch,
                       int64_t scratch_bytes, void* stream) {
    g_err[0] = 0;
    if (n_sets < 0 || n < 0 || m < 1 || c < 1 || gmax < 0) FAIL(DVID_ERR_ARG, "set criterion: bad sizes (%d head outputs, %d images, %d queries, %d classes)", n_sets, n, m, c);
    if (ota_k < 1 || ota_k > DVID_CRITERION_MAX_OTA_K)
        FAIL(DVID_ERR_UNSUPPORTED, "set criterion: OTA_K %d, the limit is 1 .. %d (DVID_CRITERION_MAX_OTA_K)", ota_k, DVID_CRITERION_MAX_OTA_K);
    if (m < ota_k || m > DVID_CRITERION_MAX_ROWS)
        FAIL(DVID_ERR_UNSUPPORTED, "set criterion: %d queries per image, the limit is OTA_K = %d <= queries <= %d (DVID_CRITERION_MAX_ROWS)", m, ota_k,
             DVID_CRITERION_MAX_ROWS);
    if (c > DVID_MAX_CLASSES) FAIL(DVID_ERR_UNSUPPORTED, "set criterion: %d classes exceed the limit of %d (DVID_MAX_CLASSES)", c, DVID_MAX_CLASSES);
    if (gmax > DVID_CRITERION_MAX_GT)
        FAIL(DVID_ERR_UNSUPPORTED, "set criterion: gmax %d exceeds the limit of %d (DVID_CRITERION_MAX_GT)", gmax, DVID_CRITERION_MAX_GT);
    if ((long long)n_sets * n > 65535) FAIL(DVID_ERR_UNSUPPORTED, "set criterion: %d head outputs x %d images exceed 65535 sets per call", n_sets, n);
    if (n_sets == 0 || n == 0) return DVID_OK;
    if (!logits || !boxes || !gt_starts || !gt_starts_host || !sizes || !assign || !matched_query || !sums || !status) FAIL(DVID_ERR_ARG, "set criterion: null pointer");
    int most = 0;
    TRY(csr_starts_ok("set criterion", "gt_starts", "image", gt_starts_host, n, &most, LIMIT(DVID_CRITERION_MAX_GT)));
    for (int i = 0; most > gmax && i < n; ++i)          // name the first image over gmax
        if (const int g = gt_starts_host[i + 1] - gt_starts_host[i]; g > gmax)
            FAIL(DVID_ERR_ARG, "set criterion: image %d holds %d ground-truth boxes, gmax is %d", i, g, gmax);
    if (gt_starts_host[n] > 0 && (!gt_boxes || !gt_labels)) FAIL(DVID_ERR_ARG, "set criterion: null ground truth");
    const long long need = dvid_set_criterion_scratch_bytes_host(n_sets, n, m, gmax);
    TRY(scratch_ok("set criterion", scratch, scratch_bytes, need));
    TRY(dvid_set_criterion_launch(logits, boxes, n_sets, n, m, c, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma, ota_k, cost_class, cost_bbox, cost_giou,
                                  assign, matched_query, gmax, sums, status, scratch, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_set_criterion_backward(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes, const int* gt_labels,
                                const int* gt_starts, const int* gt_starts_host, const float* sizes, float alpha, float gamma, const int* assign,
                                const int* status, const double* coef, float* d_logits, float* d_boxes, void* stream) {
    g_err[0] = 0;
    if (n_sets < 0 || n < 0 || m < 1 || c < 1)
        FAIL(DVID_ERR_ARG, "set criterion backward: bad sizes (%d head outputs, %d images, %d queries, %d classes)", n_sets, n, m, c);
    if (m > DVID_CRITERION_MAX_ROWS)
        FAIL(DVID_ERR_UNSUPPORTED, "set criterion backward: %d queries per image, the limit is %d (DVID_CRITERION_MAX_ROWS)", m, DVID_CRITERION_MAX_ROWS);
    if (c > DVID_MAX_CLASSES) FAIL(DVID_ERR_UNSUPPORTED, "set criterion backward: %d classes exceed the limit of %d (DVID_MAX_CLASSES)", c, DVID_MAX_CLASSES);
    if ((long long)n_sets * n > 65535)
        FAIL(DVID_ERR_UNSUPPORTED, "set criterion backward: %d head outputs x %d images exceed 65535 sets per call", n_sets, n);
    if (n_sets == 0 || n == 0) return DVID_OK;
    if (!logits || !boxes || !gt_starts || !gt_starts_host || !sizes || !assign || !status || !coef || !d_logits || !d_boxes)
        FAIL(DVID_ERR_ARG, "set criterion backward: null pointer");
    TRY(csr_starts_ok("set criterion backward", "gt_starts", "image", gt_starts_host, n, nullptr, LIMIT(DVID_CRITERION_MAX_GT)));
    if (gt_starts_host[n] > 0 && (!gt_boxes || !gt_labels)) FAIL(DVID_ERR_ARG, "set criterion backward: null ground truth");
    TRY(dvid_set_criterion_backward_launch(logits, boxes, n_sets, n, m, c, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma, assign, status, coef, d_logits,
                                           d_boxes, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int64_t dvid_head_tail_backward_scratch_bytes(int n, int m, int dff, int num_classes, int num_cls, int num_reg, int has_cond) {
    return dvid_head_tail_backward_scratch_bytes_host(n, m, dff, num_classes, num_cls, num_reg, has_cond);
}

int dvid_head_tail_backward(const float* x, const float* boxes_in, const float* time_emb, const float* cond, int n, int m, int hidden, int dff,
                            int num_classes, int num_cls, int num_reg, const float* const* params, int n_params, float wx, float wy, float ww, float wh,
                            float scale_clamp, const float* d_logits, const float* d_boxes, const float* d_obj, float* logits_out, float* boxes_out,
                            float* obj_out, float* d_x, float* d_time_emb, float* d_cond, float* const* grads, void* scratch, int64_t scratch_bytes,
                            void* stream) {
    g_err[0] = 0;
    const char* what = "head tail backward";
    if (hidden != 256) FAIL(DVID_ERR_UNSUPPORTED, "%s: hidden size %d, the kernels take 256", what, hidden);
    if (dff < DVID_HEAD_TAIL_BWD_TILE || dff % DVID_HEAD_TAIL_BWD_TILE)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: dim_feedforward %d is not a positive multiple of the product tile, %d (DVID_HEAD_TAIL_BWD_TILE)", what, dff,
             DVID_HEAD_TAIL_BWD_TILE);
    if (num_classes < 1 || num_classes > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: %d classes, the limit is 1 .. %d (DVID_MAX_CLASSES)", what, num_classes, DVID_MAX_CLASSES);
    if (num_cls < 0 || num_cls > 4 || num_reg < 0 || num_reg > 4)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: NUM_CLS %d / NUM_REG %d, the forward takes 0 .. 4 of each", what, num_cls, num_reg);
    if (n < 1 || m < 1) FAIL(DVID_ERR_ARG, "%s: %d images x %d boxes: no rows", what, n, m);
    if (n > 65535 || (long long)n * m > DVID_HEAD_TAIL_BWD_MAX_ROWS)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: %d images x %d boxes, the limit is 65535 images and %d rows (DVID_HEAD_TAIL_BWD_MAX_ROWS)", what, n, m,
             DVID_HEAD_TAIL_BWD_MAX_ROWS);
    if (n_params != 14 + 3 * (num_cls + num_reg))
        FAIL(DVID_ERR_ARG, "%s: %d parameter pointers, NUM_CLS %d and NUM_REG %d make it %d", what, n_params, num_cls, num_reg, 14 + 3 * (num_cls + num_reg));
    if (!x || !boxes_in || !time_emb || !params || !scratch) FAIL(DVID_ERR_ARG, "%s: null pointer", what);
    const bool backward = grads || d_x || d_time_emb || d_cond;
    if (backward && (!grads || !d_x || !d_time_emb || (cond && !d_cond))) FAIL(DVID_ERR_ARG, "%s: null pointer among the gradient outputs", what);
    if (!backward && (d_logits || d_boxes || d_obj)) FAIL(DVID_ERR_ARG, "%s: cotangents without gradient outputs", what);
    for (int i = 0; i < n_params; ++i) {
        if ((i == 8 || i == 9) && !cond) continue;          // c_mlp.1 belongs to the cond head
        if (!params[i] || (backward && !grads[i])) FAIL(DVID_ERR_ARG, "%s: null pointer for parameter %d", what, i);
    }
    TRY(scratch_ok(what, scratch, scratch_bytes, dvid_head_tail_backward_scratch_bytes_host(n, m, dff, num_classes, num_cls, num_reg, cond != nullptr)));
    HeadTailBwdArgs a{x, boxes_in, time_emb, cond, n, m, dff, num_classes, num_cls, num_reg, params, wx, wy, ww, wh, scale_clamp, d_logits, d_boxes, d_obj,
                      logits_out, boxes_out, obj_out, d_x, d_time_emb, d_cond, backward ? grads : nullptr, scratch};
    TRY(dvid_head_tail_backward_launch(a, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int64_t dvid_inst_interact_backward_scratch_bytes(int rows) { return dvid_inst_interact_backward_scratch_bytes_host(rows); }

int dvid_inst_interact_backward(const float* p, const float* roi, int rows, int hidden, int dim_dynamic, int pooler, const float* const* params,
                                int n_params, const float* d_y, float* y_out, float* d_p, float* d_roi, float* const* grads, void* scratch,
                                int64_t scratch_bytes, void* stream) {
    g_err[0] = 0;
    const char* what = "instance interaction backward";
    if (hidden != 256) FAIL(DVID_ERR_UNSUPPORTED, "%s: hidden size %d, the kernels take 256", what, hidden);
    if (dim_dynamic != 64) FAIL(DVID_ERR_UNSUPPORTED, "%s: dim_dynamic %d, the kernels take 64", what, dim_dynamic);
    if (pooler != 7) FAIL(DVID_ERR_UNSUPPORTED, "%s: a %d x %d pooler, the kernels take 7 x 7", what, pooler, pooler);
    if (rows < 1) FAIL(DVID_ERR_ARG, "%s: %d rows", what, rows);
    if (rows > DVID_HEAD_TAIL_BWD_MAX_ROWS)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: %d rows, the limit is %d (DVID_HEAD_TAIL_BWD_MAX_ROWS)", what, rows, DVID_HEAD_TAIL_BWD_MAX_ROWS);
    if (n_params != 12) FAIL(DVID_ERR_ARG, "%s: %d parameter pointers, the link has 12", what, n_params);
    if (!p || !roi || !params || !scratch) FAIL(DVID_ERR_ARG, "%s: null pointer", what);
    const bool backward = grads || d_p || d_roi;
    if (backward && (!grads || !d_p)) FAIL(DVID_ERR_ARG, "%s: null pointer among the gradient outputs", what);
    if (!backward && d_y) FAIL(DVID_ERR_ARG, "%s: a cotangent without gradient outputs", what);
    for (int i = 0; i < n_params; ++i)
        if (!params[i] || (backward && !grads[i])) FAIL(DVID_ERR_ARG, "%s: null pointer for parameter %d", what, i);
    TRY(scratch_ok(what, scratch, scratch_bytes, dvid_inst_interact_backward_scratch_bytes_host(rows)));
    InstInteractBwdArgs a{p, roi, rows, params, d_y, y_out, d_p, d_roi, backward ? grads : nullptr, scratch};
    TRY(dvid_inst_interact_backward_launch(a, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int64_t dvid_self_attn_backward_scratch_bytes(int n, int m) { return dvid_self_attn_backward_scratch_bytes_host(n, m); }

int dvid_self_attn_backward(const float* x, int n, int m, int hidden, int nheads, const float* const* params, int n_params, const float* d_y,
                            float* y_out, float* d_x, float* const* grads, void* scratch, int64_t scratch_bytes, void* stream) {
    g_err[0] = 0;
    const char* what = "self-attention backward";
    if (hidden != 256) FAIL(DVID_ERR_UNSUPPORTED, "%s: hidden size %d, the kernels take 256", what, hidden);
    if (nheads != 8) FAIL(DVID_ERR_UNSUPPORTED, "%s: %d heads, the kernels take 8 of 32", what, nheads);
    if (n < 1 || m < 1) FAIL(DVID_ERR_ARG, "%s: %d images of %d rows", what, n, m);
    if (m > DVID_CRITERION_MAX_ROWS) FAIL(DVID_ERR_UNSUPPORTED, "%s: %d rows per image, the limit is %d (DVID_CRITERION_MAX_ROWS)", what, m, DVID_CRITERION_MAX_ROWS);
    if ((long long)n * m > DVID_HEAD_TAIL_BWD_MAX_ROWS)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: %lld rows, the limit is %d (DVID_HEAD_TAIL_BWD_MAX_ROWS)", what, (long long)n * m, DVID_HEAD_TAIL_BWD_MAX_ROWS);
    if (n > 65535) FAIL(DVID_ERR_UNSUPPORTED, "%s: %d images, the limit is 65535", what, n);
    if (n_params != 6) FAIL(DVID_ERR_ARG, "%s: %d parameter pointers, the link has 6", what, n_params);
    if (!x || !params || !scratch) FAIL(DVID_ERR_ARG, "%s: null pointer", what);
    const bool backward = grads || d_x;
    if (backward && (!grads || !d_x)) FAIL(DVID_ERR_ARG, "%s: null pointer among the gradient outputs", what);
    if (!backward && d_y) FAIL(DVID_ERR_ARG, "%s: a cotangent without gradient outputs", what);
    for (int i = 0; i < n_params; ++i)
        if (!params[i] || (backward && !grads[i])) FAIL(DVID_ERR_ARG, "%s: null pointer for parameter %d", what, i);
    TRY(scratch_ok(what, scratch, scratch_bytes, dvid_self_attn_backward_scratch_bytes_host(n, m)));
    SelfAttnBwdArgs a{x, n, m, params, d_y, y_out, d_x, backward ? grads : nullptr, scratch};
    TRY(dvid_self_attn_backward_launch(a, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

// What dvid_coco_eval_match and dvid_lvis_eval_match check alike; `what` names the protocol, `pointers` is false when one the entry needs
// is null, *max_gt gets the greatest box count of one image
static int image_eval_args_ok(const char* what, bool pointers, int n_images, int cap, int num_classes, const int* gt_starts_host, int limit,
                              const char* limit_name, int* max_gt) {
    if (!pointers) FAIL(DVID_ERR_ARG, "%s: null pointer", what);
    if (n_images < 0 || cap < 1 || num_classes < 1) FAIL(DVID_ERR_ARG, "%s: bad sizes (%d images, %d rows per image, %d classes)", what, n_images, cap, num_classes);
    if (cap > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: %d rows per image exceed the limit of %d (DVID_NMS_MAX_CANDIDATES)", what, cap, DVID_NMS_MAX_CANDIDATES);
    if (num_classes > DVID_MAX_CLASSES) FAIL(DVID_ERR_UNSUPPORTED, "%s: %d classes exceed the limit of %d (DVID_MAX_CLASSES)", what, num_classes, DVID_MAX_CLASSES);
    return csr_starts_ok(what, "gt_starts", "image", gt_starts_host, n_images, max_gt, limit, limit_name);
}

int dvid_coco_eval_match(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                         const unsigned char* gt_crowd, const int* gt_labels, const int* gt_starts, const int* gt_starts_host,
                         const double* iou_thrs, const double* area_ranges, int num_classes, signed char* match, signed char* ignore,
                         int* rank, int* npig, void* stream) {
    g_err[0] = 0;
    TRY(image_eval_args_ok("COCO evaluation", dets && counts && gt_starts && gt_starts_host && iou_thrs && area_ranges && match && ignore && rank && npig,
                           n_images, cap, num_classes, gt_starts_host, LIMIT(DVID_COCO_EVAL_MAX_GT), nullptr));
    if (gt_starts_host[n_images] > 0 && (!gt_boxes || !gt_areas || !gt_crowd || !gt_labels)) FAIL(DVID_ERR_ARG, "COCO evaluation: null ground truth");
    TRY(dvid_coco_eval_match_launch(dets, counts, n_images, cap, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, iou_thrs, area_ranges, num_classes,
                                    match, ignore, rank, npig, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_lvis_eval_match(const float* dets, const int* counts, int n_images, int cap, const double* gt_boxes, const double* gt_areas,
                         const unsigned char* gt_ignore, const int* gt_labels, const int* gt_starts, const int* gt_starts_host,
                         const int* neg_starts, const int* neg_labels, const int* neg_starts_host, const int* nex_starts, const int* nex_labels,
                         const int* nex_starts_host, const double* iou_thrs, const double* area_ranges, int num_classes, signed char* match,
                         signed char* ignore, int* rank, int* npig, void* stream) {
    g_err[0] = 0;
    int max_gt = 0;
    TRY(image_eval_args_ok("LVIS evaluation", dets && counts && gt_starts && gt_starts_host && neg_starts && neg_starts_host && nex_starts && nex_starts_host &&
                                                  iou_thrs && area_ranges && match && ignore && rank && npig,
                           n_images, cap, num_classes, gt_starts_host, LIMIT(DVID_LVIS_EVAL_MAX_GT), &max_gt));
    TRY(csr_starts_ok("LVIS evaluation", "neg_starts", "image", neg_starts_host, n_images));
    TRY(csr_starts_ok("LVIS evaluation", "nex_starts", "image", nex_starts_host, n_images));
    if (gt_starts_host[n_images] > 0 && (!gt_boxes || !gt_areas || !gt_ignore || !gt_labels)) FAIL(DVID_ERR_ARG, "LVIS evaluation: null ground truth");
    if ((neg_starts_host[n_images] > 0 && !neg_labels) || (nex_starts_host[n_images] > 0 && !nex_labels))
        FAIL(DVID_ERR_ARG, "LVIS evaluation: null negative or not-exhaustive labels");
    TRY(dvid_lvis_eval_match_launch(dets, counts, n_images, cap, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts, max_gt, neg_starts, neg_labels,
                                    nex_starts, nex_labels, iou_thrs, area_ranges, num_classes, match, ignore, rank, npig,
                                    reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

long long dvid_eval_accumulate_scratch_bytes(int n_images, int cap, int max_dets_count) {
    return dvid_eval_accumulate_scratch_size(n_images, cap, max_dets_count);
}

int dvid_eval_accumulate(const float* dets, const int* counts, const int* rank, const signed char* match, const signed char* ignore,
                         const int* npig, int n_images, int cap, int num_classes, int n_areas, int n_thresholds, const int* max_dets,
                         int max_dets_count, const double* rec_thrs, int n_rec_thrs, double* precision, double* recall, void* scratch,
                         long long scratch_bytes, void* stream) {
    g_err[0] = 0;
    if (n_images < 0 || cap < 1 || num_classes < 1)
        FAIL(DVID_ERR_ARG, "evaluation accumulate: bad sizes (%d images, %d rows per image, %d classes)", n_images, cap, num_classes);
    if (n_areas != DVID_COCO_EVAL_AREAS || n_thresholds != DVID_COCO_EVAL_THRESHOLDS || n_rec_thrs != DVID_EVAL_ACCUMULATE_RECALLS)
        FAIL(DVID_ERR_ARG, "evaluation accumulate: %d area ranges, %d IoU thresholds and %d recall thresholds; the kernels are built for %d, %d and %d "
             "(DVID_COCO_EVAL_AREAS, DVID_COCO_EVAL_THRESHOLDS, DVID_EVAL_ACCUMULATE_RECALLS)", n_areas, n_thresholds, n_rec_thrs, DVID_COCO_EVAL_AREAS,
             DVID_COCO_EVAL_THRESHOLDS, DVID_EVAL_ACCUMULATE_RECALLS);
    if (max_dets_count < 1 || max_dets_count > DVID_EVAL_ACCUMULATE_MAX_LIMITS)
        FAIL(DVID_ERR_ARG, "evaluation accumulate: %d detection limits, 1 .. %d are taken (DVID_EVAL_ACCUMULATE_MAX_LIMITS)", max_dets_count,
             DVID_EVAL_ACCUMULATE_MAX_LIMITS);
    if (!max_dets || !rec_thrs || !npig || !precision || !recall) FAIL(DVID_ERR_ARG, "evaluation accumulate: null pointer");
    for (int m = 0; m < max_dets_count; ++m)
        if (max_dets[m] < 1 || (m && max_dets[m] <= max_dets[m - 1]))
            FAIL(DVID_ERR_ARG, "evaluation accumulate: max_dets must be positive and ascending (entry %d is %d)", m, max_dets[m]);
    for (int r = 1; r < n_rec_thrs; ++r)
        if (!(rec_thrs[r] >= rec_thrs[r - 1])) FAIL(DVID_ERR_ARG, "evaluation accumulate: rec_thrs decreases at entry %d", r);
    if (cap > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "evaluation accumulate: %d rows per image exceed the limit of %d (DVID_NMS_MAX_CANDIDATES)", cap, DVID_NMS_MAX_CANDIDATES);
    if (num_classes > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "evaluation accumulate: %d classes exceed the limit of %d (DVID_MAX_CLASSES)", num_classes, DVID_MAX_CLASSES);
    const long long rows = (long long)n_images * cap;
    if (rows >= (1ll << 31))
        FAIL(DVID_ERR_UNSUPPORTED, "evaluation accumulate: %d images x %d rows are %lld rows, the limit is %lld (rows are indexed with int32)", n_images, cap,
             rows, (1ll << 31) - 1);
    const long long need = dvid_eval_accumulate_scratch_size(n_images, cap, max_dets_count);
    if (need > DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES)
        FAIL(DVID_ERR_UNSUPPORTED, "evaluation accumulate: %lld bytes of sort buffers for %lld rows (56 bytes per row) exceed the limit of %lld "
             "(DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES): evaluate fewer images per call", need, rows, (long long)DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES);
    TRY(scratch_ok("evaluation accumulate", scratch, scratch_bytes, need));
    if (rows > 0 && (!dets || !counts || !rank || !match || !ignore)) FAIL(DVID_ERR_ARG, "evaluation accumulate: null pointer");
    TRY(dvid_eval_accumulate_launch(dets, counts, rank, match, ignore, npig, n_images, cap, num_classes, max_dets, max_dets_count, rec_thrs, precision,
                                    recall, scratch, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_cdist(const float* x, int n, int d, float* dist, void* stream) {
    g_err[0] = 0;
    TRY(dvid_cdist_launch(x, n, d, dist, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_fps_greedy(const float* dist, int n, int mm, int bs_emul, int* idx, void* stream) {
    g_err[0] = 0;
    TRY(dvid_fps_launch(dist, n, mm, bs_emul, idx, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_gather_rows(const float* x, const int* idx, float* y, int mm, int d, void* stream) {
    g_err[0] = 0;
    TRY(dvid_gather_rows_launch(x, idx, y, mm, d, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

// the grouped forms: every argument is checked here, before the first launch
static int groups_args_ok(const char* what, int groups, int n, int mm, int d) {
    if (groups < 1 || groups > 65535 || n < 1 || mm < 1 || mm > n || d < 4 || d % 4)
        FAIL(DVID_ERR_ARG, "%s: 1 <= groups <= 65535, 1 <= m <= n and d %% 4 == 0 (got groups %d, n %d, m %d, d %d)", what, groups, n, mm, d);
    const long long need = (long long)groups * n * n * 4;
    if (need > DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES)
        FAIL(DVID_ERR_UNSUPPORTED, "%s: %d groups x %d x %d distances are %lld bytes, the limit is %lld (DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES): "
             "run fewer groups per call", what, groups, n, n, need, (long long)DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES);
    return DVID_OK;
}
int dvid_cdist_groups(const float* x, int groups, int n, int d, float* dist, void* stream) {
    g_err[0] = 0;
    if (const int rc = groups_args_ok("dvid_cdist_groups", groups, n, 1, d); rc != DVID_OK) return rc;          // the shape first: a caller over the limit has no buffer to give
    if (!x || !dist) FAIL(DVID_ERR_ARG, "dvid_cdist_groups: null pointer");
    TRY(dvid_cdist_groups_launch(x, groups, n, d, dist, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_fps_greedy_groups(const float* dist, int groups, int n, int mm, int bs_emul, int* idx, void* stream) {
    g_err[0] = 0;
    if (!dist || !idx) FAIL(DVID_ERR_ARG, "dvid_fps_greedy_groups: null pointer");
    if (const int rc = groups_args_ok("dvid_fps_greedy_groups", groups, n, mm, 4); rc != DVID_OK) return rc;
    TRY(dvid_fps_groups_launch(dist, groups, n, mm, bs_emul, idx, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_gather_rows_groups(const float* x, const int* idx, float* y, int groups, int n, int mm, int d, void* stream) {
    g_err[0] = 0;
    if (!x || !idx || !y) FAIL(DVID_ERR_ARG, "dvid_gather_rows_groups: null pointer");
    if (groups < 1 || groups > 65535 || n < 1 || mm < 1 || d < 4 || d % 4)
        FAIL(DVID_ERR_ARG, "dvid_gather_rows_groups: 1 <= groups <= 65535, n >= 1, m >= 1 and d %% 4 == 0 (got groups %d, n %d, m %d, d %d)", groups, n, mm, d);
    TRY(dvid_gather_rows_groups_launch(x, idx, y, groups, n, mm, d, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_update_memory_groups(const float* merged, int groups, int n, int d, int mm, float* dist_scratch, int* idx, float* out, void* stream) {
    g_err[0] = 0;
    if (const int rc = groups_args_ok("dvid_update_memory_groups", groups, n, mm, d); rc != DVID_OK) return rc;
    if (!merged || !dist_scratch || !idx || !out) FAIL(DVID_ERR_ARG, "dvid_update_memory_groups: null pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TRY(dvid_cdist_groups_launch(merged, groups, n, d, dist_scratch, s));
    TRY(dvid_fps_groups_launch(dist_scratch, groups, n, mm, 0, idx, s));
    TRY(dvid_gather_rows_groups_launch(merged, idx, out, groups, n, mm, d, s));
    return DVID_OK;
}

int dvid_conv2d_nhwc_f16(const void* in, const void* w, const float* bias, const void* residual, void* out, int n, int h, int wd,
                         int cin, int cout, int kh, int kw, int stride, int pad, int kpad, int relu, int out_f32, int residual_mode,
                         void* stream) {
    g_err[0] = 0;
    ConvW cw;
    cw.w = reinterpret_cast<half_t*>(const_cast<void*>(w));
    cw.bias = const_cast<float*>(bias);
    cw.cin = cin;
    cw.cout = cout;
    cw.kh = kh;
    cw.kw = kw;
    cw.stride = stride;
    cw.pad = pad < 0 ? -pad : pad;
    cw.same_size = pad < 0;          // pad < 0: |pad| before, as many after as keep the output at the input's size (stride 1)
    cw.kpad = kpad;
    if (pad < 0 && stride != 1) FAIL(DVID_ERR_ARG, "same-size padding needs stride 1");
    TRY(conv_run(cw, reinterpret_cast<const half_t*>(in), n, h, wd, out, reinterpret_cast<hipStream_t>(stream),
                 {.relu = relu, .out_f32 = out_f32, .res = residual, .res_mode = residual_mode}));
    return DVID_OK;
}

int dvid_bottleneck64_tail_f16(const void* t1, const void* w2, const float* b2, const void* w3, const float* b3, const void* residual,
                               const void* w_shortcut, const float* b_shortcut, const void* w1_next, const float* b1_next, int next_channels,
                               void* out, void* t1_next, int n, int h, int wd, void* stream) {
    g_err[0] = 0;
    const int rc = bneck_tail(reinterpret_cast<const half_t*>(t1), reinterpret_cast<const half_t*>(w2), b2, reinterpret_cast<const half_t*>(w3),
                              b3, reinterpret_cast<const half_t*>(residual), reinterpret_cast<const half_t*>(w_shortcut), b_shortcut,
                              reinterpret_cast<const half_t*>(w1_next), b1_next, next_channels, reinterpret_cast<half_t*>(out),
                              reinterpret_cast<half_t*>(t1_next), n, h, wd, reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "bottleneck tail: bad argument (n %d, %d x %d, next conv1 with %d channels)", n, h, wd, next_channels);
    return DVID_OK;
}

int dvid_bottleneck128_tail_f16(const void* t1, const void* w2, const float* b2, const void* w3, const float* b3, const void* residual,
                                const void* w1_next, const float* b1_next, void* out, void* t1_next, int n, int h, int wd, void* stream) {
    g_err[0] = 0;
    const int rc = bneck128_tail(reinterpret_cast<const half_t*>(t1), reinterpret_cast<const half_t*>(w2), b2, reinterpret_cast<const half_t*>(w3),
                                 b3, reinterpret_cast<const half_t*>(residual), reinterpret_cast<const half_t*>(w1_next), b1_next,
                                 reinterpret_cast<half_t*>(out), reinterpret_cast<half_t*>(t1_next), n, h, wd,
                                 reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "bottleneck tail (128): bad argument (n %d, %d x %d)", n, h, wd);
    return DVID_OK;
}

int dvid_mha_f16(const void* q, const void* k, const void* v, void* out, void* vt_scratch, int batch, int lq, int lk, int nheads,
                 int q_ld, int kv_ld, int out_ld, int64_t q_bs, int64_t kv_bs, int64_t out_bs, void* stream) {
    g_err[0] = 0;
    TRY(dvid_mha_mfma_launch(reinterpret_cast<const half_t*>(q), reinterpret_cast<const half_t*>(k), reinterpret_cast<const half_t*>(v),
                             reinterpret_cast<half_t*>(out), reinterpret_cast<half_t*>(vt_scratch), batch, lq, lk, nheads, q_ld, kv_ld,
                             out_ld, q_bs, kv_bs, out_bs, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_dynconv(const void* roi, const void* params, const float* g1, const float* b1, const float* g2, const float* b2, void* out,
                 int rows, void* stream) {
    g_err[0] = 0;
    TRY(dvid_dynconv_launch(reinterpret_cast<const half_t*>(roi), reinterpret_cast<const half_t*>(params), g1, b1, g2, b2,
                            reinterpret_cast<half_t*>(out), rows, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_add_layernorm(const float* x, const float* r, const float* g, const float* b, float* y, int rows, int d, int relu,
                       void* stream) {
    g_err[0] = 0;
    TRY(dvid_add_layernorm_launch(x, r, g, b, y, nullptr, rows, d, relu, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_swin_window_attn_f16(const void* qkv, const void* qkv_bias16, const float* relbias, void* out, int batch, int H, int W, int C,
                              int nheads, int shift, void* stream) {
    g_err[0] = 0;
    if (!qkv || !qkv_bias16 || !relbias || !out) FAIL(DVID_ERR_ARG, "swin window attention: null pointer");
    if (batch <= 0 || H <= 0 || W <= 0 || nheads <= 0 || shift < 0 || shift >= 7)
        FAIL(DVID_ERR_ARG, "swin window attention: bad sizes (batch %d, %d x %d tokens, %d heads, shift %d)", batch, H, W, nheads, shift);
    const int rc = dvid_swin_window_attn_launch(reinterpret_cast<const half_t*>(qkv), reinterpret_cast<const half_t*>(qkv_bias16), relbias,
                                                reinterpret_cast<half_t*>(out), batch, H, W, C, nheads, shift, reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "swin window attention: C %d with %d heads on %d x %d x %d tokens is not supported", C, nheads, batch, H, W);
    return DVID_OK;
}

int dvid_swin_window_attn_f16_ws(const void* qkv, const void* qkv_bias16, const float* relbias, void* out, int batch, int H, int W, int C,
                                 int nheads, int shift, int window, void* stream) {
    if (window == 7) return dvid_swin_window_attn_f16(qkv, qkv_bias16, relbias, out, batch, H, W, C, nheads, shift, stream);
    g_err[0] = 0;
    if (window != 12) FAIL(DVID_ERR_UNSUPPORTED, "swin window attention: window size %d (7 and 12 are built)", window);
    if (!qkv || !qkv_bias16 || !relbias || !out) FAIL(DVID_ERR_ARG, "swin window attention: null pointer");
    if (batch <= 0 || H <= 0 || W <= 0 || nheads <= 0 || shift < 0 || shift >= window)
        FAIL(DVID_ERR_ARG, "swin window attention: bad sizes (batch %d, %d x %d tokens, %d heads, shift %d, window %d)", batch, H, W, nheads, shift, window);
    const int rc = dvid_swin_window12_attn_launch(reinterpret_cast<const half_t*>(qkv), reinterpret_cast<const half_t*>(qkv_bias16), relbias,
                                                  reinterpret_cast<half_t*>(out), batch, H, W, C, nheads, shift, reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "swin window attention (window 12): C %d with %d heads on %d x %d x %d tokens is not supported", C, nheads, batch, H, W);
    return DVID_OK;
}

int dvid_patch_merge_ln(const float* x, const float* g, const float* b, void* y16, float* y32, int B, int H, int W, int C, void* stream) {
    g_err[0] = 0;
    if (!x || !g || !b || (!y16 && !y32)) FAIL(DVID_ERR_ARG, "patch merge: null pointer (at least one of y16 / y32 is needed)");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) FAIL(DVID_ERR_ARG, "patch merge: bad sizes (%d x %d x %d tokens, C %d)", B, H, W, C);
    const int rc = dvid_patch_merge_ln_launch(x, g, b, reinterpret_cast<half_t*>(y16), B, H, W, C, reinterpret_cast<hipStream_t>(stream), y32);
    if (rc != DVID_OK) FAIL(rc, "patch merge: C %d is not supported (a multiple of 4, at most 512)", C);
    return DVID_OK;
}

int dvid_nhwc_from_nchw(const float* in, void* out_f16, int n, int h, int w, int c, void* stream) {
    g_err[0] = 0;
    TRY(dvid_nhwc_from_nchw_launch(in, reinterpret_cast<half_t*>(out_f16), n, h, w, c, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_nchw_from_nhwc(const void* in_f16, float* out, int n, int h, int w, int c, void* stream) {
    g_err[0] = 0;
    TRY(dvid_nchw_from_nhwc_launch(reinterpret_cast<const half_t*>(in_f16), out, n, h, w, c, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
int dvid_f32_to_f16(const float* x, void* y, int64_t n, void* stream) {
    g_err[0] = 0;
    TRY(dvid_f32_to_f16_launch(x, reinterpret_cast<half_t*>(y), (long)n, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_resize_u8_to_f32(const void* src_hwc, int h, int w, void* tmp, float* out_chw, int oh, int ow, int ph, int pw,
                          const int* xbounds, const int* xk, int xksize, const int* ybounds, const int* yk, int yksize, void* stream) {
    g_err[0] = 0;
    if (!src_hwc || !out_chw) FAIL(DVID_ERR_ARG, "null image");
    const int rc = dvid_resize_u8_launch(reinterpret_cast<const unsigned char*>(src_hwc), h, w, reinterpret_cast<unsigned char*>(tmp),
                                         out_chw, oh, ow, ph, pw, xbounds, xk, xksize, ybounds, yk, yksize,
                                         reinterpret_cast<hipStream_t>(stream));
    if (rc != DVID_OK) FAIL(rc, "resize %dx%d -> %dx%d (padded %dx%d): bad sizes or missing tables / scratch", h, w, oh, ow, ph, pw);
    return DVID_OK;
}

int dvid_resize_views_u8(const void* const* srcs, int n, const long long* plan, const long long* plan_host, const int* bounds,
                         int64_t n_bound_rows, const int* weights, int64_t n_weights, void* tmp, int64_t tmp_bytes, float* out, int ph, int pw,
                         int flip, void* stream) {
    g_err[0] = 0;
    if (!srcs || !plan || !plan_host || !bounds || !weights || !tmp || !out) FAIL(DVID_ERR_ARG, "resize views: null pointer");
    if (n < 1 || n > 65535 || ph < 1 || pw < 1 || ph > 65535) FAIL(DVID_ERR_ARG, "resize views: %d images on a %d x %d canvas", n, ph, pw);
    int max_h = 0, max_ow = 0;
    for (int i = 0; i < n; ++i) {          // every offset the kernels add is checked here, against the sizes of what they index
        const long long* d = plan_host + (long)i * 11;
        const long long h = d[0], w = d[1], oh = d[2], ow = d[3];
        if (h < 1 || w < 1 || oh < 1 || ow < 1 || h > 65535 || oh > ph || ow > pw)
            FAIL(DVID_ERR_ARG, "resize views: image %d is %lld x %lld -> %lld x %lld on a %d x %d canvas", i, h, w, oh, ow, ph, pw);
        const long long axis[2][4] = {{d[4], d[5], d[6], ow}, {d[7], d[8], d[9], oh}};
        for (int a = 0; a < 2; ++a) {
            const long long row = axis[a][0], k0 = axis[a][1], ks = axis[a][2], len = axis[a][3];
            if ((row < 0) != (a == 0 ? ow == w : oh == h))
                FAIL(DVID_ERR_ARG, "resize views: image %d has %s tables for its %s pass", i, row < 0 ? "no" : "unexpected", a == 0 ? "x" : "y");
            if (row >= 0 && (row + len > n_bound_rows || k0 < 0 || ks < 1 || k0 + len * ks > n_weights))
                FAIL(DVID_ERR_ARG, "resize views: the %s tables of image %d lie outside the concatenated tables", a == 0 ? "x" : "y", i);
        }
        if (d[4] >= 0) {
            if (d[10] < 0 || d[10] + h * ow * 3 > tmp_bytes) FAIL(DVID_ERR_ARG, "resize views: image %d's intermediate rows lie outside the %lld scratch bytes", i, (long long)tmp_bytes);
            if (h > max_h) max_h = (int)h;
        }
        if (ow > max_ow) max_ow = (int)ow;
    }
    TRY(dvid_resize_views_u8_launch(reinterpret_cast<const unsigned char* const*>(srcs), n, plan, bounds, weights,
                                    reinterpret_cast<unsigned char*>(tmp), out, ph, pw, flip, max_h, max_ow, reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_bbox_aug_merge(const float* boxes, const float* scores, const int* labels, const int* counts, const float* table, int n, int views,
                        int cap, float* cand_boxes, float* cand_scores, int* cand_labels, int* live, void* stream) {
    g_err[0] = 0;
    if (!boxes || !scores || !labels || !counts || !table || !cand_boxes || !cand_scores || !cand_labels || !live)
        FAIL(DVID_ERR_ARG, "bbox aug merge: null pointer");
    if (((uintptr_t)boxes | (uintptr_t)cand_boxes) & 15) FAIL(DVID_ERR_ARG, "bbox aug merge: the box arrays must be 16-byte aligned");
    if (n < 1 || views < 1 || cap < 1) FAIL(DVID_ERR_ARG, "bbox aug merge: bad sizes (%d images, %d views, cap %d)", n, views, cap);
    if (views > DVID_BBOX_AUG_MAX_VIEWS) FAIL(DVID_ERR_UNSUPPORTED, "bbox aug merge: %d views exceed the limit of %d", views, DVID_BBOX_AUG_MAX_VIEWS);
    if ((long)views * cap > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "bbox aug merge: %d views x %d rows = %ld candidates per image exceed the NMS's limit of %d", views, cap,
             (long)views * cap, DVID_NMS_MAX_CANDIDATES);
    TRY(dvid_bbox_aug_merge_launch(boxes, scores, labels, counts, table, n, views, cap, cand_boxes, cand_scores, cand_labels, live,
                                   reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int dvid_jpeg_reconstruct_u8(const int16_t* coef, int64_t n_coef, const uint16_t* quant, int64_t n_quant, const long long* plan,
                             const long long* plan_host, int n, void* planes, int64_t planes_bytes, void* out, int64_t out_bytes, void* stream) {
    g_err[0] = 0;
    if (!coef || !quant || !plan || !plan_host || !planes || !out) FAIL(DVID_ERR_ARG, "jpeg reconstruct: null pointer");
    if (n < 1 || n_coef < 1 || n_quant < 1 || out_bytes < 1) FAIL(DVID_ERR_ARG, "jpeg reconstruct: %d frames, %lld coefficients, %lld table entries, %lld output bytes", n, (long long)n_coef, (long long)n_quant, (long long)out_bytes);
    if (n > 65535) FAIL(DVID_ERR_UNSUPPORTED, "jpeg reconstruct: %d frames exceed the limit of 65535 per call", n);
    if (n_coef > DVID_JPEG_MAX_COEFS)
        FAIL(DVID_ERR_UNSUPPORTED, "jpeg reconstruct: %lld coefficients exceed the limit of %lld (DVID_JPEG_MAX_COEFS: int32 indices)", (long long)n_coef, DVID_JPEG_MAX_COEFS);
    if (planes_bytes < n_coef) FAIL(DVID_ERR_ARG, "jpeg reconstruct: the planes hold %lld bytes, %lld coefficients need as many", (long long)planes_bytes, (long long)n_coef);
    if (((uintptr_t)coef | (uintptr_t)quant) & 15 || (uintptr_t)planes & 7) FAIL(DVID_ERR_ARG, "jpeg reconstruct: coef and quant must be 16-byte aligned, planes 8-byte aligned");
    long long coef_end = 0, out_end = 0;
    int max_blocks = 0, max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {          // every offset the kernels add is checked here, against the sizes of what they index
        const long long* d = plan_host + (long)i * DVID_JPEG_PLAN_COLS;
        const long long w = d[0], h = d[1], nc = d[2], hs = d[3], vs = d[4];
        if (w < 1 || h < 1 || w > 65535 || h > 65535) FAIL(DVID_ERR_ARG, "jpeg reconstruct: frame %d is %lld x %lld (1 .. 65535 each)", i, w, h);
        if ((nc != 1 && nc != 3) || !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) || (nc == 1 && hs * vs != 1))
            FAIL(DVID_ERR_ARG, "jpeg reconstruct: frame %d has %lld components with luma sampling %lld x %lld (1 component at 1x1, or 3 at 1x1, 2x1, 2x2)", i, nc, hs, vs);
        const long long mw = (w + 8 * hs - 1) / (8 * hs), mh = (h + 8 * vs - 1) / (8 * vs);
        const long long blocks[3] = {mw * hs * mh * vs, nc == 3 ? mw * mh : 0, nc == 3 ? mw * mh : 0};
        for (int c = 0; c < nc; ++c) {
            const long long off = d[5 + c];
            if (off < coef_end || off % 64)
                FAIL(DVID_ERR_ARG, "jpeg reconstruct: component %d of frame %d starts at coefficient %lld: offsets are multiples of 64 and ascend without overlap (the one before ends at %lld)", c, i, off, coef_end);
            coef_end = off + blocks[c] * 64;
            if (coef_end > n_coef)
                FAIL(DVID_ERR_ARG, "jpeg reconstruct: component %d of frame %d ends at coefficient %lld, the buffer holds %lld", c, i, coef_end, (long long)n_coef);
        }
        if (d[8] < 0 || d[8] % 64 || d[8] + 64 * nc > n_quant)
            FAIL(DVID_ERR_ARG, "jpeg reconstruct: the tables of frame %d start at entry %lld of %lld (a multiple of 64, %lld entries)", i, d[8], (long long)n_quant, 64 * nc);
        if (d[9] < out_end) FAIL(DVID_ERR_ARG, "jpeg reconstruct: frame %d's pixels start at byte %lld and overlap the frame before, which ends at %lld", i, d[9], out_end);
        out_end = d[9] + h * w * 3;
        if (out_end > out_bytes) FAIL(DVID_ERR_ARG, "jpeg reconstruct: frame %d's pixels end at byte %lld, the output holds %lld", i, out_end, (long long)out_bytes);
        const long long nb = blocks[0] + blocks[1] + blocks[2];
        if (nb > max_blocks) max_blocks = (int)nb;
        if (w > max_w) max_w = (int)w;
        if (h > max_h) max_h = (int)h;
    }
    TRY(dvid_jpeg_reconstruct_launch(coef, quant, plan, n, max_blocks, max_w, max_h, reinterpret_cast<unsigned char*>(planes),
                                     reinterpret_cast<unsigned char*>(out), reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}

int64_t dvid_overlay_scratch_bytes(int n, int cap) {
    (void)cap;          // the rows are sorted in LDS: the draw lists are all the scratch there is
    return n < 0 ? 0 : dvid_overlay_scratch_bytes_for(n);
}

int dvid_overlay_tile(int* tile_w, int* tile_h) {
    g_err[0] = 0;
    if (!tile_w || !tile_h) FAIL(DVID_ERR_ARG, "overlay tile: null pointer");
    dvid_overlay_tile_size(tile_w, tile_h);
    return DVID_OK;
}

int dvid_overlay_detections(void* const* frames, const int* sizes, const int* sizes_host, int n, const float* dets, const int* counts, int cap,
                            const float* ratios, const unsigned char* names, int num_classes, const unsigned char* atlas, int gh, int gw,
                            float threshold, int thickness, int text_scale, void* scratch, int64_t scratch_bytes, void* stream) {
    g_err[0] = 0;
    if (!frames || !sizes || !sizes_host || !dets || !counts || !ratios || !names || !atlas || !scratch) FAIL(DVID_ERR_ARG, "overlay: null pointer");
    if (n < 1 || n > 65535 || cap < 1 || num_classes < 1 || gh < 1 || gw < 1)
        FAIL(DVID_ERR_ARG, "overlay: bad sizes (%d frames, cap %d, %d classes, glyph cell %d x %d)", n, cap, num_classes, gw, gh);
    if (!(threshold == threshold)) FAIL(DVID_ERR_ARG, "overlay: the threshold is NaN");
    if (cap > DVID_NMS_MAX_CANDIDATES)
        FAIL(DVID_ERR_UNSUPPORTED, "overlay: %d rows per frame exceed the limit of %d (DVID_NMS_MAX_CANDIDATES)", cap, DVID_NMS_MAX_CANDIDATES);
    if (num_classes > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "overlay: %d classes exceed the limit of %d (DVID_MAX_CLASSES)", num_classes, DVID_MAX_CLASSES);
    if (gh > 32 || gw > 32) FAIL(DVID_ERR_UNSUPPORTED, "overlay: a glyph cell of %d x %d exceeds the limit of 32 x 32", gw, gh);
    if (thickness < 1 || thickness > 16) FAIL(DVID_ERR_UNSUPPORTED, "overlay: thickness %d, the limits are 1 .. 16", thickness);
    if (text_scale < 1 || text_scale > 4) FAIL(DVID_ERR_UNSUPPORTED, "overlay: text_scale %d, the limits are 1 .. 4", text_scale);
    const long long need = dvid_overlay_scratch_bytes_for(n);
    if (scratch_bytes < need)
        FAIL(DVID_ERR_UNSUPPORTED, "overlay: %lld bytes of scratch, %d frames need %lld (dvid_overlay_scratch_bytes)", (long long)scratch_bytes, n, need);
    if ((uintptr_t)scratch & 3) FAIL(DVID_ERR_ARG, "overlay: the scratch must be 4-byte aligned");
    int max_h = 0, max_w = 0;
    for (int i = 0; i < n; ++i) {          // the grid comes from the host's copy of the sizes
        const int h = sizes_host[2 * i], w = sizes_host[2 * i + 1];
        if (h < 1 || w < 1 || h > 65535 || w > 65535) FAIL(DVID_ERR_ARG, "overlay: frame %d is %d x %d, the limits are 1 .. 65535", i, h, w);
        if (h > max_h) max_h = h;
        if (w > max_w) max_w = w;
    }
    TRY(dvid_overlay_launch(reinterpret_cast<unsigned char* const*>(frames), sizes, n, max_h, max_w, dets, counts, cap, ratios, names, num_classes,
                            atlas, gh, gw, threshold, thickness, text_scale, reinterpret_cast<int*>(scratch), reinterpret_cast<hipStream_t>(stream)));
    return DVID_OK;
}
}  // extern "C"
