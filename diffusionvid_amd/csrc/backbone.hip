// The backbones: ResNet + FPN and Swin-Transformer + FPN, each with DTYPE float16 and float32, the scaffolding they share (pixel
// normaliser, sub-batch chains and their workspace slices, the FPN) and their entry points (dvid_backbone_*).
#include <type_traits>

#include "runtime.h"

namespace {
// every block of the stage is a 64-wide stride-1 bottleneck with 256 outputs; block 0 has a shortcut convolution over 64 channels
// (R-50 / R-101 res2), the others take the block input as the residual
bool bneck64_stage(const std::vector<Block>& blocks) {
    if (blocks.empty()) return false;
    for (size_t b = 0; b < blocks.size(); ++b) {
        const Block& k = blocks[b];
        const int cin = b == 0 ? 64 : 256;
        if (k.c1.kh != 1 || k.c1.stride != 1 || k.c1.cin != cin || k.c1.cout != 64 || k.c1.kpad != cin || !k.c1.bias) return false;
        if (k.c2.kh != 3 || k.c2.kw != 3 || k.c2.stride != 1 || k.c2.pad != 1 || k.c2.cin != 64 || k.c2.cout != 64 || k.c2.kpad != 576 ||
            !k.c2.bias)
            return false;
        if (k.c3.kh != 1 || k.c3.stride != 1 || k.c3.cin != 64 || k.c3.cout != 256 || k.c3.kpad != 64 || !k.c3.bias) return false;
        if (k.has_sc != (b == 0)) return false;
        if (k.has_sc && (k.sc.kh != 1 || k.sc.stride != 1 || k.sc.cin != 64 || k.sc.cout != 256 || k.sc.kpad != 64 || !k.sc.bias)) return false;
    }
    return true;
}

// res3 of R-50 / R-101: 128-wide bottlenecks with 512 outputs; the first block has the stride and a shortcut convolution, the others
// are stride-1 identity blocks
bool bneck128_stage(const std::vector<Block>& blocks) {
    if (blocks.size() < 2) return false;
    for (size_t b = 0; b < blocks.size(); ++b) {
        const Block& k = blocks[b];
        if (k.c3.kh != 1 || k.c3.stride != 1 || k.c3.cin != 128 || k.c3.cout != 512 || k.c3.kpad != 128 || !k.c3.bias) return false;
        if (k.c2.kh != 3 || k.c2.kw != 3 || k.c2.pad != 1 || k.c2.cin != 128 || k.c2.cout != 128 || k.c2.kpad != 1152 || !k.c2.bias) return false;
        if (k.has_sc != (b == 0)) return false;
        if (b == 0) {
            if (k.sc.cout != 512) return false;
            continue;
        }
        if (k.c1.kh != 1 || k.c1.stride != 1 || k.c1.cin != 512 || k.c1.cout != 128 || k.c1.kpad != 512 || !k.c1.bias) return false;
        if (k.c2.stride != 1) return false;
    }
    return true;
}

// the normaliser's constants: pixels are (x / 255 - mean) / stdv, the fp16 kernels multiply by inv_std
struct PixelNorm {
    float mean[3], stdv[3], inv_std[3];
    explicit PixelNorm(const dvid_config& c) {
        for (int i = 0; i < 3; ++i) {
            mean[i] = c.pixel_mean[i] / 255.f;
            stdv[i] = c.pixel_std[i] / 255.f;
            inv_std[i] = 1.f / (c.pixel_std[i] / 255.f);
        }
    }
};

// detectron2 FPN.forward over the model's levels (strides 8/16/32, with the p2 level 4/8/16/32), bottom level last: lateral 1x1 (+
// nearest-x2 top-down sum fused in the epilogue), 3x3 output conv.  Every array is indexed by stage, 0 = res2 / level 2 .. 3 = res5 /
// level 5, and read from index 4 - fpn_levels on: cin / lat / pout = the levels' inputs (c2..c5), lateral buffers and outputs, NHWC fp16
// or fp32; sh / sw = their heights / widths.
template <typename T>
int run_fpn(dvid_model* m, T* const* cin, T* const* lat, T* const* pout, int n, const int* sh, const int* sw, hipStream_t s) {
    for (int l = 3; l >= 4 - m->fpn_levels; --l) {
        const T* res = (l < 3) ? lat[l + 1] : nullptr;
        if constexpr (std::is_same<T, float>::value) {
            TRY(conv_run32(m->lateral[l], cin[l], n, sh[l], sw[l], lat[l], s, {.res = res, .res_mode = res ? 2 : 0}));
            TRY(conv_run32(m->output[l], lat[l], n, sh[l], sw[l], pout[l], s));
        } else {
            TRY(conv_run(m->lateral[l], cin[l], n, sh[l], sw[l], lat[l], s, {.res = res, .res_mode = res ? 2 : 0}));
            TRY(conv_run(m->output[l], lat[l], n, sh[l], sw[l], pout[l], s));
        }
    }
    return DVID_OK;
}

// Frames are independent through the backbone.  They are processed as `nchain` sub-batches on separate HIP
// streams: a layer of one sub-batch rarely fills 256 CUs evenly (e.g. res4: 304-608 tiles), and with two chains
// in flight the blocks of one chain's next kernel start on the CUs the other chain's tail leaves idle.  (A two-stream
// front / back software pipeline of HBM-bound early layers beside MFMA-bound late ones measured no gain,
// profiles/r02_backbone_pipeline_sweep.txt; it lives in the history of model.hip, where this code was.)  With DTYPE float32 the
// HBM-paced short-K layers of one chain run beside the operand-stream-paced 3x3 layers of the other.
// Small launch sequences stay on one stream: at 8 frames two 4-frame chains are slower than one 8-frame sequence (1250 vs 1273
// frames/s with the reference's one-batch-per-call protocol, 980 with four chains; profiles/r03c_chains_at_lookahead1.txt) --
// the layers are then bound by how few workgroups a launch has, and halving the rows halves them again.
// body(f0, nf, cs) launches frames [f0, f0 + nf) on stream cs; `s` waits for every chain.
template <typename Body>
int run_chains(dvid_model* m, int n, hipStream_t s, Body&& body) {
    const int nchain = (m->nchain > 1 && n >= 16 * m->nchain) ? m->nchain : 1;
    if (nchain > 1) {
        TRY(m->ensure_streams());
        HIP_TRY(hipEventRecord(m->ev_fork, s));
        for (int c = 0; c < nchain; ++c) HIP_TRY(hipStreamWaitEvent(m->cs[c], m->ev_fork, 0));
    }
    const int per = (n + nchain - 1) / nchain;
    for (int c = 0; c < nchain; ++c) {
        const int f0 = c * per, nf = (f0 + per <= n) ? per : n - f0;
        if (nf <= 0) continue;
        hipStream_t cs = nchain > 1 ? m->cs[c] : s;
        TRY(body(f0, nf, cs));
        if (nchain > 1) {
            HIP_TRY(hipEventRecord(m->ev_join[c], cs));
            HIP_TRY(hipStreamWaitEvent(s, m->ev_join[c], 0));
        }
    }
    return DVID_OK;
}

// A chain's slice of every ResNet workspace buffer starts at its first frame (f0 + nf <= n <= ws_frames for any chain count, so no
// slice can run past the end).  T = half_t or float: dvid_workspace_reserve sizes every buffer as its element count times sizeof(T).
template <typename T>
struct ChainSlices {
    T *img, *bx, *by, *t1, *t2, *sc;
    T* stage_out[4];          // res3..res5 outputs persist for the FPN (c3, c4, c5); res2's (c2) only in a model with the p2 level
    T* lat[4];                // by stage, as run_fpn reads them; [0] null without the p2 level
    ChainSlices(dvid_model* m, int f0, int height, int width) {
        const size_t fo = (size_t)f0, px = (size_t)height * width, px4 = px / 16, big = fo * px4 * 256;
        img = m->img8.as<T>() + fo * px * (16 / sizeof(T));          // NHWC8 fp16 / NHWC4 fp32: 16 bytes per pixel
        bx = m->bufX.as<T>() + big;
        by = m->bufY.as<T>() + big;
        t1 = m->bufT1.as<T>() + big;
        t2 = m->bufT2.as<T>() + big;
        sc = m->bufSC.as<T>() + big;
        const bool p2 = m->fpn_levels == 4;
        stage_out[0] = p2 ? m->c2.as<T>() + big : nullptr;
        stage_out[1] = m->c3.as<T>() + fo * (px4 / 4) * 512;
        stage_out[2] = m->c4.as<T>() + fo * (px4 / 16) * 1024;
        stage_out[3] = m->c5.as<T>() + fo * (px4 / 64) * 2048;
        lat[0] = p2 ? m->lat[0].as<T>() + big : nullptr;
        for (int l = 1; l < 4; ++l) lat[l] = m->lat[l].as<T>() + fo * (px4 >> (2 * l)) * 256;
    }
};

// detectron2 build_resnet_fpn_backbone with DTYPE float32: normaliser -> NHWC4, BasicStem (7x7 / 2 + FrozenBN folded + ReLU + max pool),
// the bottleneck stages layer by layer, FPN; every tensor fp32 (csrc/f32.hip; prep / max pool: csrc/elementwise.hip)
int backbone_resnet_f32(dvid_model* m, const float* const* frames, int n, int height, int width, float* const* pyr, hipStream_t s) {
    const PixelNorm px(m->cfg);
    return run_chains(m, n, s, [&](int f0, int nf, hipStream_t cs) -> int {
        const ChainSlices<float> k(m, f0, height, width);
        float *img = k.img, *bx = k.bx, *by = k.by, *t1 = k.t1, *t2 = k.t2, *sc = k.sc;
        float* const* stage_out = k.stage_out;
        TRY(dvid_f32_prep_images_launch(frames + f0, img, nf, height, width, px.mean, px.stdv, cs));
        int h = height, w = width;
        TRY(conv_run32(m->stem, img, nf, h, w, t1, cs, {.relu = 1, .ho_out = &h, .wo_out = &w}));
        TRY(prof_other("maxpool_f32", (long)nf * h * w, 64, 9, 0.0, (double)nf * h * w * 64 * 4.0 * 1.25, cs,
                       [&] { return dvid_f32_maxpool3x3s2_launch(t1, bx, nf, h, w, 64, cs); }));
        h = (h + 2 - 3) / 2 + 1;
        w = (w + 2 - 3) / 2 + 1;
        float* cur = bx;
        int sh[4], sw[4];
        for (int st = 0; st < 4; ++st) {
            const int nb = (int)m->blocks[st].size();
            for (int b = 0; b < nb; ++b) {
                const Block& blk = m->blocks[st][b];
                int h2 = h, w2 = w;
                TRY(conv_run32(blk.c1, cur, nf, h, w, t1, cs, {.relu = 1}));
                TRY(conv_run32(blk.c2, t1, nf, h, w, t2, cs, {.relu = 1, .ho_out = &h2, .wo_out = &w2}));
                const float* res = cur;
                if (blk.has_sc) {
                    TRY(conv_run32(blk.sc, cur, nf, h, w, sc, cs));
                    res = sc;
                }
                float* dst = (b == nb - 1 && stage_out[st]) ? stage_out[st] : (cur == bx ? by : bx);
                TRY(conv_run32(blk.c3, t2, nf, h2, w2, dst, cs, {.relu = 1, .res = res, .res_mode = 1}));
                h = h2;
                w = w2;
                cur = dst;
            }
            sh[st] = h;
            sw[st] = w;
        }
        float* pout[4];
        for (int l = 0; l < 4; ++l) pout[l] = pyr[l] ? pyr[l] + (size_t)f0 * sh[l] * sw[l] * 256 : nullptr;
        return run_fpn<float>(m, stage_out, k.lat, pout, nf, sh, sw, cs);
    });
}

// Swin-Transformer + FPN with DTYPE float32 (swintransformer.py:464-751): the fp16 path's launch sequence with fp32 operands everywhere
int backbone_swin_f32(dvid_model* m, const float* const* frames, int n, int height, int width, float* const* pyr, hipStream_t s) {
    const PixelNorm px(m->cfg);
    float* img = m->img8.as<float>();
    TRY(dvid_f32_prep_images_launch(frames, img, n, height, width, px.mean, px.stdv, s));
    int H = height, W = width;
    float* x = m->sw_x.as<float>();
    float* x2 = m->sw_x2.as<float>();
    TRY(conv_run32(m->swin_patch, img, n, H, W, x, s, {.ho_out = &H, .wo_out = &W}));
    TRY(dvid_add_layernorm_launch(x, nullptr, m->swin_patch_norm.g, m->swin_patch_norm.b, x, nullptr, n * H * W, m->swin[0].dim, 0, s));
    float* ln = m->sw_ln16.as<float>();
    float* qkv = m->sw_qkv16.as<float>();
    float* attn = m->sw_attn16.as<float>();
    float* hid = m->sw_h16.as<float>();
    float* stage_out[4] = {m->c2.as<float>(), m->c3.as<float>(), m->c4.as<float>(), m->c5.as<float>()};          // (c2: null without the p2 level, and stage 0 has no out norm then)
    const int ws = m->cfg.swin_window;                           // 7 or 12 (dvid_model_finalize)
    int sh[4], sw[4];
    for (int st = 0; st < 4; ++st) {
        const SwinStageW& S = m->swin[st];
        const int C = S.dim, M = n * H * W;
        for (size_t b = 0; b < S.blocks.size(); ++b) {
            const SwinBlockW& B = S.blocks[b];
            const int shift = (b % 2 == 0) ? 0 : ws / 2;
            TRY(dvid_add_layernorm_launch(x, nullptr, B.norm1.g, B.norm1.b, ln, nullptr, M, C, 0, s));
            TRY(linear_run32(B.qkv, ln, M, qkv, 0, s));
            TRY(prof_other("swin_attn_f32", M, C, ws * ws, 4.0 * M * (double)(ws * ws) * C, (double)M * C * 4.0 * 4.0, s, [&] {
                return ws == 12 ? dvid_f32_swin_window12_attn_launch(qkv, B.qkv.bias, B.relbias, attn, n, H, W, C, S.heads, shift, s)
                                : dvid_f32_swin_window_attn_launch(qkv, B.qkv.bias, B.relbias, attn, n, H, W, C, S.heads, shift, s);
            }));
            TRY(conv_run32(B.proj, attn, M, 1, 1, x, s, {.res = x, .res_mode = 1}));                                // x += proj(attn)
            TRY(dvid_add_layernorm_launch(x, nullptr, B.norm2.g, B.norm2.b, ln, nullptr, M, C, 0, s));
            TRY(linear_run32(B.fc1, ln, M, hid, 2, s));                                           // exact GELU
            TRY(conv_run32(B.fc2, hid, M, 1, 1, x, s, {.res = x, .res_mode = 1}));                                  // x += fc2(...)
        }
        sh[st] = H;
        sw[st] = W;
        if (S.has_out) TRY(dvid_add_layernorm_launch(x, nullptr, S.out_norm.g, S.out_norm.b, stage_out[st], nullptr, M, C, 0, s));
        if (S.has_down) {
            TRY(dvid_patch_merge_ln_launch(x, S.down_norm.g, S.down_norm.b, nullptr, n, H, W, C, s, hid));
            H = (H + 1) / 2;
            W = (W + 1) / 2;
            TRY(linear_run32(S.down_red, hid, n * H * W, x2, 0, s));
            float* t = x;
            x = x2;
            x2 = t;
        }
    }
    float* lat[4] = {m->lat[0].as<float>(), m->lat[1].as<float>(), m->lat[2].as<float>(), m->lat[3].as<float>()};
    return run_fpn<float>(m, stage_out, lat, pyr, n, sh, sw, s);
}

// detectron2 build_resnet_fpn_backbone (DTYPE float16): normaliser, stem + max pool, the bottleneck stages (res2 / res3 on the fused
// block kernels where their shape rules pick them), FPN; fp16 NHWC
int backbone_resnet_f16(dvid_model* m, const float* const* frames, int n, int height, int width, half_t* const* pyr, hipStream_t s) {
    const PixelNorm px(m->cfg);
    return run_chains(m, n, s, [&](int f0, int nf, hipStream_t cs) -> int {
        const ChainSlices<half_t> k(m, f0, height, width);
        half_t *img8 = k.img, *bx = k.bx, *by = k.by, *t1 = k.t1, *t2 = k.t2, *sc = k.sc;
        half_t* const* stage_out = k.stage_out;
        int h = height, w = width;
        bool pooled = false;
        if (m->use_s2d) {
            // normalise + 2x2 space-to-depth (16 halves per block: the same bytes per frame as half an NHWC8 image), then the stem
            // as a 4x4 / stride-1 convolution on the half-resolution grid
            TRY(dvid_prep_images_s2d_launch(frames + f0, img8, nf, height, width, px.mean, px.inv_std, cs));
            // (only while the patch kernels are on and no tile configuration is forced: "all layers on igemm2" runs -- conv3x3 = 0,
            // dvid_igemm_set_config -- then include the stem, whose fused kernel sums in the patch kernels' order)
            if (g_opt.stem_pool && g_opt.conv3x3 && g_opt.igemm_cfg < 0) {
                // stem + ReLU + max pool as one launch (csrc/conv3x3.hip: stem_pool_kernel): the half-resolution 64-channel map never exists
                TRY(conv_run(m->stem_s2d, img8, nf, h / 2, w / 2, bx, cs, {.relu = 1, .ho_out = &h, .wo_out = &w, .pooled = true}));
                pooled = true;
            } else {
                TRY(conv_run(m->stem_s2d, img8, nf, h / 2, w / 2, t1, cs, {.relu = 1, .ho_out = &h, .wo_out = &w}));
            }
        } else {
            TRY(dvid_prep_images_launch(frames + f0, img8, nf, height, width, px.mean, px.inv_std, cs));
            TRY(conv_run(m->stem, img8, nf, h, w, t1, cs, {.relu = 1, .ho_out = &h, .wo_out = &w}));
        }
        if (!pooled) TRY(prof_other("maxpool", (long)nf * h * w, 64, 9, 0.0, (double)nf * h * w * 64 * 2.0 * 1.25, cs, [&] { return dvid_maxpool3x3s2_launch(t1, bx, nf, h, w, 64, cs); }));
        h = (h + 2 - 3) / 2 + 1;
        w = (w + 2 - 3) / 2 + 1;
        half_t* cur = bx;  // block input
        half_t* res3_t1 = nullptr;
        int sh[4], sw[4];
        for (int st = 0; st < 4; ++st) {
            const int nb = (int)m->blocks[st].size();
            // res2 (64-wide bottlenecks, 256 out): one launch per block for everything behind conv1 -- conv2, conv3 + shortcut / residual
            // + ReLU and the next block's conv1 (csrc/bneck.hip; bit-identical to the launches below)
            if (st == 0 && bneck64_stage(m->blocks[0]) && dvid_bneck64_tail_preferred(h, w)) {
                half_t* ta = t1;
                half_t* tb = t2;
                TRY(conv_run(m->blocks[0][0].c1, cur, nf, h, w, ta, cs, {.relu = 1}));
                // the last block's launch also computes res3's first conv1 (1x1 / stride 1 over this stage's output, 256 -> 128) when
                // res3 takes the fused path too: that layer alone re-read the 512 B per pixel this launch has in registers
                const Block* r3 = nullptr;
                if (nb > 1 && bneck128_stage(m->blocks[1])) {
                    const Block& b0 = m->blocks[1][0];
                    auto osz = [](const ConvW& c, int v) { return (v + 2 * c.pad - c.kh) / c.stride + 1; };
                    if (b0.c1.kh == 1 && b0.c1.stride == 1 && b0.c1.pad == 0 && b0.c1.cin == 256 && b0.c1.cout == 128 && b0.c1.kpad == 256 &&
                        b0.c1.bias && dvid_bneck64_tail_preferred(osz(b0.c2, h), osz(b0.c2, w)))
                        r3 = &b0;
                }
                for (int b = 0; b < nb; ++b) {
                    const Block& blk = m->blocks[0][b];
                    const Block* nxt = b + 1 < nb ? &m->blocks[0][b + 1] : r3;
                    half_t* dst = (b == nb - 1 && stage_out[0]) ? stage_out[0] : (cur == bx ? by : bx);          // (c2, with the p2 level)
                    TRY(bneck_tail(ta, blk.c2.w, blk.c2.bias, blk.c3.w, blk.c3.bias, cur, blk.has_sc ? blk.sc.w : nullptr,
                                   blk.has_sc ? blk.sc.bias : nullptr, nxt ? nxt->c1.w : nullptr, nxt ? nxt->c1.bias : nullptr,
                                   nxt ? nxt->c1.cout : 0, dst, nxt ? tb : nullptr, nf, h, w, cs));
                    std::swap(ta, tb);
                    cur = dst;
                }
                if (r3) res3_t1 = ta;                     // res3's first conv1 output, already computed
                sh[st] = h;
                sw[st] = w;
                continue;
            }
            // res3 (128-wide): the first block's conv1 / strided conv2 / shortcut as their own launches, then one launch per block for
            // conv3 + residual + ReLU + the next block's conv1 (+ the next block's conv2 in front of them)
            if (st == 1 && bneck128_stage(m->blocks[1])) {
                const Block& b0 = m->blocks[1][0];
                auto osz = [](const ConvW& c, int v) { return (v + 2 * c.pad - c.kh) / c.stride + 1; };
                if (dvid_bneck64_tail_preferred(osz(b0.c2, osz(b0.c1, h)), osz(b0.c2, osz(b0.c1, w)))) {
                    int h2 = h, w2 = w;
                    half_t* c1out = res3_t1 ? res3_t1 : t1;           // (res2's last launch may have computed it)
                    half_t* c2out = c1out == t1 ? t2 : t1;
                    if (!res3_t1) TRY(conv_run(b0.c1, cur, nf, h, w, c1out, cs, {.relu = 1, .ho_out = &h2, .wo_out = &w2}));
                    const int h1 = h2, w1 = w2;
                    TRY(conv_run(b0.c2, c1out, nf, h1, w1, c2out, cs, {.relu = 1, .ho_out = &h2, .wo_out = &w2}));
                    TRY(conv_run(b0.sc, cur, nf, h, w, sc, cs));
                    h = h2;
                    w = w2;
                    half_t* ta = c1out;                   // free again: conv2 has consumed it
                    half_t* tb = c2out;
                    half_t* dst = cur == bx ? by : bx;
                    TRY(bneck128_tail(c2out, nullptr, nullptr, b0.c3.w, b0.c3.bias, sc, m->blocks[1][1].c1.w, m->blocks[1][1].c1.bias, dst, ta, nf, h,
                                      w, cs));
                    cur = dst;
                    for (int b = 1; b < nb; ++b) {
                        const Block& blk = m->blocks[1][b];
                        const Block* nxt = b + 1 < nb ? &m->blocks[1][b + 1] : nullptr;
                        dst = (b == nb - 1 && stage_out[st]) ? stage_out[st] : (cur == bx ? by : bx);
                        TRY(bneck128_tail(ta, blk.c2.w, blk.c2.bias, blk.c3.w, blk.c3.bias, cur, nxt ? nxt->c1.w : nullptr,
                                          nxt ? nxt->c1.bias : nullptr, dst, nxt ? tb : nullptr, nf, h, w, cs));
                        std::swap(ta, tb);
                        cur = dst;
                    }
                    sh[st] = h;
                    sw[st] = w;
                    continue;
                }
            }
            for (int b = 0; b < nb; ++b) {
                const Block& blk = m->blocks[st][b];
                int h2 = h, w2 = w;
                TRY(conv_run(blk.c1, cur, nf, h, w, t1, cs, {.relu = 1}));
                TRY(conv_run(blk.c2, t1, nf, h, w, t2, cs, {.relu = 1, .ho_out = &h2, .wo_out = &w2}));
                const half_t* res = cur;
                if (blk.has_sc) {
                    TRY(conv_run(blk.sc, cur, nf, h, w, sc, cs));
                    res = sc;
                }
                // res3..res5 outputs persist for the FPN; everything else ping-pongs between bufX/bufY
                half_t* dst = (b == nb - 1 && stage_out[st]) ? stage_out[st] : (cur == bx ? by : bx);
                TRY(conv_run(blk.c3, t2, nf, h2, w2, dst, cs, {.relu = 1, .res = res, .res_mode = 1}));
                h = h2;
                w = w2;
                cur = dst;
            }
            sh[st] = h;
            sw[st] = w;
        }
        // FPN: outputs go to the caller's [n, ...] tensors at this chain's frame offset
        half_t* pout[4];
        for (int l = 0; l < 4; ++l) pout[l] = pyr[l] ? pyr[l] + (size_t)f0 * sh[l] * sw[l] * 256 : nullptr;
        return run_fpn<half_t>(m, stage_out, k.lat, pout, nf, sh, sw, cs);
    });
}

// Swin-Transformer + FPN (DTYPE float16, swintransformer.py:464-751): fp32 token stream, fp16 MFMA operands
int backbone_swin_f16(dvid_model* m, const float* const* frames, int n, int height, int width, half_t* const* pyr, hipStream_t s) {
    const PixelNorm px(m->cfg);
    TRY(dvid_prep_images_launch(frames, m->img8.as<half_t>(), n, height, width, px.mean, px.inv_std, s));
    // patch embedding: 4x4/4 conv (implicit GEMM on NHWC8) -> fp32 tokens -> LayerNorm  (swintransformer.py:441-458)
    int H = height, W = width;
    float* x = m->sw_x.as<float>();
    float* x2 = m->sw_x2.as<float>();
    TRY(conv_run(m->swin_patch, m->img8.as<half_t>(), n, H, W, x, s, {.out_f32 = 1, .ho_out = &H, .wo_out = &W}));
    TRY(dvid_add_layernorm_launch(x, nullptr, m->swin_patch_norm.g, m->swin_patch_norm.b, x, nullptr, n * H * W, m->swin[0].dim, 0, s));
    half_t* ln16 = m->sw_ln16.as<half_t>();
    half_t* qkv16 = m->sw_qkv16.as<half_t>();
    half_t* attn16 = m->sw_attn16.as<half_t>();
    half_t* h16 = m->sw_h16.as<half_t>();
    half_t* stage_out[4] = {m->c2.as<half_t>(), m->c3.as<half_t>(), m->c4.as<half_t>(), m->c5.as<half_t>()};          // (c2: null without the p2 level, and stage 0 has no out norm then)
    const int ws = m->cfg.swin_window;                           // 7 or 12 (dvid_model_finalize)
    int sh[4], sw[4];
    for (int st = 0; st < 4; ++st) {
        const SwinStageW& S = m->swin[st];
        const int C = S.dim, M = n * H * W;
        for (size_t b = 0; b < S.blocks.size(); ++b) {
            const SwinBlockW& B = S.blocks[b];
            const int shift = (b % 2 == 0) ? 0 : ws / 2;                                        // window_size // 2
            TRY(dvid_add_layernorm_launch(x, nullptr, B.norm1.g, B.norm1.b, nullptr, ln16, M, C, 0, s));
            TRY(linear_run(B.qkv, ln16, M, qkv16, 0, 0, s));
            if (ws == 12) TRY(dvid_swin_window12_attn_launch(qkv16, B.qkv_bias16, B.relbias, attn16, n, H, W, C, S.heads, shift, s));
            else TRY(dvid_swin_window_attn_launch(qkv16, B.qkv_bias16, B.relbias, attn16, n, H, W, C, S.heads, shift, s));
            TRY(conv_run(B.proj, attn16, M, 1, 1, x, s, {.out_f32 = 1, .res = x, .res_mode = 1, .res_f32 = 1}));                         // x += proj(attn)   (fp32 stream)
            TRY(dvid_add_layernorm_launch(x, nullptr, B.norm2.g, B.norm2.b, nullptr, ln16, M, C, 0, s));
            TRY(linear_run(B.fc1, ln16, M, h16, 2, 0, s));                                       // GELU epilogue
            TRY(conv_run(B.fc2, h16, M, 1, 1, x, s, {.out_f32 = 1, .res = x, .res_mode = 1, .res_f32 = 1}));                             // x += fc2(...)
        }
        sh[st] = H;
        sw[st] = W;
        if (S.has_out) TRY(dvid_add_layernorm_launch(x, nullptr, S.out_norm.g, S.out_norm.b, nullptr, stage_out[st], M, C, 0, s));
        if (S.has_down) {
            TRY(dvid_patch_merge_ln_launch(x, S.down_norm.g, S.down_norm.b, h16, n, H, W, C, s));
            H = (H + 1) / 2;
            W = (W + 1) / 2;
            TRY(linear_run(S.down_red, h16, n * H * W, x2, 0, 1, s));
            float* t = x;
            x = x2;
            x2 = t;
        }
    }
    half_t* lat[4] = {m->lat[0].as<half_t>(), m->lat[1].as<half_t>(), m->lat[2].as<half_t>(), m->lat[3].as<half_t>()};
    return run_fpn<half_t>(m, stage_out, lat, pyr, n, sh, sw, s);
}

// ---- entry points: the checks, the precision switch and the contiguous-images form, once for both backbones ----------------------------
// (pyr: the outputs by stage, [0] = p2 or null .. [3] = p5)
typedef int (*BackboneF16)(dvid_model*, const float* const*, int, int, int, half_t* const*, hipStream_t);
typedef int (*BackboneF32)(dvid_model*, const float* const*, int, int, int, float* const*, hipStream_t);

int backbone_frames(dvid_model* m, int type, const char* missing, BackboneF16 f16, BackboneF32 f32, const float* const* frames, int n, int height,
                    int width, void* const* levels, int n_levels, void* stream) {
    g_err[0] = 0;
    if (!frames || n <= 0) FAIL(DVID_ERR_ARG, "no frames");
    if (!m || !m->finalized || !m->has_backbone || m->cfg.backbone_type != type) FAIL(DVID_ERR_STATE, "%s", missing);
    // capacity, not equality: a set mixes frame sizes (ImageNet-VID has 16:9 and 4:3 videos) and the workspace only grows
    if (n > m->ws_frames || height > m->ws_h || width > m->ws_w || height % 32 || width % 32)
        FAIL(DVID_ERR_STATE, "workspace reserved for %d frames of up to %dx%d, got %d of %dx%d", m->ws_frames, m->ws_h, m->ws_w, n,
             height, width);
    if (!pyramid_ok(levels, n_levels) || n_levels != m->fpn_levels)
        FAIL(DVID_ERR_ARG, "the model's backbone makes %d levels: levels must hold that many maps, finest first (got n_levels %d)", m->fpn_levels, n_levels);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    void* pyr[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < n_levels; ++l) pyr[4 - n_levels + l] = levels[l];
    if (m->precision == 1)          // DTYPE float32: the maps are fp32 NHWC
        return f32(m, frames, n, height, width, reinterpret_cast<float* const*>(pyr), s);
    return f16(m, frames, n, height, width, reinterpret_cast<half_t* const*>(pyr), s);
}

// the three-pointer entries: the array form with n_levels 3, refused by a model that has the p2 level
typedef int (*LevelsEntry)(dvid_model*, const float* const*, int, int, int, void* const*, int, void*);
int backbone_three(LevelsEntry run, dvid_model* m, const float* const* frames, int n, int height, int width, void* p3, void* p4, void* p5, void* stream) {
    if (m && m->finalized && m->has_backbone && m->fpn_levels == 4) {
        g_err[0] = 0;
        FAIL(DVID_ERR_STATE, "the model has the p2 level (backbone.fpn_lateral2): call the _levels_frames form of this entry with four maps");
    }
    void* levels[3] = {p3, p4, p5};
    return run(m, frames, n, height, width, levels, 3, stream);
}

// contiguous [n, 3, height, width] images as a frame table
typedef int (*FramesEntry)(dvid_model*, const float* const*, int, int, int, void*, void*, void*, void*);
int backbone_images(FramesEntry run, dvid_model* m, const float* images, int n, int height, int width, void* p3, void* p4, void* p5, void* stream) {
    if (!images || n <= 0) {
        g_err[0] = 0;
        FAIL(DVID_ERR_ARG, "no images");
    }
    std::vector<const float*> frames(n);
    for (int i = 0; i < n; ++i) frames[i] = images + (size_t)i * 3 * height * width;
    return run(m, frames.data(), n, height, width, p3, p4, p5, stream);
}
}  // namespace

extern "C" {
int dvid_backbone_resnet_fpn(dvid_model* m, const float* images, int n, int height, int width, void* p3, void* p4, void* p5,
                             void* stream) {
    return backbone_images(dvid_backbone_resnet_fpn_frames, m, images, n, height, width, p3, p4, p5, stream);
}
int dvid_backbone_resnet_fpn_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* p3, void* p4, void* p5,
                                    void* stream) {
    return backbone_three(dvid_backbone_resnet_fpn_levels_frames, m, frames, n, height, width, p3, p4, p5, stream);
}
int dvid_backbone_resnet_fpn_levels_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* const* levels,
                                           int n_levels, void* stream) {
    return backbone_frames(m, 0, "model not finalized or built without a ResNet backbone", backbone_resnet_f16, backbone_resnet_f32, frames, n, height,
                           width, levels, n_levels, stream);
}

int dvid_backbone_swin_fpn(dvid_model* m, const float* images, int n, int height, int width, void* p3, void* p4, void* p5,
                           void* stream) {
    return backbone_images(dvid_backbone_swin_fpn_frames, m, images, n, height, width, p3, p4, p5, stream);
}
int dvid_backbone_swin_fpn_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* p3, void* p4, void* p5,
                                  void* stream) {
    return backbone_three(dvid_backbone_swin_fpn_levels_frames, m, frames, n, height, width, p3, p4, p5, stream);
}
int dvid_backbone_swin_fpn_levels_frames(dvid_model* m, const float* const* frames, int n, int height, int width, void* const* levels,
                                         int n_levels, void* stream) {
    return backbone_frames(m, 1, "model has no Swin backbone", backbone_swin_f16, backbone_swin_f32, frames, n, height, width, levels, n_levels, stream);
}
}  // extern "C"
