// The detection head's launch sequences: one RCNNHead / RCNNHead_cond pass (DTYPE float16 and float32), the time conditioning that
// feeds it, and the global and local box-level cross attention; with their entry points (dvid_rcnn_head, dvid_global_*, dvid_local_*).
#include "runtime.h"

namespace {
// One RCNNHead / RCNNHead_cond pass over `nf` frames of `M` boxes on stream `s`; ss_dev = the frames' scale / shift rows, `ss_stride`
// floats apart (0: every frame reads the one (head, t) row).
int rcnn_head_chain(dvid_model* m, const HeadW& hw, int is_cond, const void* const* levels, int n_levels, int nf, int height, int width,
                    int M, const float* boxes, const float* pro_features, const float* cond, float* logits, float* boxes_out,
                    float* obj_features, int* bad_box_flag, const float* ss_dev, int ss_stride, hipStream_t s) {
    const int d = m->cfg.hidden_dim, R = nf * M;
    // workspace
    half_t* roi16 = m->roi.as<half_t>();
    half_t* dyn16 = m->dyn.as<half_t>();
    half_t* params16 = m->params.as<half_t>();
    half_t* qkv16 = m->qkv.as<half_t>();        // buffer is sized in fp32 units; fp16 use needs half of it
    half_t* attn16 = m->attn16.as<half_t>();
    float* f32a = m->f32a.as<float>();
    float* f32b = m->f32b.as<float>();
    float* f32c = m->f32c.as<float>();
    float* f32d = m->f32d.as<float>();
    half_t* h16a = m->h16a.as<half_t>();
    half_t* h16b = m->h16b.as<half_t>();
    half_t* hid16 = m->hid16.as<half_t>();
    float* deltas = m->deltas.as<float>();
    float* splitk = m->splitk.as<float>();
    half_t* vt = m->vt.as<half_t>();

    // --- RoIAlign ---
    const RoiLevels lv = roi_levels<half_t>(levels, n_levels, height, width, 0, d);
    float* pro32 = f32a;
    // A pass that gets its proposal features from the caller needs nothing of the tile before DynamicConv: the gather then runs INSIDE the
    // DynamicConv launch (csrc/dynconv.hip, FUSED_ROI) and the fp16 tile never reaches memory.  A pass without them takes the tile's mean
    // over the bins as its features (box_head.py:509-510) ahead of the self-attention: the two launches.
    const bool roi_fused = g_opt.roi_fuse && pro_features != nullptr && d == 256;
    double map_px = 0;
    for (int l = 0; l < lv.n_levels; ++l) map_px += (double)lv.h[l] * lv.w[l];
    if (!roi_fused) {
        // algorithmic bytes: the pyramid's maps of the launch's frames once + one 49 x d tile per box (the 784 taps per box go through L1)
        TRY(prof_other("roialign", R, d, 49, 0.0, (double)nf * map_px * d * 2.0 + (double)R * 49 * d * 2.0, s,
                       [&] { return dvid_roialign_launch(lv, d, boxes, nf, M, roi16, pro_features ? nullptr : pro32, s); }));
    }
    const float* pro = pro_features ? pro_features : pro32;
    // --- self attention + norm1 ---
    TRY(dvid_f32_to_f16_launch(pro, h16a, (long)R * d, s));
    TRY(linear_run(hw.in_proj, h16a, R, qkv16, 0, 0, s));          // fp16 q|k|v, MFMA operands
    TRY(prof_other("mha_mfma", R, d, M, 4.0 * R * (double)M * d, (double)R * d * 2.0 * 4.0, s, [&] {
        return dvid_mha_mfma_launch(qkv16, qkv16 + d, qkv16 + 2 * d, attn16, vt, nf, M, M, m->cfg.nheads, 3 * d, 3 * d, d, (long)M * 3 * d,
                                    (long)M * 3 * d, (long)M * d, s);
    }));
    TRY(linear_run(hw.out_proj, attn16, R, f32b, 0, 1, s));
    float* x1 = f32c;
    TRY(dvid_add_layernorm_launch(pro, f32b, hw.norm1.g, hw.norm1.b, x1, h16a, R, d, 0, s));
    // --- DynamicConv ---
    // dynamic_layer writes 64 KB of parameters per box that DynamicConv reads straight back (csrc/dynconv.hip)
    TRY(linear_run(hw.dynamic_layer, h16a, R, params16, 0, 0, s));
    {
        const int dd = m->cfg.dim_dynamic;
        if (roi_fused) {
            // algorithmic bytes: the maps once + the parameters + the output tile per box
            TRY(prof_other("dynconv_roi", R, d, dd, 2.0 * R * 49.0 * d * dd * 2.0, (double)nf * map_px * d * 2.0 + (double)R * (49 * d * 2.0 + 2.0 * d * dd * 2.0), s, [&] {
                return dvid_dynconv_roi_launch(lv, d, boxes, nf, M, params16, hw.dc_norm1.g, hw.dc_norm1.b, hw.dc_norm2.g, hw.dc_norm2.b, dyn16, s);
            }));
        } else {
            TRY(prof_other("dynconv", R, d, dd, 2.0 * R * 49.0 * d * dd * 2.0, (double)R * (2.0 * 49 * d * 2.0 + 2.0 * d * dd * 2.0), s,
                           [&] { return dvid_dynconv_launch(roi16, params16, hw.dc_norm1.g, hw.dc_norm1.b, hw.dc_norm2.g, hw.dc_norm2.b, dyn16, R, s); }));
        }
    }
    // out_layer: K = 49*d = 12544 on only R x d outputs -> split K over 7 workgroups per tile; the partial slabs
    // and the bias are summed inside the norm3 kernel that consumes them.
    const int osplit = ((hw.out_layer.kpad / 64) % 7 == 0) ? 7 : 1;
    if (osplit > 1) {
        TRY(conv_run(hw.out_layer, dyn16, R, 1, 1, splitk, s, {.out_f32 = 1, .splitk = osplit}));
        TRY(dvid_add_layernorm_launch(splitk, nullptr, hw.dc_norm3.g, hw.dc_norm3.b, f32b, nullptr, R, d, 1, s, osplit, (long)R * d,
                                      hw.out_layer.bias));
    } else {
        TRY(linear_run(hw.out_layer, dyn16, R, f32b, 0, 1, s));
        TRY(dvid_add_layernorm_launch(f32b, nullptr, hw.dc_norm3.g, hw.dc_norm3.b, f32b, nullptr, R, d, 1, s));
    }
    float* obj = f32d;
    TRY(dvid_add_layernorm_launch(x1, f32b, hw.norm2.g, hw.norm2.b, obj, h16a, R, d, 0, s));
    // --- FFN + norm3 + modulation + towers + class_logits + bboxes_delta + apply_deltas: one row-tile kernel (csrc/headtail.hip);
    // option head_tail = 0 (the fused-vs-layerwise parity test) or an unsupported shape takes the layer-by-layer launches below
    if (g_opt.head_tail && hw.frag.ok) {
        HeadTailParams q;
        memset(&q, 0, sizeof(q));
        q.x16 = h16a;
        q.obj32 = obj;
        q.w1f = hw.frag.w1;
        q.b1 = hw.linear1.bias;
        q.w2f = hw.frag.w2;
        q.b2 = hw.linear2.bias;
        q.n3g = hw.norm3.g;
        q.n3b = hw.norm3.b;
        q.scale = ss_dev;
        q.ss_stride = ss_stride;
        q.rows_per_frame = M;
        q.cond32 = is_cond ? cond : nullptr;
        q.wcf = hw.frag.wc;
        q.bc = hw.c_mlp.bias;
        q.num_cls = (int)hw.cls.size();
        q.num_reg = (int)hw.reg.size();
        q.num_classes = m->cfg.num_classes;
        q.dff = m->cfg.dim_feedforward;
        for (size_t i = 0; i < hw.cls.size(); ++i) {
            q.clsf[i] = hw.frag.cls[i];
            q.clsg[i] = hw.cls_ln[i].g;
            q.clsb[i] = hw.cls_ln[i].b;
        }
        for (size_t i = 0; i < hw.reg.size(); ++i) {
            q.regf[i] = hw.frag.reg[i];
            q.regg[i] = hw.reg_ln[i].g;
            q.regb[i] = hw.reg_ln[i].b;
        }
        q.wlogf = hw.frag.wlog;
        q.blog = hw.class_logits.bias;
        q.wdelf = hw.frag.wdel;
        q.bdel = hw.bboxes_delta.bias;
        q.boxes = boxes;
        q.obj_out = obj_features;
        q.logits = logits;
        q.boxes_out = boxes_out;
        q.bad_flag = bad_box_flag;
        q.R = R;
        q.wx = 2.f;
        q.wy = 2.f;
        q.ww = 1.f;
        q.wh = 1.f;
        q.clamp = logf(100000.f / 16.f);
        {
            const double dff = m->cfg.dim_feedforward, nt = (double)hw.cls.size() + (double)hw.reg.size() + (is_cond ? 1.0 : 0.0);
            return prof_other("head_tail", R, d, (int)dff, 2.0 * R * d * (2.0 * dff + nt * d + 64.0),
                              (double)R * (d * 6.0 + d * 4.0 + m->cfg.num_classes * 4.0 + 32.0), s, [&] { return dvid_head_tail_launch(q, s); });
        }
    }
    // --- FFN + norm3 ---
    TRY(linear_run(hw.linear1, h16a, R, hid16, 1, 0, s));
    TRY(linear_run(hw.linear2, hid16, R, f32b, 0, 1, s));
    TRY(dvid_add_layernorm_launch(obj, f32b, hw.norm3.g, hw.norm3.b, obj_features, nullptr, R, d, 0, s));
    // --- time / cond modulation ---
    half_t* fc16 = h16a;
    if (!is_cond) {
        TRY(dvid_modulate_launch(obj_features, ss_dev, ss_stride, ss_dev + d, 0, ss_stride, fc16, R, M, d, s));
    } else {
        TRY(dvid_silu_f16_launch(cond, h16b, (long)R * d, s));
        TRY(linear_run(hw.c_mlp, h16b, R, f32b, 0, 1, s));
        TRY(dvid_modulate_launch(obj_features, ss_dev, ss_stride, f32b, 1, d, fc16, R, M, d, s));
    }
    // --- cls tower ---
    const half_t* cur = fc16;
    for (size_t i = 0; i < hw.cls.size(); ++i) {
        TRY(linear_run(hw.cls[i], cur, R, f32b, 0, 1, s));
        TRY(dvid_add_layernorm_launch(f32b, nullptr, hw.cls_ln[i].g, hw.cls_ln[i].b, nullptr, h16b, R, d, 1, s));
        cur = h16b;
    }
    TRY(conv_run(hw.class_logits, cur, R, 1, 1, logits, s, {.out_f32 = 1, .ldc = m->cfg.num_classes}));
    // --- reg tower ---
    cur = fc16;
    half_t* regbuf[2] = {h16b, attn16};
    for (size_t i = 0; i < hw.reg.size(); ++i) {
        TRY(linear_run(hw.reg[i], cur, R, f32b, 0, 1, s));
        TRY(dvid_add_layernorm_launch(f32b, nullptr, hw.reg_ln[i].g, hw.reg_ln[i].b, nullptr, regbuf[i & 1], R, d, 1, s));
        cur = regbuf[i & 1];
    }
    TRY(conv_run(hw.bboxes_delta, cur, R, 1, 1, deltas, s, {.out_f32 = 1, .ldc = 4}));
    TRY(dvid_apply_deltas_launch(deltas, 4, boxes, boxes_out, R, 2.f, 2.f, 1.f, 1.f, logf(100000.f / 16.f), bad_box_flag, s));
    return DVID_OK;
}

// The same pass with DTYPE float32 (the f32_* kernels of csrc/roialign.hip, attention.hip, dynconv.hip, elementwise.hip; csrc/f32.hip for the layers): fp32 RoI tiles, q / k / v, dynamic parameters, hidden layers; layer by layer.
int rcnn_head_chain_f32(dvid_model* m, const HeadW& hw, int is_cond, const void* const* levels, int n_levels, int nf, int height, int width,
                        int M, const float* boxes, const float* pro_features, const float* cond, float* logits, float* boxes_out,
                        float* obj_features, int* bad_box_flag, const float* ss_dev, int ss_stride, hipStream_t s, float* tail_input = nullptr, float* interact_input = nullptr,
                        float* roi_tiles = nullptr) {
    const int d = m->cfg.hidden_dim, R = nf * M, dd = m->cfg.dim_dynamic;
    float* roi = m->roi.as<float>();
    float* dyn = m->dyn.as<float>();
    float* params = m->params.as<float>();
    float* qkv = m->qkv.as<float>();
    float* attn = m->attn16.as<float>();
    float* f32a = m->f32a.as<float>();
    float* f32b = m->f32b.as<float>();
    float* f32c = m->f32c.as<float>();
    float* f32d = m->f32d.as<float>();
    float* ha = m->h16a.as<float>();
    float* hb = m->h16b.as<float>();
    float* hid = m->hid16.as<float>();
    float* deltas = m->deltas.as<float>();

    const RoiLevels32 lv = roi_levels<float>(levels, n_levels, height, width, 0, d);
    double map_px = 0;
    for (int l = 0; l < lv.n_levels; ++l) map_px += (double)lv.h[l] * lv.w[l];
    float* pro32 = f32a;
    TRY(prof_other("roialign_f32", R, d, 49, 0.0, (double)nf * map_px * d * 4.0 + (double)R * 49 * d * 4.0, s,
                   [&] { return dvid_f32_roialign_launch(lv, d, boxes, nf, M, roi, pro_features ? nullptr : pro32, s); }));
    const float* pro = pro_features ? pro_features : pro32;
    // --- self attention + norm1 (box_head.py:512-517)
    TRY(linear_run32(hw.in_proj, pro, R, qkv, 0, s));
    TRY(prof_other("mha_f32", R, d, M, 4.0 * R * (double)M * d, (double)R * d * 4.0 * 4.0, s, [&] {
        return dvid_f32_mha_launch(qkv, qkv + d, qkv + 2 * d, attn, nf, M, M, m->cfg.nheads, 3 * d, 3 * d, d, (long)M * 3 * d, (long)M * 3 * d,
                                   (long)M * d, s);
    }));
    TRY(linear_run32(hw.out_proj, attn, R, f32b, 0, s));
    float* x1 = f32c;
    TRY(dvid_add_layernorm_launch(pro, f32b, hw.norm1.g, hw.norm1.b, x1, nullptr, R, d, 0, s));
    // the inputs of DynamicConv's backward (dvid_rcnn_head_levels_keep2): copies, as the tail's input below
    if (interact_input) HIP_TRY(hipMemcpyAsync(interact_input, x1, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (roi_tiles) HIP_TRY(hipMemcpyAsync(roi_tiles, roi, (size_t)R * 49 * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    // --- DynamicConv (box_head.py:687-711)
    TRY(linear_run32(hw.dynamic_layer, x1, R, params, 0, s));
    TRY(prof_other("dynconv_f32", R, d, dd, 2.0 * R * 49.0 * d * dd * 2.0, (double)R * (2.0 * 49 * d * 4.0 + 2.0 * d * dd * 4.0), s,
                   [&] { return dvid_f32_dynconv_launch(roi, params, hw.dc_norm1.g, hw.dc_norm1.b, hw.dc_norm2.g, hw.dc_norm2.b, dyn, R, m->f32_range_flag, s); }));
    TRY(linear_run32(hw.out_layer, dyn, R, f32b, 0, s));
    TRY(dvid_add_layernorm_launch(f32b, nullptr, hw.dc_norm3.g, hw.dc_norm3.b, f32b, nullptr, R, d, 1, s));
    float* obj = f32d;
    TRY(dvid_add_layernorm_launch(x1, f32b, hw.norm2.g, hw.norm2.b, obj, nullptr, R, d, 0, s));
    // the tail's input, kept for its backward (dvid_rcnn_head_levels_keep): a copy, so every kernel of this pass reads and writes what it did
    if (tail_input) HIP_TRY(hipMemcpyAsync(tail_input, obj, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    // --- FFN + norm3
    TRY(linear_run32(hw.linear1, obj, R, hid, 1, s));
    TRY(linear_run32(hw.linear2, hid, R, f32b, 0, s));
    TRY(dvid_add_layernorm_launch(obj, f32b, hw.norm3.g, hw.norm3.b, obj_features, nullptr, R, d, 0, s));
    // --- time / cond modulation
    float* fc = ha;
    if (!is_cond) {
        TRY(dvid_f32_modulate_launch(obj_features, ss_dev, ss_stride, ss_dev + d, 0, ss_stride, fc, R, M, d, s));
    } else {
        TRY(dvid_f32_silu_launch(cond, hb, (long)R * d, s));
        TRY(linear_run32(hw.c_mlp, hb, R, f32b, 0, s));
        TRY(dvid_f32_modulate_launch(obj_features, ss_dev, ss_stride, f32b, 1, d, fc, R, M, d, s));
    }
    // --- cls tower
    const float* cur = fc;
    for (size_t i = 0; i < hw.cls.size(); ++i) {
        TRY(linear_run32(hw.cls[i], cur, R, f32b, 0, s));
        TRY(dvid_add_layernorm_launch(f32b, nullptr, hw.cls_ln[i].g, hw.cls_ln[i].b, hb, nullptr, R, d, 1, s));
        cur = hb;
    }
    TRY(linear_run32(hw.class_logits, cur, R, logits, 0, s, m->cfg.num_classes));
    // --- reg tower
    cur = fc;
    float* regbuf[2] = {hb, attn};
    for (size_t i = 0; i < hw.reg.size(); ++i) {
        TRY(linear_run32(hw.reg[i], cur, R, f32b, 0, s));
        TRY(dvid_add_layernorm_launch(f32b, nullptr, hw.reg_ln[i].g, hw.reg_ln[i].b, regbuf[i & 1], nullptr, R, d, 1, s));
        cur = regbuf[i & 1];
    }
    TRY(linear_run32(hw.bboxes_delta, cur, R, deltas, 0, s, 4));
    TRY(dvid_apply_deltas_launch(deltas, 4, boxes, boxes_out, R, 2.f, 2.f, 1.f, 1.f, logf(100000.f / 16.f), bad_box_flag, s));
    return DVID_OK;
}

float gelu_exact(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// box_head.py:218-223 + :734-741 on the host (a handful of distinct t values per config)
const std::vector<float>& time_embedding(dvid_model* m, int64_t t) {
    auto it = m->time_cache.find(t);
    if (it != m->time_cache.end()) return it->second;
    const int d = m->cfg.hidden_dim, td = 4 * d, half = d / 2;
    std::vector<float> emb(d), h1(td), out(td);
    const float e = logf(10000.f) / (half - 1);
    for (int i = 0; i < half; ++i) {
        const float a = (float)t * expf((float)i * -e);
        emb[i] = sinf(a);
        emb[half + i] = cosf(a);
    }
    for (int o = 0; o < td; ++o) {
        double acc = m->tm1_b[o];
        for (int i = 0; i < d; ++i) acc += (double)m->tm1_w[(size_t)o * d + i] * emb[i];
        h1[o] = gelu_exact((float)acc);
    }
    for (int o = 0; o < td; ++o) {
        double acc = m->tm3_b[o];
        for (int i = 0; i < td; ++i) acc += (double)m->tm3_w[(size_t)o * td + i] * h1[i];
        out[o] = (float)acc;
    }
    return m->time_cache.emplace(t, std::move(out)).first->second;
}

// ---- attention against a projected memory (KvMemory, runtime.h): the video's global memory, the streams' grouped global memories and the
// local memories are instances of these two steps; they differ in the weights, the KvMemory and the output stage of the entry point ----
// K | V rows of `groups` memories of `lk` rows each into `mem`: one linear over all groups * lk rows.  `pad_rows`: rows the buffer is
// asked for beyond those (see KvMemory).  The shape is cleared first and set last: a failed call leaves nothing projected.
int kv_project(dvid_model* m, const ConvW& wkv, KvMemory& mem, const float* memory, int lk, int groups, int pad_rows, hipStream_t s) {
    const int d = m->cfg.hidden_dim, n = lk * groups;
    mem.lk = mem.groups = 0;
    TRY(mem.kv.ensure(((size_t)n + pad_rows) * 2 * d * 4, &m->ws_gen));
    if (m->precision == 1) {          // fp32 K | V rows
        TRY(linear_run32(wkv, memory, n, mem.kv.as<float>(), 0, s));
    } else {
        TRY(mem.src16.ensure((size_t)n * d * 2, &m->ws_gen));
        TRY(dvid_f32_to_f16_launch(memory, mem.src16.as<half_t>(), (long)n * d, s));
        TRY(linear_run(wkv, mem.src16.as<half_t>(), n, mem.kv.p, 0, 0, s));
    }
    mem.lk = lk;
    mem.groups = groups;
    return DVID_OK;
}

// attn16 = MHA(q_proj(query), K_g, V_g): rows / groups consecutive query rows per group against that group's projected rows of `mem`, Q
// projection over all rows at once; fp16 or fp32 rows as the model's precision says.  One group: batch index 0, the strides address nothing.
int kv_attend(dvid_model* m, const ConvW& wq, const KvMemory& mem, const float* query, int rows, hipStream_t s) {
    const int d = m->cfg.hidden_dim, nh = m->cfg.nheads, groups = mem.groups, lk = mem.lk, lq = rows / groups;
    const long q_bs = (long)lq * d, kv_bs = (long)lk * 2 * d;
    if (m->precision == 1) {
        float* qp = m->h16a.as<float>();
        const float* kv32 = mem.kv.as<float>();
        TRY(linear_run32(wq, query, rows, qp, 0, s));
        TRY(dvid_f32_mha_launch(qp, kv32, kv32 + d, m->attn16.as<float>(), groups, lq, lk, nh, d, 2 * d, d, q_bs, kv_bs, q_bs, s));
        return DVID_OK;
    }
    TRY(dvid_f32_to_f16_launch(query, m->h16a.as<half_t>(), (long)rows * d, s));
    TRY(linear_run(wq, m->h16a.as<half_t>(), rows, m->h16b.p, 0, 0, s));
    const half_t* kv = mem.kv.as<half_t>();
    TRY(m->vt.ensure((size_t)groups * nh * 32 * (((size_t)lk + 31) / 32 * 32 + 32) * 2, &m->ws_gen));          // per group
    TRY(dvid_mha_mfma_launch(m->h16b.as<half_t>(), kv, kv + d, m->attn16.as<half_t>(), m->vt.as<half_t>(), groups, lq, lk, nh, d, 2 * d, d, q_bs, kv_bs,
                             q_bs, s));
    return DVID_OK;
}

// out = out_proj(attn16), the output stage of both global forms
int global_out_proj(dvid_model* m, int rows, float* out, hipStream_t s) {
    if (m->precision == 1) return linear_run32(m->gout, m->attn16.as<float>(), rows, out, 0, s);
    return linear_run(m->gout, m->attn16.as<half_t>(), rows, out, 0, 1, s);
}
}  // namespace

extern "C" {
int dvid_rcnn_head(dvid_model* m, int head_index, int is_cond, const void* p3, const void* p4, const void* p5, int n_frames,
                   int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                   const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                   int* bad_box_flag, void* stream) {
    g_err[0] = 0;
    if (m && m->finalized && m->has_backbone && m->fpn_levels == 4)
        FAIL(DVID_ERR_STATE, "the model has the p2 level (backbone.fpn_lateral2): call dvid_rcnn_head_levels with its four maps");
    const void* levels[3] = {p3, p4, p5};
    return dvid_rcnn_head_levels(m, head_index, is_cond, levels, 3, n_frames, height, width, boxes_per_frame, boxes, pro_features, t, cond, logits,
                                 boxes_out, obj_features, bad_box_flag, stream);
}

int dvid_rcnn_head_levels(dvid_model* m, int head_index, int is_cond, const void* const* levels, int n_levels, int n_frames,
                          int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                          const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                          int* bad_box_flag, void* stream) {
    return dvid_rcnn_head_levels_keep2(m, head_index, is_cond, levels, n_levels, n_frames, height, width, boxes_per_frame, boxes, pro_features, t, cond,
                                       logits, boxes_out, obj_features, bad_box_flag, nullptr, nullptr, nullptr, stream);
}

int dvid_rcnn_head_levels_keep(dvid_model* m, int head_index, int is_cond, const void* const* levels, int n_levels, int n_frames,
                               int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                               const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                               int* bad_box_flag, float* tail_input, void* stream) {
    return dvid_rcnn_head_levels_keep2(m, head_index, is_cond, levels, n_levels, n_frames, height, width, boxes_per_frame, boxes, pro_features, t, cond,
                                       logits, boxes_out, obj_features, bad_box_flag, tail_input, nullptr, nullptr, stream);
}

int dvid_rcnn_head_levels_keep2(dvid_model* m, int head_index, int is_cond, const void* const* levels, int n_levels, int n_frames,
                                int height, int width, int boxes_per_frame, const float* boxes, const float* pro_features,
                                const int64_t* t, const float* cond, float* logits, float* boxes_out, float* obj_features,
                                int* bad_box_flag, float* tail_input, float* interact_input, float* roi_tiles, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized) FAIL(DVID_ERR_STATE, "model not finalized");
    if ((tail_input || interact_input || roi_tiles) && m->precision != 1)
        FAIL(DVID_ERR_UNSUPPORTED, "dvid_rcnn_head_levels_keep: the tail's input is kept for DTYPE float32 models only (fp16 gradients are out of scope)");
    if (!pyramid_ok(levels, n_levels)) FAIL(DVID_ERR_ARG, "the pyramid is 3 maps (p3..p5) or 4 (p2..p5), none of them null (got n_levels %d)", n_levels);
    if (m->has_backbone && n_levels != m->fpn_levels)
        FAIL(DVID_ERR_ARG, "n_levels %d, but the model's backbone makes %d levels", n_levels, m->fpn_levels);
    const std::vector<HeadW>& hv = is_cond ? m->heads_cond : m->heads;
    if (head_index < 0 || head_index >= (int)hv.size()) FAIL(DVID_ERR_ARG, "head_index %d out of range", head_index);
    if (is_cond && !cond) FAIL(DVID_ERR_ARG, "RCNNHead_cond needs cond");
    if (n_frames > m->ws_frames || boxes_per_frame > m->ws_boxes) FAIL(DVID_ERR_STATE, "workspace too small; call dvid_workspace_reserve");
    if (height % 32 || width % 32) FAIL(DVID_ERR_ARG, "height/width must be multiples of 32");
    const HeadW& hw = hv[head_index];
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int d = m->cfg.hidden_dim, M = boxes_per_frame;

    // --- time conditioning (box_head.py:533-536 / :645): a scale/shift row is a function of (head, t) only.  Every distinct
    // (head slot, t value) keeps ONE device row, computed on the host the first time it is seen; a call whose frames share
    // one t (every call of the reference's sampler) reads that row with frame stride 0, so the steady state -- including the 4
    // alternating time steps of the x4 sampler and any ragged tail length -- does no host math, no upload and no stream sync.
    const int slot = (is_cond ? m->cfg.num_heads : 0) + head_index;
    auto ss_row = [&](int64_t tv, const float** dev) -> int {
        auto key = std::make_pair(slot, tv);
        auto it = m->ss_rows.find(key);
        if (it == m->ss_rows.end()) {
            const int td = 4 * d;
            const std::vector<float>& te = time_embedding(m, tv);
            std::vector<float> sl(td), row(hw.bt_out);
            for (int i = 0; i < td; ++i) sl[i] = te[i] / (1.f + expf(-te[i]));  // SiLU
            for (int o = 0; o < hw.bt_out; ++o) {
                double acc = hw.bt_b[o];
                for (int i = 0; i < td; ++i) acc += (double)hw.bt_w[(size_t)o * td + i] * sl[i];
                row[o] = (float)acc;
            }
            constexpr size_t kSsSlabRows = 256, kSsRowFloats = 512;          // bt_out = 2 d <= 512 floats
            if ((size_t)hw.bt_out > kSsRowFloats) return DVID_ERR_UNSUPPORTED;
            if (m->ss_slabs.empty() || m->ss_slab_used == kSsSlabRows) {
                m->ss_slabs.emplace_back();
                TRY(m->ss_slabs.back().ensure(kSsSlabRows * kSsRowFloats * sizeof(float), &m->ws_gen));
                m->ss_slab_used = 0;
            }
            float* dst = m->ss_slabs.back().as<float>() + (m->ss_slab_used++) * kSsRowFloats;
            HIP_TRY(hipMemcpy(dst, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice));   // once per distinct (head, t)
            it = m->ss_rows.emplace(key, dst).first;
        }
        *dev = it->second;
        return DVID_OK;
    };
    const float* ss_dev = nullptr;
    int ss_stride = 0;              // floats between the rows of consecutive frames (0: one shared row)
    bool same_t = true;
    for (int f = 1; f < n_frames; ++f) same_t = same_t && t[f] == t[0];
    if (same_t) {
        TRY(ss_row(t[0], &ss_dev));
    } else {
        // frames with different time steps (not produced by the reference's sampler): the rows are laid out per frame in
        // the workspace by device-to-device copies on the launch stream
        float* tab = m->ss.as<float>() + (size_t)slot * (((size_t)m->ws_frames + 3) / 4 * 4) * 2 * d;          // slot stride of dvid_workspace_reserve
        for (int f = 0; f < n_frames; ++f) {
            const float* row = nullptr;
            TRY(ss_row(t[f], &row));
            HIP_TRY(hipMemcpyAsync(tab + (size_t)f * hw.bt_out, row, (size_t)hw.bt_out * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        ss_dev = tab;
        ss_stride = hw.bt_out;
    }

    // One launch sequence on the caller's stream.  (Frames are independent inside a head, but two sub-batch chains on two streams
    // measured slower -- 0.53 against 0.49 ms per pass, tools/bench_head.py -- the switch that kept that path is gone.)
    if (m->precision == 1)
        return rcnn_head_chain_f32(m, hw, is_cond, levels, n_levels, n_frames, height, width, M, boxes, pro_features, cond, logits, boxes_out, obj_features,
                                   bad_box_flag, ss_dev, ss_stride, s, tail_input, interact_input, roi_tiles);
    return rcnn_head_chain(m, hw, is_cond, levels, n_levels, n_frames, height, width, M, boxes, pro_features, cond, logits, boxes_out, obj_features,
                           bad_box_flag, ss_dev, ss_stride, s);
}

// K/V projections of the global memory (box_head.py:366-380 recomputes them on every call; they depend on the per-video
// memory only): projected once per memory update and kept until the next one.
int dvid_global_memory_project(dvid_model* m, const float* memory, int lk, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized || !m->gq.w) FAIL(DVID_ERR_STATE, "model not finalized or has no global attention");
    if (!memory || lk <= 0) FAIL(DVID_ERR_ARG, "empty memory");
    return kv_project(m, m->gkv, m->vmem, memory, lk, 1, 0, reinterpret_cast<hipStream_t>(stream));
}

int dvid_global_xattn(dvid_model* m, const float* query, int rows, const float* memory, int lk, float* out, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized || !m->gq.w) FAIL(DVID_ERR_STATE, "model not finalized or has no global attention");
    if (rows > m->ws_frames * m->ws_boxes) FAIL(DVID_ERR_STATE, "workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (memory) {
        TRY(dvid_global_memory_project(m, memory, lk, stream));
    } else if (m->vmem.lk <= 0 || (lk > 0 && lk != m->vmem.lk)) {
        FAIL(DVID_ERR_STATE, "no projected global memory of %d rows (call dvid_global_memory_project)", lk);
    }
    TRY(kv_attend(m, m->gq, m->vmem, query, rows, s));
    TRY(global_out_proj(m, rows, out, s));
    return DVID_OK;
}

// `groups` global memories of `lk` rows each -- one per live stream -- into a KvMemory of their OWN (gmem).  vmem, the projection a video
// holds between its calls, is neither read nor written.
int dvid_global_memory_project_groups(dvid_model* m, const float* memory, int lk, int groups, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized || !m->gq.w) FAIL(DVID_ERR_STATE, "model not finalized or has no global attention");
    if (!memory || lk <= 0 || groups <= 0) FAIL(DVID_ERR_ARG, "empty global memory (%d groups of %d rows)", groups, lk);
    if ((long)lk * groups > (1L << 24)) FAIL(DVID_ERR_ARG, "global memory of %d x %d rows", groups, lk);
    return kv_project(m, m->gkv, m->gmem, memory, lk, groups, 64, reinterpret_cast<hipStream_t>(stream));
}

// out = out_proj(MHA(q_proj(query), K_g, V_g)): rows / groups consecutive query rows per group against that group's projected memory
int dvid_global_xattn_groups(dvid_model* m, const float* query, int rows, int groups, int lk, float* out, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized || !m->gq.w) FAIL(DVID_ERR_STATE, "model not finalized or has no global attention");
    if (!query || !out || rows <= 0 || groups <= 0 || rows % groups) FAIL(DVID_ERR_ARG, "%d query rows in %d groups", rows, groups);
    if (m->gmem.lk <= 0 || lk != m->gmem.lk || groups != m->gmem.groups)
        FAIL(DVID_ERR_STATE, "no projected global memories of %d x %d rows (call dvid_global_memory_project_groups)", groups, lk);
    if (rows > m->ws_frames * m->ws_boxes) FAIL(DVID_ERR_STATE, "workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TRY(kv_attend(m, m->gq, m->gmem, query, rows, s));
    TRY(global_out_proj(m, rows, out, s));
    return DVID_OK;
}

// K/V projections of `groups` local memories of `lk` rows each (box_head.py:338, :362: key = value = proposal_feats_local[stage])
int dvid_local_memory_project(dvid_model* m, int stage, const float* memory, int lk, int groups, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized || m->local_stages == 0) FAIL(DVID_ERR_STATE, "model not finalized or has no local attention");
    if (stage != m->local_stages - 1) FAIL(DVID_ERR_ARG, "local attention stage %d: only the last stage (%d) is computed", stage, m->local_stages - 1);
    if (!memory || lk <= 0 || groups <= 0) FAIL(DVID_ERR_ARG, "empty local memory");
    if ((long)lk * groups > (1L << 24)) FAIL(DVID_ERR_ARG, "local memory of %d x %d rows", groups, lk);
    return kv_project(m, m->lkv, m->lmem, memory, lk, groups, 64, reinterpret_cast<hipStream_t>(stream));
}

// out = LayerNorm(out_proj(MHA(q_proj(query), K, V))), group g's rows / groups queries against group g's lk projected memory rows
// (box_head.py:360-363); the out-projection, its bias and the LayerNorm are one launch (csrc/localattn.hip).
int dvid_local_xattn(dvid_model* m, int stage, const float* query, int rows, int groups, int lk, float* out, void* stream) {
    g_err[0] = 0;
    if (!m || !m->finalized || m->local_stages == 0) FAIL(DVID_ERR_STATE, "model not finalized or has no local attention");
    if (stage != m->local_stages - 1) FAIL(DVID_ERR_ARG, "local attention stage %d: only the last stage (%d) is computed", stage, m->local_stages - 1);
    if (!query || !out || rows <= 0 || groups <= 0 || rows % groups) FAIL(DVID_ERR_ARG, "%d query rows in %d groups", rows, groups);
    if (m->lmem.lk <= 0 || lk != m->lmem.lk || groups != m->lmem.groups)
        FAIL(DVID_ERR_STATE, "no projected local memory of %d x %d rows (call dvid_local_memory_project)", groups, lk);
    if (rows > m->ws_frames * m->ws_boxes) FAIL(DVID_ERR_STATE, "workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TRY(kv_attend(m, m->lq, m->lmem, query, rows, s));
    OutProjLnParams p;
    memset(&p, 0, sizeof(p));
    p.bias = m->lout.bias;
    p.gamma = m->lln.g;
    p.beta = m->lln.b;
    p.out = out;
    p.rows = rows;
    p.d = m->cfg.hidden_dim;
    p.x = m->attn16.p;
    if (m->precision == 1) {
        const bool split = g_opt.f32_split != 0 && m->lout_fhi && m->lout_flo;
        p.mode = split ? 1 : 2;
        p.wf_hi = m->lout_fhi;
        p.wf_lo = m->lout_flo;
        p.w32 = m->lout.w32;
        p.wscale = m->lout.wscale32;
        p.range_flag = m->lout.range_flag;
    } else {
        p.mode = 0;
        p.wf_hi = m->lout_f;
    }
    TRY(dvid_outproj_ln_launch(p, s));
    return DVID_OK;
}
}  // extern "C"
