// Weight ingest and repack: the tensors dvid_model_set_tensor collected become, in dvid_model_finalize, device weights in the layouts
// the kernels read -- FrozenBN folded, fp16 [cout][kpad] MFMA-operand rows (and, for DTYPE float32, the un-rounded scaled rows and their
// (hi, lo) fp16 planes), MFMA fragment order for the head tail, the Swin relative-position bias gathered per window.
#include "runtime.h"

namespace {
half_t f2h(float f) { return (half_t)f; }

int upload_f32(dvid_model* m, const std::vector<float>& v, float** dev) {
    return m->upload(v.data(), v.size() * sizeof(float), reinterpret_cast<void**>(dev));
}

// weights [cout][cin][kh][kw] (OIHW; Linear: [out][in]) -> fp16 [cout][kpad], k = (ky*kw + kx)*cin_pad + c.
// `scale` (per cout, may be empty) is folded in before rounding to fp16; row_perm maps dst row -> src row.
int make_conv(dvid_model* m, const HostTensor& w, const std::vector<float>& scale, const std::vector<float>& bias, int stride, int pad,
              int cin_pad, const std::vector<int>* row_perm, ConvW* out) {
    const int cout = (int)w.shape[0], cin = (int)w.shape[1];
    const int kh = w.shape.size() == 4 ? (int)w.shape[2] : 1, kw = w.shape.size() == 4 ? (int)w.shape[3] : 1;
    const int cp = cin_pad > 0 ? cin_pad : cin;
    const int kreal = kh * kw * cp;
    const int kpad = (kreal + 63) / 64 * 64;
    const bool f32 = m->precision == 1;          // also the un-rounded rows for the fp32 kernels
    const int c4 = (cin + 3) / 4 * 4, k32 = (kh * kw * c4 + 15) / 16 * 16;
    std::vector<half_t> packed((size_t)cout * kpad, f2h(0.f));
    std::vector<float> p32(f32 ? (size_t)cout * k32 : 0, 0.f), ws(f32 ? cout : 0, 1.f);
    for (int o = 0; o < cout; ++o) {
        const int so = row_perm ? (*row_perm)[o] : o;
        const float sc = scale.empty() ? 1.f : scale[so];
        float mx = 0.f;
        for (int c = 0; c < cin; ++c)
            for (int y = 0; y < kh; ++y)
                for (int x = 0; x < kw; ++x) {
                    const float v = w.v[(((size_t)so * cin + c) * kh + y) * kw + x] * sc;
                    packed[(size_t)o * kpad + (size_t)(y * kw + x) * cp + c] = f2h(v);
                    if (f32) {
                        p32[(size_t)o * k32 + (size_t)(y * kw + x) * c4 + c] = v;
                        mx = fmaxf(mx, fabsf(v));
                    }
                }
        // the row times 2^e with its largest magnitude in [0.5, 1): the split-operand kernel keeps (hi, lo) fp16 parts of every value, and lo
        // is a full-precision fp16 number only while |v| >= 2^-3; the epilogue multiplies the sums by 2^-e (both exact)
        if (f32 && mx > 0.f && std::isfinite(mx)) {
            int e = 0;
            (void)frexpf(mx, &e);          // mx = f * 2^e, f in [0.5, 1)
            const float up = ldexpf(1.f, -e);
            for (int k = 0; k < k32; ++k) p32[(size_t)o * k32 + k] *= up;
            ws[o] = ldexpf(1.f, e);
        }
    }
    TRY(m->upload(packed.data(), packed.size() * sizeof(half_t), reinterpret_cast<void**>(&out->w)));
    if (f32) {
        TRY(upload_f32(m, p32, &out->w32));
        TRY(upload_f32(m, ws, &out->wscale32));
        std::vector<half_t> hi(p32.size()), lo(p32.size());
        for (size_t i = 0; i < p32.size(); ++i) {
            hi[i] = f2h(p32[i]);
            lo[i] = f2h(p32[i] - (float)hi[i]);
        }
        TRY(m->upload(hi.data(), hi.size() * sizeof(half_t), reinterpret_cast<void**>(&out->w16hi)));
        TRY(m->upload(lo.data(), lo.size() * sizeof(half_t), reinterpret_cast<void**>(&out->w16lo)));
        if (!m->f32_range_flag) {
            const int zero = 0;
            TRY(m->upload(&zero, sizeof(int), reinterpret_cast<void**>(&m->f32_range_flag)));
        }
        out->range_flag = m->f32_range_flag;
        out->cin32 = c4;
        out->kpad32 = k32;
    }
    out->bias = nullptr;
    if (!bias.empty()) {
        std::vector<float> b(cout);
        for (int o = 0; o < cout; ++o) b[o] = bias[row_perm ? (*row_perm)[o] : o];
        TRY(upload_f32(m, b, &out->bias));
    }
    out->cin = cp;
    out->cin_real = cin;
    out->cout = cout;
    out->kh = kh;
    out->kw = kw;
    out->stride = stride;
    out->pad = pad;
    out->kpad = kpad;
    return DVID_OK;
}

// conv + FrozenBN (eps 1e-5) folded:  y = conv(x, w * s) + (beta - mean * s),  s = gamma * rsqrt(var + eps)
int make_conv_bn(dvid_model* m, const std::string& name, int stride, int pad, int cin_pad, ConvW* out) {
    NEED(w, name + ".weight");
    NEED(g, name + ".norm.weight");
    NEED(b, name + ".norm.bias");
    NEED(mu, name + ".norm.running_mean");
    NEED(var, name + ".norm.running_var");
    const int cout = (int)w->shape[0];
    std::vector<float> s(cout), bb(cout);
    for (int o = 0; o < cout; ++o) {
        s[o] = g->v[o] / sqrtf(var->v[o] + 1e-5f);
        bb[o] = b->v[o] - mu->v[o] * s[o];
    }
    return make_conv(m, *w, s, bb, stride, pad, cin_pad, nullptr, out);
}

// The 7x7 / stride-2 / pad-3 stem over 3 channels as a 4x4 / stride-1 convolution over the 2x2 space-to-depth image (16 channels:
// (dy*2 + dx)*3 + c, 4 zero): output pixel (oy, ox) reads input rows 2oy-3 .. 2oy+3 = s2d rows oy-2 .. oy+1 (pad 2 before; the row
// after is inside or beyond the image), and original tap ky lives in s2d tap ty = (ky + 1) >> 1 at sub-row dy = (ky + 1) & 1.  FrozenBN
// folded as in make_conv_bn.  K = 16 taps x 16 channels = 256 packed columns against 49 x 8 -> 448 of the NHWC8 form.
int make_stem_s2d(dvid_model* m, const std::string& name, ConvW* out) {
    NEED(w, name + ".weight");
    NEED(g, name + ".norm.weight");
    NEED(b, name + ".norm.bias");
    NEED(mu, name + ".norm.running_mean");
    NEED(var, name + ".norm.running_var");
    const int cout = (int)w->shape[0];
    if (w->shape.size() != 4 || w->shape[1] != 3 || w->shape[2] != 7 || w->shape[3] != 7) FAIL(DVID_ERR_UNSUPPORTED, "stem must be 3 -> C, 7x7");
    const int kpad = 256;
    std::vector<half_t> packed((size_t)cout * kpad, f2h(0.f));
    std::vector<float> bias(cout);
    for (int o = 0; o < cout; ++o) {
        const float sc = g->v[o] / sqrtf(var->v[o] + 1e-5f);
        bias[o] = b->v[o] - mu->v[o] * sc;
        for (int c = 0; c < 3; ++c)
            for (int ky = 0; ky < 7; ++ky)
                for (int kx = 0; kx < 7; ++kx) {
                    const int ty = (ky + 1) >> 1, dy = (ky + 1) & 1, tx = (kx + 1) >> 1, dx = (kx + 1) & 1;
                    const float v = w->v[(((size_t)o * 3 + c) * 7 + ky) * 7 + kx] * sc;
                    packed[(size_t)o * kpad + (size_t)(ty * 4 + tx) * 16 + (dy * 2 + dx) * 3 + c] = f2h(v);
                }
    }
    TRY(m->upload(packed.data(), packed.size() * sizeof(half_t), reinterpret_cast<void**>(&out->w)));
    TRY(upload_f32(m, bias, &out->bias));
    out->cin = 16;
    out->cin_real = 3;
    out->cout = cout;
    out->kh = out->kw = 4;
    out->stride = 1;
    out->pad = 2;
    out->kpad = kpad;
    out->same_size = true;
    out->alg_k = 147;
    return DVID_OK;
}

int make_linear(dvid_model* m, const std::string& name, bool has_bias, ConvW* out, const std::vector<int>* perm = nullptr,
                int row0 = 0, int rows = -1) {
    NEED(w, name + (name.find("in_proj") != std::string::npos ? "_weight" : ".weight"));
    const HostTensor* b = nullptr;
    if (has_bias) {
        const std::string bn = name + (name.find("in_proj") != std::string::npos ? "_bias" : ".bias");
        b = m->get(bn);
        if (!b) FAIL(DVID_ERR_STATE, "missing tensor '%s'", bn.c_str());
    }
    HostTensor sub;
    const HostTensor* src = w;
    std::vector<float> bias;
    if (rows >= 0) {  // row slice (in_proj q / kv parts)
        const int in = (int)w->shape[1];
        sub.shape = {rows, in};
        sub.v.assign(w->v.begin() + (size_t)row0 * in, w->v.begin() + (size_t)(row0 + rows) * in);
        src = &sub;
        if (b) bias.assign(b->v.begin() + row0, b->v.begin() + row0 + rows);
    } else if (b) {
        bias = b->v;
    }
    if (src->shape[1] % 64) FAIL(DVID_ERR_UNSUPPORTED, "linear '%s': in_features %lld not a multiple of 64", name.c_str(),
                                 (long long)src->shape[1]);
    return make_conv(m, *src, {}, bias, 1, 0, 0, perm, out);
}

int make_ln(dvid_model* m, const std::string& name, LNW* out) {
    NEED(g, name + ".weight");
    NEED(b, name + ".bias");
    out->d = (int)g->numel();
    TRY(upload_f32(m, g->v, &out->g));
    TRY(upload_f32(m, b->v, &out->b));
    return DVID_OK;
}

// [cout][kpad] (K contiguous, on the device) -> MFMA fragment order for v_mfma_f32_32x32x16_f16 with the weights as first operand:
// block (n-tile of 32 rows, K step of 16) = 64 lanes x 8 halves, lane l = row (l & 31), k = 8 (l >> 5) .. + 8 -- one contiguous
// 1-KiB wave load per fragment (csrc/headtail.hip).  Rows are zero-padded to a whole number of tiles.
int make_frags(dvid_model* m, const ConvW& w, half_t** out) {
    if (w.kh != 1 || w.kw != 1 || w.kpad % 16) FAIL(DVID_ERR_UNSUPPORTED, "fragment order needs a 1x1 layer with K %% 16 == 0");
    const int ntile = (w.cout + 31) / 32, ks_n = w.kpad / 16;
    std::vector<half_t> src((size_t)w.cout * w.kpad), dst((size_t)ntile * 32 * w.kpad, f2h(0.f));
    HIP_TRY(hipMemcpy(src.data(), w.w, src.size() * sizeof(half_t), hipMemcpyDeviceToHost));
    for (int nt = 0; nt < ntile; ++nt)
        for (int ks = 0; ks < ks_n; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int row = nt * 32 + (l & 31);
                if (row >= w.cout) continue;
                for (int e = 0; e < 8; ++e)
                    dst[(((size_t)nt * ks_n + ks) * 64 + l) * 8 + e] = src[(size_t)row * w.kpad + ks * 16 + (l >> 5) * 8 + e];
            }
    return m->upload(dst.data(), dst.size() * sizeof(half_t), reinterpret_cast<void**>(out));
}

// the same from a [cout][kpad] fp16 plane that is not a ConvW's `w` (the (hi, lo) planes of the DTYPE float32 weights)
int make_frags_plane(dvid_model* m, const half_t* plane, int cout, int kpad, half_t** out) {
    ConvW t;
    t.w = const_cast<half_t*>(plane);
    t.cout = cout;
    t.kpad = kpad;
    return make_frags(m, t, out);
}

int make_head(dvid_model* m, const std::string& pfx, bool cond, HeadW* h) {
    const dvid_config& c = m->cfg;
    const int d = c.hidden_dim, dd = c.dim_dynamic;
    h->cond = cond;
    TRY(make_linear(m, pfx + ".self_attn.in_proj", true, &h->in_proj));
    TRY(make_linear(m, pfx + ".self_attn.out_proj", true, &h->out_proj));
    // dynamic_layer rows re-ordered so that the generated parameters come out as P1T[j][c], P2T[c][j]
    // (box_head.py:695-696 views them as param1[c][j] at c*dd + j and param2[j][c] at d*dd + j*d + c)
    std::vector<int> perm(2 * d * dd);
    for (int j = 0; j < dd; ++j)
        for (int ch = 0; ch < d; ++ch) perm[j * d + ch] = ch * dd + j;
    for (int ch = 0; ch < d; ++ch)
        for (int j = 0; j < dd; ++j) perm[d * dd + ch * dd + j] = d * dd + j * d + ch;
    TRY(make_linear(m, pfx + ".inst_interact.dynamic_layer", true, &h->dynamic_layer, &perm));
    TRY(make_linear(m, pfx + ".inst_interact.out_layer", true, &h->out_layer));
    TRY(make_ln(m, pfx + ".inst_interact.norm1", &h->dc_norm1));
    TRY(make_ln(m, pfx + ".inst_interact.norm2", &h->dc_norm2));
    TRY(make_ln(m, pfx + ".inst_interact.norm3", &h->dc_norm3));
    TRY(make_linear(m, pfx + ".linear1", true, &h->linear1));
    TRY(make_linear(m, pfx + ".linear2", true, &h->linear2));
    TRY(make_ln(m, pfx + ".norm1", &h->norm1));
    TRY(make_ln(m, pfx + ".norm2", &h->norm2));
    TRY(make_ln(m, pfx + ".norm3", &h->norm3));
    h->cls.resize(c.num_cls);
    h->cls_ln.resize(c.num_cls);
    for (int i = 0; i < c.num_cls; ++i) {
        TRY(make_linear(m, pfx + ".cls_module." + std::to_string(3 * i), false, &h->cls[i]));
        TRY(make_ln(m, pfx + ".cls_module." + std::to_string(3 * i + 1), &h->cls_ln[i]));
    }
    h->reg.resize(c.num_reg);
    h->reg_ln.resize(c.num_reg);
    for (int i = 0; i < c.num_reg; ++i) {
        TRY(make_linear(m, pfx + ".reg_module." + std::to_string(3 * i), false, &h->reg[i]));
        TRY(make_ln(m, pfx + ".reg_module." + std::to_string(3 * i + 1), &h->reg_ln[i]));
    }
    TRY(make_linear(m, pfx + ".class_logits", true, &h->class_logits));
    TRY(make_linear(m, pfx + ".bboxes_delta", true, &h->bboxes_delta));
    NEED(btw, pfx + ".block_time_mlp.1.weight");
    NEED(btb, pfx + ".block_time_mlp.1.bias");
    h->bt_w = btw->v;
    h->bt_b = btb->v;
    h->bt_out = (int)btw->shape[0];
    if (h->bt_out != (cond ? d : 2 * d)) FAIL(DVID_ERR_ARG, "%s.block_time_mlp.1: unexpected out dim %d", pfx.c_str(), h->bt_out);
    if (cond) TRY(make_linear(m, pfx + ".c_mlp.1", true, &h->c_mlp));
    if (dvid_head_tail_supported(d, c.dim_feedforward, c.num_cls, c.num_reg, c.num_classes)) {
        TRY(make_frags(m, h->linear1, &h->frag.w1));
        TRY(make_frags(m, h->linear2, &h->frag.w2));
        if (cond) TRY(make_frags(m, h->c_mlp, &h->frag.wc));
        for (int i = 0; i < c.num_cls; ++i) TRY(make_frags(m, h->cls[i], &h->frag.cls[i]));
        for (int i = 0; i < c.num_reg; ++i) TRY(make_frags(m, h->reg[i], &h->frag.reg[i]));
        TRY(make_frags(m, h->class_logits, &h->frag.wlog));
        TRY(make_frags(m, h->bboxes_delta, &h->frag.wdel));
        h->frag.ok = true;
    }
    return DVID_OK;
}
// Floats per query row of the packed bias: w*w keys rounded up to a multiple of 32 (the MFMA k-step), 64 for 7x7, 160 for 12x12.
int swin_relbias_pitch(int w) { return (w * w + 31) / 32 * 32; }
static_assert(SWIN_RELBIAS_PITCH == (7 * 7 + 31) / 32 * 32 && SWIN12_RELBIAS_PITCH == (12 * 12 + 31) / 32 * 32, "the kernels' pitches");

// Relative-position bias of a w x w window as the Swin attention kernels read it: table [(2w-1)^2][nheads] (relative_position_bias_table)
// -> out [nheads][w*w][pitch], out[h][i][j] = table[index(i, j)][h] with the relative position index of swintransformer.py:122-131,
// keys w*w.. zero.  One 256-byte (7x7) or 640-byte (12x12) row per (head, query): a lane fetches the bias of its keys as aligned
// 16-byte loads.
void pack_swin_relbias(const float* table, int nheads, int w, float* out) {
    const int nt = w * w, pitch = swin_relbias_pitch(w), span = 2 * w - 1;
    std::fill(out, out + (size_t)nheads * nt * pitch, 0.f);
    for (int h = 0; h < nheads; ++h)
        for (int i = 0; i < nt; ++i)
            for (int j = 0; j < nt; ++j) {
                const int relidx = ((i / w - j / w) + w - 1) * span + ((i % w - j % w) + w - 1);
                out[((size_t)h * nt + i) * pitch + j] = table[(size_t)relidx * nheads + h];
            }
}
}  // namespace

extern "C" {
int dvid_model_set_tensor(dvid_model* m, const char* name, const float* data, const int64_t* shape, int ndim) {
    g_err[0] = 0;
    if (!m || !name || !data || ndim < 0 || ndim > 8) FAIL(DVID_ERR_ARG, "bad argument");
    if (m->finalized) FAIL(DVID_ERR_STATE, "model already finalized");
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    t.v.assign(data, data + t.numel());
    m->raw[name] = std::move(t);
    return DVID_OK;
}

int dvid_model_finalize(dvid_model* m) {
    g_err[0] = 0;
    if (!m) FAIL(DVID_ERR_ARG, "null model");
    if (m->finalized) return DVID_OK;
    const dvid_config& c = m->cfg;
    m->has_backbone = c.backbone_type == 1 ? c.swin_depths[0] > 0 : c.res_blocks[0] > 0;
    // the p2 level: present when its lateral is (as the attention stages below); the rest of the level's tensors are then needed
    const int fpn_levels = m->get("backbone.fpn_lateral2.weight") ? 4 : 3;
    if (m->has_backbone && c.backbone_type == 0) {
        const std::string bu = "backbone.bottom_up.";
        TRY(make_conv_bn(m, bu + "stem.conv1", 2, 3, 8, &m->stem));
        TRY(make_stem_s2d(m, bu + "stem.conv1", &m->stem_s2d));
        for (int s = 0; s < 4; ++s) {
            m->blocks[s].resize(c.res_blocks[s]);
            for (int b = 0; b < c.res_blocks[s]; ++b) {
                const std::string p = bu + "res" + std::to_string(s + 2) + "." + std::to_string(b);
                Block& blk = m->blocks[s][b];
                const int stride = (b == 0 && s > 0) ? 2 : 1;  // STRIDE_IN_1X1: False -> stride on the 3x3
                TRY(make_conv_bn(m, p + ".conv1", 1, 0, 0, &blk.c1));
                TRY(make_conv_bn(m, p + ".conv2", stride, 1, 0, &blk.c2));
                TRY(make_conv_bn(m, p + ".conv3", 1, 0, 0, &blk.c3));
                blk.has_sc = (b == 0);
                if (blk.has_sc) TRY(make_conv_bn(m, p + ".shortcut", stride, 0, 0, &blk.sc));
            }
        }
    }
    if (m->has_backbone && c.backbone_type == 1) {
        if (c.swin_window != 7 && c.swin_window != 12) FAIL(DVID_ERR_UNSUPPORTED, "Swin window size %d (7 and 12 are built)", c.swin_window);
        const int ws = c.swin_window, span = 2 * ws - 1;
        const std::string bu = "backbone.bottom_up.";
        {
            NEED(pw, bu + "patch_embed.proj.weight");
            NEED(pb, bu + "patch_embed.proj.bias");
            if (pw->shape[2] != 4 || pw->shape[3] != 4) FAIL(DVID_ERR_UNSUPPORTED, "patch size must be 4");
            TRY(make_conv(m, *pw, {}, pb->v, 4, 0, 8, nullptr, &m->swin_patch));
            TRY(make_ln(m, bu + "patch_embed.norm", &m->swin_patch_norm));
        }
        for (int st = 0; st < 4; ++st) {
            SwinStageW& S = m->swin[st];
            S.dim = c.swin_embed_dim << st;
            S.heads = c.swin_heads[st];
            if (S.dim != S.heads * 32) FAIL(DVID_ERR_UNSUPPORTED, "Swin stage %d: head dim %d != 32", st, S.dim / S.heads);
            S.blocks.resize(c.swin_depths[st]);
            for (int b = 0; b < c.swin_depths[st]; ++b) {
                const std::string p = bu + "layers." + std::to_string(st) + ".blocks." + std::to_string(b);
                SwinBlockW& B = S.blocks[b];
                TRY(make_ln(m, p + ".norm1", &B.norm1));
                TRY(make_ln(m, p + ".norm2", &B.norm2));
                TRY(make_linear(m, p + ".attn.qkv", true, &B.qkv));
                TRY(make_linear(m, p + ".attn.proj", true, &B.proj));
                TRY(make_linear(m, p + ".mlp.fc1", true, &B.fc1));
                TRY(make_linear(m, p + ".mlp.fc2", true, &B.fc2));
                NEED(qb, p + ".attn.qkv.bias");
                std::vector<half_t> qb16(qb->v.size());
                for (size_t i = 0; i < qb16.size(); ++i) qb16[i] = f2h(qb->v[i]);
                TRY(m->upload(qb16.data(), qb16.size() * sizeof(half_t), reinterpret_cast<void**>(&B.qkv_bias16)));
                NEED(tb, p + ".attn.relative_position_bias_table");
                if (tb->shape[0] != span * span || tb->shape[1] != S.heads) FAIL(DVID_ERR_ARG, "%s: bad bias table shape", p.c_str());
                std::vector<float> rb((size_t)S.heads * ws * ws * swin_relbias_pitch(ws));
                pack_swin_relbias(tb->v.data(), S.heads, ws, rb.data());
                TRY(upload_f32(m, rb, &B.relbias));
            }
            S.has_down = st < 3;
            if (S.has_down) {
                const std::string p = bu + "layers." + std::to_string(st) + ".downsample";
                TRY(make_ln(m, p + ".norm", &S.down_norm));
                TRY(make_linear(m, p + ".reduction", false, &S.down_red));
            }
            S.has_out = st >= 1 || fpn_levels == 4;          // out_indices (1, 2, 3), or (0, 1, 2, 3) with the p2 level
            if (S.has_out) TRY(make_ln(m, bu + "norm" + std::to_string(st), &S.out_norm));
        }
    }
    if (m->has_backbone) {
        m->fpn_levels = fpn_levels;
        for (int l = 4 - fpn_levels; l < 4; ++l) {
            const std::string lat = "backbone.fpn_lateral" + std::to_string(l + 2);
            const std::string outn = "backbone.fpn_output" + std::to_string(l + 2);
            NEED(lw, lat + ".weight");
            NEED(lb, lat + ".bias");
            NEED(ow, outn + ".weight");
            NEED(ob, outn + ".bias");
            TRY(make_conv(m, *lw, {}, lb->v, 1, 0, 0, nullptr, &m->lateral[l]));
            TRY(make_conv(m, *ow, {}, ob->v, 1, 1, 0, nullptr, &m->output[l]));
        }
    }
    m->heads.resize(c.num_heads);
    for (int i = 0; i < c.num_heads; ++i) TRY(make_head(m, "head.head_series." + std::to_string(i), false, &m->heads[i]));
    m->heads_cond.resize(c.num_heads_cond);
    for (int i = 0; i < c.num_heads_cond; ++i)
        TRY(make_head(m, "head.head_series_cond." + std::to_string(i), true, &m->heads_cond[i]));
    if (m->get("head.global_attention.0.0.in_proj_weight")) {
        const int d = c.hidden_dim;
        TRY(make_linear(m, "head.global_attention.0.0.in_proj", true, &m->gq, nullptr, 0, d));
        TRY(make_linear(m, "head.global_attention.0.0.in_proj", true, &m->gkv, nullptr, d, 2 * d));
        TRY(make_linear(m, "head.global_attention.0.0.out_proj", true, &m->gout));
    }
    // local box-level attention: present when its tensors are (as the global stage above); box_head.py:360-363 overwrites attn_ on every
    // stage without touching the query, so the last stage alone is computed and earlier stages' tensors are accepted and ignored
    {
        int ns = 0;
        while (m->get("head.local_attention." + std::to_string(ns) + ".0.in_proj_weight")) ++ns;
        if (ns > 2)
            FAIL(DVID_ERR_UNSUPPORTED, "%d local attention stages: the reference holds two local memories (box_head.py:338, :362), STAGE > 2 is an error there", ns);
        if (ns > 0) {
            const int d = c.hidden_dim;
            if (d != 256 || c.nheads * 32 != d) FAIL(DVID_ERR_UNSUPPORTED, "local attention is built for hidden_dim 256 / head dim 32");
            const std::string p = "head.local_attention." + std::to_string(ns - 1);
            TRY(make_linear(m, p + ".0.in_proj", true, &m->lq, nullptr, 0, d));
            TRY(make_linear(m, p + ".0.in_proj", true, &m->lkv, nullptr, d, 2 * d));
            TRY(make_linear(m, p + ".0.out_proj", true, &m->lout));
            TRY(make_ln(m, p + ".2", &m->lln));
            if (m->lout.cout != d || m->lout.kpad != d || m->lln.d != d || !m->lout.bias) FAIL(DVID_ERR_ARG, "%s: unexpected out_proj / LayerNorm shape", p.c_str());
            TRY(make_frags(m, m->lout, &m->lout_f));
            if (m->precision == 1) {
                if (m->lout.kpad32 != d) FAIL(DVID_ERR_ARG, "%s: unexpected out_proj packing", p.c_str());
                TRY(make_frags_plane(m, m->lout.w16hi, d, d, &m->lout_fhi));
                TRY(make_frags_plane(m, m->lout.w16lo, d, d, &m->lout_flo));
            }
        }
        m->local_stages = ns;
    }
    {
        NEED(w1, "head.time_mlp.1.weight");
        NEED(b1, "head.time_mlp.1.bias");
        NEED(w3, "head.time_mlp.3.weight");
        NEED(b3, "head.time_mlp.3.bias");
        m->tm1_w = w1->v;
        m->tm1_b = b1->v;
        m->tm3_w = w3->v;
        m->tm3_b = b3->v;
    }
    m->raw.clear();
    m->finalized = true;
    return DVID_OK;
}

int dvid_swin_pack_relbias(const float* table, int nheads, float* out) {
    return dvid_swin_pack_relbias_ws(table, nheads, 7, out);
}
int dvid_swin_pack_relbias_ws(const float* table, int nheads, int window, float* out) {
    g_err[0] = 0;
    if (!table || !out || nheads <= 0) FAIL(DVID_ERR_ARG, "swin relative-position bias: null pointer or %d heads", nheads);
    if (window != 7 && window != 12) FAIL(DVID_ERR_UNSUPPORTED, "swin relative-position bias: window size %d (7 and 12 are built)", window);
    pack_swin_relbias(table, nheads, window, out);
    return DVID_OK;
}
}  // extern "C"
