// libdvid_hip runtime core: the single definitions of the option table and the error buffer, the layer launchers every stage is built
// from (conv_run*, linear_run*), model create / destroy / precision, the option entry points and the workspace.  Weight ingest is
// weights.hip, the stages are backbone.hip and head.hip, the stand-alone ops ops_abi.hip, profiling profile.hip.
// See include/dvid_hip.h for the contract of every exported symbol.
#include <stdarg.h>

#include "runtime.h"

DvidOptions g_opt;          // csrc/options.h: the library-wide option table (defaults = the benchmarked configuration)

thread_local char g_err[512] = "";
void set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int conv_run(const ConvW& w, const half_t* in, int n, int h, int wd, void* out, hipStream_t s, const ConvOpts& o) {
    IgemmParams p;
    memset(&p, 0, sizeof(p));
    p.in = in;
    p.w = w.w;
    p.bias = w.bias;
    p.res = o.res;
    p.out = out;
    p.H = h;
    p.W = wd;
    p.Cin = w.cin;
    p.KH = w.kh;
    p.KW = w.kw;
    p.stride = w.stride;
    p.pad = w.pad;
    p.Ho = w.same_size ? h : (h + 2 * w.pad - w.kh) / w.stride + 1;
    p.Wo = w.same_size ? wd : (wd + 2 * w.pad - w.kw) / w.stride + 1;
    p.Cout = w.cout;
    p.M = n * p.Ho * p.Wo;
    p.Kpad = w.kpad;
    p.ntaps = w.kh * w.kw;
    p.alg_k = w.alg_k ? w.alg_k : w.kh * w.kw * (w.cin_real ? w.cin_real : w.cin);
    p.ldc = o.ldc ? o.ldc : w.cout;
    p.relu = o.relu;
    p.out_f32 = o.out_f32;
    p.res_mode = o.res_mode;
    p.res_f32 = o.res_f32;
    if (o.splitk > 1) {               // fp32 partial slabs; bias/activation are applied by the consumer
        p.splitk = o.splitk;
        p.split_stride = (long)p.M * p.ldc;
        p.bias = nullptr;
    }
    if (o.ho_out) *o.ho_out = p.Ho;
    if (o.wo_out) *o.wo_out = p.Wo;
    if (o.pooled) {          // the space-to-depth stem with its max pool in the same launch: `out` is the pooled map; ho / wo stay the stem's
        if (!dvid_stem_pool_supported(p)) return DVID_ERR_UNSUPPORTED;
        // algorithmic bytes: the space-to-depth image in, the pooled map out, the weights
        return prof_other("stem_pool", p.M, 64, p.Kpad, 2.0 * p.M * 64.0 * p.alg_k, (double)p.M * 32.0 + (double)p.M / 4 * 128.0 + 64.0 * p.Kpad * 2.0, s,
                          [&] { return dvid_stem_pool_launch(p, s); }, /*family=*/true);          // an implicit-GEMM launch like the stem it replaces
    }
    return igemm(p, s);
}

// Linear on [rows, in] fp16
int linear_run(const ConvW& w, const half_t* in, int rows, void* out, int relu, int out_f32, hipStream_t s) {
    return conv_run(w, in, rows, 1, 1, out, s, {.relu = relu, .out_f32 = out_f32});
}

// ---- DTYPE float32: the same layers on the fp32 kernels (fp32 NHWC activations, un-rounded weights) ---------------------------------
int conv_run32(const ConvW& w, const float* in, int n, int h, int wd, float* out, hipStream_t s, const ConvOpts32& o) {
    if (!w.w32) return DVID_ERR_STATE;
    F32GemmParams p;
    memset(&p, 0, sizeof(p));
    p.in = in;
    p.w = w.w32;
    p.w_hi = w.w16hi;
    p.w_lo = w.w16lo;
    p.range_flag = w.range_flag;
    p.bias = w.bias;
    p.wscale = w.wscale32;
    p.res = o.res;
    p.out = out;
    p.H = h;
    p.W = wd;
    p.Cin = w.cin32;
    p.KH = w.kh;
    p.KW = w.kw;
    p.stride = w.stride;
    p.pad = w.pad;
    p.Ho = (h + 2 * w.pad - w.kh) / w.stride + 1;
    p.Wo = (wd + 2 * w.pad - w.kw) / w.stride + 1;
    p.Cout = w.cout;
    p.M = n * p.Ho * p.Wo;
    p.K = w.kh * w.kw * w.cin32;
    p.Kpad = w.kpad32;
    p.ldc = o.ldc ? o.ldc : w.cout;
    p.relu = o.relu;
    p.res_mode = o.res_mode;
    if (o.ho_out) *o.ho_out = p.Ho;
    if (o.wo_out) *o.wo_out = p.Wo;
    const double alg_k = (double)w.kh * w.kw * (w.cin_real ? w.cin_real : w.cin32);
    const double in_px = (double)p.M * (w.kh * w.kw > 1 ? w.stride * w.stride : 1);
    const double bytes = 4.0 * (in_px * p.Cin + (double)p.Cout * p.Kpad + (double)p.M * p.Cout * (o.res_mode == 1 ? 2.0 : o.res_mode == 2 ? 1.25 : 1.0));
    return prof_other("igemm_f32", p.M, p.Cout, p.Kpad, 2.0 * p.M * (double)p.Cout * alg_k, bytes, s, [&] { return dvid_f32_igemm_launch(p, s); },
                      /*family=*/true);
}
int linear_run32(const ConvW& w, const float* in, int rows, float* out, int relu, hipStream_t s, int ldc) {
    return conv_run32(w, in, rows, 1, 1, out, s, {.relu = relu, .ldc = ldc});
}

extern "C" {
const char* dvid_last_error(void) { return g_err; }
int dvid_version(void) { return 16; }

int dvid_model_create(const dvid_config* cfg, dvid_model** out) {
    g_err[0] = 0;
    if (!cfg || !out) FAIL(DVID_ERR_ARG, "null argument");
    if (cfg->hidden_dim != 256 || cfg->nheads != 8 || cfg->dim_dynamic != 64 || cfg->pooler_resolution != 7 ||
        cfg->sampling_ratio != 2)
        FAIL(DVID_ERR_UNSUPPORTED,
             "kernels are specialised for HIDDEN_DIM 256, NHEADS 8, DIM_DYNAMIC 64, POOLER_RESOLUTION 7, SAMPLING_RATIO 2");
    if (cfg->dim_feedforward % 64) FAIL(DVID_ERR_UNSUPPORTED, "DIM_FEEDFORWARD must be a multiple of 64");
    if (cfg->num_classes < 1 || cfg->num_classes > DVID_MAX_CLASSES)
        FAIL(DVID_ERR_UNSUPPORTED, "NUM_CLASSES %d: 1 <= NUM_CLASSES <= DVID_MAX_CLASSES = %d", cfg->num_classes, DVID_MAX_CLASSES);
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) FAIL(DVID_ERR_HIP, "no HIP device available");
    dvid_model* m = new dvid_model();
    m->cfg = *cfg;
    if (const char* e = getenv("DVID_CHAINS")) m->nchain = atoi(e) < 1 ? 1 : (atoi(e) > 4 ? 4 : atoi(e));
    *out = m;
    return DVID_OK;
}

int dvid_model_destroy(dvid_model* m) {
    if (!m) return DVID_OK;
    for (void* p : m->owned) (void)hipFree(p);
    delete m;          // every workspace buffer is a DevBuf member and frees itself here
    return DVID_OK;
}

int dvid_model_set_precision(dvid_model* m, int precision) {
    g_err[0] = 0;
    if (!m || (precision != 0 && precision != 1)) FAIL(DVID_ERR_ARG, "precision must be 0 (float16) or 1 (float32)");
    if (m->finalized) FAIL(DVID_ERR_STATE, "dvid_model_set_precision must precede dvid_model_finalize (the weights are packed for one precision)");
    m->precision = precision;
    return DVID_OK;
}

namespace {
struct OptEntry {
    const char* name;
    int DvidOptions::*field;
    int lo, hi;
};
const OptEntry kOptions[] = {
    {"conv3x3", &DvidOptions::conv3x3, 0, 2},       {"wstat", &DvidOptions::wstat, 0, 2},           {"bneck_fuse", &DvidOptions::bneck_fuse, 0, 2},
    {"stem_pool", &DvidOptions::stem_pool, 0, 1},   {"head_tail", &DvidOptions::head_tail, 0, 1},   {"roi_fuse", &DvidOptions::roi_fuse, 0, 1},   {"ln_rows", &DvidOptions::ln_rows, 0, 1},
    {"igemm_cfg", &DvidOptions::igemm_cfg, -1, 255}, {"igemm_tune", &DvidOptions::igemm_tune, -1, 1}, {"igemm_generic", &DvidOptions::igemm_generic, 0, 1},
    {"f32_split", &DvidOptions::f32_split, 0, 1},    {"f32_wstat", &DvidOptions::f32_wstat, 0, 2},    {"f32_conv3x3", &DvidOptions::f32_conv3x3, 0, 1},
    {"bneck_lds", &DvidOptions::bneck_lds, 0, 160 * 1024},
};
}  // namespace

int dvid_set_option(const char* name, int value) {
    g_err[0] = 0;
    if (!name) FAIL(DVID_ERR_ARG, "null option name");
    for (const OptEntry& e : kOptions)
        if (!strcmp(e.name, name)) {
            if (value < e.lo || value > e.hi) FAIL(DVID_ERR_ARG, "option %s: %d outside [%d, %d]", name, value, e.lo, e.hi);
            if (e.field == &DvidOptions::igemm_cfg && value >= dvid_igemm_num_configs()) FAIL(DVID_ERR_ARG, "igemm_cfg %d: the table has %d entries", value, dvid_igemm_num_configs());
            g_opt.*(e.field) = value;
            return DVID_OK;
        }
    FAIL(DVID_ERR_ARG, "unknown option '%s'", name);
}

int dvid_get_option(const char* name, int* value) {
    g_err[0] = 0;
    if (!name || !value) FAIL(DVID_ERR_ARG, "null argument");
    for (const OptEntry& e : kOptions)
        if (!strcmp(e.name, name)) {
            *value = g_opt.*(e.field);
            return DVID_OK;
        }
    FAIL(DVID_ERR_ARG, "unknown option '%s'", name);
}

int dvid_reset_options(void) {
    g_opt = DvidOptions();
    return DVID_OK;
}

// "name=value ..." of every option, then the environment switches the library still reads, as they are set
int dvid_effective_config(char* buf, int cap) {
    g_err[0] = 0;
    if (!buf || cap <= 0) FAIL(DVID_ERR_ARG, "no buffer");
    std::string out;
    for (const OptEntry& e : kOptions) out += std::string(e.name) + "=" + std::to_string(g_opt.*(e.field)) + " ";
    for (const char* env : {"DVID_IGEMM_TUNE", "DVID_IGEMM_TUNE_CACHE", "DVID_CHAINS", "DVID_POISON_WORKSPACE"}) {
        const char* v = getenv(env);
        out += std::string(env) + "=" + (v ? v : "") + " ";
    }
    if (!out.empty()) out.pop_back();
    if ((int)out.size() + 1 > cap) FAIL(DVID_ERR_ARG, "buffer of %d bytes, need %d", cap, (int)out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return DVID_OK;
}

// DTYPE float32 with split operands: 1 if any launch since the last call staged an activation whose magnitude exceeds the fp16 range (its
// products are then inf / NaN where fp32 arithmetic would be finite); reads 4 bytes from the device behind `stream` and clears the flag
int dvid_model_take_range_flag(dvid_model* m, int* exceeded, void* stream) {
    g_err[0] = 0;
    if (!m || !exceeded) FAIL(DVID_ERR_ARG, "null argument");
    *exceeded = 0;
    if (!m->f32_range_flag) return DVID_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(exceeded, m->f32_range_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*exceeded) HIP_TRY(hipMemsetAsync(m->f32_range_flag, 0, sizeof(int), s));
    return DVID_OK;
}

int dvid_set_stem_pool(int mode) {
    if (mode < -1 || mode > 1) return DVID_ERR_ARG;
    g_opt.stem_pool = mode < 0 ? DvidOptions().stem_pool : mode;
    return DVID_OK;
}

unsigned long long dvid_workspace_generation(const dvid_model* m) { return m ? m->ws_gen.load(std::memory_order_relaxed) : 0ull; }

int dvid_set_chains(dvid_model* m, int nchain) {
    g_err[0] = 0;
    if (!m || nchain < 1 || nchain > 4) FAIL(DVID_ERR_ARG, "nchain must be 1..4");
    m->nchain = nchain;
    return DVID_OK;
}

int dvid_set_stem_layout(dvid_model* m, int space_to_depth) {
    g_err[0] = 0;
    if (!m) FAIL(DVID_ERR_ARG, "null model");
    m->use_s2d = space_to_depth != 0;
    return DVID_OK;
}

int dvid_workspace_reserve(dvid_model* m, int max_frames, int height, int width, int boxes_per_frame) {
    g_err[0] = 0;
    if (!m || max_frames <= 0 || boxes_per_frame <= 0) FAIL(DVID_ERR_ARG, "bad argument");
    if (height % 32 || width % 32) FAIL(DVID_ERR_ARG, "height/width must be multiples of 32 (got %dx%d)", height, width);
    const size_t n = ((size_t)max_frames + 3) / 4 * 4;      // room for up to 4 equal sub-batch chains
    const size_t px4 = (size_t)(height / 4) * (width / 4);
    const size_t es = m->precision == 1 ? 2 : 1;            // DTYPE float32: every fp16 buffer below holds fp32 values instead
    if (m->has_backbone && m->cfg.backbone_type == 1) {
        const size_t C0 = m->cfg.swin_embed_dim, M0 = n * px4;      // stage-0 tokens; M*C halves per stage
        TRY(m->img8.ensure(n * height * width * 8 * 2, &m->ws_gen));
        TRY(m->sw_x.ensure(M0 * C0 * 4, &m->ws_gen));
        TRY(m->sw_x2.ensure(M0 * C0 * 4 / 2, &m->ws_gen));
        TRY(m->sw_ln16.ensure(M0 * C0 * 2 * es, &m->ws_gen));
        TRY(m->sw_qkv16.ensure(M0 * C0 * 3 * 2 * es, &m->ws_gen));
        TRY(m->sw_attn16.ensure(M0 * C0 * 2 * es, &m->ws_gen));
        TRY(m->sw_h16.ensure(M0 * C0 * 4 * 2 * es, &m->ws_gen));
        TRY(m->c3.ensure(n * (px4 / 4) * (C0 * 2) * 2 * es, &m->ws_gen));
        TRY(m->c4.ensure(n * (px4 / 16) * (C0 * 4) * 2 * es, &m->ws_gen));
        TRY(m->c5.ensure(n * (px4 / 64) * (C0 * 8) * 2 * es, &m->ws_gen));
        for (int l = 1; l < 4; ++l) TRY(m->lat[l].ensure(n * (px4 >> (2 * l)) * 256 * 2 * es, &m->ws_gen));
        if (m->fpn_levels == 4) {          // stage 0's normed output and the stride-4 lateral
            TRY(m->c2.ensure(M0 * C0 * 2 * es, &m->ws_gen));
            TRY(m->lat[0].ensure(n * px4 * 256 * 2 * es, &m->ws_gen));
        }
    }
    if (m->has_backbone && m->cfg.backbone_type == 0) {
        TRY(m->img8.ensure(n * height * width * 8 * 2, &m->ws_gen));          // (fp32: NHWC4 = the same bytes)
        const size_t big = n * px4 * 256 * 2 * es;  // largest activation: res2 output (also >= stem output)
        TRY(m->bufX.ensure(big, &m->ws_gen));
        TRY(m->bufY.ensure(big, &m->ws_gen));
        TRY(m->bufT1.ensure(big, &m->ws_gen));
        TRY(m->bufT2.ensure(big, &m->ws_gen));
        TRY(m->bufSC.ensure(big, &m->ws_gen));
        TRY(m->c3.ensure(n * (px4 / 4) * 512 * 2 * es, &m->ws_gen));
        TRY(m->c4.ensure(n * (px4 / 16) * 1024 * 2 * es, &m->ws_gen));
        TRY(m->c5.ensure(n * (px4 / 64) * 2048 * 2 * es, &m->ws_gen));
        for (int l = 1; l < 4; ++l) TRY(m->lat[l].ensure(n * (px4 >> (2 * l)) * 256 * 2 * es, &m->ws_gen));
        if (m->fpn_levels == 4) {          // res2's output persists for the FPN, and the stride-4 lateral
            TRY(m->c2.ensure(big, &m->ws_gen));
            TRY(m->lat[0].ensure(big, &m->ws_gen));
        }
    }
    const size_t R = n * boxes_per_frame;
    const int d = m->cfg.hidden_dim;
    TRY(m->roi.ensure(R * 49 * d * 2 * es, &m->ws_gen));
    TRY(m->dyn.ensure(R * 49 * d * 2 * es, &m->ws_gen));
    TRY(m->params.ensure(R * 2 * d * m->cfg.dim_dynamic * 2 * es, &m->ws_gen));
    TRY(m->qkv.ensure(R * 3 * d * 4, &m->ws_gen));
    TRY(m->attn16.ensure(R * d * 2 * es, &m->ws_gen));
    TRY(m->f32a.ensure(R * d * 4, &m->ws_gen));
    TRY(m->f32b.ensure(R * d * 4, &m->ws_gen));
    TRY(m->f32c.ensure(R * d * 4, &m->ws_gen));
    TRY(m->f32d.ensure(R * d * 4, &m->ws_gen));
    TRY(m->h16a.ensure(R * d * 2 * es, &m->ws_gen));
    TRY(m->h16b.ensure(R * d * 2 * es, &m->ws_gen));
    TRY(m->hid16.ensure(R * m->cfg.dim_feedforward * 2 * es, &m->ws_gen));
    TRY(m->ss.ensure((size_t)(m->cfg.num_heads + m->cfg.num_heads_cond) * n * 2 * d * 4, &m->ws_gen));
    TRY(m->deltas.ensure(R * 4 * 4, &m->ws_gen));
    TRY(m->splitk.ensure(R * d * 4 * 8, &m->ws_gen));          // up to 8 split-K slabs of an [R, d] fp32 output
    TRY(m->vt.ensure((size_t)n * m->cfg.nheads * 32 * (((size_t)boxes_per_frame + 31) / 32 * 32 + 32) * 2, &m->ws_gen));
    m->ws_frames = max_frames;
    m->ws_h = height;
    m->ws_w = width;
    m->ws_boxes = boxes_per_frame;
    return DVID_OK;
}
}  // extern "C"
