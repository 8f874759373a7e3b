// Internal header of the libdvid_hip host runtime: what two or more of model.hip, weights.hip, backbone.hip, head.hip, ops_abi.hip and
// profile.hip share -- the error buffer and its macros, the weight structs and `struct dvid_model`, the profiling bracket, the layer
// launchers (conv_run*, linear_run*) and the RoI level table.  The kernels' own launchers are declared in kernels.h.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/dvid_hip.h"
#include "common.h"
#include "kernels.h"
#include "options.h"

#pragma GCC visibility push(hidden)          // nothing declared here is part of the library's ABI

// ---- errors: one message buffer per host thread (defined in model.hip), cleared by every entry point and read by dvid_last_error ------
// (constant-initialised, and declared so: a use in another file is then a plain TLS access, with no call of an initialisation wrapper)
[[clang::require_constant_initialization]] extern thread_local char g_err[512];
void set_err(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
#define FAIL(code, ...)       \
    do {                      \
        set_err(__VA_ARGS__); \
        return (code);        \
    } while (0)
#define TRY(expr)                       \
    do {                                \
        int _rc = (expr);               \
        if (_rc != DVID_OK) {           \
            if (!g_err[0]) set_err("%s failed (%d) at %s:%d", #expr, _rc, __FILE__, __LINE__); \
            return _rc;                 \
        }                               \
    } while (0)
#define NEED(var, name)                                              \
    const HostTensor* var = m->get(name);                            \
    if (!var) FAIL(DVID_ERR_STATE, "missing tensor '%s'", std::string(name).c_str())

// ---------------------------------------------------------------------------------------------
// profiling of launches (bench.py roofline): events recorded on the launch stream.  The records, their event pool and the lock
// are private to profile.hip; with profiling off a launch costs one test of g_prof_on.
// ---------------------------------------------------------------------------------------------
struct ProfRec {
    hipEvent_t a, b;
    double flop, bytes;
    int M, N, K, taps, stride, res_mode;
    const char* kind;      // kernel family the launch ran on (dump / bench.py's top_kernels)
    bool family;           // counts towards the implicit-GEMM family's sums (dvid_profile_read); the other records are the heads' and the
                           // backbone's non-GEMM kernels, timed for the per-kernel table only
};
extern bool g_prof_on;                           // dvid_profile_enable
int prof_begin(ProfRec* r, hipStream_t s);       // gives `r` a pair of events (pooled) and records the first on `s`
int prof_end(const ProfRec& r, hipStream_t s);   // records the second and keeps the record
// THE event bracket: every profiled launch fills a ProfRec and goes through here
template <typename F>
int prof_bracket(ProfRec& r, hipStream_t s, F&& launch) {
    if (prof_begin(&r, s) != DVID_OK) return DVID_ERR_HIP;
    const int rc = launch();
    if (prof_end(r, s) != DVID_OK) return DVID_ERR_HIP;
    return rc;
}

// A launch outside the implicit-GEMM family (RoIAlign, DynamicConv, attention, the head tail, max pool) as a record of the per-kernel
// table: `rows` units, algorithmic FLOP and bytes of the whole launch.  Not part of the family's sums unless `family`.
template <typename F>
int prof_other(const char* kind, long rows, int n, int k, double flop, double bytes, hipStream_t s, F&& launch, bool family = false) {
    if (!g_prof_on) return launch();
    ProfRec r{.flop = flop, .bytes = bytes, .M = (int)rows, .N = n, .K = k, .taps = 0, .stride = 0, .res_mode = 0, .kind = kind, .family = family};
    return prof_bracket(r, s, launch);
}

// the implicit-GEMM family's launches with their records (profile.hip)
int igemm(const IgemmParams& p, hipStream_t s);
int bneck_tail(const half_t* t1, const half_t* w2, const float* b2, const half_t* w3, const float* b3, const half_t* res, const half_t* ws,
               const float* bs, const half_t* w1n, const float* b1n, int n_next, half_t* out, half_t* t1n, int n, int H, int W, hipStream_t s);
int bneck128_tail(const half_t* t1, const half_t* w2, const float* b2, const half_t* w3, const float* b3, const half_t* res, const half_t* w1n,
                  const float* b1n, half_t* out, half_t* t1n, int n, int H, int W, hipStream_t s);

// ---------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto d : shape) n *= d;
        return n;
    }
};

// A captured launch sequence holds raw pointers into the workspace: every model counts the moves of ITS buffers (`gen`, bumped when a
// buffer that already existed is re-allocated -- a first allocation cannot have been captured), the detector compares the counter with the
// value it saw at capture time and drops its graphs when it differs (dvid_workspace_generation).  Per model: another model's growth, or
// this model's first allocations, no longer throw this model's graphs away.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;          // one owner per allocation: a buffer frees itself where its owner dies (dvid_model_destroy)
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {          // std::vector<DevBuf> growing (ss_slabs)
        o.p = nullptr;
        o.bytes = 0;
    }
    ~DevBuf() { release(); }
    int ensure(size_t n, std::atomic<unsigned long long>* gen = nullptr) {
        if (n <= bytes) return DVID_OK;
        if (gen && p) gen->fetch_add(1, std::memory_order_relaxed);
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        bytes = 0;
        HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        // DVID_POISON_WORKSPACE=1 (diagnostics): fresh workspace starts as 0xFF bytes (NaN as fp16 / fp32), so a kernel that reads
        // workspace nothing has written shows up in the results instead of depending on what the allocation held before
        static const bool poison = getenv("DVID_POISON_WORKSPACE") && atoi(getenv("DVID_POISON_WORKSPACE")) != 0;
        if (poison) HIP_TRY(hipMemset(p, 0xFF, n));
        return DVID_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// A memory the head attends to, as the library keeps it between calls: the K | V rows of `groups` memories of `lk` rows each, projected by
// one linear over all groups * lk rows (head.hip: kv_project), and the shape they were projected for.  The callers ask for `kv` with 64
// rows more than they project in the grouped forms and with none in the single one; why is unexplained: mha_mfma_kernel clamps its K
// rows to lk - 1 and reads V through the padded transpose in `vt`, f32_mha_kernel stages only the rows below lk (attention.hip), so
// neither reads a row behind the last group's.
struct KvMemory {
    DevBuf kv;           // K | V rows, [groups * lk, 2 d], fp16 or fp32 as the model's precision says
    DevBuf src16;        // fp16 copy of the source rows (precision 0 only)
    int lk = 0, groups = 0;          // shape of what `kv` holds (0: nothing projected)
};

struct ConvW {   // conv or linear weights in MFMA-operand layout
    half_t* w = nullptr;
    float* bias = nullptr;
    int cin = 0, cout = 0, kh = 1, kw = 1, stride = 1, pad = 0, kpad = 0;
    int cin_real = 0;  // un-padded input channels (algorithmic FLOP count)
    bool same_size = false;    // output spatial size = input size whatever (kh, pad) say (the space-to-depth stem: pad 2 before, 1 after)
    int alg_k = 0;             // algorithmic K for the FLOP count when the packed layout carries structural zeros (0: kh*kw*cin_real)
    // DTYPE float32 (csrc/f32.hip): the same rows un-rounded, [cout][kpad32] fp32 with k = (ky*kw + kx)*cin32 + c, cin32 = cin rounded up to 4
    float* w32 = nullptr;
    int* range_flag = nullptr;          // the model's f32_range_flag (null for stand-alone launches)
    half_t *w16hi = nullptr, *w16lo = nullptr;          // the scaled rows as fp16 (hi, lo) planes for the split-operand kernel (csrc/f32.hip)
    float* wscale32 = nullptr;          // [cout]: 2^-e of the power-of-two scaling that puts each packed row's largest magnitude in [0.5, 1) (exact; undone in the epilogue)
    int cin32 = 0, kpad32 = 0;
};
// fragment-order copies of the head-tail weights (csrc/headtail.hip)
struct HeadFrags {
    half_t *w1 = nullptr, *w2 = nullptr, *wc = nullptr, *wlog = nullptr, *wdel = nullptr;
    half_t* cls[4] = {nullptr, nullptr, nullptr, nullptr};
    half_t* reg[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = false;
};
struct LNW {
    float* g = nullptr;
    float* b = nullptr;
    int d = 0;
};
struct HeadW {
    ConvW in_proj, out_proj, dynamic_layer, out_layer, linear1, linear2, class_logits, bboxes_delta, c_mlp;
    std::vector<ConvW> cls, reg;
    std::vector<LNW> cls_ln, reg_ln;
    LNW norm1, norm2, norm3, dc_norm1, dc_norm2, dc_norm3;
    // host copies for the time conditioning (block_time_mlp.1)
    std::vector<float> bt_w, bt_b;
    int bt_out = 0;
    bool cond = false;
    HeadFrags frag;
};
struct Block {
    ConvW c1, c2, c3, sc;
    bool has_sc = false;
};
struct SwinBlockW {
    LNW norm1, norm2;
    ConvW qkv, proj, fc1, fc2;
    half_t* qkv_bias16 = nullptr;   // q/k/v of a padded window position = the qkv bias
    float* relbias = nullptr;       // [heads][w*w][swin_relbias_pitch(w)] relative-position bias, gathered from the table at load
};
struct SwinStageW {
    std::vector<SwinBlockW> blocks;
    int dim = 0, heads = 0;
    bool has_down = false, has_out = false;
    LNW down_norm, out_norm;
    ConvW down_red;
};

struct dvid_model {
    dvid_config cfg;
    std::map<std::string, HostTensor> raw;
    bool finalized = false;
    std::atomic<unsigned long long> ws_gen{0};          // moves of this model's workspace buffers (DevBuf::ensure)
    int* f32_range_flag = nullptr;                      // DTYPE float32, split operands: set by a kernel that met |activation| > 65504 (dvid_model_take_range_flag)
    int precision = 0;         // 0: fp16 storage / fp16 MFMA (DTYPE float16), 1: fp32 storage / fp32 MFMA (DTYPE float32); dvid_model_set_precision
    std::vector<void*> owned;  // device allocations of weights

    // backbone
    bool has_backbone = false;
    ConvW stem, stem_s2d;      // NHWC8 7x7/2 form and the 2x2 space-to-depth 4x4/1 form of the same layer
    bool use_s2d = true;       // dvid_set_stem_layout(m, 0): the NHWC8 form
    std::vector<Block> blocks[4];
    int fpn_levels = 3;           // 3: p3..p5; 4: p2..p5 (backbone.fpn_lateral2.weight was set, dvid_model_finalize)
    ConvW lateral[4], output[4];  // index 0 -> level 2 (used when fpn_levels == 4), 1..3 -> levels 3..5
    // Swin backbone (backbone_type 1)
    ConvW swin_patch;
    LNW swin_patch_norm;
    SwinStageW swin[4];
    // head
    std::vector<HeadW> heads;       // head_series
    std::vector<HeadW> heads_cond;  // head_series_cond
    ConvW gq, gkv, gout;            // global attention projections
    // local box-level attention (head.local_attention.{i}.*, box_head.py:186-194): only the LAST stage is ever observable (:360-363), so only
    // its tensors are packed; local_stages = number of stages present (0: the model has none)
    int local_stages = 0;
    ConvW lq, lkv, lout;
    LNW lln;
    half_t *lout_f = nullptr, *lout_fhi = nullptr, *lout_flo = nullptr;          // out_proj in fragment order: fp16 rows / the (hi, lo) planes (DTYPE float32)
    std::vector<float> tm1_w, tm1_b, tm3_w, tm3_b;  // time_mlp host copies
    std::map<int64_t, std::vector<float>> time_cache;  // t -> time_mlp(t) [4*hidden]

    // workspace
    int ws_frames = 0, ws_h = 0, ws_w = 0, ws_boxes = 0;
    DevBuf img8, bufX, bufY, bufT1, bufT2, bufSC, c2, c3, c4, c5, lat[4];          // c2, lat[0]: models with the p2 level only
    DevBuf sw_x, sw_x2, sw_ln16, sw_qkv16, sw_attn16, sw_h16;   // Swin token buffers
    DevBuf roi, params, dyn, qkv, attn16, f32a, f32b, f32c, f32d, h16a, h16b, hid16, ss, deltas, splitk, vt;
    // (head slot, t) -> device scale/shift row [bt_out], sub-allocated from slabs of kSsSlabRows rows (a sampler that walks all
    // 1000 time steps on 4 head slots ends at 16 allocations of 512 KB, not 4000 of 2 KB; rows live until the model is destroyed)
    std::map<std::pair<int, int64_t>, float*> ss_rows;
    std::vector<DevBuf> ss_slabs;
    size_t ss_slab_used = 0;          // rows taken from the last slab

    KvMemory vmem;          // the global memory a video holds between its calls
    KvMemory gmem;          // `groups` GLOBAL memories, one per live stream: beside vmem, never in it
    KvMemory lmem;          // the local memories of the one observable local stage

    // sub-batch chains (backbone.hip: run_chains)
    int nchain = 2;
    hipStream_t cs[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    bool streams_ready = false;
    int ensure_streams() {
        if (streams_ready) return DVID_OK;
        for (int c = 0; c < 4; ++c) {
            HIP_TRY(hipStreamCreateWithFlags(&cs[c], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ev_join[c], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        streams_ready = true;
        return DVID_OK;
    }

    int upload(const void* host, size_t bytes, void** dev) {
        HIP_TRY(hipMalloc(dev, bytes));
        owned.push_back(*dev);
        HIP_TRY(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
        return DVID_OK;
    }
    const HostTensor* get(const std::string& name) const {
        auto it = raw.find(name);
        return it == raw.end() ? nullptr : &it->second;
    }
};

// ---- layer launchers (model.hip) ---------------------------------------------------------------
// What a call site does not name keeps its default: {.relu = 1}, {.out_f32 = 1, .res = x, .res_mode = 1, .res_f32 = 1}, ...
struct ConvOpts {
    int relu = 0;                  // 0 none, 1 ReLU, 2 exact GELU
    int out_f32 = 0;               // fp32 output rows
    const void* res = nullptr;     // residual, see res_mode (fp32 if res_f32)
    int res_mode = 0;              // 0 none, 1 same shape, 2 nearest-x2 upsample
    int res_f32 = 0;
    int* ho_out = nullptr;         // receive the output size
    int* wo_out = nullptr;
    int ldc = 0;                   // output row pitch (0: cout)
    int splitk = 1;                // > 1: fp32 partial slabs; bias / activation are applied by the consumer
    bool pooled = false;           // the space-to-depth stem with its max pool in the same launch
};
int conv_run(const ConvW& w, const half_t* in, int n, int h, int wd, void* out, hipStream_t s, const ConvOpts& o = {});
// Linear on [rows, in] fp16
int linear_run(const ConvW& w, const half_t* in, int rows, void* out, int relu, int out_f32, hipStream_t s);
// DTYPE float32: the same layers on the fp32 kernels (csrc/f32.hip and the f32_* kernels beside each fp16 one; fp32 NHWC activations, un-rounded weights)
struct ConvOpts32 {
    int relu = 0;
    const float* res = nullptr;
    int res_mode = 0;
    int* ho_out = nullptr;
    int* wo_out = nullptr;
    int ldc = 0;
};
int conv_run32(const ConvW& w, const float* in, int n, int h, int wd, float* out, hipStream_t s, const ConvOpts32& o = {});
int linear_run32(const ConvW& w, const float* in, int rows, float* out, int relu, hipStream_t s, int ldc = 0);

// The FPN levels of a `height` x `width` image as RoIAlign reads them (detectron2 ROIPooler as built at box_head.py:250-271), finest
// first and ending at p5: n_levels 3 = p3..p5 (strides 8 / 16 / 32), 4 = p2..p5 (strides 4 .. 32); starting at frame `frame_offset` of
// each [n, h, w, channels] map.  The callers have checked n_levels (pyramid_ok).
template <typename T>
RoiLevelsT<T> roi_levels(const void* const* levels, int n_levels, int height, int width, size_t frame_offset, int channels) {
    RoiLevelsT<T> lv = {};
    lv.n_levels = n_levels;
    lv.min_level = 6 - n_levels;
    for (int l = 0; l < n_levels; ++l) {
        const int stride = 4 << (lv.min_level - 2 + l);
        lv.h[l] = height / stride;
        lv.w[l] = width / stride;
        lv.feat[l] = reinterpret_cast<const T*>(levels[l]) + frame_offset * lv.h[l] * lv.w[l] * channels;
        lv.scale[l] = 1.f / (float)stride;
    }
    return lv;
}
inline bool pyramid_ok(const void* const* levels, int n_levels) {
    if (!levels || (n_levels != 3 && n_levels != 4)) return false;
    for (int l = 0; l < n_levels; ++l)
        if (!levels[l]) return false;
    return true;
}

#pragma GCC visibility pop
