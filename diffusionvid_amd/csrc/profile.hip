// libdvid_hip profiling: the launch records and their event pool, the event bracket every profiled launch goes through (runtime.h), the
// records of the implicit-GEMM family's launches, and the dvid_profile_* entry points (include/dvid_hip.h) bench.py reads them with.
#include <mutex>

#include "runtime.h"

bool g_prof_on = false;

namespace {
std::mutex g_prof_mu;                 // models on different host threads may launch concurrently
std::vector<ProfRec> g_prof;
std::vector<ProfRec> g_prof_pool;     // the events of records dvid_profile_reset dropped

int prof_take(ProfRec* r) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof_pool.empty()) {
        r->a = g_prof_pool.back().a;
        r->b = g_prof_pool.back().b;
        g_prof_pool.pop_back();
        return DVID_OK;
    }
    HIP_TRY(hipEventCreate(&r->a));
    HIP_TRY(hipEventCreate(&r->b));
    return DVID_OK;
}
}  // namespace

int prof_begin(ProfRec* r, hipStream_t s) {
    if (prof_take(r) != DVID_OK) return DVID_ERR_HIP;
    HIP_TRY(hipEventRecord(r->a, s));
    return DVID_OK;
}
int prof_end(const ProfRec& r, hipStream_t s) {
    HIP_TRY(hipEventRecord(r.b, s));
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof.push_back(r);
    return DVID_OK;
}

int igemm(const IgemmParams& p, hipStream_t s) {
    if (!g_prof_on) return dvid_igemm_launch(p, s);
    ProfRec r{.M = p.M, .N = p.Cout, .K = p.Kpad, .taps = p.ntaps, .stride = p.stride, .res_mode = p.res_mode, .family = true};
    r.flop = 2.0 * p.M * (double)p.Cout * (double)p.alg_k;
    // algorithmic HBM bytes: every operand touched once (input pixels, packed weights, output, residual)
    const double in_px = (double)p.M * (p.ntaps > 1 ? p.stride * p.stride : 1);
    r.bytes = in_px * p.Cin * 2.0 + (double)p.Cout * p.Kpad * 2.0 +
              (double)p.M * p.Cout * (p.out_f32 ? 4.0 : 2.0) * (p.splitk > 1 ? p.splitk : 1) +
              (p.res_mode == 1 ? (double)p.M * p.Cout * (p.res_f32 ? 4.0 : 2.0) : p.res_mode == 2 ? (double)p.M * p.Cout * 0.5 : 0.0);
    // the kernel the shape rules of dvid_igemm_launch pick (runs with a forced tile configuration or with the wstat / conv3x3 options off are labelled by the rule)
    r.kind = dvid_wstat_preferred(p) ? (p.res_mode == 1 ? "wstat2" : "wstat") : dvid_conv3x3_halo_preferred(p) ? (p.Cin == 16 ? "conv4x4_s2d" : p.Cout == 64 ? "conv3x3_c64" : "conv3x3_halo") : "igemm2";
    return prof_bracket(r, s, [&] { return dvid_igemm_launch(p, s); });
}

// The fused tail of a res2 bottleneck block (bneck.hip) as one record of the implicit-GEMM family: its algorithmic work is the sum
// of the products it computes (conv2 + conv3 [+ shortcut] [+ next conv1]), its bytes what the launch touches once.
int bneck_tail(const half_t* t1, const half_t* w2, const float* b2, const half_t* w3, const float* b3, const half_t* res, const half_t* ws,
               const float* bs, const half_t* w1n, const float* b1n, int n_next, half_t* out, half_t* t1n, int n, int H, int W, hipStream_t s) {
    if (!g_prof_on) return dvid_bneck64_tail_launch(t1, w2, b2, w3, b3, res, ws, bs, w1n, b1n, n_next, out, t1n, n, H, W, s);
    const double M = (double)n * H * W;
    const int nn = w1n ? n_next : 0;
    const int kk = 576 + 256 + (ws ? 256 : 0) + 4 * nn;               // MACs per pixel / 64
    ProfRec r{.M = (int)M, .N = 256, .K = kk, .taps = 9, .stride = 1, .family = true};
    r.flop = 2.0 * M * 64.0 * kk;
    r.bytes = M * 2.0 * (64 + (ws ? 64 : 256) + 256 + nn) + 2.0 * 64 * kk;
    r.kind = "bneck64_tail";
    r.res_mode = ws ? 4 : 3;                  // CSV marker: 3 = fused block tail, 4 = with the shortcut convolution
    return prof_bracket(r, s, [&] { return dvid_bneck64_tail_launch(t1, w2, b2, w3, b3, res, ws, bs, w1n, b1n, n_next, out, t1n, n, H, W, s); });
}

int bneck128_tail(const half_t* t1, const half_t* w2, const float* b2, const half_t* w3, const float* b3, const half_t* res, const half_t* w1n,
                  const float* b1n, half_t* out, half_t* t1n, int n, int H, int W, hipStream_t s) {
    if (!g_prof_on) return dvid_bneck128_tail_launch(t1, w2, b2, w3, b3, res, w1n, b1n, out, t1n, n, H, W, s);
    const double M = (double)n * H * W;
    const int kk = (w2 ? 1152 : 0) + 512 + (w1n ? 512 : 0);            // MACs per pixel / 128
    ProfRec r{.M = (int)M, .N = 512, .K = kk, .taps = w2 ? 9 : 1, .stride = 1, .family = true};
    r.flop = 2.0 * M * 128.0 * kk;
    r.bytes = M * 2.0 * (128 + 512 + 512 + (w1n ? 128 : 0)) + 2.0 * 128 * kk;
    r.kind = "bneck128_tail";
    r.res_mode = 3;
    return prof_bracket(r, s, [&] { return dvid_bneck128_tail_launch(t1, w2, b2, w3, b3, res, w1n, b1n, out, t1n, n, H, W, s); });
}

extern "C" {
int dvid_profile_enable(int on) {
    g_prof_on = on != 0;
    return DVID_OK;
}
int dvid_profile_reset(void) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto& r : g_prof) g_prof_pool.push_back(r);
    g_prof.clear();
    return DVID_OK;
}
int dvid_profile_read_bytes(double* igemm_alg_bytes) {
    g_err[0] = 0;
    double b = 0;
    for (auto& r : g_prof)
        if (r.family) b += r.bytes;
    if (igemm_alg_bytes) *igemm_alg_bytes = b;
    return DVID_OK;
}

static int profile_sum(double* ms_out, double* flop_out, double* bytes_out, int64_t* n_out) {
    double ms = 0, fl = 0, by = 0;
    int64_t n = 0;
    for (auto& r : g_prof) {
        if (!r.family) continue;
        HIP_TRY(hipEventSynchronize(r.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        ms += t;
        fl += r.flop;
        by += r.bytes;
        ++n;
    }
    if (ms_out) *ms_out = ms;
    if (flop_out) *flop_out = fl;
    if (bytes_out) *bytes_out = by;
    if (n_out) *n_out = n;
    return DVID_OK;
}

int dvid_profile_read(double* igemm_ms, double* igemm_flop, int64_t* igemm_launches) {
    g_err[0] = 0;
    return profile_sum(igemm_ms, igemm_flop, nullptr, igemm_launches);
}

// one CSV line per recorded launch: kernel,family,M,N,K,taps,stride,res_mode,ms,tflops,alg_mbytes,alg_gbs
int dvid_profile_dump(const char* path) {
    g_err[0] = 0;
    FILE* f = fopen(path, "w");
    if (!f) FAIL(DVID_ERR_ARG, "cannot open %s", path);
    fprintf(f, "kernel,family,M,N,K,taps,stride,res_mode,ms,tflops,alg_mbytes,alg_gbs\n");
    for (auto& r : g_prof) {
        HIP_TRY(hipEventSynchronize(r.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        fprintf(f, "%s,%d,%d,%d,%d,%d,%d,%d,%.5f,%.2f,%.3f,%.1f\n", r.kind, (int)r.family, r.M, r.N, r.K, r.taps, r.stride, r.res_mode, t, r.flop / (t * 1e-3) / 1e12,
                r.bytes / 1e6, r.bytes / (t * 1e-3) / 1e9);
    }
    fclose(f);
    return DVID_OK;
}
}  // extern "C"
