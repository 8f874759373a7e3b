// The backward of the tail of an RCNNHead / RCNNHead_cond pass (box_head.py:524-548 / :636-664; the forward is csrc/headtail.hip):
// FFN (linear1, ReLU, linear2) + residual + norm3, the time (and cond) modulation, the cls tower + class_logits, the reg tower +
// bboxes_delta, apply_deltas.  dvid_head_tail_backward recomputes that forward in fp32 into scratch, keeping the activations the
// backward needs (the inference kernel and its bits stay untouched), and then walks it back.
//
// Arithmetic: fp32 storage, fp32 products, fp32 accumulation.  Every product runs on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate, a
// k-ordered fmaf chain), NOT on the split-operand three-pass fp16 scheme of f32_split.h: a cotangent is routinely below fp16's normal
// range (6e-5), where the `lo` half of a split operand is lost.  No fp16 gradients, no range flag.
//
//   gemm_kernel            C[i][j] = sum_r A(i, r) B(j, r) with both operands given by strides, so the one kernel is the forward product
//                          X W^T, the data gradient dY W and the weight gradient dY^T X.  64 x 64 tiles, 4 waves of 32 x 32, K step 16
//                          through LDS.  blockIdx.z splits the reduction into fixed chunks whose tiles go to scratch as partials
//   reduce_partials_kernel adds those partials in ascending chunk order: NO atomics anywhere, two runs give the same bits
//   colsum_partial_kernel  column sums over rows (bias, LayerNorm gamma / beta gradients) and over the rows of one image (d_scale,
//                          d_shift: image boundaries do not fall on row tiles, so the chunks are counted from each image's first row)
//   ln_fwd / ln_bwd        LayerNorm (+ residual, + ReLU) per row, one wave per row, fp32 statistics kept (xhat, rstd)
//   the rest is elementwise: SiLU and its derivative, the modulation, apply_deltas and its backward.
// The first five and their host launchers live in csrc/bwd_kernels.h, which csrc/interact_bwd.hip includes too.
//
// The kinks (part of the contract, include/dvid_hip.h): ReLU passes nothing at a pre-activation of exactly 0; clamp(max = scale_clamp)
// passes the gradient at equality and nothing above; a clamped dw leaves dx / dy their gradients; a zero-width box gives exact zeros.
#include <math.h>

#include "../../include/dvid_hip.h"
#include "common.h"
#include "kernels.h"
#include "bwd_kernels.h"

namespace {

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void silu_kernel(const float* __restrict__ x, long count, float* __restrict__ y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) y[i] = x[i] * sigmoidf(x[i]);
}
// dx = dy * d SiLU(x) / dx = dy * s (1 + x (1 - s))
__global__ void silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, long count, float* __restrict__ dx) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float s = sigmoidf(x[i]);
    dx[i] = dy[i] * (s * (1.f + x[i] * (1.f - s)));
}

// fc = obj * (scale + 1) + shift; scale row of image f at ss + f * ss_ld; shift per image (ss + f * ss_ld + 256) or per row (shift_rows)
__global__ void modulate_kernel(const float* __restrict__ obj, const float* __restrict__ ss, int ss_ld, const float* __restrict__ shift_rows, int m, long R,
                                float* __restrict__ fc) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * D) return;
    const long row = i / D;
    const int col = (int)(i - row * D);
    const float* s = ss + (row / m) * ss_ld;
    fc[i] = obj[i] * (s[col] + 1.f) + (shift_rows ? shift_rows[i] : s[D + col]);
}
// d_obj_total = d_fc * (scale + 1) + d_obj (the cotangent; null = zeros)
__global__ void modulate_bwd_kernel(const float* __restrict__ dfc, const float* __restrict__ ss, int ss_ld, const float* __restrict__ dobj, int m, long R,
                                    float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * D) return;
    const long row = i / D;
    const int col = (int)(i - row * D);
    const float v = dfc[i] * (ss[(row / m) * ss_ld + col] + 1.f);
    out[i] = dobj ? v + dobj[i] : v;
}

struct DeltaW {
    float wx, wy, ww, wh, clamp;
};

__global__ void apply_deltas_fwd_kernel(const float* __restrict__ deltas, const float* __restrict__ boxes, long R, DeltaW w, float* __restrict__ out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float4v b = *reinterpret_cast<const float4v*>(boxes + r * 4), d = *reinterpret_cast<const float4v*>(deltas + r * 4);
    const float widths = b[2] - b[0], heights = b[3] - b[1];
    const float ctr_x = b[0] + 0.5f * widths, ctr_y = b[1] + 0.5f * heights;
    const float dx = d[0] / w.wx, dy = d[1] / w.wy, dw = fminf(d[2] / w.ww, w.clamp), dh = fminf(d[3] / w.wh, w.clamp);
    const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y, pw = expf(dw) * widths, ph = expf(dh) * heights;
    *reinterpret_cast<float4v*>(out + r * 4) = (float4v){pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph};
}
// d_deltas from d_boxes (null = zeros).  dw above the clamp: no gradient for it, dx and dy keep theirs; at equality it passes.  Every term
// carries the width (height) as a factor, so a box of zero width gives exact zeros.
__global__ void apply_deltas_bwd_kernel(const float* __restrict__ deltas, const float* __restrict__ boxes, const float* __restrict__ dboxes, long R, DeltaW w,
                                        float* __restrict__ ddeltas) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    float4v o = {0.f, 0.f, 0.f, 0.f};
    if (dboxes) {
        const float4v b = *reinterpret_cast<const float4v*>(boxes + r * 4), d = *reinterpret_cast<const float4v*>(deltas + r * 4);
        const float4v g = *reinterpret_cast<const float4v*>(dboxes + r * 4);
        const float widths = b[2] - b[0], heights = b[3] - b[1];
        const float rw = d[2] / w.ww, rh = d[3] / w.wh;
        const float d_pcx = g[0] + g[2], d_pcy = g[1] + g[3], d_pw = 0.5f * g[2] - 0.5f * g[0], d_ph = 0.5f * g[3] - 0.5f * g[1];
        o[0] = d_pcx * widths / w.wx;
        o[1] = d_pcy * heights / w.wy;
        o[2] = rw <= w.clamp ? d_pw * widths * expf(rw) / w.ww : 0.f;
        o[3] = rh <= w.clamp ? d_ph * heights * expf(rh) / w.wh : 0.f;
    }
    *reinterpret_cast<float4v*>(ddeltas + r * 4) = o;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

struct Layout {
    float *h1, *dh1, *tmp, *xhat3, *rstd3, *obj, *ste, *ss, *sc, *shiftc, *fc, *txhat[8], *trstd[8], *tact[8], *logits, *deltas, *ddeltas, *ga, *gb, *dy, *dfc,
        *dss, *gte, *part;
    long long bytes;
};

Layout lay_out(void* scratch, int n, int m, int dff, int c, int layers, bool cond) {
    const long R = (long)n * m;
    Layout L;
    Bump b{static_cast<char*>(scratch)};
    L.h1 = b.take(R * dff);
    L.dh1 = b.take(R * dff);
    L.tmp = b.take(R * D);
    L.xhat3 = b.take(R * D);
    L.rstd3 = b.take(R);
    L.obj = b.take(R * D);
    L.ste = b.take((long)n * 4 * D);
    L.ss = b.take((long)n * 2 * D);
    L.sc = b.take(cond ? R * D : 0);
    L.shiftc = b.take(cond ? R * D : 0);
    L.fc = b.take(R * D);
    for (int l = 0; l < 8; ++l) {
        L.txhat[l] = b.take(l < layers ? R * D : 0);
        L.trstd[l] = b.take(l < layers ? R : 0);
        L.tact[l] = b.take(l < layers ? R * D : 0);
    }
    L.logits = b.take(R * c);
    L.deltas = b.take(R * 4);
    L.ddeltas = b.take(R * 4);
    L.ga = b.take(R * D);
    L.gb = b.take(R * D);
    L.dy = b.take(R * D);
    L.dfc = b.take(R * D);
    L.dss = b.take((long)n * 2 * D);
    L.gte = b.take((long)n * 4 * D);
    // partials: the largest weight gradient (linear1 / linear2, class_logits or block_time_mlp.1: 512 x 1024) times the row chunks, or the
    // per-image column sums (chunks counted from each image's first row)
    const long chunks = ceil_div(R, (long)CHUNK);
    const long widest = (long)(dff > c ? (dff > 8 * D ? dff : 8 * D) : (c > 8 * D ? c : 8 * D)) * D;
    const long per_image = (long)n * ceil_div(m, CHUNK) * D;
    L.part = b.take(chunks * widest > per_image ? chunks * widest : per_image);
    L.bytes = b.off;
    return L;
}

}  // namespace

long long dvid_head_tail_backward_scratch_bytes_host(int n, int m, int dff, int num_classes, int num_cls, int num_reg, int has_cond) {
    if (n < 1 || m < 1 || dff < 1 || num_classes < 1 || num_cls < 0 || num_reg < 0 || num_cls > 4 || num_reg > 4) return -1;
    return lay_out(nullptr, n, m, dff, num_classes, num_cls + num_reg, has_cond != 0).bytes;
}

int dvid_head_tail_backward_launch(const HeadTailBwdArgs& a, hipStream_t s) {
    const long R = (long)a.n * a.m;
    const int dff = a.dff, C = a.num_classes, layers = a.num_cls + a.num_reg, m = a.m, n = a.n;
    const bool cond = a.cond != nullptr;
    const Layout L = lay_out(a.scratch, n, m, dff, C, layers, cond);
    Run run{s, L.part};
    const float* const* P = a.params;
    const float *W1 = P[0], *b1 = P[1], *W2 = P[2], *b2 = P[3], *n3g = P[4], *n3b = P[5], *Wt = P[6], *bt = P[7], *Wc = P[8], *bc = P[9], *Wl = P[10],
                *bl = P[11], *Wd = P[12], *bd = P[13];
    const float* const* T = P + 14;          // layer l: T[3 l] Linear weight, T[3 l + 1] LayerNorm weight, T[3 l + 2] LayerNorm bias
    const DeltaW dw{a.wx, a.wy, a.ww, a.wh, a.scale_clamp};
    const unsigned eb = 256;
    auto blocks = [&](long count) { return dim3((unsigned)ceil_div(count, (long)eb)); };
    const dim3 rows4((unsigned)ceil_div(R, 4L));
    const int ssw = cond ? D : 2 * D;          // the time MLP gives scale and shift, or scale alone (cond head)

    // ---- forward, recomputed in fp32
    run.fwd(a.x, W1, b1, 1, R, dff, D, L.h1);
    run.fwd(L.h1, W2, b2, 0, R, D, dff, L.tmp);
    float* obj = a.obj_out ? a.obj_out : L.obj;
    hipLaunchKernelGGL(ln_fwd_kernel, rows4, dim3(256), 0, s, L.tmp, a.x, n3g, n3b, 0, R, obj, L.xhat3, L.rstd3);
    hipLaunchKernelGGL(silu_kernel, blocks((long)n * 4 * D), dim3(eb), 0, s, a.time_emb, (long)n * 4 * D, L.ste);
    run.fwd(L.ste, Wt, bt, 0, n, ssw, 4 * D, L.ss);
    if (cond) {
        hipLaunchKernelGGL(silu_kernel, blocks(R * D), dim3(eb), 0, s, a.cond, R * D, L.sc);
        run.fwd(L.sc, Wc, bc, 0, R, D, D, L.shiftc);
    }
    hipLaunchKernelGGL(modulate_kernel, blocks(R * D), dim3(eb), 0, s, obj, L.ss, ssw, cond ? L.shiftc : nullptr, m, R, L.fc);
    const float* tin[8];          // the input of tower layer l
    const float* feat[2];         // what class_logits / bboxes_delta read
    for (int tower = 0, l = 0; tower < 2; ++tower) {
        const float* in = L.fc;
        for (int i = 0; i < (tower ? a.num_reg : a.num_cls); ++i, ++l) {
            tin[l] = in;
            run.fwd(in, T[3 * l], nullptr, 0, R, D, D, L.tmp);
            hipLaunchKernelGGL(ln_fwd_kernel, rows4, dim3(256), 0, s, L.tmp, nullptr, T[3 * l + 1], T[3 * l + 2], 1, R, L.tact[l], L.txhat[l], L.trstd[l]);
            in = L.tact[l];
        }
        feat[tower] = in;
    }
    float* logits = a.logits_out ? a.logits_out : L.logits;
    run.fwd(feat[0], Wl, bl, 0, R, C, D, logits);
    run.fwd(feat[1], Wd, bd, 0, R, 4, D, L.deltas);
    if (a.boxes_out) hipLaunchKernelGGL(apply_deltas_fwd_kernel, blocks(R), dim3(eb), 0, s, L.deltas, a.boxes_in, R, dw, a.boxes_out);
    if (run.rc != DVID_OK) return run.rc;
    LAUNCH_CHECK();
    if (!a.grads) return DVID_OK;          // forward only

    // ---- backward
    float* const* G = a.grads;
    float* const* GT = G + 14;
    // one tower back from the gradient `g` of its last activation (layers [l0, l0 + count)); its end lands in dfc (added when `add`)
    auto tower_bwd = [&](const float* g, int l0, int count, bool add) {
        for (int l = l0 + count - 1; l >= l0; --l) {
            hipLaunchKernelGGL(ln_bwd_kernel, rows4, dim3(256), 0, s, g, L.tact[l], L.txhat[l], L.trstd[l], T[3 * l + 1], R, L.dy, L.tmp);
            run.colsum(L.dy, L.txhat[l], D, (int)R, 1, GT[3 * l + 1], 0);
            run.colsum(L.dy, nullptr, D, (int)R, 1, GT[3 * l + 2], 0);
            run.wgrad(L.tmp, tin[l], R, D, D, GT[3 * l]);
            float* out = l == l0 ? L.dfc : (g == L.ga ? L.gb : L.ga);
            run.dgrad(L.tmp, T[3 * l], R, D, D, out, l == l0 && add ? L.dfc : nullptr);
            g = out;
        }
    };
    // cls: class_logits, then its tower
    if (a.d_logits) {
        run.colsum(a.d_logits, nullptr, C, (int)R, 1, G[11], 0);
        run.wgrad(a.d_logits, feat[0], R, C, D, G[10]);
        run.dgrad(a.d_logits, Wl, R, C, D, a.num_cls ? L.ga : L.dfc);
    } else {
        HIP_TRY(hipMemsetAsync(G[11], 0, (size_t)C * 4, s));
        HIP_TRY(hipMemsetAsync(G[10], 0, (size_t)C * D * 4, s));
        HIP_TRY(hipMemsetAsync(a.num_cls ? L.ga : L.dfc, 0, (size_t)R * D * 4, s));
    }
    tower_bwd(L.ga, 0, a.num_cls, false);
    // reg: apply_deltas, bboxes_delta, then its tower
    hipLaunchKernelGGL(apply_deltas_bwd_kernel, blocks(R), dim3(eb), 0, s, L.deltas, a.boxes_in, a.d_boxes, R, dw, L.ddeltas);
    run.colsum(L.ddeltas, nullptr, 4, (int)R, 1, G[13], 0);
    run.wgrad(L.ddeltas, feat[1], R, 4, D, G[12]);
    run.dgrad(L.ddeltas, Wd, R, 4, D, a.num_reg ? L.ga : L.dfc, a.num_reg ? nullptr : L.dfc);
    tower_bwd(L.ga, a.num_cls, a.num_reg, true);
    // modulation: d_scale (and d_shift) are sums over the m rows of an image
    run.colsum(L.dfc, obj, D, m, n, L.dss, ssw);
    if (cond) {
        run.colsum(L.dfc, nullptr, D, (int)R, 1, G[9], 0);
        run.wgrad(L.dfc, L.sc, R, D, D, G[8]);
        run.dgrad(L.dfc, Wc, R, D, D, L.ga);
        hipLaunchKernelGGL(silu_bwd_kernel, blocks(R * D), dim3(eb), 0, s, a.cond, L.ga, R * D, a.d_cond);
    } else {
        run.colsum(L.dfc, nullptr, D, m, n, L.dss + D, ssw);
    }
    run.colsum(L.dss, nullptr, ssw, n, 1, G[7], 0);
    run.wgrad(L.dss, L.ste, n, ssw, 4 * D, G[6]);
    run.dgrad(L.dss, Wt, n, ssw, 4 * D, L.gte);
    hipLaunchKernelGGL(silu_bwd_kernel, blocks((long)n * 4 * D), dim3(eb), 0, s, a.time_emb, L.gte, (long)n * 4 * D, a.d_time_emb);
    // norm3 (+ the residual) and the FFN
    hipLaunchKernelGGL(modulate_bwd_kernel, blocks(R * D), dim3(eb), 0, s, L.dfc, L.ss, ssw, a.d_obj, m, R, L.ga);
    hipLaunchKernelGGL(ln_bwd_kernel, rows4, dim3(256), 0, s, L.ga, nullptr, L.xhat3, L.rstd3, n3g, R, nullptr, L.gb);
    run.colsum(L.ga, L.xhat3, D, (int)R, 1, G[4], 0);
    run.colsum(L.ga, nullptr, D, (int)R, 1, G[5], 0);
    run.colsum(L.gb, nullptr, D, (int)R, 1, G[3], 0);
    run.wgrad(L.gb, L.h1, R, D, dff, G[2]);
    run.dgrad(L.gb, W2, R, D, dff, L.dh1, nullptr, L.h1);
    run.colsum(L.dh1, nullptr, dff, (int)R, 1, G[1], 0);
    run.wgrad(L.dh1, a.x, R, dff, D, G[0]);
    run.dgrad(L.dh1, W1, R, dff, D, a.d_x, L.gb);          // d_x = the FFN path + the skip
    if (run.rc != DVID_OK) return run.rc;
    LAUNCH_CHECK();
    return DVID_OK;
}
