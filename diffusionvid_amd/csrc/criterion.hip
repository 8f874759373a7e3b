// The training objective, values and gradient (modeling/roi_heads/box_head/loss.py restates the same on the host; the reference's
// box_head/loss.py:257-688 and diffusion_det.py:681-725):
//
//   q_sample_boxes_kernel    the noisy boxes of a labelled batch: ground truth padded to NUM_PROPOSALS, diffused to step t, as absolute xyxy
//   criterion_match_kernel   the dynamic-k matcher, one workgroup per (head output, image)
//   criterion_loss_kernel    the focal, L1 and 1 - GIoU sums over a chunk of CL_ROWS queries, fp32 terms added in float64 by a fixed tree
//   criterion_sum_kernel     the chunks' partial sums added in chunk order
//   criterion_grad_kernel    the gradient of a weighted sum of those sums with respect to every logit and box, one pass, fp32
//
// The matcher.  The M x G cost matrix lives in global scratch, column-major (cost[g * M + m]: a wave that walks a column reads
// consecutive addresses), with one byte per entry of the matching matrix beside it; LDS holds the ground truth and the per-column and
// per-row vectors (dynamic k, column counts, row counts, the rows that held several columns before the repair loop).
//   cost       a lane per query: ((cost_bbox * L1 + cost_class * class) + cost_giou * (-GIoU)) + 100 * !(in box and centre), then + 10000
//              on the queries outside every box and centre region -- fp32, contraction off, in the reference's order
//   selections a wave per column: the OTA_K largest IoUs (dynamic k = max(1, int(their sum))) and the k cheapest queries by repeated
//              wave-wide extremum over 64-bit keys (value bits, row), so equal values go to the lower row
//   conflicts  a lane per row that held several columns: the row's least cost over ALL columns (equal costs: the lower column)
//   repair     while a column is empty, at most G + DVID_CRITERION_REPAIR_SLACK rounds: + 100000 on the matched rows, every empty column
//              takes its cheapest row, and if any row now holds several columns the rows that held several BEFORE the loop are resolved
//              again (the reference never refreshes that mask; another row keeps its columns and reports the lowest)
// Nothing here is ordered by an atomic: the LDS counters are integers, and every float sum has a fixed order.
#include "../../include/dvid_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

typedef unsigned long long u64;

#define CM_THREADS 256
#define CM_WAVES (CM_THREADS / WAVE)
#define CL_THREADS 256
#define CL_ROWS 16
#define CG_DEPTH 4

struct CritParams {
    float alpha, gamma, cost_class, cost_bbox, cost_giou;
    int ota_k;
};

__device__ __forceinline__ float cr_sigmoid(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }
__device__ __forceinline__ float cr_pow(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }
__device__ __forceinline__ float cr_area(const float4v b) { return (b[2] - b[0]) * (b[3] - b[1]); }

// torchvision's box_iou and the reference's generalized_box_iou, one pair
__device__ __forceinline__ float cr_iou(const float4v a, const float area_a, const float4v b, const float area_b, float* union_out) {
    const float w = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f), h = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
    const float inter = w * h, uni = (area_a + area_b) - inter;
    *union_out = uni;
    return __fdiv_rn(inter, uni);
}
__device__ __forceinline__ float cr_giou(const float4v a, const float area_a, const float4v b, const float area_b, float* iou_out) {
    float uni;
    const float iou = cr_iou(a, area_a, b, area_b, &uni);
    const float w = fmaxf(fmaxf(a[2], b[2]) - fminf(a[0], b[0]), 0.f), h = fmaxf(fmaxf(a[3], b[3]) - fminf(a[1], b[1]), 0.f);
    const float area = w * h;
    *iou_out = iou;
    return iou - __fdiv_rn(area - uni, area);
}

// a float as an unsigned that orders the same way (-0 and +0 are one value)
__device__ __forceinline__ unsigned cr_ordered(float f) {
    if (f == 0.f) f = 0.f;
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ u64 cr_wave_min(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = ((u64)__shfl_xor((unsigned)(v >> 32), o, 64) << 32) | __shfl_xor((unsigned)v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}
__device__ __forceinline__ u64 cr_wave_max(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = ((u64)__shfl_xor((unsigned)(v >> 32), o, 64) << 32) | __shfl_xor((unsigned)v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}
__device__ __forceinline__ double cr_wave_sum(double v) {          // a fixed butterfly: every lane ends with the same bits
    for (int o = 32; o > 0; o >>= 1) {
        const u64 b = (u64)__double_as_longlong(v);
        const u64 other = ((u64)__shfl_xor((unsigned)(b >> 32), o, 64) << 32) | __shfl_xor((unsigned)b, o, 64);
        v = v + __longlong_as_double((long long)other);
    }
    return v;
}

// ---- boxes diffused from the ground truth ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void q_sample_boxes_kernel(const float* __restrict__ gt, const int* __restrict__ gt_starts, int n, int M,
                                                             const int* __restrict__ t, const float* __restrict__ sqrt_ac,
                                                             const float* __restrict__ sqrt_omac, int timesteps, const float* __restrict__ noise,
                                                             const float* __restrict__ placeholder, float scale, const float* __restrict__ sizes,
                                                             float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * M) return;
    const int i = idx / M, j = idx - i * M;
    const int g0 = gt_starts[i], G = min(max(gt_starts[i + 1] - g0, 0), M);
    const int real = G > 0 ? G : 1;          // no ground truth: one fake box over the whole image
    float x[4];
    if (j < G) {
        for (int k = 0; k < 4; ++k) x[k] = gt[(size_t)(g0 + j) * 4 + k];
    } else if (j < real) {
        x[0] = 0.5f, x[1] = 0.5f, x[2] = 1.f, x[3] = 1.f;
    } else {          // the padding: the reference's draw of M - real rows follows the boxes
        const float* p = placeholder + ((size_t)i * M + (j - real)) * 4;
        for (int k = 0; k < 4; ++k) x[k] = __fdiv_rn(p[k], 6.f) + 0.5f;
        x[2] = fmaxf(x[2], 1e-4f), x[3] = fmaxf(x[3], 1e-4f);
    }
    const int ti = min(max(t[i], 0), timesteps - 1);
    const float a = sqrt_ac[ti], b = sqrt_omac[ti];
    const float* nz = noise + (size_t)idx * 4;
    for (int k = 0; k < 4; ++k) {
        const float start = (x[k] * 2.f - 1.f) * scale;
        float v = a * start + b * nz[k];
        v = fminf(fmaxf(v, -1.f * scale), scale);
        x[k] = __fdiv_rn(__fdiv_rn(v, scale) + 1.f, 2.f);
    }
    const float w = sizes[2 * i], h = sizes[2 * i + 1];
    float* o = out + (size_t)idx * 4;
    o[0] = (x[0] - 0.5f * x[2]) * w, o[1] = (x[1] - 0.5f * x[3]) * h, o[2] = (x[0] + 0.5f * x[2]) * w, o[3] = (x[1] + 0.5f * x[3]) * h;
}

int dvid_q_sample_boxes_launch(const float* gt, const int* gt_starts, int n, int m, const int* t, const float* sqrt_ac, const float* sqrt_omac,
                               int timesteps, const float* noise, const float* placeholder, float scale, const float* sizes, float* out, hipStream_t s) {
    if (n < 0 || m < 1 || timesteps < 1) return DVID_ERR_ARG;
    if (n == 0) return DVID_OK;
    hipLaunchKernelGGL(q_sample_boxes_kernel, dim3(ceil_div(n * m, 256)), dim3(256), 0, s, gt, gt_starts, n, m, t, sqrt_ac, sqrt_omac, timesteps, noise,
                       placeholder, scale, sizes, out);
    LAUNCH_CHECK();
    return DVID_OK;
}

// ---- the matcher -----------------------------------------------------------------------------------------------------------------------
// rows [tid, tid + CM_THREADS, ...) that held several columns before the repair loop go to the column of their least cost
__device__ __forceinline__ void cm_resolve(float* __restrict__ cost, unsigned char* __restrict__ match, int M, int G, const unsigned char* s_held,
                                           int* s_row, int* s_col) {
    for (int m = threadIdx.x; m < M; m += CM_THREADS) {
        if (!s_held[m]) continue;
        float best = cost[m];
        int arg = 0;
        for (int g = 1; g < G; ++g) {
            const float c = cost[(size_t)g * M + m];
            if (c < best) best = c, arg = g;
        }
        for (int g = 0; g < G; ++g)
            if (match[(size_t)g * M + m]) {
                match[(size_t)g * M + m] = 0;
                atomicSub(&s_col[g], 1);
            }
        match[(size_t)arg * M + m] = 1;
        atomicAdd(&s_col[arg], 1);
        s_row[m] = 1;
    }
}

__global__ __launch_bounds__(CM_THREADS) void criterion_match_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, int n, int M, int C,
                                                                     const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                                     const int* __restrict__ gt_starts, const float* __restrict__ sizes, CritParams p,
                                                                     float* __restrict__ cost_all, unsigned char* __restrict__ match_all, int gmax,
                                                                     int* __restrict__ assign, int* __restrict__ matched_query,
                                                                     int* __restrict__ status) {
    __shared__ float4v s_gt[DVID_CRITERION_MAX_GT], s_gn[DVID_CRITERION_MAX_GT], s_gin[DVID_CRITERION_MAX_GT], s_gct[DVID_CRITERION_MAX_GT];
    __shared__ float s_garea[DVID_CRITERION_MAX_GT];
    __shared__ int s_lab[DVID_CRITERION_MAX_GT], s_k[DVID_CRITERION_MAX_GT], s_col[DVID_CRITERION_MAX_GT];
    __shared__ unsigned char s_empty[DVID_CRITERION_MAX_GT];
    __shared__ int s_row[DVID_CRITERION_MAX_ROWS];
    __shared__ unsigned char s_held[DVID_CRITERION_MAX_ROWS];
    __shared__ int s_bad, s_any, s_multi, s_sticky;

    const int set = blockIdx.x, img = set % n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = gt_starts[img], G = min(max(gt_starts[img + 1] - g0, 0), min(gmax, DVID_CRITERION_MAX_GT));
    const float* lg = logits + (size_t)set * M * C;
    const float* bx = boxes + (size_t)set * M * 4;
    float* cost = cost_all + (size_t)set * gmax * M;
    unsigned char* match = match_all + (size_t)set * gmax * M;
    int* asg = assign + (size_t)set * M;
    int* mq = matched_query + (size_t)set * gmax;
    const float iw = sizes[2 * img], ih = sizes[2 * img + 1];

    if (tid == 0) s_bad = 0, s_sticky = 0;
    __syncthreads();
    // ---- the ground truth: the box, its normalised form, the box after (cx, cy, w, h) and back, the centre region ----
    for (int g = tid; g < G; g += CM_THREADS) {
        const float* b = gt_boxes + (size_t)(g0 + g) * 4;
        const float4v q = {b[0], b[1], b[2], b[3]};
        const int l = gt_labels[g0 + g] - 1;
        if (q[2] < q[0] || q[3] < q[1]) atomicOr(&s_bad, DVID_CRITERION_ERR_DEGENERATE);
        if (l < 0 || l >= C) atomicOr(&s_bad, DVID_CRITERION_ERR_LABEL);
        const float cx = __fdiv_rn(q[0] + q[2], 2.f), cy = __fdiv_rn(q[1] + q[3], 2.f), w = q[2] - q[0], h = q[3] - q[1];
        const float4v in = {cx - 0.5f * w, cy - 0.5f * h, cx + 0.5f * w, cy + 0.5f * h};
        const float rx = 2.5f * (in[2] - in[0]), ry = 2.5f * (in[3] - in[1]);
        s_gt[g] = q, s_gin[g] = in, s_gct[g] = (float4v){cx - rx, cy - ry, cx + rx, cy + ry};
        s_gn[g] = (float4v){__fdiv_rn(q[0], iw), __fdiv_rn(q[1], ih), __fdiv_rn(q[2], iw), __fdiv_rn(q[3], ih)};
        s_garea[g] = cr_area(q), s_lab[g] = l, s_col[g] = 0;
    }
    for (int m = tid; m < M; m += CM_THREADS) {
        const float* b = bx + (size_t)m * 4;
        if (b[2] < b[0] || b[3] < b[1]) atomicOr(&s_bad, DVID_CRITERION_ERR_DEGENERATE);
        s_row[m] = 0, s_held[m] = 0;
        asg[m] = -1;
    }
    for (int g = tid; g < gmax; g += CM_THREADS) mq[g] = -1;
    __syncthreads();
    if (s_bad || G == 0) {          // uniform
        if (tid == 0) status[set] = s_bad;
        return;
    }

    // ---- the cost matrix ----
    for (int m = tid; m < M; m += CM_THREADS) {
        const float* b = bx + (size_t)m * 4;
        const float4v q = {b[0], b[1], b[2], b[3]};
        const float cx = __fdiv_rn(q[0] + q[2], 2.f), cy = __fdiv_rn(q[1] + q[3], 2.f), area = cr_area(q);
        const float4v qn = {__fdiv_rn(q[0], iw), __fdiv_rn(q[1], ih), __fdiv_rn(q[2], iw), __fdiv_rn(q[3], ih)};
        bool fg = false;
        for (int g = 0; g < G; ++g) {
            const float4v in = s_gin[g], ct = s_gct[g];
            fg = fg || (cx > in[0] && cx < in[2] && cy > in[1] && cy < in[3]) || (cx > ct[0] && cx < ct[2] && cy > ct[1] && cy < ct[3]);
        }
        bool bad = false;
        for (int g = 0; g < G; ++g) {
            const float4v in = s_gin[g], ct = s_gct[g], gn = s_gn[g];
            const bool both = (cx > in[0] && cx < in[2] && cy > in[1] && cy < in[3]) && (cx > ct[0] && cx < ct[2] && cy > ct[1] && cy < ct[3]);
            const float pr = cr_sigmoid(lg[(size_t)m * C + s_lab[g]]);
            const float neg = ((1.f - p.alpha) * cr_pow(pr, p.gamma)) * (-logf((1.f - pr) + 1e-8f));
            const float pos = (p.alpha * cr_pow(1.f - pr, p.gamma)) * (-logf(pr + 1e-8f));
            const float cls = pos - neg;
            const float l1 = ((fabsf(qn[0] - gn[0]) + fabsf(qn[1] - gn[1])) + fabsf(qn[2] - gn[2])) + fabsf(qn[3] - gn[3]);
            float iou;
            const float giou = cr_giou(q, area, s_gt[g], s_garea[g], &iou);
            float c = ((p.cost_bbox * l1 + p.cost_class * cls) + p.cost_giou * (-giou)) + 100.f * (both ? 0.f : 1.f);
            if (!fg) c = c + 10000.f;
            bad = bad || !isfinite(c) || !isfinite(iou);
            cost[(size_t)g * M + m] = c;
            match[(size_t)g * M + m] = 0;
        }
        if (bad) atomicOr(&s_bad, DVID_CRITERION_ERR_NONFINITE);
    }
    __syncthreads();
    if (s_bad) {          // uniform
        if (tid == 0) status[set] = s_bad;
        return;
    }

    // ---- dynamic k and the k cheapest queries, a wave per column ----
    const int top = min(p.ota_k, M);
    for (int g = wave; g < G; g += CM_WAVES) {
        const float4v gb = s_gt[g];
        const float ga = s_garea[g];
        u64 prev = ~(u64)0;
        float sum = 0.f;
        for (int it = 0; it < top; ++it) {
            u64 best = 0;
            for (int m = lane; m < M; m += WAVE) {
                const float* b = bx + (size_t)m * 4;
                const float4v q = {b[0], b[1], b[2], b[3]};
                float uni;
                const float iou = cr_iou(q, cr_area(q), gb, ga, &uni);
                const u64 key = ((u64)__float_as_uint(iou == 0.f ? 0.f : iou) << 32) | (u64)(0xffffffffu - (unsigned)m);
                if (key < prev && key > best) best = key;
            }
            best = cr_wave_max(best);
            prev = best;
            const float v = __uint_as_float((unsigned)(best >> 32));
            sum = it == 0 ? v : sum + v;
        }
        const int k = min(max((int)sum, 1), M);
        if (lane == 0) s_k[g] = k;
        const float* col = cost + (size_t)g * M;
        u64 low = 0;
        for (int it = 0; it < k; ++it) {
            u64 best = ~(u64)0;
            for (int m = lane; m < M; m += WAVE) {
                const u64 key = ((u64)cr_ordered(col[m]) << 32) | (u64)m;
                if ((it == 0 || key > low) && key < best) best = key;
            }
            best = cr_wave_min(best);
            low = best;
            if (lane == 0) {
                const int r = (int)(best & 0xffffffffu);
                if (r < M) {          // (always: the column holds M finite costs and k <= M)
                    match[(size_t)g * M + r] = 1;
                    atomicAdd(&s_row[r], 1);
                }
            }
        }
        if (lane == 0) s_col[g] = k;
    }
    __syncthreads();
    for (int m = tid; m < M; m += CM_THREADS) s_held[m] = s_row[m] > 1;
    __syncthreads();
    cm_resolve(cost, match, M, G, s_held, s_row, s_col);

    // ---- the repair loop ----
    int st = 0;
    for (int round = 0;; ++round) {
        if (tid == 0) s_any = 0, s_multi = 0;
        __syncthreads();
        for (int g = tid; g < G; g += CM_THREADS) {
            const bool e = s_col[g] == 0;
            s_empty[g] = e;
            if (e) s_any = 1;
        }
        __syncthreads();
        if (!s_any) break;
        if (round == G + DVID_CRITERION_REPAIR_SLACK) {
            st = DVID_CRITERION_ERR_ROUNDS;
            break;
        }
        for (int g = 0; g < G; ++g)
            for (int m = tid; m < M; m += CM_THREADS)
                if (s_row[m] > 0) cost[(size_t)g * M + m] = cost[(size_t)g * M + m] + 100000.f;
        __syncthreads();
        for (int g = wave; g < G; g += CM_WAVES) {
            if (!s_empty[g]) continue;
            const float* col = cost + (size_t)g * M;
            u64 best = ~(u64)0;
            for (int m = lane; m < M; m += WAVE) {
                const u64 key = ((u64)cr_ordered(col[m]) << 32) | (u64)m;
                if (key < best) best = key;
            }
            best = cr_wave_min(best);
            if (lane == 0) {
                const int r = (int)(best & 0xffffffffu);
                if (r < M) {
                    match[(size_t)g * M + r] = 1;
                    if (atomicAdd(&s_row[r], 1) >= 1) {
                        if (s_held[r]) s_multi = 1;
                        else s_sticky = 1;
                    }
                    s_col[g] = 1;
                }
            }
        }
        __syncthreads();
        if (s_multi || s_sticky) cm_resolve(cost, match, M, G, s_held, s_row, s_col);          // uniform
        __syncthreads();
    }

    // ---- the outputs ----
    for (int m = tid; m < M; m += CM_THREADS) {
        if (s_row[m] == 0) continue;
        int first = -1;
        for (int g = 0; g < G && first < 0; ++g)
            if (match[(size_t)g * M + m]) first = g;
        asg[m] = first;
    }
    for (int g = wave; g < G; g += CM_WAVES) {
        const float* col = cost + (size_t)g * M;
        const unsigned char* mc = match + (size_t)g * M;
        u64 best = ~(u64)0;
        for (int m = lane; m < M; m += WAVE) {
            if (!mc[m]) continue;
            const u64 key = ((u64)cr_ordered(col[m]) << 32) | (u64)m;
            if (key < best) best = key;
        }
        best = cr_wave_min(best);
        if (lane == 0) mq[g] = best == ~(u64)0 ? 0 : (int)(best & 0xffffffffu);          // an empty column is all +inf: torch.min gives row 0
    }
    if (tid == 0) status[set] = st;
}

// ---- the loss sums ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CL_THREADS) void criterion_loss_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, int n, int M, int C,
                                                                    const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                                    const int* __restrict__ gt_starts, const float* __restrict__ sizes, CritParams p,
                                                                    const int* __restrict__ assign, double* __restrict__ partial, int n_chunks,
                                                                    int* __restrict__ status) {
    __shared__ int s_cls[CL_ROWS];
    __shared__ double s_part[CL_THREADS / WAVE][4];
    const int chunk = blockIdx.x, set = blockIdx.y, img = set % n, tid = threadIdx.x;
    const int r0 = chunk * CL_ROWS, rows = min(CL_ROWS, M - r0);
    const int g0 = gt_starts[img], G = max(gt_starts[img + 1] - g0, 0);
    double focal = 0.0, l1s = 0.0, gious = 0.0, cnt = 0.0;
    if (tid < rows) {
        const int a = assign[(size_t)set * M + r0 + tid];
        int cls = -1;
        if (a >= 0 && a < G) {
            cls = gt_labels[g0 + a] - 1;
            const float iw = sizes[2 * img], ih = sizes[2 * img + 1];
            const float* b = boxes + ((size_t)set * M + r0 + tid) * 4;
            const float* t = gt_boxes + (size_t)(g0 + a) * 4;
            const float4v q = {b[0], b[1], b[2], b[3]}, gt = {t[0], t[1], t[2], t[3]};
            // the L1 target: the ground truth normalised, to (cx, cy, w, h) and back
            const float n0 = __fdiv_rn(gt[0], iw), n1 = __fdiv_rn(gt[1], ih), n2 = __fdiv_rn(gt[2], iw), n3 = __fdiv_rn(gt[3], ih);
            const float cx = __fdiv_rn(n0 + n2, 2.f), cy = __fdiv_rn(n1 + n3, 2.f), w = n2 - n0, h = n3 - n1;
            const float d0 = fabsf(__fdiv_rn(q[0], iw) - (cx - 0.5f * w)), d1 = fabsf(__fdiv_rn(q[1], ih) - (cy - 0.5f * h));
            const float d2 = fabsf(__fdiv_rn(q[2], iw) - (cx + 0.5f * w)), d3 = fabsf(__fdiv_rn(q[3], ih) - (cy + 0.5f * h));
            float iou;
            const float giou = cr_giou(q, cr_area(q), gt, cr_area(gt), &iou);
            l1s = (double)(((d0 + d1) + d2) + d3), gious = (double)(1.f - giou), cnt = 1.0;
        }
        s_cls[tid] = cls;
    }
    __syncthreads();
    const float* lg = logits + ((size_t)set * M + r0) * C;
    const int total = rows * C;
    bool bad = false;
    for (int e = tid; e < total; e += CL_THREADS) {
        const int r = e / C, c = e - r * C;
        const float x = lg[e];
        const float t = s_cls[r] == c ? 1.f : 0.f;
        bad = bad || !isfinite(x);
        const float pr = cr_sigmoid(x);
        const float ce = (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x)));
        const float pt = pr * t + (1.f - pr) * (1.f - t);
        float loss = ce * cr_pow(1.f - pt, p.gamma);
        if (p.alpha >= 0.f) loss = (p.alpha * t + (1.f - p.alpha) * (1.f - t)) * loss;
        focal = focal + (double)loss;
    }
    if (bad) atomicOr(&status[set], DVID_CRITERION_ERR_NONFINITE);
    focal = cr_wave_sum(focal), l1s = cr_wave_sum(l1s), gious = cr_wave_sum(gious), cnt = cr_wave_sum(cnt);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) s_part[wave][0] = focal, s_part[wave][1] = l1s, s_part[wave][2] = gious, s_part[wave][3] = cnt;
    __syncthreads();
    if (tid < 4) {
        double v = s_part[0][tid];
        for (int w = 1; w < CL_THREADS / WAVE; ++w) v = v + s_part[w][tid];
        partial[((size_t)set * n_chunks + chunk) * 4 + tid] = v;
    }
}

__global__ __launch_bounds__(256) void criterion_sum_kernel(const double* __restrict__ partial, int n_sets, int n_chunks, double* __restrict__ sums) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_sets * 4) return;
    const int set = idx >> 2, q = idx & 3;
    double v = 0.0;
    for (int c = 0; c < n_chunks; ++c) v = v + partial[((size_t)set * n_chunks + c) * 4 + q];
    sums[idx] = v;
}

// ---- the gradient of the loss sums -----------------------------------------------------------------------------------------------------
// d/dq of coef2 * (1 - GIoU(q, gt)), one operation of cr_giou at a time backwards, with torch's conventions at the kinks: a maximum or
// minimum of equal operands hands each half of the gradient, clamp(min = 0) passes it at exactly 0.
__device__ __forceinline__ float cr_share_max(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }          // d max(a, b) / da
__device__ __forceinline__ float cr_share_min(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ void cr_giou_grad(const float4v a, const float4v b, float c2, float* g) {
    const float wa = a[2] - a[0], ha = a[3] - a[1], area_a = wa * ha, area_b = cr_area(b);
    const float wr = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), hr = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
    const float w = fmaxf(wr, 0.f), h = fmaxf(hr, 0.f), inter = w * h, uni = (area_a + area_b) - inter;
    const float cwr = fmaxf(a[2], b[2]) - fminf(a[0], b[0]), chr = fmaxf(a[3], b[3]) - fminf(a[1], b[1]);
    const float cw = fmaxf(cwr, 0.f), ch = fmaxf(chr, 0.f), area_c = cw * ch;
    const float g_giou = -c2;                                                             // the loss is 1 - giou
    const float g_areac = -g_giou * __fdiv_rn(uni, area_c * area_c);                      // giou = iou - (area_c - uni) / area_c
    const float g_uni = __fdiv_rn(g_giou, area_c) - g_giou * __fdiv_rn(inter, uni * uni);
    const float g_inter = __fdiv_rn(g_giou, uni) - g_uni;
    const float g_wr = wr >= 0.f ? g_inter * h : 0.f, g_hr = hr >= 0.f ? g_inter * w : 0.f;
    const float g_cwr = cwr >= 0.f ? g_areac * ch : 0.f, g_chr = chr >= 0.f ? g_areac * cw : 0.f;
    g[0] = (-g_wr * cr_share_max(a[0], b[0]) - g_cwr * cr_share_min(a[0], b[0])) - g_uni * ha;
    g[1] = (-g_hr * cr_share_max(a[1], b[1]) - g_chr * cr_share_min(a[1], b[1])) - g_uni * wa;
    g[2] = (g_wr * cr_share_min(a[2], b[2]) + g_cwr * cr_share_max(a[2], b[2])) + g_uni * ha;
    g[3] = (g_hr * cr_share_min(a[3], b[3]) + g_chr * cr_share_max(a[3], b[3])) + g_uni * wa;
}

// coef0 * d/dx of the element criterion_loss_kernel sums: ce * (1 - p_t)^gamma * alpha_t.  With q = 1 - p_t (1 - p on the one-hot
// element, p elsewhere): d/dx = +-alpha_t * q^gamma * (q + gamma * p_t * ce), minus on the one-hot element; k_hot = -coef0 * alpha_t of
// the one-hot element, k_cold = coef0 * alpha_t of the others.  p and 1 - p both come from e = exp(-|x|) -- sigmoid(|x|) = 1 / (1 + e),
// sigmoid(-|x|) = e / (1 + e) -- so neither is a difference of near-equal numbers, and log1p(e) = -log(sigmoid(|x|)).  The pass is
// paced by these operations, not by memory, so they are the hardware's: v_exp_f32, v_rcp_f32, v_log_f32 (1 ulp each; an error of 1e-7
// in ce moves the result by under 2e-8 * coef0, the q^gamma * p_t in front of it is at most 0.15).  gamma == 2 is a product, decided
// once per launch; any other gamma takes powf.
template <bool GAMMA2>
__device__ __forceinline__ float cr_focal_grad(float x, bool hot, float k_hot, float k_cold, float gamma) {
    const float e = __expf(-fabsf(x)), big = __builtin_amdgcn_rcpf(1.f + e), small = e * big;
    const bool up = hot == (x >= 0.f);          // the one-hot element of a positive logit, another element of a negative one: q is the small one
    const float q = up ? small : big, pt = up ? big : small;
    const float ce = (fmaxf(x, 0.f) - (hot ? x : 0.f)) - __logf(big);
    const float pw = GAMMA2 ? q * q : powf(q, gamma);
    return (hot ? k_hot : k_cold) * (pw * (q + (gamma * pt) * ce));
}

// One workgroup per chunk of CL_ROWS queries of one (head output, image), criterion_loss_kernel's decomposition.  The first `rows`
// threads write the rows' d_boxes and leave the one-hot class in LDS; then all threads walk the chunk's flat rows * C range: scalars up to
// the first 16-byte boundary, float4 from there, a scalar tail.  Every element of d_logits and d_boxes has exactly one writer.
template <bool GAMMA2>
__global__ __launch_bounds__(CL_THREADS) void criterion_grad_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, int n, int M, int C,
                                                                    const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                                    const int* __restrict__ gt_starts, const float* __restrict__ sizes, float alpha,
                                                                    float gamma, const int* __restrict__ assign, const int* __restrict__ status,
                                                                    const double* __restrict__ coef, float* __restrict__ d_logits,
                                                                    float* __restrict__ d_boxes) {
    __shared__ int s_cls[CL_ROWS];
    const int chunk = blockIdx.x, set = blockIdx.y, img = set % n, head = set / n, tid = threadIdx.x;
    const int r0 = chunk * CL_ROWS, rows = min(CL_ROWS, M - r0);
    const bool dead = (status[set] & (DVID_CRITERION_ERR_DEGENERATE | DVID_CRITERION_ERR_NONFINITE | DVID_CRITERION_ERR_LABEL)) != 0;          // uniform
    const float c0 = dead ? 0.f : (float)coef[head * 3], c1 = dead ? 0.f : (float)coef[head * 3 + 1], c2 = dead ? 0.f : (float)coef[head * 3 + 2];
    if (tid < rows) {
        const int g0 = gt_starts[img], G = max(gt_starts[img + 1] - g0, 0);
        const int a = dead ? -1 : assign[(size_t)set * M + r0 + tid];
        int cls = -1;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (a >= 0 && a < G) {
            cls = gt_labels[g0 + a] - 1;
            const float iw = sizes[2 * img], ih = sizes[2 * img + 1];
            const float* b = boxes + ((size_t)set * M + r0 + tid) * 4;
            const float* t = gt_boxes + (size_t)(g0 + a) * 4;
            const float4v q = {b[0], b[1], b[2], b[3]}, gt = {t[0], t[1], t[2], t[3]};
            if (c2 != 0.f) cr_giou_grad(q, gt, c2, g);
            if (c1 != 0.f) {          // the L1 target as criterion_loss_kernel forms it
                const float n0 = __fdiv_rn(gt[0], iw), n1 = __fdiv_rn(gt[1], ih), n2 = __fdiv_rn(gt[2], iw), n3 = __fdiv_rn(gt[3], ih);
                const float cx = __fdiv_rn(n0 + n2, 2.f), cy = __fdiv_rn(n1 + n3, 2.f), w = n2 - n0, h = n3 - n1;
                const float d0 = __fdiv_rn(q[0], iw) - (cx - 0.5f * w), d1 = __fdiv_rn(q[1], ih) - (cy - 0.5f * h);
                const float d2 = __fdiv_rn(q[2], iw) - (cx + 0.5f * w), d3 = __fdiv_rn(q[3], ih) - (cy + 0.5f * h);
                const float sw = __fdiv_rn(c1, iw), sh = __fdiv_rn(c1, ih);
                g[0] = g[0] + (d0 > 0.f ? sw : (d0 < 0.f ? -sw : 0.f)), g[1] = g[1] + (d1 > 0.f ? sh : (d1 < 0.f ? -sh : 0.f));
                g[2] = g[2] + (d2 > 0.f ? sw : (d2 < 0.f ? -sw : 0.f)), g[3] = g[3] + (d3 > 0.f ? sh : (d3 < 0.f ? -sh : 0.f));
            }
        }
        float* o = d_boxes + ((size_t)set * M + r0 + tid) * 4;
        o[0] = g[0], o[1] = g[1], o[2] = g[2], o[3] = g[3];
        s_cls[tid] = cls;
    }
    __syncthreads();
    const size_t base = ((size_t)set * M + r0) * C;
    const float* lg = logits + base;
    float* dl = d_logits + base;
    const int total = rows * C;
    // the float4 range: both pointers must reach a 16-byte boundary after the same number of elements (they do whenever the two tensors
    // start on one; a chunk starts r0 * C = a multiple of 4 elements into its set, but the set itself starts anywhere when M * C is odd)
    const unsigned in_mis = (unsigned)((uintptr_t)lg & 15), out_mis = (unsigned)((uintptr_t)dl & 15);
    const int lead = in_mis != out_mis ? total : min(total, (int)(((16u - in_mis) & 15u) >> 2));
    const int nvec = (total - lead) >> 2, tail0 = lead + 4 * nvec;
    if (c0 == 0.f) {          // uniform: exact zeros, and the logits are not read
        for (int e = tid; e < lead; e += CL_THREADS) dl[e] = 0.f;
        for (int v = tid; v < nvec; v += CL_THREADS) *reinterpret_cast<float4v*>(dl + lead + 4 * v) = (float4v){0.f, 0.f, 0.f, 0.f};
        for (int e = tail0 + tid; e < total; e += CL_THREADS) dl[e] = 0.f;
        return;
    }
    const unsigned inv = C > 1 ? 0xffffffffu / (unsigned)C + 1u : 0u;          // e / C = umulhi(e, inv): exact while e * C < 2^32 (e < 16 * 1280)
    const float k_hot = -(c0 * (alpha >= 0.f ? alpha : 1.f)), k_cold = c0 * (alpha >= 0.f ? 1.f - alpha : 1.f);
    for (int e = tid; e < lead; e += CL_THREADS) {          // (lead <= 3 on the float4 path, the whole chunk otherwise)
        const int r = C > 1 ? (int)__umulhi((unsigned)e, inv) : e;
        dl[e] = cr_focal_grad<GAMMA2>(lg[e], s_cls[r] == e - r * C, k_hot, k_cold, gamma);
    }
    // CG_DEPTH float4 loads of a thread are in flight before the first is used: at 16 rows x 1203 classes a workgroup makes 4.7 such rounds
    for (int v0 = tid; v0 < nvec; v0 += CG_DEPTH * CL_THREADS) {
        float4v x[CG_DEPTH];
#pragma unroll
        for (int k = 0; k < CG_DEPTH; ++k)
            if (v0 + k * CL_THREADS < nvec) x[k] = *reinterpret_cast<const float4v*>(lg + lead + 4 * (v0 + k * CL_THREADS));
#pragma unroll
        for (int k = 0; k < CG_DEPTH; ++k) {
            if (v0 + k * CL_THREADS >= nvec) break;
            const int e = lead + 4 * (v0 + k * CL_THREADS);
            int r = C > 1 ? (int)__umulhi((unsigned)e, inv) : e, c = e - r * C;
            float4v o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = cr_focal_grad<GAMMA2>(x[k][j], s_cls[r] == c, k_hot, k_cold, gamma);          // r < rows: the element lies inside the chunk
                if (++c == C) c = 0, ++r;
            }
            *reinterpret_cast<float4v*>(dl + e) = o;
        }
    }
    for (int e = tail0 + tid; e < total; e += CL_THREADS) {
        const int r = C > 1 ? (int)__umulhi((unsigned)e, inv) : e;
        dl[e] = cr_focal_grad<GAMMA2>(lg[e], s_cls[r] == e - r * C, k_hot, k_cold, gamma);
    }
}

int dvid_set_criterion_backward_launch(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes,
                                       const int* gt_labels, const int* gt_starts, const float* sizes, float alpha, float gamma, const int* assign,
                                       const int* status, const double* coef, float* d_logits, float* d_boxes, hipStream_t s) {
    if (n_sets < 0 || n < 0 || m < 1 || m > DVID_CRITERION_MAX_ROWS || c < 1 || c > DVID_MAX_CLASSES) return DVID_ERR_ARG;
    const long long sets = (long long)n_sets * n;
    if (sets == 0) return DVID_OK;
    if (sets > 65535) return DVID_ERR_ARG;          // grid y
    const dim3 grid((unsigned)ceil_div(m, CL_ROWS), (unsigned)sets);
    if (gamma == 2.f)
        hipLaunchKernelGGL(criterion_grad_kernel<true>, grid, dim3(CL_THREADS), 0, s, logits, boxes, n, m, c, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma,
                           assign, status, coef, d_logits, d_boxes);
    else
        hipLaunchKernelGGL(criterion_grad_kernel<false>, grid, dim3(CL_THREADS), 0, s, logits, boxes, n, m, c, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma,
                           assign, status, coef, d_logits, d_boxes);
    LAUNCH_CHECK();
    return DVID_OK;
}

static long long cr_align16(long long v) { return (v + 15) & ~15ll; }
static int cr_chunks(int m) { return ceil_div(m, CL_ROWS); }

long long dvid_set_criterion_scratch_bytes_host(int n_sets, int n, int m, int gmax) {
    if (n_sets < 0 || n < 0 || m < 1 || gmax < 0) return 0;
    const long long sets = (long long)n_sets * n;
    return cr_align16(sets * cr_chunks(m) * 4 * (long long)sizeof(double)) + cr_align16(sets * gmax * m * (long long)sizeof(float)) +
           cr_align16(sets * gmax * m);
}

int dvid_set_criterion_launch(const float* logits, const float* boxes, int n_sets, int n, int m, int c, const float* gt_boxes, const int* gt_labels,
                              const int* gt_starts, const float* sizes, float alpha, float gamma, int ota_k, float cost_class, float cost_bbox,
                              float cost_giou, int* assign, int* matched_query, int gmax, double* sums, int* status, void* scratch, hipStream_t s) {
    if (n_sets < 0 || n < 0 || m < 1 || m > DVID_CRITERION_MAX_ROWS || c < 1 || c > DVID_MAX_CLASSES || gmax < 0 || gmax > DVID_CRITERION_MAX_GT ||
        ota_k < 1 || ota_k > DVID_CRITERION_MAX_OTA_K || ota_k > m)
        return DVID_ERR_ARG;
    const long long sets = (long long)n_sets * n;
    if (sets == 0) return DVID_OK;
    if (sets > 65535) return DVID_ERR_ARG;          // grid y
    const int chunks = cr_chunks(m);
    char* base = reinterpret_cast<char*>(scratch);
    double* partial = reinterpret_cast<double*>(base);
    float* cost = reinterpret_cast<float*>(base + cr_align16(sets * chunks * 4 * (long long)sizeof(double)));
    unsigned char* match = reinterpret_cast<unsigned char*>(reinterpret_cast<char*>(cost) + cr_align16(sets * gmax * m * (long long)sizeof(float)));
    const CritParams p = {alpha, gamma, cost_class, cost_bbox, cost_giou, ota_k};
    hipLaunchKernelGGL(criterion_match_kernel, dim3((unsigned)sets), dim3(CM_THREADS), 0, s, logits, boxes, n, m, c, gt_boxes, gt_labels, gt_starts, sizes, p,
                       cost, match, gmax, assign, matched_query, status);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(criterion_loss_kernel, dim3((unsigned)chunks, (unsigned)sets), dim3(CL_THREADS), 0, s, logits, boxes, n, m, c, gt_boxes, gt_labels,
                       gt_starts, sizes, p, assign, partial, chunks, status);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(criterion_sum_kernel, dim3(ceil_div((int)sets * 4, 256)), dim3(256), 0, s, partial, (int)sets, chunks, sums);
    LAUNCH_CHECK();
    return DVID_OK;
}
