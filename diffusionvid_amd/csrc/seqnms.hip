// Seq-NMS over a video's detections (TEST.SEQ_NMS; the reference's seq_nms.py: createLinks / maxPath / findMaxPath / rescore /
// deleteLink), one workgroup per (video, class), classes independent of each other.
//
//   links     box i of frame f -> box j of frame f + 1 (same class) when their IoU (+ 1 extents) is >= 0.5, on the boxes present at the
//             start: bit rows [n_f][ceil(n_{f+1} / 64)] in the scratch
//   a round   a[f][j] = score (0 for a box that has been on a path) improved through the links by a[f-1][i] + score[j] where that is
//             strictly greater, the lowest i first; argmax over (frame, box) in row-major first-occurrence order; backtrack; stop when the
//             sum is below 1e-2 or no link is left; the path's boxes get sum / length; in every frame of the path the boxes whose IoU
//             with the path's box is >= 0.3 (the path's box among them) lose their links, and all of them but the path's box are zeroed
//             (box and score) and dropped at the end
//
// Arithmetic: seq_nms.py computes the IoU terms and the running sums in float32 and sum / length as a float64 quotient stored to
// float32, which is the correctly rounded float32 quotient.  Every expression below that feeds a comparison or a stored score is
// therefore float32 with contraction off (`#pragma clang fp contract(off)`: no a * b + c becomes one fma) and its division is
// __fdiv_rn, the IEEE one; the result is the reference's bit for bit.  `sum < 1e-2` is a float64 comparison there (numpy's table is
// float64, the threshold a Python float), so it is one here.
//
// Frames are sequential in the sweep (one barrier per frame), the boxes of a frame parallel; after a path rooted at frame r is removed
// a[f] for f < r is unchanged, so the next sweep starts at r and the per-frame maxima before r are kept.  The tables live in the
// scratch, not in LDS (a VID-val video runs to ~2900 frames).  The round loop is bounded by the class's box count + 1: every round
// takes at least one box out of play, so reaching the bound is a logic error and ends as DVID_SEQ_NMS_ERR_ROUNDS in the status word.
#include <string.h>

#include <vector>

#include "../../include/dvid_hip.h"
#include "kernels.h"

typedef unsigned long long u64;

#define SEQ_THREADS 256
#define SEQ_WAVES (SEQ_THREADS / WAVE)
#define SEQ_ON_PATH 1
#define SEQ_DELETED 2

// one per (video, class) at the head of the scratch, written by the host
struct SeqNmsClass {
    long long plan_off;          // bytes from the scratch base: box_off[frames + 1], link_off[frames + 1], mask_off[frames + 1] (uint32); < 0: nothing to do
    long long work_off;          // bytes from the scratch base: the working arrays, see seq_nms_work_bytes
    int frame0, frames, boxes, pad;
    unsigned long long link_words;
};

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
static size_t seq_nms_plan_bytes(int frames) { return align16((size_t)3 * (frames + 1) * 4); }
// box f32[4N] | links u64[L] | dmask u64[M] | score f32[N] | a f32[N] | bp i32[N] | idx i32[N] | state i32[N] | fmax f32[F] | farg i32[F] | path i32[F]
static size_t seq_nms_work_bytes(int frames, size_t boxes, size_t link_words, size_t mask_words) {
    return align16(boxes * 16 + (link_words + mask_words) * 8 + boxes * 20 + (size_t)frames * 12);
}

// IoU of seq_nms.py:55-76 / :188-199: (x2 - x1 + 1) * (y2 - y1 + 1) areas, max(0, .) extents, inter / (area1 + area2 - inter)
__device__ __forceinline__ float seq_area(const float4v b) {
#pragma clang fp contract(off)
    const float w = (b[2] - b[0]) + 1.f, h = (b[3] - b[1]) + 1.f;
    return w * h;
}
__device__ __forceinline__ float seq_iou(const float4v p, const float pa, const float4v q) {
#pragma clang fp contract(off)
    const float x1 = fmaxf(p[0], q[0]), y1 = fmaxf(p[1], q[1]), x2 = fminf(p[2], q[2]), y2 = fminf(p[3], q[3]);
    const float w = fmaxf(0.f, (x2 - x1) + 1.f), h = fmaxf(0.f, (y2 - y1) + 1.f);
    const float inter = w * h;
    const float qa = seq_area(q);
    return __fdiv_rn(inter, (pa + qa) - inter);
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int lane) {
    const unsigned lo = __shfl((unsigned)v, lane, 64), hi = __shfl((unsigned)(v >> 32), lane, 64);
    return ((u64)hi << 32) | lo;
}

// keep = 1 and the input score for every row in front of counts[f]; the class workgroups overwrite the rows they own
__global__ void seq_nms_init_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int cap, long total, unsigned char* __restrict__ keep,
                                    float* __restrict__ scores) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long f = i / cap;
    const int r = (int)(i - f * cap);
    const bool live = r < counts[f];
    keep[i] = live ? 1 : 0;
    scores[i] = live ? dets[i * 6 + 4] : 0.f;
}

__global__ __launch_bounds__(SEQ_THREADS) void seq_nms_class_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int cap, int num_classes,
                                                                    char* __restrict__ scratch, unsigned char* __restrict__ keep,
                                                                    float* __restrict__ scores, int* __restrict__ status) {
    const SeqNmsClass hd = reinterpret_cast<const SeqNmsClass*>(scratch)[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (hd.plan_off < 0) {
        if (tid == 0) status[blockIdx.x] = 0;
        return;
    }
    const int label = (int)(blockIdx.x % num_classes) + 1;
    const int F = hd.frames, N = hd.boxes;
    const unsigned* box_off = reinterpret_cast<const unsigned*>(scratch + hd.plan_off);
    const unsigned* link_off = box_off + (F + 1);
    const unsigned* mask_off = link_off + (F + 1);
    float4v* box = reinterpret_cast<float4v*>(scratch + hd.work_off);
    u64* links = reinterpret_cast<u64*>(box + N);
    u64* dmask = links + hd.link_words;
    float* score = reinterpret_cast<float*>(dmask + mask_off[F]);
    float* a = score + N;
    int* bp = reinterpret_cast<int*>(a + N);
    int* idx = bp + N;
    int* state = idx + N;
    float* fmax = reinterpret_cast<float*>(state + N);
    int* farg = reinterpret_cast<int*>(fmax + F);
    int* path = farg + F;

    __shared__ int s_bad, s_links, s_removed, s_root, s_len, s_stop;
    __shared__ float s_sum;
    __shared__ float s_rv[SEQ_WAVES];
    __shared__ int s_rf[SEQ_WAVES];
    if (tid == 0) s_bad = 0, s_links = 0;
    __syncthreads();

    // ---- the class's boxes, in their order within the frame (a wave per frame) ----
    for (int f = wave; f < F; f += SEQ_WAVES) {
        const long fr = (long)hd.frame0 + f;
        const int cnt = min(counts[fr], cap), nf = (int)(box_off[f + 1] - box_off[f]);
        const float* d = dets + fr * cap * 6;
        int seen = 0;
        for (int r0 = 0; r0 < cnt; r0 += WAVE) {
            const int r = r0 + lane;
            const bool mine = r < cnt && (int)d[(long)r * 6 + 5] == label;
            const u64 m = __ballot(mine);
            const int k = seen + __popcll(m & (((u64)1 << lane) - 1));
            if (mine && k < nf) {
                const unsigned o = box_off[f] + k;
                box[o] = (float4v){d[(long)r * 6], d[(long)r * 6 + 1], d[(long)r * 6 + 2], d[(long)r * 6 + 3]};
                score[o] = d[(long)r * 6 + 4];
                idx[o] = r;
                state[o] = 0;
            }
            seen += __popcll(m);
        }
        if (seen != nf && lane == 0) s_bad = 1;          // the host's table of per-(frame, class) counts does not describe `dets`
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) status[blockIdx.x] = DVID_SEQ_NMS_ERR_COUNTS;
        return;
    }

    // ---- links: row i of frame f, one 64-bit word per wave step ----
    {
        int made = 0;
        for (int f = 0; f + 1 < F; ++f) {
            const int n1 = (int)(box_off[f + 1] - box_off[f]), n2 = (int)(box_off[f + 2] - box_off[f + 1]), W = (n2 + 63) >> 6;
            for (int it = wave; it < n1 * W; it += SEQ_WAVES) {
                const int i = it / W, w = it - i * W, j = w * 64 + lane;
                const float4v p = box[box_off[f] + i];
                bool on = false;
                if (j < n2) on = seq_iou(p, seq_area(p), box[box_off[f + 1] + j]) >= 0.5f;
                const u64 m = __ballot(on);
                if (lane == 0) links[link_off[f] + it] = m, made += __popcll(m);
            }
        }
        if (lane == 0 && made) atomicAdd(&s_links, made);
    }
    __syncthreads();

    int rounds = 0, err = 0, start = 0;
    for (;; ++rounds) {
        if (rounds > N) {          // cannot happen: a round takes at least the path's own boxes out of play
            err = DVID_SEQ_NMS_ERR_ROUNDS;
            break;
        }
        // ---- the sweep, from the frame the last path was rooted at ----
        for (int f = start; f < F; ++f) {
            const int n = (int)(box_off[f + 1] - box_off[f]);
            const int np = f ? (int)(box_off[f] - box_off[f - 1]) : 0, W = (n + 63) >> 6;
            for (int jb = wave * WAVE; jb < n; jb += SEQ_THREADS) {
                const int j = jb + lane, w = jb >> 6;
                const bool live = j < n;
                const float s = live ? score[box_off[f] + j] : 0.f;
                float best = live && !(state[box_off[f] + j] & SEQ_ON_PATH) ? s : 0.f;
                int from = -1;
                for (int ib = 0; ib < np; ib += WAVE) {          // 64 rows of the previous frame at a time: lane l holds row ib + l's word and sum
                    const bool has = ib + lane < np;
                    const u64 word = has ? links[link_off[f - 1] + (size_t)(ib + lane) * W + w] : 0;
                    const float prev = has ? a[box_off[f - 1] + ib + lane] : 0.f;
                    u64 rows = __ballot(word != 0);
                    while (rows) {          // ascending i: on a tie the lowest predecessor stays
                        const int l = __ffsll((long long)rows) - 1;
                        rows &= rows - 1;
                        const u64 wd = shfl_u64(word, l);
                        const float cand = __shfl(prev, l, 64) + s;
                        if (((wd >> lane) & 1) && cand > best) best = cand, from = ib + l;
                    }
                }
                if (live) a[box_off[f] + j] = best, bp[box_off[f] + j] = from;
            }
            __syncthreads();
        }
        // ---- per-frame maxima (first occurrence), a wave per frame ----
        for (int f = start + wave; f < F; f += SEQ_WAVES) {
            const int n = (int)(box_off[f + 1] - box_off[f]);
            float v = -INFINITY;
            int at = 0x7fffffff;
            for (int j = lane; j < n; j += WAVE) {
                const float x = a[box_off[f] + j];
                if (x > v) v = x, at = j;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(v, o, 64);
                const int oa = __shfl_xor(at, o, 64);
                if (ov > v || (ov == v && oa < at)) v = ov, at = oa;
            }
            if (lane == 0) fmax[f] = v, farg[f] = at;
        }
        __syncthreads();
        // ---- the argmax over frames (lowest frame on a tie) and the backtrack ----
        {
            float v = -INFINITY;
            int at = 0x7fffffff;
            for (int f = tid; f < F; f += SEQ_THREADS) {
                const float x = fmax[f];
                if (x > v) v = x, at = f;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(v, o, 64);
                const int oa = __shfl_xor(at, o, 64);
                if (ov > v || (ov == v && oa < at)) v = ov, at = oa;
            }
            if (lane == 0) s_rv[wave] = v, s_rf[wave] = at;
            __syncthreads();
            if (tid == 0) {
                for (int k = 1; k < SEQ_WAVES; ++k)
                    if (s_rv[k] > v || (s_rv[k] == v && s_rf[k] < at)) v = s_rv[k], at = s_rf[k];
                // seq_nms.py:106: maxsum < MAX_THRESH (float64) or sum_links == 0; a class without a positive entry ends here too
                const bool stop = !(v > 0.f) || (double)v < 1e-2 || s_links <= 0 || at >= F;
                s_stop = stop;
                if (!stop) {
                    int f = at, j = farg[f], len = 1;
                    path[f] = j;
                    while (f > 0 && len <= F) {
                        const int i = bp[box_off[f] + j];
                        if (i < 0) break;
                        --f, j = i, ++len;
                        path[f] = j;
                    }
                    s_root = f, s_len = len, s_sum = v, s_removed = 0;
                }
            }
            __syncthreads();
        }
        if (s_stop) break;
        const int root = s_root, len = s_len;
        float fresh;
        {
#pragma clang fp contract(off)
            fresh = __fdiv_rn(s_sum, (float)len);
        }
        // ---- deleteLink, step 1: the boxes of each path frame within IoU 0.3 of the path's box, as a bit row (boxes as they are now) ----
        for (int t = wave; t < len; t += SEQ_WAVES) {
            const int f = root + t, n = (int)(box_off[f + 1] - box_off[f]);
            const float4v p = box[box_off[f] + path[f]];
            const float pa = seq_area(p);
            for (int w = 0; w * 64 < n; ++w) {
                const int k = w * 64 + lane;
                const bool del = k < n && seq_iou(p, pa, box[box_off[f] + k]) >= 0.3f;
                const u64 m = __ballot(del);
                if (lane == 0) dmask[mask_off[f] + w] = m;
            }
        }
        __syncthreads();
        // ---- step 2: their outgoing links go; all of them but the path's box are zeroed; the path's box is rescored ----
        int gone = 0;
        for (int t = wave; t < len; t += SEQ_WAVES) {
            const int f = root + t, n = (int)(box_off[f + 1] - box_off[f]), p = path[f];
            const int W = f + 1 < F ? ((int)(box_off[f + 2] - box_off[f + 1]) + 63) >> 6 : 0;
            for (int k = lane; k < n; k += WAVE) {
                if (!((dmask[mask_off[f] + (k >> 6)] >> (k & 63)) & 1) && k != p) continue;
                const unsigned o = box_off[f] + k;
                if (k == p) {
                    score[o] = fresh;
                    state[o] |= SEQ_ON_PATH;
                } else {
                    box[o] = (float4v){0.f, 0.f, 0.f, 0.f};
                    score[o] = 0.f;
                    state[o] |= SEQ_DELETED;
                }
                for (int w = 0; w < W; ++w) {
                    u64* row = links + link_off[f] + (size_t)k * W + w;
                    gone += __popcll(*row);
                    *row = 0;
                }
            }
        }
        __syncthreads();
        // ---- step 3: the links that point at them go ----
        for (int t = wave; t < len; t += SEQ_WAVES) {
            const int f = root + t;
            if (f == 0) continue;
            const int np = (int)(box_off[f] - box_off[f - 1]), W = ((int)(box_off[f + 1] - box_off[f]) + 63) >> 6;
            for (int e = lane; e < np * W; e += WAVE) {
                u64* row = links + link_off[f - 1] + e;
                const u64 m = dmask[mask_off[f] + e % W], old = *row;
                if (old & m) {
                    gone += __popcll(old & m);
                    *row = old & ~m;
                }
            }
        }
        if (gone) atomicAdd(&s_removed, gone);
        __syncthreads();
        if (tid == 0) s_links -= s_removed;
        start = root;
        __syncthreads();
    }

    // ---- results, at the rows the boxes came from ----
    if (!err)
        for (int f = wave; f < F; f += SEQ_WAVES) {
            const long base = ((long)hd.frame0 + f) * cap;
            for (unsigned o = box_off[f] + lane; o < box_off[f + 1]; o += WAVE) {
                const bool dead = state[o] & SEQ_DELETED;
                keep[base + idx[o]] = dead ? 0 : 1;
                scores[base + idx[o]] = dead ? 0.f : score[o];
            }
        }
    if (tid == 0) status[blockIdx.x] = err ? err : rounds;
}

// ---- host: the plan (per class the offsets of its frames' boxes, link rows and mask words) and the scratch size ----
// class_counts [frames of all videos][num_classes] (host): boxes of label c + 1 in the frame.  Returns the scratch bytes, 0 where no
// class has work, -1 for bad arguments; with `image` the plan (headers + offset tables) is written there.
static long long seq_nms_plan(const int* class_counts, const int* video_starts, int n_videos, int num_classes, std::vector<char>* image) {
    if (!class_counts || !video_starts || n_videos < 1 || num_classes < 1) return -1;
    const size_t heads = align16((size_t)n_videos * num_classes * sizeof(SeqNmsClass));
    size_t plan = heads, work = 0;
    std::vector<SeqNmsClass> hd((size_t)n_videos * num_classes);
    bool any = false;
    for (int pass = 0; pass < 2; ++pass) {          // 0: sizes; 1: offsets behind the whole plan, and the tables
        size_t plan_at = heads, work_at = plan;
        if (pass && image) image->assign(plan, 0);
        for (int v = 0; v < n_videos; ++v) {
            const int f0 = video_starts[v], F = video_starts[v + 1] - f0;
            if (f0 < 0 || F < 0) return -1;
            for (int c = 0; c < num_classes; ++c) {
                SeqNmsClass& h = hd[(size_t)v * num_classes + c];
                size_t boxes = 0, lw = 0, mw = 0;
                for (int f = 0; f < F; ++f) {
                    const int n = class_counts[(size_t)(f0 + f) * num_classes + c];
                    if (n < 0) return -1;
                    boxes += n;
                    mw += (n + 63) / 64;
                    if (f + 1 < F) lw += (size_t)n * ((class_counts[(size_t)(f0 + f + 1) * num_classes + c] + 63) / 64);
                }
                h = SeqNmsClass{-1, 0, f0, F, (int)boxes, 0, lw};
                if (F < 2 || lw == 0) continue;          // one frame, or no box next to another frame's: no link can exist, the input stands
                any = true;
                const size_t pb = seq_nms_plan_bytes(F), wb = seq_nms_work_bytes(F, boxes, lw, mw);
                if (pass) {
                    h.plan_off = (long long)plan_at, h.work_off = (long long)work_at;
                    if (image) {
                        unsigned* t = reinterpret_cast<unsigned*>(image->data() + plan_at);
                        unsigned b = 0, l = 0, m = 0;
                        for (int f = 0; f <= F; ++f) {
                            t[f] = b, t[F + 1 + f] = l, t[2 * (F + 1) + f] = m;
                            if (f == F) break;
                            const int n = class_counts[(size_t)(f0 + f) * num_classes + c];
                            b += n, m += (n + 63) / 64;
                            if (f + 1 < F) l += (unsigned)n * ((class_counts[(size_t)(f0 + f + 1) * num_classes + c] + 63) / 64);
                        }
                    }
                }
                plan_at += pb, work_at += wb;
                if (!pass) plan += pb, work += wb;
            }
        }
    }
    if (!any) return 0;
    if (image) memcpy(image->data(), hd.data(), hd.size() * sizeof(SeqNmsClass));
    return (long long)(plan + work);
}

long long dvid_seq_nms_scratch_size(const int* class_counts, const int* video_starts, int n_videos, int num_classes) {
    return seq_nms_plan(class_counts, video_starts, n_videos, num_classes, nullptr);
}

int dvid_seq_nms_launch(const float* dets, const int* counts, const int* class_counts, const int* video_starts, int n_videos, int cap, int num_classes,
                        unsigned char* keep, float* scores, int* status, void* scratch, hipStream_t s) {
    std::vector<char> image;
    const long long bytes = seq_nms_plan(class_counts, video_starts, n_videos, num_classes, nullptr);
    if (bytes < 0) return DVID_ERR_ARG;
    if (bytes > DVID_SEQ_NMS_MAX_SCRATCH_BYTES) return DVID_ERR_UNSUPPORTED;          // the 32-bit offsets of the plan hold below this
    if (bytes > 0) seq_nms_plan(class_counts, video_starts, n_videos, num_classes, &image);
    const long total = (long)video_starts[n_videos] * cap;
    if (total > 0) {
        hipLaunchKernelGGL(seq_nms_init_kernel, dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, s, dets, counts, cap, total, keep, scores);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipMemsetAsync(status, 0, (size_t)n_videos * num_classes * sizeof(int), s));
    if (bytes == 0) return DVID_OK;
    if (!scratch) return DVID_ERR_ARG;
    // the plan goes up before the launch and `image` dies with this call: wait for the copy
    HIP_TRY(hipMemcpyAsync(scratch, image.data(), image.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    hipLaunchKernelGGL(seq_nms_class_kernel, dim3((unsigned)(n_videos * num_classes)), dim3(SEQ_THREADS), 0, s, dets, counts, cap, num_classes,
                       reinterpret_cast<char*>(scratch), keep, scores, status);
    LAUNCH_CHECK();
    return DVID_OK;
}
