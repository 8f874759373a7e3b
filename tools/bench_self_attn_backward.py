"""Time ops.self_attn_backward (csrc/selfattn_bwd.hip: the fp32 recompute of self-attention + norm1 and its backward, one call) against
torch's autograd through attention.self_attention_host on the same GPU tensors (forward with the graph, then backward), and the whole
DiffusionDet.head_gradients call against autograd through the host composition of all heads.  A record, not a gate:

    python tools/bench_self_attn_backward.py > profiles/self_attn_backward_bench.txt

The times are device times from torch.profiler (the sum of the kernels' own times over the repetitions, so launch gaps and the host are
left out) with the wall time of the synchronised loop beside them.  First lines: 8 images x 500 rows and 8 x 300, hidden 256, 8 heads.
The FLOP count is the one of the shapes: per row the forward multiplies 768 x 256 (in_proj) + 256 x 256 (out_proj) + 2 x m x 256 (q k^T and
P v over the image's m rows); the call is a recompute plus a backward of twice the forward, three times the forward in all.  The kernels
form S three more times than that count (once more in the forward for the statistics, once in each backward pass): the price of never
storing P.  The share of the fp32 MFMA peak is that count over the device time over 157.3 TFLOP/s.  Last line: head_gradients on a
DTYPE float32 model with one bottleneck per ResNet stage, six heads, 8 images x 500 boxes -- the forward, the criterion and the chain --
against autograd (forward with the graph + backward) through _self_attn_cases.chain_host on the call's kept tiles and boxes."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _self_attn_cases as SC  # noqa: E402
from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import attention as A  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(fn, reps):
    """-> (device ms per call from torch.profiler, wall ms per call)"""
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps * 1e3
    device = sum(getattr(e, "self_device_time_total", getattr(e, "self_cuda_time_total", 0)) for e in prof.key_averages())
    return device / reps / 1e3, wall


def link():
    params = {k: v.cuda() for k, v in SC.link_params(3).items()}
    for n, m in ((8, 500), (8, 300)):
        R = n * m
        g = torch.Generator().manual_seed(R)
        x = torch.nn.functional.layer_norm(torch.randn(R, 256, generator=g), (256,)).cuda()
        d_y = (torch.randn(R, 256, generator=g) / 16).cuda()
        run = lambda: ops.self_attn_backward(x, n, params, d_y=d_y)

        def autograd():
            xl = x.clone().requires_grad_(True)
            w = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            (d_y * A.self_attention_host(xl, n, w)).sum().backward()
            return xl.grad, w

        ours, (gx, gw) = run(), autograd()
        k = "self_attn.in_proj_weight"
        agree = max(SC.deviation(ours["d_x"], gx), SC.deviation(ours["param_grads"][k], gw[k].grad))
        flop = 2.0 * R * 3 * (768 * 256 + 256 * 256 + 2 * m * 256)
        (d_ours, w_ours), (d_auto, w_auto) = timed(run, 10), timed(autograd, 10)
        print("%d x %-4d %6.2f GFLOP  self_attn_backward %8.3f ms device (%5.1f TFLOP/s, %4.1f %% of the fp32 MFMA peak), %8.3f ms wall  scratch %5.1f MB  "
              "autograd forward + backward %8.3f ms device, %8.3f ms wall  x%.2f device  d_x / d in_proj_weight agree to %.1e of their largest"
              % (n, m, flop / 1e9, d_ours, flop / d_ours / 1e9, 100 * flop / d_ours / 1e9 / PEAK_TFLOPS, w_ours, ops.self_attn_backward_scratch_bytes(n, m) / 1e6,
                 d_auto, w_auto, d_auto / d_ours, agree))


def whole(n=8, boxes=500, heads=6):
    import test_gpu_e2e as E
    from test_gpu_head_tail_e2e import BLOCKS, SMALL
    from diffusionvid_amd.structures.bounding_box import BoxList
    from diffusionvid_amd.utils import synthetic
    extra = SMALL + ["MODEL.DiffusionDet.NUM_HEADS", heads, "MODEL.DiffusionDet.NUM_PROPOSALS", boxes, "MODEL.DiffusionDet.DEEP_SUPERVISION", True]
    _, model = E._build(1, BLOCKS, "trained_like", extra=extra, dtype="float32")
    model.noise_fn = synthetic.noise_fn
    images, targets, ids = [], [], list(range(100, 100 + n))
    for i in range(n):
        h, w = (128, 160) if i % 2 else (160, 128)
        images.append(synthetic.synthetic_frame(70 + i, h, w, smooth=True))
        t = BoxList(torch.tensor([[10.0 + i, 12.0, 70.0 + 5 * i, 90.0], [40.0, 30.0 + 2 * i, 110.0, 120.0]]), (w, h), mode="xyxy")
        t.add_field("labels", torch.tensor([1 + i, 20 - i], dtype=torch.int64))
        targets.append(t)
    run = lambda: model.head_gradients(images, targets, ids, roi_gradients=True)
    out = run()
    R = n * boxes
    sd = model.state_dict()
    pfx = ("head.head_series.", "head.time_mlp.")
    time_emb = model.objective.time_embedding(torch.tensor([model.objective.train_step(i) for i in ids], dtype=torch.int64))

    def autograd():
        w = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pfx)}
        per = [{k.split(".", 3)[3]: v for k, v in w.items() if k.startswith("head.head_series.%d." % h)} for h in range(heads)]
        tiles = [out["roi_tiles"][h].clone().requires_grad_(True) for h in range(heads)]
        logits, bxs = SC.chain_host(tiles, out["boxes_in"][0], time_emb, per, heads, boxes_in=[out["boxes_in"][h].reshape(R, 4) for h in range(heads)])
        sum((out["d_logits"][h].reshape(R, -1) * logits[h]).sum() + (out["d_boxes"][h].reshape(R, 4) * bxs[h]).sum() for h in range(heads)).backward()
        return w

    k = "head.head_series.0.self_attn.in_proj_weight"
    agree = SC.deviation(out["param_grads"][k], autograd()[k].grad)
    (d_ours, w_ours), (d_auto, w_auto) = timed(run, 3), timed(autograd, 3)
    print("head_gradients %d x %d, %d heads (forward + criterion + the chain over all heads, roi_gradients=True) %9.3f ms device, %9.3f ms wall;  autograd "
          "through the host composition of the heads alone (time_mlp held fixed; not kept off the ReLU kinks) %9.3f ms device, %9.3f ms wall;  d head 0 in_proj_weight "
          "agree to %.1e of its largest" % (n, boxes, heads, d_ours, w_ours, d_auto, w_auto, agree))


def main():
    print("self-attention backward: ops.self_attn_backward (fp32 recompute + backward, one call) against torch autograd through self_attention_host on "
          "the same GPU tensors (forward with the graph + backward); %s" % torch.cuda.get_device_name(0))
    link()
    whole()


if __name__ == "__main__":
    main()
