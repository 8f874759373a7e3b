"""Time ops.inst_interact_backward (csrc/interact_bwd.hip: the fp32 recompute of DynamicConv + norm2 and its backward, one call) against
torch's autograd through interact.inst_interact_host on the same GPU tensors (forward with the graph, then backward).  A record, not a gate:

    python tools/bench_inst_interact_backward.py > profiles/inst_interact_backward_bench.txt

8 images x 500 boxes and 8 x 300, hidden 256, dim_dynamic 64, 7 x 7 bins.  The FLOP count is the one of the shapes: per box the forward
multiplies 256 x 32768 (dynamic_layer) + 2 x 49 x 256 x 64 (the two bmm's) + 12544 x 256 (out_layer) = 13.2 MMAC, and the backward twice that (a data and a
weight gradient per product); the call is a recompute plus the backward, three times the forward: about 79 MFLOP per box (the second
recompute of params and the bmm's in front of each slab's backward is not counted: it is the price of the bounded scratch).  The share of the fp32 MFMA peak is that count over the time over 157.3 TFLOP/s."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _inst_interact_cases as IC  # noqa: E402
from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import interact as I  # noqa: E402

PEAK_TFLOPS = 157.3
MMAC_FORWARD = (256 * 32768 + 2 * 49 * 256 * 64 + 12544 * 256) / 1e6


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    print("instance interaction backward: ops.inst_interact_backward (fp32 recompute + backward, one call) against torch autograd through "
          "inst_interact_host on the same GPU tensors (forward with the graph + backward); the rows are NOT kept off the ReLU kinks as the tests' are, so the two agree only as far "
          "as no unit changes side; %s" % torch.cuda.get_device_name(0))
    params = {k: v.cuda() for k, v in IC.link_params(3).items()}
    for n, m in ((8, 500), (8, 300)):
        R = n * m
        g = torch.Generator().manual_seed(R)
        p = torch.nn.functional.layer_norm(torch.randn(R, 256, generator=g), (256,)).cuda()
        roi = (0.5 * torch.randn(R, 49, 256, generator=g)).cuda()
        d_y = (torch.randn(R, 256, generator=g) / 16).cuda()
        run = lambda: ops.inst_interact_backward(p, roi, params, d_y=d_y)

        def autograd():
            pl, rl = p.clone().requires_grad_(True), roi.clone().requires_grad_(True)
            w = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            (d_y * I.inst_interact_host(pl, rl, w)).sum().backward()
            return pl.grad, w

        ours, (gp, gw) = run(), autograd()
        k = "inst_interact.dynamic_layer.weight"
        agree = max(IC.deviation(ours["d_p"], gp), IC.deviation(ours["param_grads"][k], gw[k].grad))
        flop = 2e6 * R * 3 * MMAC_FORWARD
        t_ours, t_auto = timed(run, 5), timed(autograd, 3)
        print("%d x %-4d %7.1f GFLOP  inst_interact_backward %9.3f ms per call (%5.1f TFLOP/s, %4.1f %% of the fp32 MFMA peak)  scratch %6.1f MB  autograd "
              "forward + backward %9.3f ms  x%.2f  d_p / d dynamic_layer.weight agree to %.1e of their largest"
              % (n, m, flop / 1e9, t_ours, flop / t_ours / 1e9, 100 * flop / t_ours / 1e9 / PEAK_TFLOPS, ops.inst_interact_backward_scratch_bytes(R) / 1e6,
                 t_auto, t_auto / t_ours, agree))


if __name__ == "__main__":
    main()
