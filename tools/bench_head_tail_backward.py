"""Time ops.head_tail_backward (csrc/headtail_bwd.hip: the tail's fp32 recompute and its backward, one call) against torch's autograd
through tail.head_tail_host on the same GPU tensors (forward with the graph, then backward).  A record, not a gate:

    python tools/bench_head_tail_backward.py > profiles/head_tail_backward_bench.txt

Case one: 8 images x 500 boxes x 80 classes; case two: 8 x 300 x 1203; plain head, NUM_CLS 1, NUM_REG 3, hidden 256, dff 2048.  The FLOP
count is the one of the shapes: per box row the forward multiplies 2 x (2 x 256 x dff + 4 x 256 x 256 + 256 x (C + 4)) and the backward
twice that (a data and a weight gradient per product); the call is a recompute plus the backward, three times the forward.  The share of
the fp32 MFMA peak is that count over the time over 157.3 TFLOP/s (v_mfma_f32_32x32x2_f32: 256 FLOP per cycle and CU, 256 CUs, 2.4 GHz)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _head_tail_cases as HC  # noqa: E402
from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import tail as T  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    print("head tail backward: ops.head_tail_backward (fp32 recompute + backward, one call) against torch autograd through head_tail_host on the same "
          "GPU tensors (forward with the graph + backward); %s" % torch.cuda.get_device_name(0))
    for n, m, c in ((8, 500, 80), (8, 300, 1203)):
        case = HC.make_case(100 + c, n, m, c)
        dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in case.items() if k not in ("params", "cots")}
        params = {k: v.cuda() for k, v in case["params"].items()}
        cots = {k: v.cuda() for k, v in case["cots"].items() if v is not None}
        run = lambda: ops.head_tail_backward(dev["x"], dev["boxes_in"], dev["time_emb"], params, d_logits=cots["logits"], d_boxes=cots["boxes"])

        def autograd():
            x, te = dev["x"].clone().requires_grad_(True), dev["time_emb"].clone().requires_grad_(True)
            p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            lg, bx, _ = T.head_tail_host(x, dev["boxes_in"], te, p)
            ((cots["logits"] * lg).sum() + (cots["boxes"] * bx).sum()).backward()
            return x.grad, p

        ours, (gx, gp) = run(), autograd()
        agree = max(HC.deviation(ours["d_x"], gx), HC.deviation(ours["param_grads"]["linear1.weight"], gp["linear1.weight"].grad))
        R = n * m
        flop = 3.0 * R * 2 * (2 * 256 * 2048 + 4 * 256 * 256 + 256 * (c + 4))
        t_ours, t_auto = timed(run, 10), timed(autograd, 5)
        print("%d x %d x %-5d %6.1f GFLOP  head_tail_backward %8.3f ms per call (%5.1f TFLOP/s, %4.1f %% of the fp32 MFMA peak)  autograd forward + backward "
              "%8.3f ms  x%.2f  d_x / d linear1.weight agree to %.1e of their largest" % (n, m, c, flop / 1e9, t_ours, flop / t_ours / 1e9,
                                                                                        100 * flop / t_ours / 1e9 / PEAK_TFLOPS, t_auto, t_auto / t_ours, agree))


if __name__ == "__main__":
    main()
