"""Time ops.set_criterion (csrc/criterion.hip) against the host restatement's torch code run on the same GPU tensors -- the per-image
loop of modeling/roi_heads/box_head/loss.py (match_image + the loss terms), no kernel of ours -- and report the matcher and the loss-sum
kernels separately (torch.profiler's device times per kernel name).  A record, not a gate:

    python tools/bench_criterion.py > profiles/criterion_bench.txt

    python tools/bench_criterion.py --backward > profiles/criterion_backward_bench.txt

--backward times the gradient instead: ops.set_criterion_backward (one launch for all head outputs) against torch's autograd through the
same per-image loop -- the loop run once on inputs that require grad (the matcher on detached tensors, as the reference runs it), then
`.backward()` of the weighted reference losses timed on the retained graph.  Beside each time: the bytes the gradient has to move (logits
read, d_logits written, boxes, d_boxes, assign) and the rate they amount to.

Case one: 8 images x 6 head outputs x 500 boxes x 80 classes; case two: 8 x 6 x 300 x 1203; 7 ground-truth boxes per image."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _criterion_cases as CC  # noqa: E402
from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import loss as L  # noqa: E402


def torch_loop(logits, boxes, gt, lab, starts, sizes):
    """the restatement's own torch code on device tensors, set by set (what a port of the reference's criterion to this GPU would run)"""
    S, n = logits.shape[:2]
    total = torch.zeros((S, 4), dtype=torch.float64, device=logits.device)
    idx = torch.arange(logits.shape[2], device=logits.device)
    for i in range(n):
        g, l0 = gt[starts[i]:starts[i + 1]], lab[starts[i]:starts[i + 1]].long() - 1
        whwh = torch.stack((sizes[i, 0], sizes[i, 1], sizes[i, 0], sizes[i, 1]))
        for s in range(S):
            a, _, _ = _match_on_device(logits[s, i].detach(), boxes[s, i].detach(), g, l0, whwh, idx)
            rows = torch.nonzero(a >= 0)[:, 0]
            onehot = torch.zeros_like(logits[s, i])
            onehot[rows, l0[a[rows]]] = 1
            d = (boxes[s, i][rows] / whwh - g[a[rows]] / whwh).abs().sum(1)
            giou = torch.diagonal(L._giou_pairs(boxes[s, i][rows], g[a[rows]])[0])
            total[s] += torch.stack((L.focal_terms(logits[s, i], onehot, CC.ALPHA, CC.GAMMA).double().sum(), d.double().sum(), (1 - giou).double().sum(),
                                     torch.tensor(float(rows.numel()), dtype=torch.float64, device=d.device)))
    return total


def _match_on_device(lg, bx, g, l0, whwh, idx):
    # match_image builds its index tensors on the CPU; on device tensors the same code runs with torch's default-device context
    with torch.device(lg.device):
        return L.match_image(lg, bx, g, l0, whwh, CC.ALPHA, CC.GAMMA, CC.OTA_K, CC.W_CLASS, CC.W_L1, CC.W_GIOU)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def kernel_times(fn, reps=20, names=("criterion_match_kernel", "criterion_loss_kernel", "criterion_sum_kernel")):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        for name in names:
            if name in e.key:
                out[name] = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / reps / 1e3
    return out


def backward_main():
    """the gradient launch against autograd's backward pass through the per-image loop"""
    print("set criterion gradient: ops.set_criterion_backward against torch autograd's backward through the per-image loop on the same GPU tensors "
          "(%s)" % torch.cuda.get_device_name(0))
    w = torch.tensor([CC.W_CLASS, CC.W_L1, CC.W_GIOU], dtype=torch.float64, device="cuda")
    for name, (n, S, M, C) in (("8 x 6 x 500 x 80", (8, 6, 500, 80)), ("8 x 6 x 300 x 1203", (8, 6, 300, 1203))):
        logits, boxes, gt, lab, starts, sizes = CC.random_set(100 + C, S, M, C, [7] * n, sizes=[(1333, 800)] * n)
        dev = [t.cuda() for t in (logits, boxes, gt, lab)]
        sizes_d, st = sizes.cuda(), starts.tolist()
        assign, _, sums, status = ops.set_criterion(*dev, starts, sizes_d, *CC.PARAMS)
        cnt = sums[:, :, 3].sum(1)
        coef = L.coef_from_counts(w[None, :].expand(S, 3), cnt)
        out = ops.set_criterion_backward(*dev, starts, sizes_d, CC.ALPHA, CC.GAMMA, assign, status, coef)
        run = lambda: ops.set_criterion_backward(*dev, starts, sizes_d, CC.ALPHA, CC.GAMMA, assign, status, coef, out=out)
        nbytes = logits.numel() * 8 + boxes.numel() * 8 + assign.numel() * 4
        ours = timed(run, 200)
        kern = kernel_times(run, 50, ("criterion_grad_kernel",)).get("criterion_grad_kernel", float("nan"))
        lg, bx = dev[0].clone().requires_grad_(True), dev[1].clone().requires_grad_(True)
        t0 = time.perf_counter()
        total = torch_loop(lg, bx, dev[2], dev[3], st, sizes_d)
        objective = (total[:, :3] * coef).sum()
        torch.cuda.synchronize()
        fwd = (time.perf_counter() - t0) * 1e3

        def autograd():
            lg.grad, bx.grad = None, None
            objective.backward(retain_graph=True)
        loop = timed(autograd, 3)
        scale = (float(out[0].abs().max()), float(out[1].abs().max()))
        dev_l, dev_b = float((lg.grad - out[0]).abs().max()) / scale[0], float((bx.grad - out[1]).abs().max()) / scale[1]
        print("%-20s %6.1f MB moved  set_criterion_backward %7.4f ms per call (%6.1f GB/s), criterion_grad_kernel %7.4f ms (%6.1f GB/s)  "
              "autograd backward %8.2f ms (%5.2f GB/s; its forward with the graph %9.1f ms)  x%.0f  gradients agree to %.1e / %.1e of their largest, "
              "matched %d" % (name, nbytes / 1e6, ours, nbytes / ours / 1e6, kern, nbytes / kern / 1e6, loop, nbytes / loop / 1e6, fwd, loop / ours,
                              dev_l, dev_b, int(cnt.sum())))


def main():
    assert torch.cuda.is_available()
    if "--backward" in sys.argv:
        return backward_main()
    print("set criterion: ops.set_criterion against the torch per-image loop on the same GPU tensors (ms per call, %s)" % torch.cuda.get_device_name(0))
    for name, (n, S, M, C) in (("8 x 6 x 500 x 80", (8, 6, 500, 80)), ("8 x 6 x 300 x 1203", (8, 6, 300, 1203))):
        logits, boxes, gt, lab, starts, sizes = CC.random_set(100 + C, S, M, C, [7] * n, sizes=[(1333, 800)] * n)
        dev = [t.cuda() for t in (logits, boxes, gt, lab)]
        sizes_d, st = sizes.cuda(), starts.tolist()
        out = ops.set_criterion(*dev, starts, sizes_d, *CC.PARAMS)
        run = lambda: ops.set_criterion(*dev, starts, sizes_d, *CC.PARAMS, out=out)
        ours = timed(run, 50)
        ks = kernel_times(run)
        loop = timed(lambda: torch_loop(dev[0], dev[1], dev[2], dev[3], st, sizes_d), 2)
        want = torch_loop(dev[0], dev[1], dev[2], dev[3], st, sizes_d).cpu()
        got = out[2].cpu().sum(1)
        rel = float(((got - want).abs() / want.abs().clamp(min=1e-300)).max())
        print("%-20s logits %6.1f MB  set_criterion %8.3f ms (matcher %.3f, loss sums %.3f, final sum %.3f)  torch loop %9.1f ms  x%.0f  "
              "sums agree to %.1e, matched %d" % (name, logits.numel() * 4 / 1e6, ours, ks.get("criterion_match_kernel", float("nan")),
                                                  ks.get("criterion_loss_kernel", float("nan")), ks.get("criterion_sum_kernel", float("nan")), loop,
                                                  loop / ours, rel, int(got[:, 3].sum())))


if __name__ == "__main__":
    main()
