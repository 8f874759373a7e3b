"""Generate the golden gradients of the training objective by running the REFERENCE's own criterion on inputs that require grad and
backpropagating through it on the CPU (build container only).

    python tests/golden/make_golden_criterion_grads.py            # writes tests/golden/criterion/grads.npz
    python tests/golden/make_golden_criterion_grads.py --check    # regenerates in memory and compares with the committed file

The reference is imported by make_golden_criterion.py (same shims, same stand-ins for box_iou, box_area and sigmoid_focal_loss_jit), and
the cases are the committed ones of criterion/sets.npz, read, not made again.  Only data is stored.

Per case: the reference's SetCriterionDynamicK on `pred_logits` / `pred_boxes` that require grad, then backward() of
2 * loss_ce + 5 * loss_bbox + 2 * loss_giou (the weights the cases were generated with), once on float64 inputs and once on fp32 inputs.

grads.npz   `<case>.d_logits` [n, M, C], `<case>.d_boxes` [n, M, 4]: the float64 run's gradients, stored as float32;
            `<case>.dev32` [2]: the deviation of the fp32 run's (d_logits, d_boxes) from the float64 run's, each as
            max|got - truth| / max|truth| (0 where both are all zero) -- the yardstick of the gradient tests is its largest value per
            column over all cases.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_criterion as G  # noqa: E402  (installs the shims and the stand-ins, imports the reference)

import torch  # noqa: E402

OUT = G.OUT


def deviation(got, truth):
    scale = float(truth.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, "the truth is all zero, the fp32 run is not"
        return 0.0
    return float((got.double() - truth).abs().max()) / scale


def run_reference(case, dtype):
    """-> (d_logits [n, M, C], d_boxes [n, M, 4]) of the weighted loss, in `dtype`"""
    logits = torch.from_numpy(case["logits"]).to(dtype).requires_grad_(True)
    boxes = torch.from_numpy(case["boxes"]).to(dtype).requires_grad_(True)
    starts = case["gt_starts"].tolist()
    targets = G._targets(torch.from_numpy(case["gt_boxes"]), torch.from_numpy(case["gt_labels"]), starts, torch.from_numpy(case["sizes"]), dtype)
    crit = G._criterion(logits.shape[-1])
    losses = crit({"pred_logits": logits, "pred_boxes": boxes}, targets)
    total = G.W_CLASS * losses["loss_ce"] + G.W_L1 * losses["loss_bbox"] + G.W_GIOU * losses["loss_giou"]
    total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad          # no ground truth anywhere: the box losses are constants
    return zero(logits).detach(), zero(boxes).detach()


def make_grads():
    z = np.load(os.path.join(OUT, "sets.npz"))
    names = sorted({k.split(".")[0] for k in z.files})
    out, report = {}, []
    for name in names:
        case = {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(name + ".")}
        l64, b64 = run_reference(case, torch.float64)
        l32, b32 = run_reference(case, torch.float32)
        assert l32.dtype == torch.float32 and l64.dtype == torch.float64
        dev = (deviation(l32, l64), deviation(b32, b64))
        out[name + ".d_logits"], out[name + ".d_boxes"] = l64.numpy().astype(np.float32), b64.numpy().astype(np.float32)
        out[name + ".dev32"] = np.array(dev, dtype=np.float64)
        report.append("%-18s max|d_logits| %.6e  max|d_boxes| %.6e  fp32 run: d_logits %.3e  d_boxes %.3e" % (
            name, float(l64.abs().max()), float(b64.abs().max()), dev[0], dev[1]))
    return out, report


def main():
    torch.set_num_threads(1)
    arrays, report = make_grads()
    if "--check" in sys.argv:
        have = np.load(os.path.join(OUT, "grads.npz"))
        assert sorted(have.files) == sorted(arrays), "grads.npz: the keys differ"
        for k, v in arrays.items():
            assert have[k].dtype == v.dtype and np.array_equal(have[k], v), "grads.npz: %s differs from the committed fixture" % k
        print("criterion gradient fixtures reproduced")
        return
    np.savez_compressed(os.path.join(OUT, "grads.npz"), **arrays)
    print("grads.npz", os.path.getsize(os.path.join(OUT, "grads.npz")), "bytes")
    print("\n".join(report))
    print("yardstick: d_logits %.3e  d_boxes %.3e" % tuple(max(arrays[n + ".dev32"][j] for n in {k.split(".")[0] for k in arrays}) for j in (0, 1)))


if __name__ == "__main__":
    main()
