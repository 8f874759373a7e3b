"""What the criterion's gradient tests share: the fixture tests/golden/criterion/grads.npz (made by tests/golden/
make_golden_criterion_grads.py from the reference's own criterion and torch's autograd), the deviation measure and its bound, and the
coefficients of the weighted loss."""
import os

import numpy as np
import torch

import _criterion_cases as CC

WEIGHTS = (CC.W_CLASS, CC.W_L1, CC.W_GIOU)          # 2 * loss_ce + 5 * loss_bbox + 2 * loss_giou: what the fixture backpropagates

_grads = None


def grads():
    global _grads
    if _grads is None:
        z = np.load(os.path.join(CC.HERE, "golden", "criterion", "grads.npz"))
        _grads = {n: {k: z["%s.%s" % (n, k)] for k in ("d_logits", "d_boxes", "dev32")} for n in CC.NAMES}
    return _grads


# The gradient bound, per tensor.  Measure: max|got - truth| / max|truth| over a case's tensor; an all-zero truth must be met exactly.
# Truth: the fixture's float64 run of the reference.  Yardstick: the reference's own fp32 run against that truth, the largest value over
# all cases as the generator recorded it in `dev32`: 2.779e-07 for d_logits (case boxes_65), 1.921e-07 for d_boxes (case boxes_256);
# profiles/criterion_grad_parity.txt lists every case.  The device and the host path get 8x that, with a floor of 16 x 2^-24 = 9.54e-07
# (the rule of _criterion_cases.BOUND: room for another order of the fp32 operations).
def yardstick():
    return tuple(max(float(g["dev32"][j]) for g in grads().values()) for j in (0, 1))


def bound():
    """(bound on d_logits, bound on d_boxes)"""
    return tuple(max(8 * y, 16 * 2.0 ** -24) for y in yardstick())


def deviation(got, truth):
    """max|got - truth| / max|truth| in float64; where the truth is all zero, `got` must be all zero exactly"""
    got, truth = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(truth).detach().cpu().double()
    assert got.shape == truth.shape, (got.shape, truth.shape)
    scale = float(truth.abs().max()) if truth.numel() else 0.0
    if scale == 0.0:
        assert not bool(got.any()), "the truth is all zero, got up to %r" % float(got.abs().max())
        return 0.0
    return float((got - truth).abs().max()) / scale


def reference_coef(assign, weights=WEIGHTS):
    """assign [S, n, M] -> coef [S, 3] float64 of the weighted reference losses: weight / max(matched, 1), the box terms 0 when nothing
    matched (formed here independently of loss.coef_from_counts)"""
    cnt = (assign >= 0).sum((1, 2)).to(torch.float64)
    w = torch.tensor(weights, dtype=torch.float64, device=assign.device)
    coef = w[None, :] / cnt.clamp(min=1)[:, None]
    coef[:, 1:] = coef[:, 1:] * (cnt > 0).to(torch.float64)[:, None]
    return coef


def host_gradients(L, logits, boxes, packed, assign, dtype, alpha=CC.ALPHA, gamma=CC.GAMMA, weights=WEIGHTS):
    """torch's autograd on loss.losses_host in `dtype` on the CPU: -> (losses [S, 3], d_logits, d_boxes) of sum_s weights . losses[s]"""
    lg = logits.detach().cpu().to(dtype).requires_grad_(True)
    bx = boxes.detach().cpu().to(dtype).requires_grad_(True)
    losses = L.losses_host(lg, bx, tuple(torch.as_tensor(t).cpu() for t in packed), assign.cpu(), alpha, gamma)
    (losses * torch.tensor(weights, dtype=torch.float64)).sum().backward()
    return losses.detach(), lg.grad, bx.grad
