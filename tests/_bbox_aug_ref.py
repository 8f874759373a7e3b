"""CPU restatement of the TEST.BBOX_AUG merge (mega_core/engine/bbox_aug.py: im_detect_bbox_aug) with this package's BoxList: the views'
detections mapped into view 0 by BoxList.transpose / resize and concatenated, a plain class-aware NMS clipped to view 0, and the cut of
filter_results.  `nms` may be replaced (the end-to-end GPU test passes the library's own tiled NMS, so that only new code is compared)."""
import torch

from diffusionvid_amd.structures.bounding_box import FLIP_LEFT_RIGHT, BoxList


def to_view0(bl, v, view, view0):
    """a view's BoxList (size (w_v, h_v)) in view 0's frame: im_detect_bbox_hflip's transpose(0), then add_preds_t's resize"""
    assert bl.size == (view.w, view.h)
    if view.flip:
        bl = bl.transpose(FLIP_LEFT_RIGHT)
    return bl if v == 0 else bl.resize((view0.w, view0.h))


def candidates(per_view, views):
    """[BoxList per view] -> (boxes [N, 4], scores [N], labels [N]) in (view, row) order, in view 0's frame"""
    mapped = [to_view0(bl, v, view, views[0]) for v, (bl, view) in enumerate(zip(per_view, views))]
    return (torch.cat([m.bbox for m in mapped]), torch.cat([m.get_field("scores") for m in mapped]),
            torch.cat([m.get_field("labels") for m in mapped]))


def iou(a, b):
    """torchvision's box IoU (no + 1), float32"""
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    w = (torch.minimum(a[2], b[2]) - torch.maximum(a[0], b[0])).clamp(min=0)
    h = (torch.minimum(a[3], b[3]) - torch.maximum(a[1], b[1])).clamp(min=0)
    inter = w * h
    return float(inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter))


def iou_many(a, b):
    """IoU of box a [4] with every row of b [k, 4]"""
    w = (torch.minimum(a[2], b[:, 2]) - torch.maximum(a[0], b[:, 0])).clamp(min=0)
    h = (torch.minimum(a[3], b[:, 3]) - torch.maximum(a[1], b[:, 1])).clamp(min=0)
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def iou_margin(boxes, labels, thr):
    """smallest |IoU - thr| over the pairs of one label: how far the hand-placed boxes stay from the NMS's decision"""
    worst = 1.0
    for i in range(len(boxes) - 1):
        rest = labels[i + 1:] == labels[i]
        if bool(rest.any()):
            worst = min(worst, float((iou_many(boxes[i], boxes[i + 1:][rest]) - thr).abs().min()))
    return worst


def plain_nms(boxes, scores, labels, size_wh, thr):
    """greedy NMS inside every class on the unclipped boxes -> survivors in (score desc, position asc) order, clipped to the image"""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    keep = []
    for i in order:
        k = torch.tensor(keep, dtype=torch.int64)
        if not bool(((labels[k] == labels[i]) & (iou_many(boxes[i], boxes[k]) > thr)).any()):
            keep.append(i)
    keep = torch.tensor(keep, dtype=torch.int64)
    out = boxes[keep].clone()
    out[:, 0::2] = out[:, 0::2].clamp(0, size_wh[0] - 1)
    out[:, 1::2] = out[:, 1::2].clamp(0, size_wh[1] - 1)
    return out, scores[keep], labels[keep]


def cut(boxes, scores, labels, max_det):
    """filter_results' limit: more than max_det > 0 rows -> those scoring >= the max_det-th (score order: a prefix that keeps ties)"""
    if 0 < max_det < len(scores):
        n = int((scores >= scores[max_det - 1]).sum())
        return boxes[:n], scores[:n], labels[:n]
    return boxes, scores, labels


def merge(per_view, views, thr, max_det, nms=plain_nms):
    size0 = (views[0].w, views[0].h)
    boxes, scores, labels = cut(*nms(*candidates(per_view, views), size0, thr), max_det)
    out = BoxList(boxes, size0, mode="xyxy")
    out.add_field("scores", scores)
    out.add_field("labels", labels.to(torch.int64))
    return out


def boxlist(boxes, scores, labels, size_wh):
    bl = BoxList(torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4), size_wh, mode="xyxy")
    bl.add_field("scores", torch.as_tensor(scores, dtype=torch.float32))
    bl.add_field("labels", torch.as_tensor(labels, dtype=torch.int64))
    return bl
