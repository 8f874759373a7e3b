"""Inference loop and result gathering (mirror of mega_core/engine/inference.py:22-181).

`compute_on_dataset` keeps the reference's conventions: one dataset item per call, wall time
around `model(images)` with a device sync (inference.py:30, :70-73), outputs moved to the CPU and
zipped with the item's image ids (:75, :91-93).  Multi-GPU: ranks own disjoint video ranges and
never talk during inference; at the end ONE collective gathers fixed-layout tensors
[frames, max_det, 6] (+ per-frame counts and ids) to rank 0 -- over RCCL/xGMI each non-root rank
has its own link to root -- replacing the reference's pickled byte all_gather to every rank
(mega_core/utils/comm.py:54-94).
"""
import time

import torch
import torch.distributed as dist

from ..structures.bounding_box import BoxList
from ..utils import comm


def lookahead_items(dataset, indices, infer_batch, lookahead):
    """The look-ahead hand-over built by the ENGINE from an unchanged dataset: yields `dataset[idx]` for idx in `indices`, in
    order, each item loaded exactly once; on the first call of every look-ahead group (frame_id a multiple of infer_batch *
    lookahead) the items of the group's later calls are read ahead and their `ref_l` frames -- exactly what those calls
    would deliver -- are attached as `ref_ahead = {batch start frame: [frames]}` (INPUT.LOOKAHEAD_BATCHES of the MI355X
    schedule).  The reference's own VIDMEGADataset (vid_mega.py:164-250) therefore needs no change: the detector still
    receives every call with its usual keys and returns the later batches' results from the group's first call's work.
    Items that already carry `ref_ahead` (datasets that emit it themselves) pass through untouched."""
    indices = list(indices)
    unit = infer_batch * lookahead
    cache = {}
    pos_of = {idx: k for k, idx in enumerate(indices)}

    def get(idx):
        if idx not in cache:
            cache[idx] = dataset[idx]
        return cache[idx]

    for idx in indices:
        item = get(idx)
        images = item[0]
        if lookahead > 1 and "ref_ahead" not in images and images["frame_id"] % unit == 0:
            f0, end = images["frame_id"], images["end_id"]
            ahead = {}
            k = pos_of[idx]
            # batches of this group after the first: fb = f0 + infer_batch, ... ; batch fb is fed by the calls fb - infer_batch + 1 .. fb
            for fb in range(f0 + infer_batch, min(f0 + unit, end + 1), infer_batch):
                frames = []
                for f in range(fb - infer_batch + 1, fb + 1):
                    j = k + (f - f0)
                    if j >= len(indices):
                        frames = None
                        break
                    nxt = get(indices[j])[0]
                    if nxt["frame_id"] != f or nxt["frame_category"] == 0:
                        frames = None             # not the same video / not consecutive: leave this batch to its own call
                        break
                    frames += list(nxt["ref_l"])
                if frames is None or len(frames) != infer_batch:
                    break
                ahead[fb] = frames
            images = dict(images)
            images["ref_ahead"] = ahead
            item = (images,) + tuple(item[1:])
        cache.pop(idx, None)
        yield idx, item


def seq_nms_boxlists(boxlists, num_classes, nms_thresh, seq_nms_fn=None, nms_fn=None):
    """TEST.SEQ_NMS on ONE video (mega_core/engine/inference.py:54-69 around the reference's seq_nms.py): `boxlists` are the video's
    per-frame results in frame order, exactly what the detector returned -- after its own top-k and, with USE_NMS, its per-frame NMS --
    split by `labels` (the hand-over; the reference reads an attribute only its R-CNN post-processor has).  Steps: pack
    (pack_predictions' layout) -> ops.seq_nms_video (links at IoU >= 0.5, best path by dynamic programming, rescored to its mean,
    0.3-suppression around it, repeated) -> suppressed rows dropped, survivors in their order with the rescored `scores` -> the
    trailing per-class NMS of :63-69 at `nms_thresh` through ops.nms_frames_tiled (class-aware, survivors in score order, clipped to
    the image) -> new BoxLists of the same class.  The reference passes its post-processor's score threshold as that IoU threshold
    (:60, :67); callers here pass MODEL.ROI_HEADS.NMS.  A video that compute_on_video_sharded spread over ranks is finished by calling
    this on the gathered, frame-ordered result.
    seq_nms_fn(dets, counts, num_classes) -> (keep, scores) and nms_fn(boxes, scores, labels, img_w, img_h, iou) -> (boxes, scores,
    labels, counts), both on [frames, cap, ...] tensors: injected by tests without a GPU; default the two library ops."""
    boxlists = list(boxlists)
    if not boxlists:
        return []
    on_gpu = seq_nms_fn is None or nms_fn is None
    if on_gpu:
        from .. import ops
    _, counts, dets, sizes = pack_predictions(dict(enumerate(boxlists)))
    n, cap = dets.shape[:2]
    if cap == 0:
        return [bl.copy_with_fields(bl.fields()) for bl in boxlists]
    dev = torch.device("cuda") if on_gpu else torch.device("cpu")
    fn = seq_nms_fn if seq_nms_fn is not None else ops.seq_nms_video
    keep, scores = fn(dets.to(dev) if seq_nms_fn is None else dets, counts.to(dev) if seq_nms_fn is None else counts, num_classes)
    keep, scores = torch.as_tensor(keep).cpu().bool(), torch.as_tensor(scores).cpu()
    # survivors to the front, in their order.  The trailing NMS takes the same number of candidates for every frame: the rows behind a
    # frame's survivors are zero-area boxes at the origin with the smallest normal score, which neither suppress nor are suppressed
    # (their IoU with anything is 0 or 0 / 0), sort behind every survivor, and leave the largest coordinate -- the class offset of the
    # NMS -- as it was (the detector's boxes are clipped to the image, so it is >= 0)
    left = keep.sum(dim=1).to(torch.int32)
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
    live = torch.arange(cap)[None, :] < left[:, None]
    boxes = torch.where(live[:, :, None], torch.gather(dets[:, :, :4], 1, order[:, :, None].expand(n, cap, 4)), torch.zeros(()))
    sc = torch.where(live, torch.gather(scores, 1, order), torch.full((), torch.finfo(torch.float32).tiny))
    lab = torch.where(live, torch.gather(dets[:, :, 5], 1, order), torch.ones(())).to(torch.int32)
    w, h = boxlists[0].size
    nms = nms_fn if nms_fn is not None else ops.nms_frames_tiled
    if nms_fn is None:
        boxes, sc, lab = boxes.to(dev), sc.to(dev), lab.to(dev)
    ob, osc, ol, oc = nms(boxes.contiguous(), sc.contiguous(), lab.contiguous(), w, h, nms_thresh)
    ob, osc, ol = torch.as_tensor(ob).cpu(), torch.as_tensor(osc).cpu(), torch.as_tensor(ol).cpu()
    oc = torch.as_tensor(oc).cpu().to(torch.int32) - (cap - left)          # the padding rows all survive, behind the frame's own
    out = unpack_predictions(torch.arange(n), oc, torch.cat([ob, osc[:, :, None], ol.to(torch.float32)[:, :, None]], dim=2), sizes)
    return [out[j] for j in range(n)]


def compute_on_dataset(model, dataset, indices, device, timer=None, do_seq_nms=False, seq_nms=None):
    """mega_core/engine/inference.py:22-94.  With INPUT.LOOKAHEAD_BATCHES > 1 on the model the hand-over is built here
    (`lookahead_items`), so any dataset that follows the reference's item protocol gets the grouped schedule.
    do_seq_nms (TEST.SEQ_NMS, :54-69, :76-89): the image ids of a video's calls are collected from its frame_id 0 on, and on the call
    with frame_id == seg_len - 1 the whole video's entries are replaced by `seq_nms(list of its BoxLists in frame order)`; results stay
    keyed by image id, so the later frames a look-ahead group returns early are simply there when the video ends.  seq_nms: default
    seq_nms_boxlists with the model's MODEL.DiffusionDet.NUM_CLASSES and MODEL.ROI_HEADS.NMS."""
    model.eval()
    results = {}
    cpu = torch.device("cpu")
    video_ids = []
    if do_seq_nms and seq_nms is None:
        cfg = model.cfg

        def seq_nms(bls):
            return seq_nms_boxlists(bls, cfg.MODEL.DiffusionDet.NUM_CLASSES, cfg.MODEL.ROI_HEADS.NMS)
    la = int(getattr(model, "lookahead", 1) or 1)
    for idx, item in lookahead_items(dataset, indices, getattr(model, "infer_batch", 1), la):
        images, _, image_ids = item
        with torch.no_grad():
            t0 = time.perf_counter()
            output = model(images)
            if device.type != "cpu":
                torch.cuda.synchronize()
            if timer is not None:
                timer.append(time.perf_counter() - t0)
            output = [o.to(cpu) for o in output]
        results.update({img_id: r for img_id, r in zip(image_ids, output)})
        if do_seq_nms:
            if images["frame_id"] == 0:
                video_ids = []
            video_ids.append(image_ids[0])
            if images["frame_id"] == images["seg_len"] - 1:
                results.update(zip(video_ids, seq_nms([results[i] for i in video_ids])))
    return results


def stream_schedule(dataset, n_streams, indices=None):
    """The slot scheduling of compute_on_streams, host logic: the dataset's videos (a video = the run of indices from a frame 0 up to the
    next one), `n_streams` at a time.  Yields one step after the other as {slot: (dataset index, item)}; a slot delivers its video's
    calls in order, one per step, and takes the next video not yet started on the step after its own ends, so every index is delivered
    exactly once and a slot is idle only when no video is left.  Video boundaries come from the dataset's `frame_seg_id` table (the
    reference's VIDMEGADataset keeps it, vid_mega.py:10-33) without loading a frame; a dataset without one is read once for them."""
    if int(n_streams) < 1:
        raise ValueError("n_streams must be at least 1, got %r" % (n_streams,))
    indices = list(range(len(dataset)) if indices is None else indices)
    seg_id = getattr(dataset, "frame_seg_id", None)
    videos = []
    for idx in indices:
        first = (seg_id[idx] == 0) if seg_id is not None else (dataset[idx][0]["frame_category"] == 0)
        if first or not videos:
            videos.append([])
        videos[-1].append(idx)
    videos = iter(videos)
    slots = {s: iter(v) for s, v in zip(range(int(n_streams)), videos)}
    while slots:
        step = {}
        for s in sorted(slots):
            idx = next(slots[s], None)
            if idx is None:          # this slot's video ended on the previous step: the next video, now
                v = next(videos, None)
                if v is None:
                    del slots[s]
                    continue
                slots[s] = iter(v)
                idx = next(slots[s])
            step[s] = (idx, dataset[idx])
        if step:
            yield step


def compute_on_streams(model, dataset, n_streams, indices=None, timer=None):
    """A streaming-protocol dataset's videos `n_streams` at a time through one StreamSet (DiffusionDet.open_streams): every step is one call
    of each running video.  Returns predictions by image id as compute_on_dataset does (CPU BoxLists), so do_vid_evaluation and
    predictions.pth work unchanged; per stream the detections are those of compute_on_dataset on that video."""
    model.eval()
    streams = model.open_streams()
    results = {}
    cpu = torch.device("cpu")
    for step in stream_schedule(dataset, n_streams, indices):
        with torch.no_grad():
            t0 = time.perf_counter()
            out = streams.step({s: item[0] for s, (_, item) in step.items()})
            if timer is not None:
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
                timer.append(time.perf_counter() - t0)
        for s, (_, item) in step.items():
            results.update({img_id: r.to(cpu) for img_id, r in zip(item[2], out[s])})
    return results


def max_detections(results):
    """largest per-frame detection count of a shard (the x4 ensemble keeps up to 3 x NUM_PROPOSALS candidates through
    NMS, diffusion_det.py:607-627, so the count is a property of the data, not of the config)"""
    return max((len(bl) for bl in results.values()), default=0)


def video_shard_plan(num_frames, infer_batch, lookahead, world):
    """One video over `world` ranks (single-video case).  The unit is a look-ahead group (`infer_batch *
    lookahead` frames): given the video's global memory every group is independent -- the memory is final after the
    first call (GLOBAL.STOP_UPDATE_AFTER_INIT_TEST), local attention is off, the local queue is exactly one batch, and the
    random draws are keyed by (video, call frame, step), not by RNG stream position.  Group g runs on rank g % world; group 0
    (whose first call also carries the global frames) therefore on rank 0.  Returns, per rank, the list of inclusive
    dataset-offset ranges (first call, last call) to feed: a group's first batch needs the `infer_batch - 1` calls before
    it, which only queue their local frame (diffusion_det.py:410-412)."""
    unit = infer_batch * lookahead
    plan = [[] for _ in range(world)]
    for g, f0 in enumerate(range(0, num_frames, unit)):
        last_batch = min(f0 + unit, -(-num_frames // infer_batch) * infer_batch) - infer_batch
        last_batch = min(last_batch, (num_frames - 1) // infer_batch * infer_batch)
        plan[g % world].append((max(0, f0 - (infer_batch - 1)), last_batch))
    return plan


def compute_on_video_sharded(model, dataset, start, num_frames, device, rank=None, world=None, broadcast=None):
    """Run ONE video (dataset indices [start, start + num_frames)) across the ranks of the process group following
    `video_shard_plan`: rank 0 runs the first call (24 global + the first local frames) and the memory it builds --
    [900, d] + [150, d] fp32, 1.07 MB -- is broadcast (RCCL over xGMI; the only data-path exchange of this mode);
    every rank then runs its own groups.  Returns this rank's {image id: BoxList}; merge with gather_predictions.
    TEST.SEQ_NMS needs the whole video: it is not applied here -- call seq_nms_boxlists on the gathered result in frame order.
    `broadcast(tensors, src)`: injected for tests; default torch.distributed.broadcast of each tensor."""
    rank = comm.get_rank() if rank is None else rank
    world = comm.get_world_size() if world is None else world
    plan = video_shard_plan(num_frames, model.infer_batch, model.lookahead, world)[rank]
    results = {}
    cpu = torch.device("cpu")

    def feed(a, b):
        for off in range(a, b + 1):
            images, _, ids = dataset[start + off]
            with torch.no_grad():
                out = model(images)
            results.update({i: o.to(cpu) for i, o in zip(ids, out)})

    todo = list(plan)
    if rank == 0:
        feed(0, 0)
        mem = [m.contiguous() for m in model.global_memory()]
    else:
        mem = [torch.empty(s, dtype=torch.float32, device=device) for s in model.global_memory_shapes()]
    if world > 1:
        if broadcast is not None:
            mem = broadcast(mem, 0)
        else:
            for m in mem:
                dist.broadcast(m, src=0)
    if rank != 0:
        model.adopt_video_memory(mem)
    for a, b in todo:
        feed(max(a, 1) if (rank == 0 and a == 0) else a, b)
    return results


def pack_predictions(results, max_det=None):
    """dict{id: BoxList} -> (ids [n] int64, counts [n] int32, dets [n, max_det, 6] fp32 = box4, score, label,
    sizes [n,2] int32).  max_det None = the shard's own maximum; a smaller explicit value is an error (nothing is
    truncated silently)."""
    ids = sorted(results.keys())
    n = len(ids)
    need = max_detections(results)
    if max_det is None:
        max_det = need
    elif need > max_det:
        raise ValueError("a frame holds %d detections but max_det is %d" % (need, max_det))
    dets = torch.zeros((n, max_det, 6), dtype=torch.float32)
    counts = torch.zeros((n,), dtype=torch.int32)
    sizes = torch.zeros((n, 2), dtype=torch.int32)
    for j, i in enumerate(ids):
        bl = results[i]
        k = len(bl)
        counts[j] = k
        sizes[j, 0], sizes[j, 1] = bl.size
        if k:
            dets[j, :k, :4] = bl.bbox
            dets[j, :k, 4] = bl.get_field("scores")
            dets[j, :k, 5] = bl.get_field("labels").to(torch.float32)
    return torch.tensor(ids, dtype=torch.int64), counts, dets, sizes


def unpack_predictions(ids, counts, dets, sizes):
    out = {}
    for j, i in enumerate(ids.tolist()):
        k = int(counts[j])
        bl = BoxList(dets[j, :k, :4].clone(), (int(sizes[j, 0]), int(sizes[j, 1])), mode="xyxy")
        bl.add_field("scores", dets[j, :k, 4].clone())
        bl.add_field("labels", dets[j, :k, 5].to(torch.int64))
        out[i] = bl
    return out


def gather_predictions(results, max_det=None, device=None, always=False):
    """Gather every rank's {image_id: BoxList} on rank 0 (returns None elsewhere).  The padded per-frame capacity is
    the maximum detection count over all ranks (exchanged with the shard sizes) unless `max_det` forces a larger one.
    always=True runs the collectives even in a one-rank group (the RCCL path on a single GPU)."""
    world = comm.get_world_size()
    if world == 1 and not (always and dist.is_available() and dist.is_initialized()):
        return results
    dev = device if (device is not None and dist.get_backend() == "nccl") else torch.device("cpu")
    n_local = torch.tensor([len(results), max_detections(results)], dtype=torch.int64, device=dev)
    all_n = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(all_n, n_local)                       # 16 bytes per rank: shard size, largest detection count
    all_n = [x.cpu() for x in all_n]
    n_max = int(max(int(x[0]) for x in all_n))
    det_max = max([int(x[1]) for x in all_n] + [int(max_det or 0), 1])
    ids, counts, dets, sizes = pack_predictions(results, det_max)
    all_n = [x[:1] for x in all_n]

    def pad(t):
        p = torch.zeros((n_max,) + tuple(t.shape[1:]), dtype=t.dtype)
        p[: t.shape[0]] = t
        return p.to(dev)

    payload = [pad(ids), pad(counts), pad(dets), pad(sizes)]
    rank = comm.get_rank()
    gathered = []
    for t in payload:                                     # the data collective: gather to rank 0
        bufs = [torch.zeros_like(t) for _ in range(world)] if rank == 0 else None
        dist.gather(t, gather_list=bufs, dst=0)
        gathered.append(bufs)
    if rank != 0:
        return None
    merged = {}
    for r in range(world):
        n = int(all_n[r].item())
        merged.update(unpack_predictions(gathered[0][r][:n].cpu(), gathered[1][r][:n].cpu(), gathered[2][r][:n].cpu(),
                                         gathered[3][r][:n].cpu()))
    return merged


def predictions_list(merged):
    """dict -> list indexed by dataset image id, as torch.save'd to predictions.pth (inference.py:101-115)."""
    ids = sorted(merged.keys())
    return [merged[i] for i in ids]


def inference(model, dataset, indices, device, output_folder=None, gt_boxlists=None, max_det=None, motion_specific=False,
              motion_ious=None, logger=None, class_module=None, seq_nms=None, eval_device=None):
    """Reference `inference` (mega_core/engine/inference.py:118-181) for the in-scope path: run this rank's share, gather on
    rank 0, write `predictions.pth` -- `predictions_seq_nms.pth` instead when the model's config has TEST.SEQ_NMS (:165-168; the
    step itself runs in compute_on_dataset, `seq_nms` as there) -- (`class_module`: see vid_eval.save_predictions) and evaluate as the reference's
    `evaluate` -> `do_vid_evaluation` does (vid_eval.py:14-78): when the dataset serves `get_img_info` / `get_groundtruth`
    the predictions are mapped from the resized frame to the annotation's original size first and `result.txt` is written;
    `gt_boxlists` (a list of BoxList, one per image id) stands in for a dataset without annotations -- each prediction is
    resized to its ground truth's size the same way.  Returns (predictions list | None off rank 0, eval | None):
    eval = the AP dict, or the list of one dict per motion range with `motion_specific`.  eval_device: a torch.device runs the
    evaluator's matching there (vid_eval.do_vid_evaluation's `device`); None keeps it in numpy."""
    import os

    from ..data.evaluation import vid_eval
    from ..utils import comm
    do_seq_nms = bool(getattr(getattr(getattr(model, "cfg", None), "TEST", None), "SEQ_NMS", False))
    results = compute_on_dataset(model, dataset, indices, device, do_seq_nms=do_seq_nms, seq_nms=seq_nms)
    merged = gather_predictions(results, max_det, device=device)
    if not comm.is_main_process():
        return None, None
    preds = predictions_list(merged)
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        vid_eval.save_predictions(preds, os.path.join(output_folder, "predictions_seq_nms.pth" if do_seq_nms else "predictions.pth"), class_module)
    source = None
    if gt_boxlists is not None:
        source = vid_eval.GroundTruthList(gt_boxlists, getattr(dataset, "map_class_id_to_class_name", None))
    elif hasattr(dataset, "get_groundtruth") and getattr(dataset, "annotations", True) is not None:
        source = dataset
    if source is None:
        return preds, None
    ev = vid_eval.do_vid_evaluation(source, preds, output_folder, motion_specific=motion_specific, logger=logger,
                                    motion_ious=motion_ious, device=eval_device)
    return preds, (ev if motion_specific else ev[0])


# ---- still images ------------------------------------------------------------------------------------------------------------------
def coco_results(predictions, label_map=None):
    """{image_id: BoxList} -> the COCO result list: one dict(image_id, category_id, bbox [x, y, w, h], score) per detection, boxes in the
    BoxList's own image size.  label_map: model label (1 ..) -> category id, a dict or a callable; None keeps the labels."""
    to_cat = (lambda l: l) if label_map is None else (label_map if callable(label_map) else label_map.__getitem__)
    out = []
    for image_id in sorted(predictions):
        bl = predictions[image_id].convert("xyxy")
        boxes = bl.bbox.detach().cpu().double()
        scores = bl.get_field("scores").detach().cpu().double().tolist()
        labels = bl.get_field("labels").detach().cpu().tolist()
        for (x1, y1, x2, y2), s, l in zip(boxes.tolist(), scores, labels):
            out.append({"image_id": int(image_id), "category_id": to_cat(int(l)), "bbox": [x1, y1, x2 - x1, y2 - y1], "score": s})
    return out


def write_coco_results(predictions, path, label_map=None):
    import json
    res = coco_results(predictions, label_map)
    with open(path, "w") as f:
        json.dump(res, f)
    return res


def _still_annotations(annotations, protocol):
    """-> ("coco" or "lvis", that evaluator's annotations object).  protocol None: LVIS exactly when the file's images carry `neg_category_ids`."""
    import json

    from ..data.evaluation import coco_eval, lvis_eval
    if protocol not in (None, "coco", "lvis"):
        raise ValueError("protocol is 'coco', 'lvis' or None, not %r" % (protocol,))
    if isinstance(annotations, coco_eval.CocoAnnotations):
        lvis = isinstance(annotations, lvis_eval.LvisAnnotations)
        if protocol is not None and lvis != (protocol == "lvis"):
            raise ValueError("protocol %r with annotations loaded as %s" % (protocol, type(annotations).__name__))
        return ("lvis" if lvis else "coco"), annotations
    if not isinstance(annotations, dict):
        with open(annotations) as f:
            annotations = json.load(f)
    if protocol == "lvis" or (protocol is None and lvis_eval.is_lvis(annotations)):
        return "lvis", lvis_eval.LvisAnnotations(annotations)
    return "coco", coco_eval.CocoAnnotations(annotations)


def inference_images(model, loader, output_folder=None, label_map=None, annotations=None, eval_device=None, bbox_aug=None, protocol=None,
                     eval_accumulate="numpy"):
    """Still images: `loader` yields (images, image_ids, original (w, h) per image) batches (data/datasets/still.py: batches, or a DataLoader
    over StillImageDataset with OrientationBatchSampler and collate_images); every batch goes through model.detect_images with its ids
    -- so an image's draws, and with them its detections, do not depend on its batch -- and every BoxList is mapped back to the image's
    original size (BoxList.resize).  -> {image_id: BoxList} on the host; with `output_folder` also `predictions.pth` (that dict) and
    `coco_results.json` (coco_results with `label_map`).
    annotations (a COCO annotation file, its dict or a coco_eval.CocoAnnotations): the predictions are scored with the COCO bbox
    protocol (coco_eval.do_coco_evaluation; `coco_eval.txt` in `output_folder`) -> (predictions, the ordered dict of the twelve
    numbers); `label_map` then defaults to the annotations' label -> category id map, and a prediction for an image that the
    annotations do not list is an error that names the id.  eval_device: a torch.device runs the evaluator's matching there; None keeps
    it in numpy.  eval_accumulate: "device" runs the evaluator's accumulation on `eval_device` as well (the same numbers and files);
    "numpy" keeps it on the host.
    protocol ("coco", "lvis" or None): None takes the LVIS bbox protocol (lvis_eval.do_lvis_evaluation: the federated protocol, thirteen
    numbers, `lvis_eval.txt`, and `lvis_results.json` with at most 300 rows per image) exactly when the file's images carry
    `neg_category_ids`, which a COCO file's never do.
    bbox_aug (None: the model's TEST.BBOX_AUG.ENABLED, as the reference's inference(bbox_aug=...) is called): the batches are lists of
    uint8 images at their native size (still.batches(..., raw=True), collate_raw) and go to model.detect_images_aug, whose BoxLists are in
    the plain test transform's size; everything behind it is the same."""
    import os
    from ..data.evaluation.coco_eval import check_accumulate
    check_accumulate(eval_accumulate, eval_device, "eval_accumulate", "eval_device")
    if bbox_aug is None:
        bbox_aug = bool(getattr(getattr(getattr(getattr(model, "cfg", None), "TEST", None), "BBOX_AUG", None), "ENABLED", False))
    detect = model.detect_images_aug if bbox_aug else model.detect_images
    ann = None
    if annotations is not None:
        protocol, ann = _still_annotations(annotations, protocol)
        if label_map is None:
            label_map = ann.category_of
    predictions = {}
    cpu = torch.device("cpu")
    with torch.no_grad():
        for images, image_ids, sizes in loader:
            out = detect(images, image_ids)
            for bl, image_id, size in zip(out, image_ids, sizes):
                if int(image_id) in predictions:
                    raise ValueError("image id %d appears twice" % int(image_id))
                if ann is not None and int(image_id) not in ann.images:
                    raise ValueError("there is a prediction for image id %d, which the annotations do not list" % int(image_id))
                predictions[int(image_id)] = bl.to(cpu).resize((int(size[0]), int(size[1])))
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        torch.save(predictions, os.path.join(output_folder, "predictions.pth"))
        write_coco_results(predictions, os.path.join(output_folder, "coco_results.json"), label_map)
    if ann is None:
        return predictions
    from ..data.evaluation import coco_eval, lvis_eval
    if protocol == "lvis":
        if output_folder:
            import json
            with open(os.path.join(output_folder, "lvis_results.json"), "w") as f:
                json.dump(lvis_eval.lvis_results(predictions, label_map), f)
        return predictions, lvis_eval.do_lvis_evaluation(ann, predictions, output_folder, device=eval_device, accumulate=eval_accumulate)
    return predictions, coco_eval.do_coco_evaluation(ann, predictions, output_folder, device=eval_device, accumulate=eval_accumulate)


def validation_losses(model, loader, output_folder=None):
    """The weighted training losses of a labelled data set of still images, forward only: `loader` yields (images, targets, image_ids)
    batches -- what model.compute_losses takes -- and every batch goes through model.loss_sums.  The set's losses are formed with the
    reference's normalisation over the WHOLE set: the focal, L1 and 1 - GIoU sums and the matched counts of all batches are added (float64)
    and divided once, per head output; per-batch ratios are not averaged, so the result does not depend on the batching.  -> an ordered
    dict {loss_ce, loss_bbox, loss_giou, then `_0 .. _{S-2}`, and `total_loss`, their sum} of Python floats, times CLASS_WEIGHT / L1_WEIGHT /
    GIOU_WEIGHT; with `output_folder` also written to `losses.txt`, one `name value` line each."""
    import os
    from collections import OrderedDict

    from ..modeling.roi_heads.box_head.loss import losses_from_sums
    total, seen = None, set()
    for images, targets, image_ids in loader:
        for i in image_ids:
            if int(i) in seen:
                raise ValueError("image id %d appears twice" % int(i))
            seen.add(int(i))
        sums, _ = model.loss_sums(images, targets, image_ids)
        sums = sums.sum(1, keepdim=True)
        total = sums if total is None else total + sums
    if total is None:
        raise ValueError("validation_losses: the loader yielded no batch")
    weights = model.objective.weights
    out = OrderedDict((k, v * weights.get(k, 1.0)) for k, v in losses_from_sums(total).items())
    out["total_loss"] = sum(out.values())
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        with open(os.path.join(output_folder, "losses.txt"), "w") as f:
            for k, v in out.items():
                f.write("%s %.9g\n" % (k, v))
    return out
