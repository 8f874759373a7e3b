"""Batches of still images on a DiffusionDet's weights: the admission of a batch, its uploads and launch sequences, the plain detection
(DiffusionDet.detect_images) and the TEST.BBOX_AUG one (detect_images_aug).

A `StillImages` holds the detector and none of its video state: it reads the configuration, the head, the draws' source and the
stateless helpers (_get_engine, _time_pairs, _ddim_ensemble, _to_boxlists), never the queue, the look-ahead tables, the captured graphs
or the memory streams.  The training objective (detector/objective.py) admits and chunks its batches through the same object.
"""
import numpy as np
import torch

from ... import ops
from ...structures.bounding_box import BoxList
from ...structures.image_list import to_image_list
from .diffusion_det import _result_class


class StillImages:
    def __init__(self, detector):
        self.det = detector
        self._aug_tables = {}          # resample tables by (in, out) size: a dataset repeats its sizes

    # ---- admission ------------------------------------------------------------------------------------------------------------------------
    def _refuse(self, what):
        """what no entry point for still batches runs; before anything is built or launched"""
        det = self.det
        if det.training:
            raise NotImplementedError("%s: training is out of scope of the MI355X inference path" % what)
        vid = det.cfg.MODEL.VID
        if vid.MEGA.GLOBAL.ENABLE:
            raise NotImplementedError("%s: MODEL.VID.MEGA.GLOBAL.ENABLE is True, and a still image has no global memory to condition on" % what)
        if vid.ROI_BOX_HEAD.ATTENTION.ENABLE:
            raise NotImplementedError("%s: MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE is True, and a still image has no local memory to condition on" % what)
        if det.num_heads_local > 0:
            raise NotImplementedError("%s: MODEL.DiffusionDet.NUM_HEADS_LOCAL is %d: the conditioned heads have nothing to be conditioned on "
                                      "(still images need NUM_HEADS_LOCAL 0)" % (what, det.num_heads_local))

    @staticmethod
    def _ids(what, image_ids, n):
        ids = list(range(n)) if image_ids is None else [int(i) for i in image_ids]
        if len(ids) != n:
            raise ValueError("%s: %d image_ids for %d images" % (what, len(ids), n))
        return ids

    def admit(self, what, images, image_ids=None):
        """The refusals and the checks of a still batch for the entry point `what` -> (canvas ImageList, [(w, h)] per image, ids).
        images: an ImageList (this package's or another's), an [n, 3, H, W] or [3, h, w] tensor, or a list of [3, h, w] tensors, which are
        zero-padded to one canvas divisible by 32; image_ids default to 0 .. n-1."""
        self._refuse(what)
        div = self.det.size_divisibility
        if isinstance(images, torch.Tensor):
            images = list(images) if images.dim() == 4 else [images]
        imgs = to_image_list(images, div)
        n, ch, H, W = imgs.tensors.shape
        if ch != 3 or H % div or W % div:
            raise ValueError("%s: the canvas must be [n, 3, H, W] with H and W multiples of %d, got %s" % (what, div, tuple(imgs.tensors.shape)))
        sizes_wh = [(int(s[1]), int(s[0])) for s in imgs.image_sizes]
        if len(sizes_wh) != n or any(not (0 < w <= W and 0 < h <= H) for w, h in sizes_wh):
            raise ValueError("%s: image_sizes must hold one (h, w) inside the %d x %d canvas per image, got %s" % (what, H, W, list(imgs.image_sizes)))
        return imgs, sizes_wh, self._ids(what, image_ids, n)

    # ---- uploads and launch sequences -------------------------------------------------------------------------------------------------------
    def chunk(self):
        """images per launch sequence: `still_chunk`, else INFER_BATCH * LOOKAHEAD_BATCHES, the video path's group (_extract)"""
        det = self.det
        return max(1, int(det.still_chunk or det.infer_batch * det.lookahead))

    def chunks(self, canvas):
        """The launch sequences of one canvas: the workspace reserved once, then per chunk (a, b, the backbone features of slots a..b)."""
        eng = self.det._get_engine()
        n, cap = canvas.shape[0], self.chunk()
        H, W = canvas.shape[-2:]
        eng.reserve(min(cap, n), H, W, self.det.num_proposals)
        for a in range(0, n, cap):
            b = min(n, a + cap)
            yield a, b, eng.backbone_frames([canvas[i:i + 1] for i in range(a, b)])

    def draws(self, kind, ids, step, views=(0,)):
        """[n * len(views), M, 4]: the draw of every image of the batch, keyed by its id and -- in the key's `image` slot -- its view (0 for
        a plain still image), image-major; an injected noise_fn draws on the host and ONE tensor is uploaded"""
        det = self.det
        shape = (det.num_proposals, 4)
        if getattr(det.noise_fn, "on_device", False):          # per view one launch for consecutive ids: keys a fixed stride apart
            per_view = [det.noise_fn.draw_ids(kind, ids, step, shape, det.device, image=v) for v in views]
            return per_view[0] if len(views) == 1 else torch.stack(per_view, dim=1).reshape((-1,) + shape)
        if det.noise_fn is not None:
            return torch.stack([det.noise_fn(kind, i, step, v, shape) for i in ids for v in views]).to(det.device, torch.float32)
        return torch.randn((len(ids) * len(views),) + shape, device=det.device)

    def uploads(self, sizes_wh, ids, views=(0,)):
        """the size table and every draw of one launch sequence of still images (slots: image-major, then `views`), on the device"""
        det = self.det
        up = {"sizes": ops.FrameSizes(torch.tensor(sizes_wh, dtype=torch.float32), det.device)}
        if det.sampling_timesteps == 1:
            up["box_init"] = self.draws("box_init", ids, 0, views)
        else:
            up["draws"] = {"img": self.draws("img", ids, 0, views)}
            for step, (_, time_next) in enumerate(det._time_pairs()):
                if time_next >= 0:
                    up["draws"][step] = (self.draws("ddim", ids, step, views), self.draws("renew", ids, step, views))
        return up

    def launches(self, canvas, up):
        """the launch sequences of one canvas of still images: -> per chunk of `chunk()` slots the detection buffers (boxes, scores,
        labels, counts) of postproc_topk_nms.  Queues kernels only."""
        det = self.det
        pairs = det._time_pairs()
        sizes, box_init, draws = up["sizes"], up.get("box_init"), up.get("draws")
        outs = []
        for a, b, feats in self.chunks(canvas):
            fs = sizes[a:b]
            if det.sampling_timesteps == 1:
                t = torch.full((b - a,), pairs[0][0], dtype=torch.long)
                logits, boxes = det.head.plain_heads(feats, ops.noise_to_boxes(box_init[a:b], det.scale, fs), t)
                if det.debug_taps is not None:
                    det.debug_taps.setdefault("still_final_0", []).append((logits, boxes))
                outs.append(ops.postproc_topk_nms(logits, boxes, fs, None, 0.5, det.use_nms))
            else:
                chunk = {k: (v[a:b] if k == "img" else (v[0][a:b], v[1][a:b])) for k, v in draws.items()}
                outs.append(det._ddim_ensemble(feats, fs, b - a, pairs, chunk, skip_last=True))
        return outs

    # ---- DiffusionDet.detect_images ---------------------------------------------------------------------------------------------------------
    def detect(self, images, image_ids=None):
        det = self.det
        result_cls = det.boxlist_cls or _result_class(images)
        imgs, sizes_wh, ids = self.admit("detect_images", images, image_ids)
        if not ids:
            return []
        with det._on_device():
            return self._detect(imgs.tensors, sizes_wh, ids, result_cls)

    def _detect(self, canvas, sizes_wh, ids, result_cls):
        # every upload of the call -- the size table, the frames of a host-side loader, the draws -- BEFORE any kernel is queued (the rule
        # of _extract: a host->device copy from pageable memory blocks the host until the stream has drained)
        up = self.uploads(sizes_wh, ids)
        outs = self.launches(canvas.to(self.det.device, torch.float32).contiguous(), up)
        cap, results = self.chunk(), []          # the host reads the counts only behind the last chunk's launches
        for k, out in enumerate(outs):
            results += self.det._to_boxlists(*out, sizes_wh[k * cap:(k + 1) * cap], result_cls=result_cls)
        return results

    # ---- DiffusionDet.detect_images_aug -----------------------------------------------------------------------------------------------------
    def detect_aug(self, images, image_ids=None):
        det = self.det
        self._refuse("detect_images_aug")
        if not det.cfg.TEST.BBOX_AUG.ENABLED:
            raise NotImplementedError("detect_images_aug: TEST.BBOX_AUG.ENABLED is False (detect_images is the plain path)")
        images = list(images)
        ids = self._ids("detect_images_aug", image_ids, len(images))
        if not images:
            return []
        with det._on_device():
            return self._detect_aug(images, ids)

    def _detect_aug(self, images, ids):
        from ...data import transforms as T
        det = self.det
        result_cls = det.boxlist_cls or BoxList
        n, div = len(images), det.size_divisibility
        # every upload of the call first (the rule of detect): the images, their pointer table, per scale group the resample plan,
        # the size table and the draws, then the merge's table and view 0's sizes
        dev_images = []
        for im in images:
            if not isinstance(im, (torch.Tensor, np.ndarray)):
                im = np.array(im.convert("RGB"))          # a PIL image (a writable copy)
            if im.dtype not in (torch.uint8, np.uint8) or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("detect_images_aug takes uint8 [h, w, 3] images, got %s %s" % (im.dtype, tuple(im.shape)))
            if isinstance(im, np.ndarray):
                im = torch.from_numpy(np.ascontiguousarray(im))
            dev_images.append(im.to(det.device).contiguous())
        srcs = ops.ImageTable(dev_images)
        views = [T.bbox_aug_views(det.cfg, (w, h)) for h, w in srcs.sizes_hw]
        V = len(views[0])
        groups, v0 = [], 0
        for g, (_, _, nv) in enumerate(T.bbox_aug_scales(det.cfg)):
            out_hw = [(vs[v0].h, vs[v0].w) for vs in views]
            plan = T.ViewsPlan(srcs.sizes_hw, out_hw, cache=self._aug_tables).to(det.device)
            PH, PW = -(-plan.max_oh // div) * div, -(-plan.max_ow // div) * div
            sizes_wh = [(ow, oh) for oh, ow in out_hw for _ in range(nv)]
            groups.append((plan, PH, PW, nv, self.uploads(sizes_wh, ids, tuple(range(v0, v0 + nv)))))
            v0 += nv
        if len(self._aug_tables) > 4096:
            self._aug_tables.clear()
        table = ops.bbox_aug_table(views).to(det.device)
        sizes0_wh = [(vs[0].w, vs[0].h) for vs in views]
        sizes0 = ops.FrameSizes(torch.tensor(sizes0_wh, dtype=torch.float32), det.device)
        # launches only from here on
        per_group = []
        for plan, PH, PW, nv, up in groups:
            canvas = ops.resize_views_u8(srcs, plan, PH, PW, nv == 2)
            outs = self.launches(canvas, up)
            ob, osc, ol, oc = (outs[0] if len(outs) == 1 else [torch.cat([o[k] for o in outs]) for k in range(4)])
            cap = osc.shape[1]
            per_group.append((ob.reshape(n, nv, cap, 4), osc.reshape(n, nv, cap), ol.reshape(n, nv, cap), oc.reshape(n, nv)))
        if len(per_group) == 1:
            ob, osc, ol, oc = per_group[0]
        else:
            ob, osc, ol, oc = (torch.cat([g[k] for g in per_group], dim=1) for k in range(4))
        cap = osc.shape[2]
        cand = ops.bbox_aug_merge(ob.reshape(n * V, cap, 4), osc.reshape(n * V, cap), ol.reshape(n * V, cap), oc.reshape(n * V), table, V)
        heads = det.cfg.MODEL.ROI_HEADS
        out = ops.bbox_aug_finish(*cand, sizes0, float(heads.NMS), int(heads.DETECTIONS_PER_IMG))
        return det._to_boxlists(*out, sizes0_wh, result_cls=result_cls)
