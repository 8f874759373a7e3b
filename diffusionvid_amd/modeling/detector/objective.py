"""The training objective of a DiffusionDet on labelled batches of still images (diffusion_det.py:338-375): the criterion, the diffusion
step of an image, the ragged ground truth, the forward that DiffusionDet.loss_sums / compute_losses / loss_gradients share, and the
gradient with respect to the head outputs.  A batch is admitted and chunked by the detector's StillImages (detector/stills.py); like it,
an `Objective` holds the detector and none of its video state.
"""
import functools
import math

import torch
import torch.nn.functional as F

from ... import ops
from ..roi_heads.box_head import attention as A
from ..roi_heads.box_head import interact as I
from ..roi_heads.box_head import tail as T
from ..roi_heads.box_head.loss import (LOSS_KEYS, HungarianMatcherDynamicK, SetCriterionDynamicK, check_limits, coef_from_counts,
                                       losses_from_sums)


TAIL_PARAMS = ("linear1.", "linear2.", "norm3.", "block_time_mlp.", "cls_module.", "reg_module.", "class_logits.", "bboxes_delta.")


class Objective:
    def __init__(self, detector):
        self.det = detector

    @functools.cached_property
    def criterion(self):
        """SetCriterionDynamicK over HungarianMatcherDynamicK with the weights of diffusion_det.py:275-299, built on first use: a config the
        criterion refuses (USE_FED_LOSS) still detects"""
        det = self.det
        d = det.cfg.MODEL.DiffusionDet
        matcher = HungarianMatcherDynamicK(cfg=det.cfg, cost_class=d.CLASS_WEIGHT, cost_bbox=d.L1_WEIGHT, cost_giou=d.GIOU_WEIGHT, use_focal=det.use_focal)
        weights = {"loss_ce": d.CLASS_WEIGHT, "loss_bbox": d.L1_WEIGHT, "loss_giou": d.GIOU_WEIGHT}
        if d.DEEP_SUPERVISION:
            for i in range(det.num_heads + det.num_heads_local - 1):
                weights.update({k + "_%d" % i: v for k, v in list(weights.items())[:3]})
        return SetCriterionDynamicK(cfg=det.cfg, num_classes=det.num_classes, matcher=matcher, weight_dict=weights, eos_coef=d.NO_OBJECT_WEIGHT,
                                    losses=["labels", "boxes"], use_focal=det.use_focal)

    @property
    def weights(self):
        """{loss name: CLASS_WEIGHT / L1_WEIGHT / GIOU_WEIGHT}, every head output's names with DEEP_SUPERVISION"""
        return self.criterion.weight_dict

    def train_step(self, image_id):
        """The diffusion step of an image's loss, a uniform integer in [0, num_timesteps): the reference draws torch.randint per image
        (diffusion_det.py:695).  With a noise_fn it is derived from the image's key on the host: z = the one N(0, 1) draw of kind
        "train_t" keyed (image_id, step 0, image 0), u = Phi(z) = (1 + erf(z / sqrt 2)) / 2 in float64, t = min(floor(u * num_timesteps),
        num_timesteps - 1) -- a pure function of the id, uniform because Phi(z) is.  Without a noise_fn: torch.randint."""
        det = self.det
        if det.noise_fn is None:
            return int(torch.randint(0, det.num_timesteps, (1,)))
        z = float(det.noise_fn("train_t", int(image_id), 0, 0, (1,)).reshape(-1)[0])
        u = 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
        return min(int(u * det.num_timesteps), det.num_timesteps - 1)

    def _pack(self, what, targets, sizes_wh):
        """The ground truth, ragged, on the host -> (absolute xyxy in the image's own size, normalised (cx, cy, w, h) for q_sample, labels
        1-based, starts int32 [n + 1])"""
        M = self.det.num_proposals
        gt_abs, gt_norm, labels, starts = [], [], [], [0]
        for i, (t, (w, h)) in enumerate(zip(targets, sizes_wh)):
            if tuple(int(v) for v in t.size) != (w, h):
                raise ValueError("%s: target %d is for a %s image, the image is %s" % (what, i, tuple(t.size), (w, h)))
            if not t.has_field("labels"):
                raise ValueError("%s: target %d carries no `labels` field" % (what, i))
            b = t.convert("xyxy").bbox.detach().to("cpu", torch.float32).reshape(-1, 4)
            if b.shape[0] > M:
                raise NotImplementedError("%s: image %d holds %d ground-truth boxes, MODEL.DiffusionDet.NUM_PROPOSALS is %d (the reference's "
                                          "random subset is not built)" % (what, i, b.shape[0], M))
            nb = b / torch.tensor([w, h, w, h], dtype=torch.float32)
            gt_abs.append(b), labels.append(t.get_field("labels").detach().to("cpu", torch.int32).reshape(-1))
            gt_norm.append(torch.stack(((nb[:, 0] + nb[:, 2]) / 2, (nb[:, 1] + nb[:, 3]) / 2, nb[:, 2] - nb[:, 0], nb[:, 3] - nb[:, 1]), dim=1))
            starts.append(starts[-1] + b.shape[0])
        return torch.cat(gt_abs), torch.cat(gt_norm), torch.cat(labels), torch.tensor(starts, dtype=torch.int32)

    THROUGH = ("outputs", "tail", "interact")

    def check_through(self, through):
        """what loss_gradients(through=...) refuses, each by name, before anything is built or launched"""
        if through not in self.THROUGH:
            raise ValueError("loss_gradients: through=%r is not one of %s" % (through, ", ".join(repr(v) for v in self.THROUGH)))
        if through != "outputs":
            if self.det.dtype != "float32":
                raise NotImplementedError("loss_gradients: through=%r needs DTYPE float32, this model is %s (fp16 gradients are out of scope)"
                                          % (through, self.det.dtype))
            T.check_dropout(self.det.cfg, "loss_gradients")

    def tail_params(self, head):
        """{name without the prefix: fp32 device tensor} of head_series.<head>'s tail, copied on first use and kept while the engine lives"""
        det = self.det
        eng = det._get_engine()
        if getattr(self, "_tail_cache", (None,))[0] is not eng:
            self._tail_cache = (eng, {})
        cache = self._tail_cache[1]
        if head not in cache:
            pfx = "head.head_series.%d." % head
            cache[head] = {k[len(pfx):]: v.detach().to(det.device, torch.float32).contiguous() for k, v in det.state_dict().items()
                           if k.startswith(pfx) and k[len(pfx):].startswith(TAIL_PARAMS)}
        return cache[head]

    def interact_params(self, head):
        """{name without the prefix: fp32 device tensor} of head_series.<head>'s instance interaction and norm2, kept as tail_params keeps its own"""
        det = self.det
        eng = det._get_engine()
        if getattr(self, "_interact_cache", (None,))[0] is not eng:
            self._interact_cache = (eng, {})
        cache = self._interact_cache[1]
        if head not in cache:
            pfx = "head.head_series.%d." % head
            sd = det.state_dict()
            cache[head] = {k: sd[pfx + k].detach().to(det.device, torch.float32).contiguous() for k in I.PARAM_NAMES}
        return cache[head]

    def attn_params(self, head):
        """{name without the prefix: fp32 device tensor} of head_series.<head>'s self-attention and norm1, kept as tail_params keeps its own"""
        det = self.det
        eng = det._get_engine()
        if getattr(self, "_attn_cache", (None,))[0] is not eng:
            self._attn_cache = (eng, {})
        cache = self._attn_cache[1]
        if head not in cache:
            pfx = "head.head_series.%d." % head
            sd = det.state_dict()
            cache[head] = {k: sd[pfx + k].detach().to(det.device, torch.float32).contiguous() for k in A.PARAM_NAMES}
        return cache[head]

    def check_chain(self):
        """what head_gradients refuses, each by name, before anything is built or launched: check_through("interact")'s conditions"""
        if self.det.dtype != "float32":
            raise NotImplementedError("head_gradients: needs DTYPE float32, this model is %s (fp16 gradients are out of scope)" % self.det.dtype)
        T.check_dropout(self.det.cfg, "head_gradients")

    def chain_backward(self, tail_in, boxes_in, interact_in, roi_tiles, obj, steps, d_logits, d_boxes, roi_gradients):
        """The backward over ALL heads, from the last to the first: per head ops.head_tail_backward (the head's own d_logits / d_boxes, null
        for a head without a loss of its own, and d_obj = the next head's d_attn_in), ops.inst_interact_backward, ops.self_attn_backward.
        A head's x is the previous head's obj_features (`obj`), the first head's the mean over the bins of its RoI tiles, whose share
        d_attn_in[0] / 49 is added to every bin of d_roi[0].  time_mlp's four gradients: torch's autograd through time_embedding's arithmetic
        with the summed d_time_emb.  tail_in / interact_in / obj [H, R, d], roi_tiles [H, R, 49, d], boxes_in [H, n, M, 4]; d_logits /
        d_boxes [S, n, M, .] with S = H (DEEP_SUPERVISION) or 1 (the last head's).  -> {"param_grads"} and, with roi_gradients, "d_roi"."""
        H, R = tail_in.shape[:2]
        n = steps.numel()
        S = d_logits.shape[0]
        time_emb = self.time_embedding(steps)
        grads, d_time_emb, d_attn_in, d_roi = {}, torch.zeros_like(time_emb), None, [None] * H
        for h in reversed(range(H)):
            s = h - (H - S)          # the head's own output among the kept ones
            own = (d_logits[s].reshape(R, -1), d_boxes[s].reshape(R, 4)) if s >= 0 else (None, None)
            t = ops.head_tail_backward(tail_in[h], boxes_in[h].reshape(R, 4), time_emb, self.tail_params(h), d_logits=own[0], d_boxes=own[1], d_obj=d_attn_in)
            i = ops.inst_interact_backward(interact_in[h], roi_tiles[h], self.interact_params(h), d_y=t["d_x"], want_d_roi=roi_gradients)
            x = obj[h - 1] if h > 0 else roi_tiles[0].mean(1)
            a = ops.self_attn_backward(x, n, self.attn_params(h), d_y=i["d_p"])
            for part in (t, i, a):
                grads.update({"head.head_series.%d.%s" % (h, k): v for k, v in part["param_grads"].items()})
            d_time_emb += t["d_time_emb"]
            d_attn_in, d_roi[h] = a["d_x"], i["d_roi"]
        grads.update(self.time_mlp_gradients(steps, d_time_emb))
        out = {"param_grads": grads}
        if roi_gradients:
            d_roi[0] = d_roi[0] + (d_attn_in / roi_tiles.shape[2])[:, None, :]
            out["d_roi"] = torch.stack(d_roi)
        return out

    def time_mlp_gradients(self, steps, d_time_emb):
        """{"head.time_mlp.<1|3>.<weight|bias>": gradient} of sum(d_time_emb * time_mlp(t)): torch's autograd through time_embedding's own
        arithmetic on the device -- n rows, plumbing"""
        names = ["head.time_mlp." + k for k in ("1.weight", "1.bias", "3.weight", "3.bias")]
        sd = self.det.state_dict()
        with torch.enable_grad():
            w = {k: sd[k].detach().to(self.det.device, torch.float32).requires_grad_(True) for k in names}
            emb = self.time_embedding(steps, {k[len("head.time_mlp."):]: v for k, v in w.items()})
            got = torch.autograd.grad(emb, [w[k] for k in names], d_time_emb)
        return dict(zip(names, got))

    def interact_backward(self, kept_heads, out, interact_in, roi_tiles, roi_gradients):
        """ops.inst_interact_backward for every kept head on the tail's d_tail_in -> the entries loss_gradients(through="interact") adds to
        the tail's dict `out`.  An earlier head's d_tail_in lacks the next head's path through pro_features, so its twelve go to "partial"."""
        out.update({"d_interact_in": [], "interact_in": interact_in, "roi_tiles": roi_tiles})
        d_roi = []
        for s, head in enumerate(kept_heads):
            g = ops.inst_interact_backward(interact_in[s], roi_tiles[s], self.interact_params(head), d_y=out["d_tail_in"][s], want_d_roi=roi_gradients)
            whole = "param_grads" if head == self.det.num_heads - 1 else "partial"
            for k, v in g["param_grads"].items():
                out[whole]["head.head_series.%d.%s" % (head, k)] = v
            out["d_interact_in"].append(g["d_p"])
            d_roi.append(g["d_roi"])
        out["d_interact_in"] = torch.stack(out["d_interact_in"])
        if roi_gradients:
            out["d_roi"] = torch.stack(d_roi)
        return out

    def time_embedding(self, steps, weights=None):
        """time_mlp(t) [n, 4 d] in fp32 on the device (box_head.py:218-223: sinusoidal embedding, Linear, GELU, Linear); `weights`
        {"1.weight", ...}: those tensors instead of the state dict's (time_mlp_gradients differentiates through them)"""
        det = self.det
        sd = det.state_dict()
        d = det.cfg.MODEL.DiffusionDet.HIDDEN_DIM
        half = d // 2
        freq = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000.0) / (half - 1)))
        arg = steps.to(torch.float32)[:, None] * freq[None, :]
        emb = torch.cat((arg.sin(), arg.cos()), dim=-1).to(det.device)
        w = lambda k: sd["head.time_mlp." + k].detach().to(det.device, torch.float32) if weights is None else weights[k]
        return F.linear(F.gelu(F.linear(emb, w("1.weight"), w("1.bias"))), w("3.weight"), w("3.bias")).contiguous()

    def tail_backward(self, kept_heads, tail_in, boxes_in, steps, d_logits, d_boxes):
        """ops.head_tail_backward for every kept head -> the tail entries of loss_gradients(through="tail")"""
        n, M = d_logits.shape[1:3]
        time_emb = self.time_embedding(steps)
        out = {"param_grads": {}, "partial": {}, "d_tail_in": [], "d_time_emb": torch.zeros_like(time_emb), "tail_in": tail_in, "boxes_in": boxes_in,
               "time_emb": time_emb}
        for s, head in enumerate(kept_heads):
            g = ops.head_tail_backward(tail_in[s], boxes_in[s].reshape(n * M, 4), time_emb, self.tail_params(head), d_logits=d_logits[s].reshape(n * M, -1),
                                       d_boxes=d_boxes[s].reshape(n * M, 4))
            last = head == self.det.num_heads - 1
            for k, v in g["param_grads"].items():
                whole = last or not k.startswith(("linear1.", "linear2.", "norm3."))
                out["param_grads" if whole else "partial"]["head.head_series.%d.%s" % (head, k)] = v
            out["d_tail_in"].append(g["d_x"])
            out["d_time_emb"] += g["d_time_emb"]
        out["d_tail_in"] = torch.stack(out["d_tail_in"])
        return out

    def forward(self, images, targets, image_ids, gradients, through="outputs", roi_gradients=False, chain=False):
        """The forward sums and gradients share -> (the device tuple of ops.set_criterion, None or (d_logits, d_boxes) of the sum of the
        weighted losses with respect to the kept head outputs, from ops.set_criterion_backward on the same stream; with through="tail" a
        third entry, the dict of tail_backward, which through="interact" extends by interact_backward's).  chain=True (head_gradients; with
        through="interact"): the same forward, the inputs of ALL heads kept with or without DEEP_SUPERVISION and every head's obj_features;
        the third entry is then chain_backward's dict with "roi_tiles" and "boxes_in"."""
        det = self.det
        what = "head_gradients" if chain else "loss_gradients" if gradients else "compute_losses"
        tail = gradients and through in ("tail", "interact")
        interact = gradients and through == "interact"
        if isinstance(images, dict):
            raise NotImplementedError("%s: the video item dict (cur / ref_l / ref_g) of the training protocol is not built; "
                                      "hand over a batch of still images" % what)
        imgs, sizes_wh, ids = det.stills.admit(what, images)
        n = len(sizes_wh)
        if image_ids is not None:
            ids = [int(i) for i in image_ids]
        if len(ids) != n or len(targets) != n:
            raise ValueError("%s: %d image_ids and %d targets for %d images" % (what, len(ids), len(targets), n))
        if n == 0:
            raise ValueError("%s: an empty batch has no loss" % what)
        criterion = self.criterion          # refuses USE_FED_LOSS by key
        gt_abs, gt_norm, labels, starts = self._pack(what, targets, sizes_wh)
        check_limits(det.num_proposals, det.num_classes, criterion.matcher.ota_k, (starts[1:] - starts[:-1]).tolist())
        steps = torch.tensor([self.train_step(i) for i in ids], dtype=torch.int64)
        deep = det.cfg.MODEL.DiffusionDet.DEEP_SUPERVISION
        keep_all = deep or chain          # every head's inputs, or the last head's
        with torch.no_grad(), det._on_device():
            dev = det.device
            # every upload and draw before any kernel is queued (the rule of StillImages.detect)
            sizes = ops.FrameSizes(torch.tensor(sizes_wh, dtype=torch.float32), dev)
            noise, placeholder = det.stills.draws("train_noise", ids, 0), det.stills.draws("train_placeholder", ids, 0)
            up = [t.to(dev) for t in (gt_abs, gt_norm, labels)]
            if gradients:          # the weights of the kept head outputs, the final one last
                sfx = ["_%d" % s for s in range(det.num_heads - 1)] + [""] if deep else [""]
                weights = torch.tensor([[float(self.weights.get(k + x, 1.0)) for k in LOSS_KEYS] for x in sfx], dtype=torch.float64).to(dev)
            canvas = imgs.tensors.to(dev, torch.float32).contiguous()
            x_boxes = ops.q_sample_boxes(up[1], starts, steps, det.sqrt_alphas_cumprod, det.sqrt_one_minus_alphas_cumprod, noise, placeholder,
                                         det.scale, sizes)
            logits, boxes, tail_in, boxes_in, inter_in, tiles, objs = [], [], [], [], [], [], []
            for a, b, feats in det.stills.chunks(canvas):
                if tail:          # the same launches plus one copy per head: every head's tail input, and the boxes each head started from
                    if interact:          # and two more: the norm1 output and the RoI tiles
                        lg, bx, tx, px, rx, *ox = det.head.plain_heads(feats, x_boxes[a:b].contiguous(), steps[a:b], intermediate=True, tail_inputs=True,
                                                                       interact_inputs=True, obj_features=chain)
                        inter_in.append(px.reshape(px.shape[0], b - a, -1, px.shape[-1]) if keep_all else px[-1:].reshape(1, b - a, -1, px.shape[-1]))
                        tiles.append(rx.reshape(rx.shape[0], b - a, -1, *rx.shape[-2:]) if keep_all else rx[-1:].reshape(1, b - a, -1, *rx.shape[-2:]))
                        if chain:
                            objs.append(ox[0].reshape(ox[0].shape[0], b - a, -1, ox[0].shape[-1]))
                    else:
                        lg, bx, tx = det.head.plain_heads(feats, x_boxes[a:b].contiguous(), steps[a:b], intermediate=True, tail_inputs=True)
                    bi = torch.cat((x_boxes[a:b][None], bx[:-1]))
                    tail_in.append(tx.reshape(tx.shape[0], b - a, -1, tx.shape[-1]) if keep_all else tx[-1:].reshape(1, b - a, -1, tx.shape[-1]))
                    boxes_in.append(bi if keep_all else bi[-1:])
                else:
                    lg, bx = det.head.plain_heads(feats, x_boxes[a:b].contiguous(), steps[a:b], intermediate=True)
                if not deep:
                    lg, bx = lg[-1:], bx[-1:]
                logits.append(lg), boxes.append(bx)
            logits, boxes = torch.cat(logits, dim=1), torch.cat(boxes, dim=1)
            if det.debug_taps is not None:
                det.debug_taps.setdefault("train_heads", []).append((logits, boxes, x_boxes, steps))
            out = criterion.sums(logits, boxes, (up[0], up[2], starts, sizes))
            if not gradients:
                return out, None
            # d(sum of the weighted losses): weight / denominator per head output, the denominators from the matched counts on the device
            assert logits.shape[0] == weights.shape[0], "one row of weights per kept head output"
            p = criterion.matcher.params()
            coef = coef_from_counts(weights, out[2][:, :, 3].sum(1))
            grads = ops.set_criterion_backward(logits, boxes, up[0], up[2], starts, sizes, p["alpha"], p["gamma"], out[0], out[3], coef)
            if not tail:
                return out, grads
            tail_in = torch.cat(tail_in, dim=1)
            if chain:
                rows = lambda ts: (lambda t: t.reshape(t.shape[0], -1, *t.shape[3:]).contiguous())(torch.cat(ts, dim=1))
                boxes_in, tiles = torch.cat(boxes_in, dim=1).contiguous(), rows(tiles)
                res = self.chain_backward(rows([tail_in]), boxes_in, rows(inter_in), tiles, rows(objs), steps, grads[0], grads[1], roi_gradients)
                return out, grads, dict(res, roi_tiles=tiles, boxes_in=boxes_in)
            kept = list(range(det.num_heads)) if deep else [det.num_heads - 1]
            res = self.tail_backward(kept, tail_in.reshape(tail_in.shape[0], -1, tail_in.shape[-1]).contiguous(),
                                     torch.cat(boxes_in, dim=1).contiguous(), steps, grads[0], grads[1])
            if interact:
                inter_in, tiles = torch.cat(inter_in, dim=1), torch.cat(tiles, dim=1)
                res = self.interact_backward(kept, res, inter_in.reshape(inter_in.shape[0], -1, inter_in.shape[-1]).contiguous(),
                                             tiles.reshape(tiles.shape[0], -1, *tiles.shape[-2:]).contiguous(), roi_gradients)
            return out, grads, res

    def _weighted(self, sums):
        return {k: v * self.weights.get(k, 1.0) for k, v in losses_from_sums(sums).items()}

    def sums(self, images, targets, image_ids=None):
        out = self.forward(images, targets, image_ids, False)[0]
        return out[2].detach().to("cpu", torch.float64), out

    def losses(self, images, targets, image_ids=None):
        return self._weighted(self.sums(images, targets, image_ids)[0])

    def head_gradients(self, images, targets, image_ids=None, roi_gradients=False):
        self.check_chain()
        out, grads, res = self.forward(images, targets, image_ids, True, "interact", roi_gradients, chain=True)
        keep = ("param_grads", "d_roi", "roi_tiles", "boxes_in") if roi_gradients else ("param_grads",)
        return dict({k: res[k] for k in keep}, losses=self._weighted(out[2].detach().to("cpu", torch.float64)), d_logits=grads[0], d_boxes=grads[1])

    def gradients(self, images, targets, image_ids=None, through="outputs", roi_gradients=False):
        self.check_through(through)
        res = self.forward(images, targets, image_ids, True, through, roi_gradients)
        out, grads = res[:2]
        losses = self._weighted(out[2].detach().to("cpu", torch.float64))
        if through == "outputs":
            return losses, grads[0], grads[1]
        return dict(res[2], losses=losses, d_logits=grads[0], d_boxes=grads[1])
