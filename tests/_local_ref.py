"""Test-local restatement of the local box-level attention branch (mega_core/modeling/roi_heads/box_head/box_head.py:338, :360-363;
mega_core/modeling/detector/diffusion_det.py:398-400, :507-512) from the oracle's existing primitives.  oracle/ itself is a yardstick
and stays as it is; tests/test_local_attention.py pins this restatement to the reference through g18, and the GPU tests take their
expected values from it."""
from collections import deque

import torch

from oracle import detector as odet, head as ohead, precision, schedule
from oracle.schedule import time_mlp


def local_attention(sd, pfx, proposal_features, local, stages, cfg, groups=1):
    """The reference's loop as written: every stage attends the UN-updated query, the last one wins.  proposal_features [1, R, d];
    local = [memory of stage 0, memory of stage 1], each `groups` equal blocks (block g serves the g-th block of the queries)."""
    d = proposal_features.shape[-1]
    query_ = proposal_features.permute(1, 0, 2)
    rows = query_.shape[0] // groups
    attn_ = None
    for i in range(stages):
        lk = local[i].shape[0] // groups
        outs = []
        for g in range(groups):
            kv = local[i][g * lk:(g + 1) * lk].unsqueeze(1)
            with precision.stage("head.local_attention"):
                a = ohead._mha(sd, f"{pfx}local_attention.{i}.0", query_[g * rows:(g + 1) * rows], kv, kv, cfg.nheads)
            outs.append(ohead._ln(a, sd, f"{pfx}local_attention.{i}.2"))
        attn_ = torch.cat(outs)
    return attn_.reshape(-1, d)


def head_final_local(sd, pfx, features, init_bboxes, t, cfg, cached, local, stages, groups=1):
    """DynamicHead.forward, box_extract == 0, ATTENTION.ENABLE True / GLOBAL.ENABLE False (box_head.py:300-302, :319-432)."""
    time = time_mlp(sd, pfx, t, cfg.hidden_dim)
    if cfg.sampling_timesteps > 1:
        bboxes, proposal_features = init_bboxes, None
        for i in range(cfg.num_heads):
            class_logits, bboxes, proposal_features = ohead.rcnn_head(sd, f"{pfx}head_series.{i}", features, bboxes, proposal_features, time, cfg)
    else:
        class_logits, bboxes, proposal_features = cached
    attn_ = local_attention(sd, pfx, proposal_features, local, stages, cfg, groups)
    query_ = proposal_features.permute(1, 0, 2)
    for i in range(cfg.num_heads_local):
        class_logits, bboxes, pf2 = ohead.rcnn_head(sd, f"{pfx}head_series_cond.{i}", features, bboxes, query_.permute(1, 0, 2), time, cfg, cond=attn_)
        query_ = pf2.permute(1, 0, 2)
    return class_logits[None], bboxes[None]


def fill_indices(frame_category, frame_id, start_id, n_local, key_frame_location, interval):
    """diffusion_det.py:491-496"""
    if frame_category == 0:
        lead = key_frame_location - (frame_id - start_id)
        return [0] * lead + list(range(n_local)) + [n_local - 1] * (interval - (lead + n_local))
    return list(range(n_local))


class LocalOracleDet(odet.OracleDiffusionDet):
    """The oracle detector carrying the reference's two local deques (proposals_feat: each queued frame's top-75 features,
    proposals_feat_dis: its top-25), conditioned on them instead of the global memory."""

    def __init__(self, sd, cfg, noise_fn, stages, **kw):
        super().__init__(sd, cfg, noise_fn, **kw)
        self.stages = stages
        self.local_log = []          # head.proposal_feats_local after every working call

    def forward(self, images):
        c = self.cfg
        if images["frame_category"] == 0:
            self.proposals_feat = deque(maxlen=c.all_frame_interval)
            self.proposals_feat_dis = deque(maxlen=c.all_frame_interval)
            waiting = 0
        else:
            waiting = len(self.local_img_queue)
        self._meta = (images["frame_category"], images["frame_id"], images["start_id"], waiting + len(images["ref_l"]))
        self._k, self._filled = [], False
        return super().forward(images)

    def _fill(self):
        c = self.cfg
        cat, frame_id, start_id, n_local = self._meta
        k1 = torch.cat([a for a, _ in self._k]).view(-1, c.head.top_k[0], c.hidden_dim)[:n_local]
        k2 = torch.cat([b for _, b in self._k]).view(-1, c.head.top_k[1], c.hidden_dim)[:n_local]
        for i in fill_indices(cat, frame_id, start_id, n_local, c.key_frame_location, c.all_frame_interval):
            self.proposals_feat.append(k1[i])
            self.proposals_feat_dis.append(k2[i])
        self.local = [torch.cat(list(self.proposals_feat)), torch.cat(list(self.proposals_feat_dis))]
        self.local_log.append(self.local)
        self._filled = True

    def model_predictions(self, feats, images_whwh, x, t, cached=None, mem=None, box_extract=0):
        if box_extract:
            out = super().model_predictions(feats, images_whwh, x, t, box_extract=box_extract)
            self._k.append((out[1], out[2]))
            return out
        if not self._filled:
            self._fill()
        c = self.cfg
        x_boxes = schedule.noise_to_boxes(x, images_whwh, c.snr_scale)
        outputs_class, outputs_coord = head_final_local(self.sd, "head.", feats, x_boxes, t, c.head, cached, self.local, self.stages)
        x_start = schedule.boxes_to_x_start(outputs_coord[-1], images_whwh, c.snr_scale)
        return (schedule.predict_noise_from_start(self.buf, x, t, x_start), x_start), outputs_class, outputs_coord
