"""DynamicHead -- host-side mirror of the reference decoder's plugin surface
(mega_core/modeling/roi_heads/box_head/box_head.py:155-435), computing on libdvid_hip.

Same constructor signature, attributes the detector mutates (`proposal_feats_global`,
`proposal_feats_local`, `proposals_feat_cur`, `top_k`, `num_heads_local`, `use_topk`) and
`forward(features, init_bboxes, t, init_features, box_extract=0)` return conventions:

  box_extract > 0 : ([class_logits [B,M,C], bboxes [B,M,4], proposal_features [1,B*M,d]],
                     top-75 features [B*75,d], top-25 features [B*25,d])      (:286-317)
  box_extract == 0: (class_logits[None], pred_bboxes[None]) of the conditioned head (:319-432)

Every RCNNHead / RCNNHead_cond pass, the global and the local cross-attention and the top-k feature
selection run as HIP kernels (ops.Model); this class only sequences them.  Training is out of scope.

Local box-level attention (MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE, box_head.py:186-194, :360-363):
`attn_ = LayerNorm_i(MHA_i(query, key = value = proposal_feats_local[i]))` for i < STAGE, with the query
never updated and no residual -- only the LAST stage's result survives, so only it is launched
(STAGE 1: the top-75 memory, STAGE 2: the top-25 memory with `local_attention.1`'s parameters; STAGE > 2
indexes past the two memories in the reference and is refused here).  With GLOBAL.ENABLE also true the
global stage overwrites `attn_` (:366-371, adaptive_norm is hard-wired True): the local product is
unobservable and the local launch is skipped -- local + global computes what global alone computes.
`proposal_feats_local_groups` (this repo's addition, default 1): the two local memories hold that many
equal blocks, block g serving the g-th block of the call's frames (the detector's look-ahead schedule
finishes several batches in one call, each with its own local memory).
"""
import torch
from torch import nn

from .... import ops


class DynamicHead(nn.Module):
    def __init__(self, cfg, roi_input_shape=None, engine_provider=None):
        super().__init__()
        d = cfg.MODEL.DiffusionDet
        self.num_classes = d.NUM_CLASSES
        self.d_model = d.HIDDEN_DIM
        self.num_heads = d.NUM_HEADS
        self.num_heads_local = d.NUM_HEADS_LOCAL
        self.adaptive_norm = True
        self.return_intermediate = d.DEEP_SUPERVISION
        self.local_enable = cfg.MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE
        self.global_enable = cfg.MODEL.VID.MEGA.GLOBAL.ENABLE
        self.global_stage = cfg.MODEL.VID.MEGA.GLOBAL.RES_STAGE
        self.local_stage = 0
        if self.local_enable:
            self.local_stage = int(cfg.MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE)
            if not 1 <= self.local_stage <= 2:
                raise NotImplementedError("MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE must be 1 or 2, got %d: stage i attends proposal_feats_local[i] "
                                          "and there are two local memories (top-75, top-25); the reference fails on a third" % self.local_stage)
        if self.global_enable and self.global_stage != 1:
            raise NotImplementedError("GLOBAL.RES_STAGE != 1 is not supported")
        self.infer_batch = cfg.INPUT.INFER_BATCH
        self.top_k = [min(x, d.NUM_PROPOSALS) for x in (75, 25)]          # box_head.py:235-236
        self.sampling_timesteps = d.SAMPLE_STEP
        self.use_topk = False
        self.proposal_feats_global = [None, None]
        self.proposal_feats_local = [None, None]
        self.proposal_feats_local_groups = 1
        # this repo's addition: None, or a tensor [G, lk, d] of G global memories read INSTEAD of proposal_feats_global[0] -- the pass's frames
        # are G equal blocks, block g attending memory g (detector/streams.py sets it around a step's final stage and clears it)
        self.proposal_feats_global_groups = None
        self.proposals_feat_cur = []
        self._engine_provider = engine_provider

    # ------------------------------------------------------------------------------------
    def _engine(self):
        if self._engine_provider is None:
            raise ops._lib.DvidError("DynamicHead has no compute engine attached (build it through DiffusionDet)")
        return self._engine_provider()

    @staticmethod
    def _as_nhwc(features, eng):
        """The engine's layout: NHWC in its feature dtype (fp16, or fp32 with DTYPE float32).  The detector hands its own backbone
        outputs over in that layout; a caller with the reference's NCHW maps (box_head.py:273: list[Tensor NCHW]) gets them converted."""
        feats = []
        for f in features:
            c = eng.hidden_dim
            if f.dtype == eng.feat_dtype and f.dim() == 4 and f.shape[-1] == c and (f.dtype == torch.float16 or f.shape[1] != c):
                feats.append(f)                       # already the engine's layout
            elif eng.feat_dtype == torch.float32:
                if f.dim() != 4 or f.shape[1] != c:
                    raise ops._lib.DvidError("DynamicHead: feature maps must be NCHW with %d channels (or the engine's NHWC tensors)" % c)
                feats.append(f.float().permute(0, 2, 3, 1).contiguous())
            else:
                feats.append(ops.nhwc_from_nchw(f.float()))   # reference layout: NCHW
        return feats

    def forward(self, features, init_bboxes, t, init_features, box_extract=0):
        if self.training:
            raise NotImplementedError("training is out of scope of the MI355X inference path")
        if init_features is not None:
            raise NotImplementedError("init_features is unused by DiffusionVID inference (always None, diffusion_det.py:662-664)")
        eng = self._engine()
        feats = self._as_nhwc(features, eng)
        bs, num_boxes = init_bboxes.shape[:2]
        if len(feats) not in (3, 4):
            raise ops._lib.DvidError("DynamicHead: the pyramid is [p3, p4, p5] or [p2, p3, p4, p5], got %d maps" % len(feats))
        stride = 32 >> (len(feats) - 1)          # of the finest map: 8 for p3..p5, 4 for p2..p5
        height, width = feats[0].shape[1] * stride, feats[0].shape[2] * stride
        eng.reserve(max(bs, self.infer_batch), height, width, num_boxes)
        t_host = torch.as_tensor(t).to("cpu", torch.int64)
        flag = self._bad_flag(init_bboxes.device)
        bboxes = init_bboxes

        if box_extract > 0 or self.sampling_timesteps > 1:
            proposal_features = None
            for i in range(self.num_heads):
                class_logits, bboxes, proposal_features = eng.rcnn_head(i, feats, height, width, bboxes, proposal_features, t_host,
                                                                       bad_flag=flag)
        else:
            class_logits, bboxes, proposal_features = self.proposals_feat_cur.pop()      # box_head.py:300-302
            proposal_features = proposal_features.reshape(-1, self.d_model)

        if box_extract > 0:
            k1, k2 = ops.select_topk_features(class_logits, proposal_features, self.top_k[0], self.top_k[1])
            return [class_logits, bboxes, proposal_features.unsqueeze(0)], k1, k2

        if not self.global_enable and not self.local_enable:
            return class_logits[None], bboxes[None]

        if self.global_enable:
            # (with local attention also on, its product would be overwritten here: it is not launched, see the module docstring)
            grouped = self.proposal_feats_global_groups
            memory = self.proposal_feats_global[0] if grouped is None else grouped
            if memory is None:
                raise RuntimeError("proposal_feats_global is empty: the detector fills it from the global frames of a video")
            if grouped is not None:          # [G, lk, d], one memory per live stream: frame block g attends memory g
                attn_ = eng.global_xattn_groups(proposal_features, memory)
            else:
                attn_ = eng.global_xattn(proposal_features, memory)                       # box_head.py:366-394
        else:
            stage = self.local_stage - 1                                                  # the only stage whose result survives
            memory = self.proposal_feats_local[stage]
            if memory is None:
                raise RuntimeError("proposal_feats_local is empty: the detector fills it from the local frame queue")
            if eng.local_stages != self.local_stage:
                raise ops._lib.DvidError("ATTENTION.STAGE %d but the weights hold %d local attention stage(s)" % (self.local_stage, eng.local_stages))
            attn_ = eng.local_xattn(proposal_features, memory, groups=self.proposal_feats_local_groups, stage=stage)   # box_head.py:360-363
        class_logits2, bboxes2 = class_logits, bboxes
        for i in range(self.num_heads_local):
            class_logits2, bboxes2, proposal_features = eng.rcnn_head(i, feats, height, width, bboxes2, proposal_features, t_host,
                                                                      cond=attn_, bad_flag=flag)
        return class_logits2[None], bboxes2[None]

    def plain_heads(self, features, init_bboxes, t, intermediate=False, tail_inputs=False, interact_inputs=False, obj_features=False):
        """The NUM_HEADS RCNNHeads on `init_bboxes` and nothing else -> (class_logits [B, M, C], bboxes [B, M, 4]): what forward computes for
        a model without attention, with no cache popped or filled and no memory read (the detector's still-image path).
        intermediate=True: every head's output, stacked -> (class_logits [NUM_HEADS, B, M, C], bboxes [NUM_HEADS, B, M, 4]), the last one
        being what the default returns (the deep supervision of the training objective reads them all).  tail_inputs=True (DTYPE float32
        models only): one more return value, every head's tail input -- its fp32 norm2 output, what box_head.tail.head_tail takes as x --
        stacked [NUM_HEADS, B * M, d]; the other values keep their bits.  interact_inputs=True (float32 models only): two more behind
        those, what box_head.interact.inst_interact takes as p and roi -- every head's fp32 norm1 output [NUM_HEADS, B * M, d] and its fp32
        RoI tiles [NUM_HEADS, B * M, 49, d]; the other values keep their bits.  obj_features=True: one more behind everything else,
        every head's obj_features stacked [NUM_HEADS, B * M, d] -- head h + 1 takes head h's as its pro_features, the x of
        box_head.attention.self_attention; they are held between the heads anyway, so nothing is copied and the other values keep their bits."""
        eng = self._engine()
        feats = self._as_nhwc(features, eng)
        if len(feats) not in (3, 4):
            raise ops._lib.DvidError("DynamicHead: the pyramid is [p3, p4, p5] or [p2, p3, p4, p5], got %d maps" % len(feats))
        bs, num_boxes = init_bboxes.shape[:2]
        stride = 32 >> (len(feats) - 1)
        height, width = feats[0].shape[1] * stride, feats[0].shape[2] * stride
        eng.reserve(bs, height, width, num_boxes)
        t_host = torch.as_tensor(t).to("cpu", torch.int64)
        flag = self._bad_flag(init_bboxes.device)
        class_logits, bboxes, proposal_features = None, init_bboxes, None
        kept, tails, inters, tiles, objs = [], [], [], [], []
        for i in range(self.num_heads):
            if interact_inputs:
                res = eng.rcnn_head(i, feats, height, width, bboxes, proposal_features, t_host, bad_flag=flag, keep_tail_input=tail_inputs,
                                    keep_interact_input=True)
                class_logits, bboxes, proposal_features = res[:3]
                tails.append(res[3]) if tail_inputs else None
                inters.append(res[-2]), tiles.append(res[-1])
            elif tail_inputs:
                class_logits, bboxes, proposal_features, x = eng.rcnn_head(i, feats, height, width, bboxes, proposal_features, t_host, bad_flag=flag,
                                                                           keep_tail_input=True)
                tails.append(x)
            else:
                class_logits, bboxes, proposal_features = eng.rcnn_head(i, feats, height, width, bboxes, proposal_features, t_host, bad_flag=flag)
            if intermediate:
                kept.append((class_logits, bboxes))
            if obj_features:
                objs.append(proposal_features)
        out = (torch.stack([k[0] for k in kept]), torch.stack([k[1] for k in kept])) if intermediate else (class_logits, bboxes)
        out = out + (torch.stack(tails),) if tail_inputs else out
        out = out + (torch.stack(inters), torch.stack(tiles)) if interact_inputs else out
        return out + (torch.stack(objs),) if obj_features else out

    # device flag standing in for `assert (pred_boxes[:, 2:] >= pred_boxes[:, :2]).all()` (box_head.py:588)
    def _bad_flag(self, device):
        f = getattr(self, "_flag", None)
        if f is None or f.device != device:
            self._flag = torch.zeros(1, dtype=torch.int32, device=device)
        return self._flag

    def check_boxes_valid(self):
        """Raises the reference's AssertionError if any head produced x2<x1 / y2<y1 (host sync)."""
        f = getattr(self, "_flag", None)
        if f is not None and int(f.item()) != 0:
            f.zero_()
            raise AssertionError("pred_boxes[:, 2:] >= pred_boxes[:, :2] violated (box_head.py:588)")
