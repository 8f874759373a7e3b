"""Several live streams on one model: one frame of each per call.

The latency-oriented protocol (INFER_BATCH 1, ALL_FRAME_INTERVAL 1, MAX_OFFSET 0, GLOBAL.STOP_UPDATE_AFTER_INIT_TEST False) delivers one
frame and one new global frame per call and re-prunes both global memories on every call: two-frame launches and two single-workgroup
farthest-point sweeps, which cannot fill the chip.  A `StreamSet` (DiffusionDet.open_streams) takes one such call of EACH of N streams
per `step` and runs them together on the one set of weights:

  1. one extraction sequence (backbone, the extraction heads, top-k selection) over all frames of all items, `frames_per_launch` at a time;
  2. the memory updates, grouped: streams whose memory holds the same rows and receives the same number of new rows are pruned by ONE
     ops.update_erase_memory_groups per memory (a workgroup per stream for the sweep), the 150-row launch on a second stream beside the
     900-row one.  In the steady state a group's memories live in one [G, rows, d] tensor that the update writes and the attention reads;
  3. the final stage once per distinct memory shape, through DiffusionDet._final_stage_launch with one slot per stream and the grouped
     global attention (ops.Model.global_xattn_groups).

The contract: per stream, the detections and the memories are bit-equal to what a private model of the same weights returns for the same
items through `model(item)`, call by call -- whatever other streams share the step, in whatever order, at whatever `frames_per_launch`.
It holds because every stage is per-frame independent, the grouped kernels compute each group as the single form does, and the draws
keep the video path's keys: (kind, the stream's own frame_id, split, image), `box_init` split 0 the frame, splits 1.. its global frames.

A step reads and writes no state of the detector's video path (queue, look-ahead results, head.proposal_feats_global, captured graphs,
the engine's single-memory projection): a video run through `model(item)` between steps gets what it gets alone.  Nothing is replayed
from a hipGraph.
"""
import torch

from ... import ops
from ...structures.image_list import to_image_list
from .diffusion_det import _result_class, take


def refuse_unless_streaming(cfg):
    """NotImplementedError unless `cfg` is the streaming protocol with an updating global memory; every message names its keys and values"""
    mega = cfg.MODEL.VID.MEGA
    lookahead = max(1, int(getattr(cfg.INPUT, "LOOKAHEAD_BATCHES", 1)))
    if not (cfg.INPUT.INFER_BATCH == 1 and mega.ALL_FRAME_INTERVAL == 1 and mega.MAX_OFFSET == 0 and mega.KEY_FRAME_LOCATION == 0 and lookahead == 1):
        raise NotImplementedError(
            "open_streams serves the streaming protocol only: INPUT.INFER_BATCH == MODEL.VID.MEGA.ALL_FRAME_INTERVAL == 1, MODEL.VID.MEGA.MAX_OFFSET == 0, "
            "MODEL.VID.MEGA.KEY_FRAME_LOCATION == 0, INPUT.LOOKAHEAD_BATCHES == 1 (got INFER_BATCH %d, ALL_FRAME_INTERVAL %d, MAX_OFFSET %d, "
            "KEY_FRAME_LOCATION %d, LOOKAHEAD_BATCHES %d)"
            % (cfg.INPUT.INFER_BATCH, mega.ALL_FRAME_INTERVAL, mega.MAX_OFFSET, mega.KEY_FRAME_LOCATION, lookahead))
    if not mega.GLOBAL.ENABLE:
        raise NotImplementedError("open_streams: MODEL.VID.MEGA.GLOBAL.ENABLE is False, and a stream is conditioned on its global memory "
                                  "(local-attention-only streams are not built)")
    if mega.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST:
        raise NotImplementedError("open_streams: MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST is True: the memory of a live stream is updated on "
                                  "every call (set it to False)")


def plan_memory_groups(rows, new_rows, targets):
    """The grouping of one step, host logic.  rows: {stream: (rows held of memory 0, of memory 1)} (0: none yet), new_rows: {stream: (rows
    arriving for memory 0, for memory 1)}, targets: (900, 150); the dicts' order is the streams' layout order.
    -> (updates, finals): updates[i] = [((rows held, new rows), [streams])] for memory i, streams receiving nothing left out;
    finals = [(rows of memory 0 after the update, [streams])], the final stage's passes."""
    updates = []
    for i in range(2):
        groups = {}
        for s, held in rows.items():
            if new_rows[s][i] > 0:
                groups.setdefault((held[i], new_rows[s][i]), []).append(s)
        updates.append(list(groups.items()))
    finals = {}
    for s, held in rows.items():
        finals.setdefault(min(held[0] + new_rows[s][0], targets[0]), []).append(s)
    return updates, list(finals.items())


class StreamSet:
    def __init__(self, detector, frames_per_launch=32):
        refuse_unless_streaming(detector.cfg)
        if int(frames_per_launch) < 1:
            raise ValueError("frames_per_launch must be at least 1, got %r" % (frames_per_launch,))
        self.det = detector
        self.frames_per_launch = int(frames_per_launch)
        self.targets = (detector.mem_management_size_test, 150)          # diffusion_det.py:479-488
        self._mem = {}          # stream id -> [memory 0, memory 1]: rows of a packed [G, rows, d] tensor in the steady state
        self._opened = {}       # stream id -> its rank in the layout order (the order of opening)
        self._n_opened = 0
        self._packs = [{}, {}]          # per memory: (stream ids) -> the [G, rows, d] tensor those streams' memories are rows of
        self._frame_shape = None        # (padded shape, (h, w)) of the set's first frame
        self._side = None

    # ---- stream state ---------------------------------------------------------------------------------------------------------------------
    def streams(self):
        return list(self._opened)

    def _open(self, sid):
        if sid not in self._opened:
            self._opened[sid] = self._n_opened
            self._n_opened += 1

    def close(self, sid):
        """drops the stream's state (its id may be opened again later, as a new stream)"""
        self._opened.pop(sid, None)
        self._drop_memory(sid)

    def global_memory(self, sid):
        """[memory 0, memory 1] of the stream (copies), the counterpart of DiffusionDet.global_memory()"""
        if sid not in self._mem:
            raise KeyError("stream %r holds no memory" % (sid,))
        return [m.clone() for m in self._mem[sid]]

    def adopt_memory(self, sid, memory):
        """installs [memory 0, memory 1] as the stream's memories (opening it if need be), the counterpart of adopt_video_memory()"""
        memory = list(memory)
        d = self.det.hidden_dim
        if len(memory) != 2 or any(m.dim() != 2 or m.shape[1] != d or m.shape[0] < 1 for m in memory):
            raise ValueError("adopt_memory takes [memory 0 [rows, %d], memory 1 [rows, %d]]" % (d, d))
        self._open(sid)
        self._drop_memory(sid)
        self._mem[sid] = [m.detach().to(self.det.device, torch.float32).clone().contiguous() for m in memory]

    # ---- one step -------------------------------------------------------------------------------------------------------------------------
    def _validate(self, items):
        """everything `step` refuses, before any launch -> {stream: (frame ImageList, [global ImageLists])}"""
        parsed, first = {}, self._frame_shape
        for sid, item in items.items():
            if not isinstance(item, dict):
                raise TypeError("stream %r: an item is the dict of one call of the streaming protocol" % (sid,))
            ref_l = [to_image_list(im) for im in item["ref_l"]]
            ref_g = [to_image_list(im) for im in item["ref_g"]]
            if len(ref_l) != 1:
                raise ValueError("stream %r: an item carries exactly one local frame (ref_l), got %d" % (sid, len(ref_l)))
            if item["frame_category"] != 0 and sid not in self._mem:
                raise ValueError("stream %r holds no memory and its item is not an opening one (frame_category %r, frame_id %r): a stream starts "
                                 "with frame_category 0 or with adopt_memory" % (sid, item["frame_category"], item["frame_id"]))
            if item["frame_category"] == 0 and not ref_g:
                raise ValueError("stream %r: an opening item (frame_category 0) carries the global frames its memory is built from (ref_g is empty)" % (sid,))
            cur = to_image_list(item["cur"])
            for im in [cur] + ref_l + ref_g:
                shape = (tuple(im.tensors.shape), tuple(int(v) for v in im.image_sizes[0]))
                first = first or shape
                if shape != first or im.tensors.shape[0] != 1:
                    raise ValueError("stream %r: a frame of padded shape %s and size %s in a set whose first frame has %s and %s (one set, one frame size)"
                                     % (sid, shape[0], shape[1], first[0], first[1]))
            parsed[sid] = (ref_l[0], ref_g)
        self._frame_shape = first
        return parsed

    def step(self, items):
        """items: {stream id: item}, an item being exactly the dict the dataset emits for one call of the streaming protocol (cur, ref_l
        with one frame, ref_g, frame_category, frame_id, start_id, end_id); frame_category 0 (re)starts that stream's video, an unseen id
        is opened.  -> {stream id: [BoxList]}: what a private model returns for the item."""
        det = self.det
        if det.training:
            raise NotImplementedError("training is out of scope of the MI355X inference path")
        if not items:
            return {}
        parsed = self._validate(items)
        for sid in items:
            self._open(sid)
        with det._on_device():
            return self._step(items, parsed)

    def _step(self, items, parsed):
        det = self.det
        held, new_rows = {}, {}
        for sid in items:
            if items[sid]["frame_category"] == 0:          # a new video: its memory starts empty
                self._drop_memory(sid)
            mem = self._mem.get(sid)
            held[sid] = (mem[0].shape[0], mem[1].shape[0]) if mem is not None else (0, 0)
            new_rows[sid] = tuple(len(parsed[sid][1]) * k for k in det.top_k)
        # the layout order: streams of one final-stage pass side by side, inside a pass by order of opening -- whatever the dict's order
        after0 = {sid: min(held[sid][0] + new_rows[sid][0], self.targets[0]) for sid in items}
        order = sorted(items, key=lambda s: (-after0[s], self._opened[s]))
        held = {s: held[s] for s in order}
        updates, finals = plan_memory_groups(held, new_rows, self.targets)

        local, glob = self._extract(order, items, parsed)
        self._update_memories(updates, glob)

        h, w = parsed[order[0]][0].image_sizes[0]
        size, pairs = (int(w), int(h)), det._time_pairs()
        launched, pos = [], {s: i for i, s in enumerate(order)}
        for _, sids in finals:
            a, b = pos[sids[0]], pos[sids[-1]] + 1          # a pass's streams are adjacent in the layout
            sp = local(a, b)
            ddim = {items[s]["frame_id"]: det._ddim_draws(1, items[s]["frame_id"], pairs) for s in sids} if det.sampling_timesteps > 1 else {}
            memory = self._packed(0, sids)
            det.head.proposal_feats_global_groups = memory
            try:
                out = det._final_stage_launch(sp["feats"], (sp["logits"], sp["boxes"], sp["obj"]), size, pairs,
                                              [(items[s]["frame_id"], 1) for s in sids], ddim, slots=1)
            finally:
                det.head.proposal_feats_global_groups = None
            launched.append((sids, out))
        results = {}          # the host reads the counts only behind the last pass's launches
        cls = det.boxlist_cls
        for sids, out in launched:
            boxlists = det._to_boxlists(*out, size, result_cls=cls or _result_class(items[sids[0]]["cur"]))
            for s, bl in zip(sids, boxlists):
                results[s] = [bl]
        return {s: results[s] for s in items}

    def _drop_memory(self, sid):
        self._mem.pop(sid, None)
        for packs in self._packs:
            for ids in [k for k in packs if sid in k]:
                # the other streams keep their rows of the pack (views); the pack itself is no longer one group's memory
                del packs[ids]

    def _packed(self, i, sids):
        """[G, rows, d]: memory `i` of the streams `sids` -- the tensor their memories are rows of when they were pruned together, else a stack"""
        ids = tuple(sids)
        pack = self._packs[i].get(ids)
        if pack is not None:
            return pack
        return torch.stack([self._mem[s][i] for s in sids])

    # ---- 1. extraction ----------------------------------------------------------------------------------------------------------------------
    def _extract(self, order, items, parsed):
        """Backbone + the extraction heads + top-k selection over [every stream's frame | every stream's global frames], in launch sequences
        of `frames_per_launch` frames; -> (local(a, b): the split of the frames of streams a..b of the layout, {stream: (k1 rows, k2 rows)
        of its global frames}).  DiffusionDet._extract for several calls at once: the same stages, the same keys for the draws."""
        det = self.det
        eng, M, d = det._get_engine(), det.num_proposals, det.hidden_dim
        frames = [parsed[s][0].tensors for s in order]
        noise = [det._noise("box_init", items[s]["frame_id"], 0, 0, (1, M, 4)) for s in order]
        g_at = {}
        for s in order:
            g_at[s] = (len(frames), len(frames) + len(parsed[s][1]))
            for bi, im in enumerate(parsed[s][1]):
                frames.append(im.tensors)
                noise.append(det._noise("box_init", items[s]["frame_id"], bi + 1, 0, (1, M, 4)))
        n_local, n_total = len(order), len(frames)
        # every upload -- host frames, host draws -- BEFORE any kernel is queued (the rule of DiffusionDet._extract)
        as_list = all(f.is_cuda and f.device == det.device and f.dtype == torch.float32 and f.shape[0] == 1 for f in frames)
        total = None if as_list else torch.cat(frames).to(det.device, torch.float32)
        box_init_all = torch.cat(noise)
        fh, fw = frames[0].shape[-2:]
        hh, ww = parsed[order[0]][0].image_sizes[0]
        size = (int(ww), int(hh))
        cap = self.frames_per_launch
        eng.reserve(min(cap, n_total), fh, fw, M)
        per_frame = []
        for ci, a in enumerate(range(0, n_total, cap)):
            b = min(n_total, a + cap)
            feats = eng.backbone_frames(frames[a:b]) if as_list else eng.backbone(total[a:b].contiguous())
            res = det._extract_launch(feats, size, box_init_all[a:b], max(n_local, a) - a, b - a, ci)
            per_frame += [(res, i) for i in range(b - a)]

        glob = {}
        for s, (a, b) in g_at.items():
            if b > a:
                sp = take(per_frame, a, b, keys=("k1", "k2"), with_feats=False)
                glob[s] = (sp["k1"].reshape(-1, d), sp["k2"].reshape(-1, d))
        return (lambda a, b: take(per_frame, a, b, keys=("logits", "boxes", "obj"))), glob

    # ---- 2. memory update -------------------------------------------------------------------------------------------------------------------
    def _update_memories(self, updates, glob):
        det = self.det
        eng = det._get_engine()
        side = det.memory_on_side_stream and bool(updates[0]) and bool(updates[1])
        cur = torch.cuda.current_stream()
        if side:
            if self._side is None:
                self._side = torch.cuda.Stream(device=det.device)
            self._side.wait_stream(cur)
        packs = [{}, {}]
        for i in (1, 0):          # the 150-row launches beside the 900-row ones, as DiffusionDet._build_memory runs them
            on_side = side and i == 1
            with torch.cuda.stream(self._side if on_side else cur):
                for (rows, _), sids in updates[i]:
                    ids = tuple(sids)
                    new = torch.stack([glob[s][i] for s in sids])
                    old = None if rows == 0 else self._packed(i, sids)
                    inplace = old is not None and rows == self.targets[i] and self._packs[i].get(ids) is old
                    mem, _ = ops.update_erase_memory_groups(new, old, self.targets[i], out=old if inplace else None)
                    if on_side:
                        new.record_stream(self._side)
                        if not inplace:
                            mem.record_stream(cur)
                    for g, s in enumerate(sids):
                        self._mem.setdefault(s, [None, None])[i] = mem[g]
                    packs[i][ids] = mem
        if side:
            cur.wait_stream(self._side)
        for i in range(2):
            for ids, pack in self._packs[i].items():          # a pack nobody updated this step stays what it was
                if ids not in packs[i] and not any(set(ids) & set(k) for k in packs[i]):
                    packs[i][ids] = pack
        self._packs = packs
        eng.invalidate_memory_groups()          # a pack written in place keeps its version counter
