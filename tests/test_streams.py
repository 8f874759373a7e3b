"""Several live streams on one model, the host side: the C ABI surface of the grouped kernels, the refusals of open_streams and of
StreamSet.step (all before any engine exists), the grouping of streams by memory shape, and the slot scheduling of
engine.inference.compute_on_streams on a stub model.  No GPU."""
import os
import re

import pytest
import torch

from conftest import ROOT

BASE = os.path.join(ROOT, "configs", "BASE_RCNN_1gpu.yaml")
R101_YAML = os.path.join(ROOT, "configs", "vid_R_101_DiffusionVID.yaml")
STREAMING = ["INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0, "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1,
             "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0, "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False]
# symbol -> number of arguments in include/dvid_hip.h
SYMBOLS = {"dvid_cdist_groups": 6, "dvid_fps_greedy_groups": 7, "dvid_gather_rows_groups": 8, "dvid_update_memory_groups": 9,
           "dvid_global_memory_project_groups": 5, "dvid_global_xattn_groups": 7}


def _detector(opts=()):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector.diffusion_det import DiffusionDet
    cfg = get_cfg(R101_YAML, STREAMING + list(opts), BASE)
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    return DiffusionDet(cfg).eval()


def test_grouped_symbols_in_header_library_and_bindings():
    from diffusionvid_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    lib = _lib.load()
    assert lib.dvid_version() >= 4
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/dvid_hip.h" % name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    assert "DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES (1ll << 30)" in header
    from diffusionvid_amd import ops
    assert ops.UPDATE_MEMORY_MAX_SCRATCH_BYTES == 1 << 30
    for fn in ("cdist_groups", "fps_greedy_groups", "gather_rows_groups", "update_erase_memory_groups"):
        assert callable(getattr(ops, fn))
    for fn in ("global_xattn_groups", "ensure_memory_groups_projected", "invalidate_memory_groups"):
        assert callable(getattr(ops.Model, fn))


def test_grouped_ops_refuse_host_tensors():
    from diffusionvid_amd import _lib, ops
    with pytest.raises(_lib.DvidError):
        ops.cdist_groups(torch.zeros(2, 4, 8))
    with pytest.raises(_lib.DvidError):
        ops.update_erase_memory_groups(torch.zeros(2, 4, 8), torch.zeros(2, 3, 8), 5)
    with pytest.raises(_lib.DvidError, match=r"\[G, k, d\]"):
        ops.update_erase_memory_groups(torch.zeros(4, 8), None, 2)


@pytest.mark.parametrize("opts,keys", [
    (["INPUT.INFER_BATCH", 8, "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 8, "MODEL.VID.MEGA.MAX_OFFSET", 7], ["INFER_BATCH 8", "ALL_FRAME_INTERVAL 8", "MAX_OFFSET 7"]),
    (["MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 3], ["ALL_FRAME_INTERVAL 3"]),
    (["MODEL.VID.MEGA.MAX_OFFSET", 2], ["MAX_OFFSET 2"]),
    (["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0], ["GLOBAL.ENABLE is False"]),
    (["MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", True], ["STOP_UPDATE_AFTER_INIT_TEST is True"]),
])
def test_open_streams_refuses_other_protocols_naming_the_key(opts, keys):
    det = _detector(opts)
    with pytest.raises(NotImplementedError) as e:
        det.open_streams()
    for k in keys:
        assert k in str(e.value), (k, str(e.value))
    assert det._engine is None          # refused before any engine exists


def test_open_streams_refuses_key_frame_location_and_lookahead():
    from diffusionvid_amd.modeling.detector import streams
    det = _detector()
    mega = det.cfg.MODEL.VID.MEGA
    mega.KEY_FRAME_LOCATION = 1
    with pytest.raises(NotImplementedError, match="KEY_FRAME_LOCATION 1"):
        streams.refuse_unless_streaming(det.cfg)
    mega.KEY_FRAME_LOCATION = 0
    det.cfg.INPUT.LOOKAHEAD_BATCHES = 2
    with pytest.raises(NotImplementedError, match="LOOKAHEAD_BATCHES 2"):
        streams.refuse_unless_streaming(det.cfg)
    det.cfg.INPUT.LOOKAHEAD_BATCHES = 1
    streams.refuse_unless_streaming(det.cfg)
    with pytest.raises(ValueError, match="frames_per_launch"):
        det.open_streams(frames_per_launch=0)


def _item(frame_id, n_g, h=64, w=96, category=None):
    f = lambda: torch.zeros(1, 3, h, w)
    return {"cur": f(), "ref_l": [f()], "ref_g": [f() for _ in range(n_g)], "frame_category": (0 if frame_id == 0 else 1) if category is None else category,
            "frame_id": frame_id, "start_id": 0, "end_id": 9}


def test_step_refusals_come_before_any_launch():
    det = _detector()
    s = det.open_streams()
    assert s.step({}) == {}
    with pytest.raises(ValueError, match=r"stream 'a'.*exactly one local frame.*got 2"):
        bad = _item(0, 2)
        bad["ref_l"] = bad["ref_l"] * 2
        s.step({"a": bad})
    with pytest.raises(ValueError, match=r"stream 'b' holds no memory.*frame_category 1.*frame_id 3"):
        s.step({"b": _item(3, 1)})
    with pytest.raises(ValueError, match=r"stream 'b'.*\(1, 3, 32, 96\).*\(1, 3, 64, 96\).*one set, one frame size"):
        s.step({"a": _item(0, 2), "b": _item(0, 2, h=32)})
    with pytest.raises(ValueError, match="ref_g is empty"):
        s.step({"a": _item(0, 0)})
    assert det._engine is None and s.streams() == []          # nothing ran, nothing was opened
    s.close("c")          # an unknown id: nothing to drop
    with pytest.raises(KeyError):
        s.global_memory("c")
    with pytest.raises(ValueError, match="adopt_memory takes"):
        s.adopt_memory("c", [torch.zeros(900, 128), torch.zeros(150, 256)])


def test_streams_are_grouped_by_memory_shape():
    from diffusionvid_amd.modeling.detector.streams import plan_memory_groups
    # a: steady; b: steady; c: opening with 24 global frames; d: opening with 4; e: growing (300 / 100 rows held); f: no global frame
    rows = {"a": (900, 150), "b": (900, 150), "c": (0, 0), "d": (0, 0), "e": (300, 100), "f": (900, 150)}
    new = {"a": (75, 25), "b": (75, 25), "c": (1800, 600), "d": (300, 100), "e": (75, 25), "f": (0, 0)}
    updates, finals = plan_memory_groups(rows, new, (900, 150))
    assert updates[0] == [((900, 75), ["a", "b"]), ((0, 1800), ["c"]), ((0, 300), ["d"]), ((300, 75), ["e"])]
    assert updates[1] == [((150, 25), ["a", "b"]), ((0, 600), ["c"]), ((0, 100), ["d"]), ((100, 25), ["e"])]
    # the final stage runs once per distinct shape of memory 0 AFTER the update: 900 rows (a, b, c, f), 300 (d), 375 (e)
    assert finals == [(900, ["a", "b", "c", "f"]), (300, ["d"]), (375, ["e"])]
    # memory 1 reaches its 150 rows before memory 0 reaches 900: grouped per memory, so e and a second stream at (450, 150) share nothing
    updates, finals = plan_memory_groups({"e": (375, 125), "g": (450, 150)}, {"e": (75, 25), "g": (75, 25)}, (900, 150))
    assert updates[1] == [((125, 25), ["e"]), ((150, 25), ["g"])] and finals == [(450, ["e"]), (525, ["g"])]


class _StubDataset:
    """videos of unequal length following the streaming item protocol, with the reference's frame_seg_id table"""

    def __init__(self, lengths, with_table=True):
        self.items, seg = [], []
        for v, n in enumerate(lengths):
            for f in range(n):
                seg.append(f)
                self.items.append(({"cur": None, "ref_l": [None], "ref_g": [None], "frame_category": 0 if f == 0 else 1, "frame_id": f, "start_id": 0,
                                    "end_id": n - 1, "video": v}, None, [len(self.items)]))
        if with_table:
            self.frame_seg_id = seg
        self.loads = []

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        self.loads.append(idx)
        return self.items[idx]


class _StubStreams:
    def __init__(self, log):
        self.log, self.frame = log, {}

    def step(self, items):
        self.log.append({s: (it["video"], it["frame_id"]) for s, it in items.items()})
        out = {}
        for s, it in items.items():
            assert it["frame_id"] == (0 if it["frame_category"] == 0 else self.frame[s] + 1), "a slot delivers its video's calls in order"
            self.frame[s] = it["frame_id"]
            out[s] = [_StubResult((it["video"], it["frame_id"]))]
        return out


class _StubResult:
    def __init__(self, tag):
        self.tag = tag

    def to(self, device):
        return self


class _StubModel:
    def __init__(self):
        self.log = []

    def eval(self):
        return self

    def open_streams(self):
        return _StubStreams(self.log)


@pytest.mark.parametrize("with_table", [True, False])
def test_compute_on_streams_slot_scheduling(with_table):
    from diffusionvid_amd.engine import inference as eng
    lengths = [3, 1, 2, 4, 1]
    ds, model = _StubDataset(lengths, with_table), _StubModel()
    results = eng.compute_on_streams(model, ds, 2)
    # every image id exactly once, carrying its own video's frame
    assert sorted(results) == list(range(sum(lengths)))
    expect = [(v, f) for v, n in enumerate(lengths) for f in range(n)]
    assert [results[i].tag for i in range(len(expect))] == expect
    # slot 1's one-frame video ends on step 0: it holds video 2 on step 1; slot 0 ends video 0 on step 2 and holds video 3 on step 3
    assert model.log == [{0: (0, 0), 1: (1, 0)}, {0: (0, 1), 1: (2, 0)}, {0: (0, 2), 1: (2, 1)}, {0: (3, 0), 1: (4, 0)}, {0: (3, 1)}, {0: (3, 2)}, {0: (3, 3)}]
    if with_table:
        assert sorted(ds.loads) == list(range(sum(lengths)))          # every item loaded once
    # more slots than videos, and one slot: the video order
    assert len(_run(eng, lengths, 8)) == max(lengths)
    assert [list(s.values())[0] for s in _run(eng, lengths, 1)] == expect
    with pytest.raises(ValueError, match="n_streams"):
        eng.compute_on_streams(_StubModel(), _StubDataset(lengths), 0)


def _run(eng, lengths, n):
    model = _StubModel()
    eng.compute_on_streams(model, _StubDataset(lengths), n)
    return model.log
