"""The demo surface on the CPU: hand-worked frames, the product's numpy path against the painter of _overlay_ref.py, the score text, the
colours, the tables, the frame list without an index file, and the C ABI.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _overlay_cases as C
import _overlay_ref as R
from conftest import ROOT

from diffusionvid_amd.engine import demo


def _blank(h, w, v=7):
    return np.full((h, w, 3), v, dtype=np.uint8)


def _changed(a, b):
    return sorted((int(x), int(y)) for y, x in zip(*np.nonzero((a != b).any(axis=2))))


EMPTY_NAMES = [""] * 8          # the text is the score alone: "0.90", four characters


def test_hand_worked_thickness_one():
    """12 x 16 frame, one box (3, 7) .. (12, 10), t = 1 (o = 0, i = 1), label 7: the ring is the box's outline, the plate of "0.90" with a
    6 x 11 font spans [3, 3 + 4 * 6 + 2 - 1] x [7, 7 + 11 + 2 - 1] = [3, 28] x [7, 19], clipped to x <= 15, y <= 11."""
    src = _blank(12, 16)
    atlas = demo.glyph_atlas()
    assert atlas.shape == (95, 11, 6)
    det = np.array([[3, 7, 12, 10, 0.9, 7]], dtype=np.float32)
    out = demo.render_numpy(src.copy(), det, (1.0, 1.0), demo.name_table(EMPTY_NAMES), 0.7, 1, 1, atlas)
    ring = [(x, y) for y in range(7, 11) for x in range(3, 13) if x in (3, 12) or y in (7, 10)]
    plate = [(x, y) for y in range(7, 12) for x in range(3, 16)]
    assert _changed(out, src) == sorted(set(ring) | set(plate))
    # 2^8 = 1 (mod 255), so 2^25 - 1 = 1, 2^15 - 1 = 127, 2^21 - 1 = 31: the BGR triple of label 7 is (7, 889 % 255, 217) = (7, 124, 217)
    colour = (217, 124, 7)
    text_rows = np.concatenate([atlas[ord(c) - 32] for c in "0.90"], axis=1)          # [11, 24]
    for x, y in plate:
        white = 1 <= y - 7 <= 11 and 1 <= x - 3 <= 24 and text_rows[y - 7 - 1, x - 3 - 1]
        assert tuple(out[y, x]) == ((255, 255, 255) if white else colour), (x, y)
    assert sum(tuple(out[y, x]) == (255, 255, 255) for x, y in plate) > 0
    ref, _ = R.render(src, det, 1, (1.0, 1.0), EMPTY_NAMES, atlas, 0.7, 1, 1)
    assert np.array_equal(out, ref)


def test_hand_worked_thickness_two_at_the_corner():
    """t = 2 (o = 1, i = 1) on a box at (0, 0) .. (5, 4) of a 12 x 16 frame: the outer rectangle starts at x1 - o = -1 and is clipped; the
    hole is [1, 4] x [1, 3], which the plate covers anyway"""
    src = _blank(12, 16, 200)
    atlas = demo.glyph_atlas()
    det = np.array([[0, 0, 5, 4, 0.9, 1]], dtype=np.float32)
    out = demo.render_numpy(src.copy(), det, (1.0, 1.0), demo.name_table(EMPTY_NAMES), 0.7, 2, 1, atlas)
    ring = [(x, y) for y in range(0, 6) for x in range(0, 7) if not (1 <= x <= 4 and 1 <= y <= 3)]
    plate = [(x, y) for y in range(0, 12) for x in range(0, 16)]          # [0, 25] x [0, 12] clipped: the whole frame
    assert _changed(out, src) == sorted(set(ring) | set(plate))
    ref, info = R.render(src, det, 1, (1.0, 1.0), EMPTY_NAMES, atlas, 0.7, 2, 1)
    assert np.array_equal(out, ref) and (info["kind"] != R.KIND_NONE).all()
    # the ring where the plate is not: the same box at x1 = 30 of a wider frame, seen left of it
    wide = _blank(12, 40, 200)
    out = demo.render_numpy(wide.copy(), np.array([[30, 0, 35, 4, 0.9, 1]], dtype=np.float32), (1.0, 1.0), demo.name_table(EMPTY_NAMES), 0.7, 2, 1, atlas)
    got = [(x, y) for x, y in _changed(out, wide) if x < 30]
    assert got == sorted((29, y) for y in range(0, 6))          # x1 - o = 29: the ring's outer column, rows -1 .. 5 clipped to 0 .. 5


@pytest.mark.parametrize("name", sorted(C.random_cases()))
def test_random_cases_meet_their_conditions_and_numpy_equals_the_painter(name):
    case = C.random_cases()[name]
    names = demo.name_table(case["class_names"])
    two = False
    for f, frame in enumerate(case["frames"]):
        args = (case["threshold"], case["thickness"], case["text_scale"])
        ref, info = R.render(frame, case["dets"][f], case["counts"][f], case["ratios"][f], case["class_names"], case["atlas"], *args)
        diff = (ref != frame).any(axis=2)
        assert (diff & (info["kind"] == R.KIND_RING)).any(), "no ring pixel changes"
        assert (diff & (info["kind"] == R.KIND_GLYPH)).any(), "no glyph pixel changes"
        two = two or bool((info["cover"] >= 2).any())
        got = demo.render_numpy(frame.copy(), case["dets"][f, :case["counts"][f]], case["ratios"][f], names, *args, case["atlas"])
        assert np.array_equal(got, ref), (name, f)
    assert two, "no pixel under two drawn detections"


def _all_cases():
    geo, geo_drawn = C.geometry_case()
    ties, ties_drawn = C.ties_case()
    many, many_drawn = C.many_case()
    cases = [("geometry", geo, geo_drawn), ("ties", ties, ties_drawn), ("many", many, many_drawn), ("labels", C.labels_case(), None)]
    cases += [("empty %d" % k, c, []) for k, c in enumerate(C.empty_cases())]
    cases += [("thickness %d scale %d" % (t, s), C.thick_case(t, s), None) for t in (1, 2, 5, 16) for s in (1, 3)]
    cases += [("random atlas", C.thick_case(2, 2, C.random_atlas()), None)]
    return cases


@pytest.mark.parametrize("name,case,drawn", _all_cases(), ids=[c[0] for c in _all_cases()])
def test_hand_made_cases_numpy_equals_the_painter(name, case, drawn):
    names = demo.name_table(case["class_names"])
    for f, frame in enumerate(case["frames"]):
        args = (case["threshold"], case["thickness"], case["text_scale"])
        ref, info = R.render(frame, case["dets"][f], case["counts"][f], case["ratios"][f], case["class_names"], case["atlas"], *args)
        if drawn is not None and (f == 0 or drawn == []):
            assert info["drawn"] == drawn
        if drawn == []:
            assert np.array_equal(ref, frame)
        got = demo.render_numpy(frame.copy(), case["dets"][f, :case["counts"][f]], case["ratios"][f], names, *args, case["atlas"])
        assert np.array_equal(got, ref), (name, f)


def test_labels_case_texts():
    case = C.labels_case()
    _, info = R.render(case["frames"][0], case["dets"][0], case["counts"][0], case["ratios"][0], case["class_names"], case["atlas"])
    assert info["texts"] == ["bg: 0.75", "0.76", "0.77", "a-name-of-24-bytes-xxxxx: 0.78", "0.79", "a name of more than twen: 0.80", "caf??: 0.81"]
    assert len(C.NAMES[2].encode()) == 24


def test_score_text_is_pythons():
    f32 = np.float32
    assert [demo.score_text(f32(v)) for v in (0.125, 0.375, 0.995, 0.705)] == ["0.12", "0.38", "1.00", "0.70"]
    rng = np.random.RandomState(0)
    values = np.concatenate([rng.uniform(0, 9.98, 20000), np.arange(0, 9990) / 1000.0, np.arange(0, 9000) / 8.0 / 125.0,
                             [0.0, 1e-45, 1e-40, 1e-30, 0.004999, 0.005, 0.0050001, 9.985, -0.0, -0.125, -0.5]]).astype(np.float32)
    for v in values:
        assert demo.score_text(v) == "{:.2f}".format(float(v)), repr(v)
    assert demo.score_text(f32(9.994)) == "9.99" and demo.score_text(f32(123.0)) == "9.99"          # hundredths clamp at 999


def test_colours_are_the_references():
    palette = torch.tensor([2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1])
    labels = torch.tensor(list(range(1, 31)) + [1280])
    bgr = ((labels[:, None] * palette) % 255).numpy().astype("uint8")          # compute_colors_for_labels
    for lab, c in zip(labels.tolist(), bgr.tolist()):
        assert demo.label_colour(lab) == (c[2], c[1], c[0])
    assert 1280 * (2 ** 25 - 1) >= 2 ** 32


def test_name_table_and_atlas():
    t = demo.name_table(["", "cat", "x" * 30, "café", "tab\there"])
    assert t.shape == (5, 24) and t.dtype == np.uint8
    assert not t[0].any() and bytes(t[1][:3]) == b"cat" and not t[1][3:].any()
    assert bytes(t[2]) == b"x" * 24 and bytes(t[3][:5]) == b"caf??" and bytes(t[4][:8]) == b"tab?here"
    a = demo.glyph_atlas()
    assert a.shape[0] == 95 and a.dtype == np.uint8 and a.shape[1] <= 32 and a.shape[2] <= 32 and set(np.unique(a)) == {0, 1}
    assert not a[0].any() and a[ord("A") - 32].any()          # the blank, and a letter


def test_select_top_predictions_is_strict_ascending_and_stable():
    from diffusionvid_amd.structures.bounding_box import BoxList
    bl = BoxList(torch.arange(24, dtype=torch.float32).reshape(6, 4), (100, 80))
    bl.add_field("scores", torch.tensor([0.9, 0.7, 0.8, 0.9, 0.95, 0.2]))
    bl.add_field("labels", torch.arange(6))
    top = demo.select_top_predictions(bl, 0.7)
    assert top.get_field("labels").tolist() == [2, 0, 3, 4]


def test_frame_list_from_lengths_equals_an_index_file(tmp_path):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.datasets.vid import VIDFrameList, VIDMEGATestDataset
    lengths = {"val/a": 11, "val/b": 3}
    lines, n = [], 0
    for name, L in lengths.items():
        for f in range(L):
            n += 1
            lines.append("%s %d %d %d" % (name, n, f, L))
    index = tmp_path / "index.txt"
    index.write_text("\n".join(lines) + "\n")
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), ["MODEL.VID.MEGA.GLOBAL.SHUFFLE", False], os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.freeze()
    a = VIDMEGATestDataset(cfg, "dir", str(index), loader=lambda p: p)
    b = VIDMEGATestDataset(cfg, "dir", VIDFrameList.from_lengths(lengths), loader=lambda p: p)
    for key in ("image_set_index", "pattern", "frame_id", "frame_seg_id", "frame_seg_len", "video_format"):
        assert getattr(a.frames, key) == getattr(b.frames, key), key
    assert len(a) == len(b) == 14 and a.start_index == b.start_index
    for i in range(len(a)):
        (ia, _, ida), (ib, _, idb) = a[i], b[i]
        assert ida == idb and set(ia) == set(ib)
        for k in ia:
            assert ia[k] == ib[k], (i, k)
    with pytest.raises(ValueError):
        VIDFrameList.from_lengths({})


def test_run_on_video_refuses():
    d = demo.VIDDemo.__new__(demo.VIDDemo)
    with pytest.raises(NotImplementedError, match="video decoder"):
        d.run_on_video("clip.mp4")


def test_generate_images_writes_numbered_jpegs(tmp_path):
    d = demo.VIDDemo.__new__(demo.VIDDemo)
    d.output_folder = str(tmp_path / "out")
    paths = d.generate_images([_blank(8, 10), torch.from_numpy(_blank(8, 10, 90))])
    assert [os.path.basename(p) for p in paths] == ["000000.jpg", "000001.jpg"] and all(os.path.getsize(p) > 0 for p in paths)
    assert sorted(os.listdir(d.output_folder)) == ["000000.jpg", "000001.jpg"]


def test_c_abi_carries_the_overlay_entry():
    import ctypes
    from diffusionvid_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.dvid_version() >= 10
    for name, nargs in (("dvid_overlay_detections", 19), ("dvid_overlay_scratch_bytes", 2), ("dvid_overlay_tile", 2)):
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    defines = dict(re.findall(r"#define (DVID_OVERLAY_\w+) (\d+)", header))
    assert int(defines["DVID_OVERLAY_MAX_DRAWN"]) == ops.OVERLAY_MAX_DRAWN == demo.MAX_DRAWN == R.MAX_DRAWN == 256
    assert int(defines["DVID_OVERLAY_NAME_MAX"]) == ops.OVERLAY_NAME_MAX == demo.NAME_MAX == R.NAME_MAX == 24
    tw, th = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.dvid_overlay_tile(ctypes.byref(tw), ctypes.byref(th)))
    assert (tw.value, th.value) == ops.OVERLAY_TILE == C.TILE
    assert callable(ops.overlay_detections) and ops.overlay_scratch_bytes(3, 100) > 0
