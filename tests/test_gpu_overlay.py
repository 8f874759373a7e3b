"""ops.overlay_detections on the GPU, bit-equal to the painter of _overlay_ref.py on every case of _overlay_cases.py (whose input
conditions tests/test_overlay.py checks on the CPU): odd widths (53, 2 * tw + 1), heights 1 / 37 / 2 * th + 1, a list of three sizes in one
launch and the [n, H, W, 3] form, frames with nothing to draw, boxes on tile edges and frame borders, skipped and non-finite rows, garbage
behind `counts`, ties, the 256-row cut, labels and names at their limits, every thickness and text scale, two atlases."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _overlay_cases as C  # noqa: E402
import _overlay_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert ops.OVERLAY_TILE == C.TILE
    return ops


def _reference(case):
    args = (case["threshold"], case["thickness"], case["text_scale"])
    return [R.render(fr, case["dets"][f], case["counts"][f], case["ratios"][f], case["class_names"], case["atlas"], *args)
            for f, fr in enumerate(case["frames"])]


def _run(dv, case, batch=False):
    """the kernels on a case -> list of numpy frames; batch: the [n, H, W, 3] form (frames of one size)"""
    from diffusionvid_amd.engine import demo
    frames = [torch.from_numpy(f).cuda() for f in case["frames"]]
    if batch:
        frames = torch.stack(frames)
    names = torch.from_numpy(demo.name_table(case["class_names"])).cuda()
    out = dv.overlay_detections(frames, torch.from_numpy(case["dets"]).cuda(), torch.from_numpy(case["counts"]).cuda(), torch.from_numpy(case["ratios"]).cuda(),
                                names, torch.from_numpy(case["atlas"]).cuda(), case["threshold"], case["thickness"], case["text_scale"])
    assert out is frames          # in place
    return [f.cpu().numpy() for f in out]


def _assert_equal(got, ref, what):
    for f, (g, (want, _)) in enumerate(zip(got, ref)):
        bad = np.nonzero((g != want).any(axis=2))
        assert len(bad[0]) == 0, "%s, frame %d: %d pixels differ, the first at (x, y) = (%d, %d)" % (what, f, len(bad[0]), bad[1][0], bad[0][0])


@pytest.mark.parametrize("name", sorted(C.random_cases()))
def test_random_cases(dv, name):
    case = C.random_cases()[name]
    ref = _reference(case)
    for f, (want, info) in enumerate(ref):          # the conditions on the inputs, on the reference alone
        diff = (want != case["frames"][f]).any(axis=2)
        assert (diff & (info["kind"] == R.KIND_RING)).any() and (diff & (info["kind"] == R.KIND_GLYPH)).any()
    assert any((info["cover"] >= 2).any() for _, info in ref)
    _assert_equal(_run(dv, case), ref, name)
    if len(case["frames"]) == 1:
        _assert_equal(_run(dv, case, batch=True), ref, name + " [n, H, W, 3]")


def test_batch_form_of_several_frames(dv):
    case = C.random_case(40, [(37, 53)] * 3)
    _assert_equal(_run(dv, case, batch=True), _reference(case), "three frames as one tensor")


def test_nothing_to_draw_leaves_the_bytes(dv):
    for k, case in enumerate(C.empty_cases()):
        got = _run(dv, case)
        for g, src in zip(got, case["frames"]):
            assert np.array_equal(g, src), k
        _assert_equal(got, _reference(case), "empty %d" % k)


def test_geometry(dv):
    for t in (1, 2, 5):
        case, drawn = C.geometry_case(t)
        ref = _reference(case)
        assert ref[0][1]["drawn"] == drawn
        _assert_equal(_run(dv, case), ref, "geometry, thickness %d" % t)


def test_ties_and_the_256_row_cut(dv):
    for make in (C.ties_case, C.many_case):
        case, drawn = make()
        ref = _reference(case)
        assert ref[0][1]["drawn"] == drawn and case["counts"][0] == case["dets"].shape[1]          # counts == cap
        _assert_equal(_run(dv, case), ref, make.__name__)
    assert len(drawn) == 256


def test_labels_and_names(dv):
    case = C.labels_case()
    ref = _reference(case)
    assert ref[0][1]["texts"][:3] == ["bg: 0.75", "0.76", "0.77"] and len(ref[0][1]["texts"]) == 7
    _assert_equal(_run(dv, case), ref, "labels")


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("thickness", [1, 2, 5, 16])
def test_thickness_and_scale(dv, thickness, scale):
    for atlas in (None, C.random_atlas()):
        case = C.thick_case(thickness, scale, atlas)
        _assert_equal(_run(dv, case), _reference(case), "thickness %d scale %d" % (thickness, scale))


def test_refusals_carry_the_numbers(dv):
    from diffusionvid_amd import _lib
    from diffusionvid_amd.engine import demo
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    names = torch.from_numpy(demo.name_table(C.NAMES)).cuda()
    atlas = torch.from_numpy(C.pillow_atlas()).cuda()
    counts, ratios = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones((1, 2), device="cuda")

    def go(cap=4, names=names, atlas=atlas, **kw):
        dv.overlay_detections([frame], torch.zeros((1, cap, 6), device="cuda"), counts, ratios, names, atlas, **kw)
    with pytest.raises(_lib.DvidError, match=r"4097 rows per frame exceed the limit of 4096"):
        go(cap=4097)
    with pytest.raises(_lib.DvidError, match=r"1281 classes exceed the limit of 1280"):
        go(names=torch.zeros((1282, 24), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.DvidError, match=r"glyph cell of 33 x 8 exceeds"):
        go(atlas=torch.zeros((95, 8, 33), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.DvidError, match=r"thickness 17"):
        go(thickness=17)
    with pytest.raises(_lib.DvidError, match=r"text_scale 5"):
        go(text_scale=5)
    with pytest.raises(_lib.DvidError, match=r"8 bytes of scratch, 1 frames need %d" % dv.overlay_scratch_bytes(1, 4)):
        table = torch.tensor([frame.data_ptr()], dtype=torch.int64).cuda()
        sizes, dets, small = torch.tensor([[8, 8]], dtype=torch.int32), torch.zeros((1, 4, 6), device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        _lib.call("dvid_overlay_detections", _lib.ptr(table), _lib.ptr(sizes.cuda()), _lib.ptr(sizes), 1, _lib.ptr(dets), _lib.ptr(counts), 4, _lib.ptr(ratios),
                  _lib.ptr(names), len(C.NAMES) - 1, _lib.ptr(atlas), atlas.shape[1], atlas.shape[2], 0.7, 2, 1, _lib.ptr(small), 8, _lib.stream_ptr())
    go()
    torch.cuda.synchronize()
    assert not frame.any()
