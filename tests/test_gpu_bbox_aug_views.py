"""ops.resize_views_u8 (dvid_resize_views_u8): the views of TEST.BBOX_AUG built on the device from uint8 sources of different sizes, bit
for bit against data/transforms.resize_u8_numpy (= Pillow, tests/test_bbox_aug.py) and its mirror."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# source (h, w) -> view (oh, ow): a strong downscale with a 9-tap filter and odd ow; an upscale x2.2 with even ow; a height that stays
# (no y pass); a width that stays (no x pass); nothing to resample at all
CASES = [((101, 150), (30, 45)), ((20, 30), (44, 66)), ((40, 64), (40, 32)), ((40, 64), (20, 64)), ((24, 40), (24, 40))]


def _source(k):
    hw = CASES[k][0]
    return np.random.default_rng(10 + k).integers(0, 256, size=hw + (3,), dtype=np.uint8)


def _expected(ks, PH, PW, flip):
    from diffusionvid_amd.data.transforms import resize_u8_numpy
    out = torch.zeros(len(ks) * (1 + flip), 3, PH, PW)
    for i, k in enumerate(ks):
        oh, ow = CASES[k][1]
        view = resize_u8_numpy(_source(k), (oh, ow))
        for f in range(1 + flip):
            v = np.ascontiguousarray(view[:, ::-1] if f else view)
            out[i * (1 + flip) + f, :, :oh, :ow] = torch.from_numpy(v).permute(2, 0, 1).to(torch.float32).div(255)
    return out


def _run(ks, PH, PW, flip):
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.transforms import ViewsPlan
    plan = ViewsPlan([CASES[k][0] for k in ks], [CASES[k][1] for k in ks])
    got = ops.resize_views_u8([torch.from_numpy(_source(k)).cuda() for k in ks], plan, PH, PW, flip)
    torch.cuda.synchronize()
    return got.cpu()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("ks,PH,PW", [((0, 1, 2), 44, 66), ((0, 1, 2), 64, 96), ((3, 4, 0), 32, 64), ((1,), 64, 96), ((4,), 24, 40)])
def test_views_equal_the_host_resize_and_its_mirror(ks, PH, PW, flip):
    """three sources of different sizes in one call on a canvas that the upscaled view fills exactly (44 x 66: the other two are padded
    on both sides) and on a larger one; skipped passes on either axis and on both; one image alone"""
    want = _expected(ks, PH, PW, int(flip))
    got = _run(ks, PH, PW, flip)
    assert got.shape == want.shape == (len(ks) * (1 + flip), 3, PH, PW) and got.dtype == torch.float32
    for s in range(got.shape[0]):
        assert torch.equal(got[s], want[s]), f"slot {s} (image {ks[s // (1 + flip)]}{', mirrored' if flip and s % 2 else ''})"
    for i, k in enumerate(ks):
        oh, ow = CASES[k][1]
        for f in range(1 + flip):
            slot = got[i * (1 + flip) + f]
            assert not slot[:, oh:, :].any() and not slot[:, :, ow:].any()          # the padding is exactly zero
            assert slot[:, :oh, :ow].max() > 0.5
    if flip:          # the mirror lies inside the image's own columns, not the canvas's
        oh, ow = CASES[ks[0]][1]
        assert torch.equal(got[1][:, :oh, :ow], got[0][:, :oh, :ow].flip(-1)) and not torch.equal(got[1], got[0])


def test_views_equal_the_single_image_kernels():
    """the existing dvid_resize_u8_to_f32 on each image alone gives the same canvas slot"""
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.transforms import resample_tables
    got = _run((0, 1, 2), 64, 96, False)
    for i in range(3):
        (h, w), (oh, ow) = CASES[i]
        tabs = [tuple(torch.from_numpy(t).cuda() for t in resample_tables(a, b)) if a != b else None for a, b in ((w, ow), (h, oh))]
        one = ops.resize_u8_to_f32(torch.from_numpy(_source(i)).cuda(), oh, ow, 64, 96, tabs[0], tabs[1])
        assert torch.equal(one[0].cpu(), got[i]), i


def test_a_plan_that_does_not_fit_is_refused_before_any_launch():
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.transforms import ViewsPlan
    srcs = [torch.from_numpy(_source(k)).cuda() for k in (0, 1)]
    plan = ViewsPlan([CASES[0][0], CASES[1][0]], [CASES[0][1], CASES[1][1]])
    with pytest.raises(ops._lib.DvidError, match="canvas"):
        ops.resize_views_u8(srcs, plan, 44, 64, False)          # image 1 is 66 wide
    with pytest.raises(ops._lib.DvidError, match="other sizes"):
        ops.resize_views_u8(srcs[::-1], plan, 64, 96, False)
    bad = ViewsPlan([CASES[0][0], CASES[1][0]], [CASES[0][1], CASES[1][1]])
    bad.desc[1, 7] += 1          # image 1's y tables, the last ones, would end one row behind the concatenated bounds
    with pytest.raises(ops._lib.DvidError, match="outside"):
        ops.resize_views_u8(srcs, bad, 64, 96, False)
