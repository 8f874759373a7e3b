"""The device half of the split JPEG decode (csrc/jpeg.hip, ops.jpeg_reconstruct_u8, data/jpeg.py) on the GPU: Pillow's bits for every
file of the shared set (tests/_jpeg_ref.py: the sizes and why), alone and all in one call, the fallback, the loaders behind the datasets,
and the refusals.  Every file is written by Pillow here; nothing the host stage rejected is fed to the device."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _upload(coefs):
    """coefficients, tables and plan of some files the plain way (one tensor each), for the calls that go to ops directly"""
    from diffusionvid_amd.data import jpeg as J
    plan, n_coef, _ = J.plan_rows([c.info for c in coefs])
    coef = np.zeros(n_coef, dtype=np.int16)
    for row, c in zip(plan, coefs):
        coef[row[5]:row[5] + c.info.coef_count] = c.coef
    quant = np.stack([c.info.quant for c in coefs]).astype(np.uint16).view(np.int16).reshape(-1)
    return torch.from_numpy(coef).to(DEV), torch.from_numpy(quant).to(DEV), torch.from_numpy(plan)


@pytest.fixture(scope="module")
def decoded():
    """the entropy stage over the whole set, once"""
    from diffusionvid_amd.data import jpeg as J
    return [J.entropy_decode(data) for _, data, _ in R.cases()]


@pytest.mark.parametrize("k", range(len(R.SIZES)))
def test_each_file_alone_equals_pillow(k, decoded):
    from diffusionvid_amd import ops
    m = len(R.MODES)
    for (name, _, want), c in zip(R.cases()[k * m:(k + 1) * m], decoded[k * m:(k + 1) * m]):
        coef, quant, plan = _upload([c])
        (got,) = ops.jpeg_reconstruct_u8(coef, quant, plan)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_cuda, name
        got = got.cpu().numpy()
        assert np.array_equal(got, want), "%s: %d pixels differ" % (name, int((got != want).any(-1).sum()))


def test_all_files_in_one_call_give_each_frames_own_bits(decoded):
    """sizes and samplings mixed, the order shuffled: one call (two launches) over the 48 frames gives, frame by frame, Pillow's array --
    which is what each frame alone gives (the test above)"""
    from diffusionvid_amd import ops
    from diffusionvid_amd.data import jpeg as J
    order = np.random.default_rng(11).permutation(len(decoded))
    coef, quant, plan = _upload([decoded[i] for i in order])
    got = ops.jpeg_reconstruct_u8(coef, quant, plan)
    assert len(got) == len(order)
    for i, g in zip(order, got):
        name, _, want = R.cases()[i]
        assert np.array_equal(g.cpu().numpy(), want), name
    # and through the staged path (one pinned buffer, one upload), twice: the second call reuses nothing it should not
    for _ in range(2):
        staged = J.reconstruct([decoded[i] for i in order], DEV)
        assert all(np.array_equal(g.cpu().numpy(), R.cases()[i][2]) for i, g in zip(order, staged))


def _progressive(h=40, w=56):
    buf = io.BytesIO()
    Image.fromarray(R.picture(h, w, 77, False)).save(buf, "JPEG", quality=85, progressive=True)
    return buf.getvalue()


def test_decode_many_falls_back_for_a_progressive_file(tmp_path):
    from diffusionvid_amd.data import jpeg as J
    picks = [5, 18, 27, 46]
    items = [R.cases()[i][1] for i in picks]
    want = [R.cases()[i][2] for i in picks]
    prog = _progressive()
    items.insert(2, prog)
    want.insert(2, R.pillow_rgb(prog))
    path = tmp_path / "f.jpg"
    path.write_bytes(items[0])
    items[0] = str(path)          # paths and bytes mix
    for threads in (None, 1, 3):
        got, fallbacks = J.decode_many(items, DEV, threads=threads)
        assert fallbacks == 1 and len(got) == len(want)
        for g, w in zip(got, want):
            assert g.is_cuda and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), w)
    got, fallbacks = J.decode_many([d for _, d, _ in R.cases()], DEV)
    assert fallbacks == 0 and all(np.array_equal(g.cpu().numpy(), w) for g, (_, _, w) in zip(got, R.cases()))


def _three_files(tmp_path):
    paths = []
    for i, (hw, mode) in enumerate((((45, 70), "420"), ((64, 48), "444"), ((50, 81), "grey"))):
        p = tmp_path / ("%d.JPEG" % i)
        p.write_bytes(R.encode(R.picture(hw[0], hw[1], 300 + i, False), mode, 90))
        paths.append(str(p))
    return paths


def test_still_dataset_with_the_device_loader_equals_the_default_loader(tmp_path):
    from diffusionvid_amd.data import jpeg as J
    from diffusionvid_amd.data.datasets.still import StillImageDataset
    from diffusionvid_amd.data.transforms import ResizeToTensorDevice
    paths = _three_files(tmp_path)
    prog = tmp_path / "p.JPEG"
    prog.write_bytes(_progressive())
    paths.append(str(prog))
    decodes = []

    class Counting(J.DeviceJpegLoader):
        def __call__(self, path):
            decodes.append(path)
            return super().__call__(path)

    loader = Counting(DEV)
    ref = StillImageDataset(paths, transform=ResizeToTensorDevice(DEV, 96, 160), min_size=96, max_size=160)
    new = StillImageDataset(paths, transform=ResizeToTensorDevice(DEV, 96, 160), loader=loader, min_size=96, max_size=160)
    assert [new.original_size(i) for i in range(4)] == [ref.original_size(i) for i in range(4)] and not decodes          # headers only
    for i in range(4):
        a, b = ref[i], new[i]
        assert a[1:] == b[1:] and a[0].shape == b[0].shape and torch.equal(a[0], b[0]), paths[i]
    assert loader.fallbacks == 1 and len(decodes) == 4
    raw = StillImageDataset(paths[:3], loader=loader, raw=True)          # the TEST.BBOX_AUG path: the CUDA tensor goes through as it is
    img, _, (w, h) = raw[0]
    assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (h, w, 3)


def test_vid_dataset_with_the_device_loader_equals_the_default_loader(tmp_path):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data import jpeg as J
    from diffusionvid_amd.data.datasets.vid import VIDMEGATestDataset
    from diffusionvid_amd.data.transforms import ResizeToTensorDevice
    import os
    from conftest import ROOT
    video = tmp_path / "v"
    video.mkdir()
    for i in range(3):
        (video / ("%06d.JPEG" % i)).write_bytes(R.encode(R.picture(54, 96, 400 + i, False), "420", 90))
    from diffusionvid_amd.data.datasets.vid import VIDFrameList
    index = VIDFrameList.from_lengths({"v": 3})
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), [], os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    ref = VIDMEGATestDataset(cfg, str(tmp_path), index, transform=ResizeToTensorDevice(DEV, 64, 128), rng=np.random.RandomState(3))
    new = VIDMEGATestDataset(cfg, str(tmp_path), index, transform=ResizeToTensorDevice(DEV, 64, 128), loader=J.DeviceJpegLoader(DEV),
                             rng=np.random.RandomState(3))          # the same shuffle of the global references
    for idx in range(3):
        a, b = ref[idx][0], new[idx][0]
        assert torch.equal(a["cur"].tensors, b["cur"].tensors) and a["cur"].image_sizes == b["cur"].image_sizes
        assert len(a["ref_l"]) == len(b["ref_l"]) and all(torch.equal(x.tensors, y.tensors) for x, y in zip(a["ref_l"], b["ref_l"]))
        assert len(a["ref_g"]) == len(b["ref_g"]) and all(torch.equal(x.tensors, y.tensors) for x, y in zip(a["ref_g"], b["ref_g"]))


def test_refusals_come_before_any_launch_and_carry_the_numbers(decoded, tmp_path):
    from diffusionvid_amd import _lib, ops
    from diffusionvid_amd.data import jpeg as J
    a, b = decoded[30], decoded[19]          # 37x53 at 4:2:0 and 16x16 greyscale
    assert a.info.ncomp == 3 and a.info.hsamp[0] == 2 and b.info.ncomp == 1
    coef, quant, plan = _upload([a, b])

    def refused(p, pattern, **kw):
        with pytest.raises(_lib.DvidError, match=pattern):
            ops.jpeg_reconstruct_u8(kw.get("coef", coef), quant, p)

    p = plan.clone()
    p[0, 0] = 70000          # oversized: a width beyond 65535
    refused(p, r"frame 0 is 70000 x %d" % a.info.height)
    p = plan.clone()
    p[1, 5] = plan[0, 5]          # frame 1's luma on top of frame 0's
    refused(p, r"component 0 of frame 1 starts at coefficient %d.*ends at %d" % (int(plan[0, 5]), int(plan[1, 5])))
    p = plan.clone()
    p[1, 5] += 8          # not a block boundary
    refused(p, r"multiples of 64")
    p = plan.clone()
    p[1, 9] = plan[0, 9] + 3          # frame 1's pixels inside frame 0's
    refused(p, r"frame 1's pixels start at byte 3 and overlap")
    p = plan.clone()
    p[1, 1] = b.info.height + 64          # more rows than frame 1 has coefficients for: it would leave the buffer
    refused(p, r"of frame 1 ends at coefficient \d+, the buffer holds %d" % coef.numel())
    p = plan.clone()
    p[0, 3], p[0, 4] = 1, 2          # luma 1x2
    refused(p, r"frame 0 has 3 components with luma sampling 1 x 2")
    p = plan.clone()
    p[0, 2] = 4
    refused(p, r"frame 0 has 4 components")
    p = plan.clone()
    p[1, 8] = 192 * 5          # tables past the table buffer
    refused(p, r"tables of frame 1 start at entry 960 of 384")
    # the limit on the coefficient count (int32 indices inside the kernels), through the ABI itself: refused before any pointer is followed
    planes = torch.empty(coef.numel(), dtype=torch.uint8, device=DEV)
    out = torch.empty(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.DvidError, match=r"2147483648 coefficients exceed the limit of 2147483647"):
        _lib.call("dvid_jpeg_reconstruct_u8", coef.data_ptr(), 2 ** 31, quant.data_ptr(), quant.numel(), plan.to(DEV).data_ptr(), plan.data_ptr(), 2,
                  planes.data_ptr(), 2 ** 31, out.data_ptr(), 64, _lib.stream_ptr())
    with pytest.raises(_lib.DvidError, match="null pointer"):
        _lib.call("dvid_jpeg_reconstruct_u8", None, coef.numel(), quant.data_ptr(), quant.numel(), plan.to(DEV).data_ptr(), plan.data_ptr(), 2,
                  planes.data_ptr(), planes.numel(), out.data_ptr(), 64, _lib.stream_ptr())
    torch.cuda.synchronize()
    # the valid plan still runs after all of that
    got = ops.jpeg_reconstruct_u8(coef, quant, plan)
    assert np.array_equal(got[0].cpu().numpy(), R.cases()[30][2]) and np.array_equal(got[1].cpu().numpy(), R.cases()[19][2])
    # a malformed file through the loader: the host stage raises with the path, nothing reaches the device
    bad = tmp_path / "broken.JPEG"
    data = R.cases()[30][1]
    bad.write_bytes(data[:len(data) // 2])
    with pytest.raises(ValueError, match=r"broken\.JPEG.*truncated scan"):
        J.DeviceJpegLoader(DEV)(str(bad))
    with pytest.raises(ValueError, match=r"broken\.JPEG"):
        J.decode_many([R.cases()[3][1], str(bad)], DEV)
