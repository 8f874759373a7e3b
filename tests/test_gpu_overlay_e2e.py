"""The demo end to end on the GPU: VIDDemo.run_on_frames (frames uploaded once as uint8, resized and detected on the device, a copy drawn on
by csrc/overlay.hip) bit-equal to the composition it stands for -- model(item) per call, BoxList.resize on the host, the painter of
_overlay_ref.py -- for the video configuration and for the streaming one, and render_boxlists on two streams of a StreamSet.
One 6-frame video of 96 x 130 frames, resized to 120 x 162 (two different ratios), BLOCKS_OVERRIDE (1, 1, 1, 1).  Untrained weights score
low, so the threshold is the median of the detections' scores: something is drawn and something is not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _overlay_ref as R  # noqa: E402

STREAMING = ["INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0, "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1,
             "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0, "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False]
H, W, L = 96, 130, 6


def _model(extra=()):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "INPUT.MIN_SIZE_TEST", 120, "INPUT.MAX_SIZE_TEST", 200,
                                                          "MODEL.VID.MEGA.GLOBAL.SHUFFLE", False] + list(extra), "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    return cfg, model


def _frames(video):
    from diffusionvid_amd.utils import synthetic
    return [(synthetic.synthetic_frame(f, H, W, video=video, smooth=True) * 255).round().byte().permute(1, 2, 0).contiguous().numpy() for f in range(L)]


def _items(cfg, frames):
    """the video's items as the dataset protocol delivers them, from frames uploaded here"""
    from diffusionvid_amd.data import transforms as T
    from diffusionvid_amd.data.datasets.vid import VIDFrameList, VIDMEGATestDataset
    dev = [torch.from_numpy(f).cuda() for f in frames]
    ds = VIDMEGATestDataset(cfg, "", VIDFrameList.from_lengths({"v": len(frames)}), loader=lambda p: dev[int(p.split("/")[-1].split(".")[0])],
                            transform=T.ResizeToTensorDevice("cuda", cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.DATALOADER.SIZE_DIVISIBILITY))
    return [ds[i] for i in range(len(ds))]


def _per_call(model, items):
    results = {}
    with torch.no_grad():
        for images, _, ids in items:
            results.update(zip(ids, model(images)))
    return [results[i] for i in range(len(items))]


def _median(preds):
    scores = torch.cat([p.get_field("scores") for p in preds]).float().cpu()
    assert len(scores) > 2
    return float(scores.median())


def _painted(frame, pred, threshold, atlas):
    """the composition: the prediction on the host, resized to the frame as the reference's compute_prediction does, then the painter"""
    from diffusionvid_amd.data.datasets.vid import VID_CLASSES
    native = pred.to("cpu").resize((frame.shape[1], frame.shape[0]))
    dets = torch.cat([native.bbox, native.get_field("scores").float()[:, None], native.get_field("labels").float()[:, None]], dim=1).numpy()
    return R.render(frame, dets, len(dets), (1.0, 1.0), list(VID_CLASSES), atlas, threshold, 2, 1)


def _same_boxlist(a, b):
    return a.size == b.size and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and \
        torch.equal(a.get_field("labels"), b.get_field("labels"))


def _check_demo(cfg, model, frames):
    from diffusionvid_amd.engine import demo
    own = _per_call(model, _items(cfg, frames))
    assert own[0].size == (162, 120)          # (w, h) of the model's frame: two different ratios toward 130 x 96
    thr = _median(own)
    d = demo.VIDDemo(cfg, model, confidence_threshold=thr)
    drawn, preds = d.run_on_frames(frames)
    assert len(drawn) == len(preds) == L and all(f.is_cuda and f.dtype == torch.uint8 for f in drawn)
    n_drawn = n_kept = 0
    for f in range(L):
        assert _same_boxlist(preds[f], own[f]), f          # the predictions are the model's own
        want, info = _painted(frames[f], own[f], thr, d.atlas)
        assert np.array_equal(drawn[f].cpu().numpy(), want), f
        n_drawn += len(info["drawn"])
        n_kept += len(own[f])
    assert 0 < n_drawn < n_kept
    assert not np.array_equal(drawn[0].cpu().numpy(), frames[0])
    return d, thr


def test_demo_on_a_video_equals_the_composition(tmp_path):
    from PIL import Image
    cfg, model = _model()
    frames = _frames(0)
    d, _ = _check_demo(cfg, model, frames)
    drawn, preds = d.run_on_frames(frames)
    again = d.run_on_image(torch.from_numpy(frames[0]).cuda(), preds[0])          # draw only, on a copy
    assert np.array_equal(again.cpu().numpy(), drawn[0].cpu().numpy())
    on_host = d.run_on_image(frames[0], preds[0].to("cpu"))          # the numpy path, the same pixels
    assert np.array_equal(on_host, drawn[0].cpu().numpy())
    for f, frame in enumerate(reversed(frames)):          # a folder of files named so that the sorted glob restores the order (lossless, .JPEG by name)
        Image.fromarray(frame).save(str(tmp_path / ("%06d.JPEG" % (L - 1 - f))), format="PNG")
    from_folder, _ = d.run_on_image_folder(str(tmp_path))
    assert len(from_folder) == L and all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(from_folder, drawn))
    paths = d.generate_images(drawn, str(tmp_path / "out"))
    assert len(paths) == L and paths[0].endswith("000000.jpg")


def test_demo_and_stream_set_in_the_streaming_configuration():
    from diffusionvid_amd.data.datasets.vid import VID_CLASSES
    from diffusionvid_amd.engine import demo
    cfg, model = _model(STREAMING)
    videos = [_frames(1), _frames(2)]
    d, _ = _check_demo(cfg, model, videos[0])
    # two streams of a StreamSet, one frame of each per step, rendered together
    private = [_per_call(model, _items(cfg, v)) for v in videos]
    thr = _median(private[0] + private[1])
    items = [_items(cfg, v) for v in videos]
    streams = model.open_streams()
    for t in range(L):
        with torch.no_grad():
            out = streams.step({s: items[s][t][0] for s in (0, 1)})
        boxlists = [out[s][0] for s in (0, 1)]
        for s in (0, 1):
            assert _same_boxlist(boxlists[s], private[s][t]), (s, t)
        frames = [torch.from_numpy(videos[s][t]).cuda() for s in (0, 1)]
        demo.render_boxlists(frames, boxlists, VID_CLASSES, thr)
        for s in (0, 1):
            want, _ = _painted(videos[s][t], private[s][t], thr, d.atlas)
            assert np.array_equal(frames[s].cpu().numpy(), want), (s, t)
