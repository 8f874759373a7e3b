"""Still images: a list of files, each detected on its own (DiffusionDet.detect_images), and the batch sampler that keeps wide and tall
images apart.

An item is `(image, image_id, (w, h))`: the image resized by its shortest edge with the video path's own transform (data/transforms.py:
ResizeToTensor on the host, ResizeToTensorDevice = dvid_resize_u8_to_f32 on the GPU) as fp32 [3, oh, ow] in [0, 1], un-padded -- the
batch's common canvas is made by the collate function -- and the ORIGINAL (w, h), to which engine.inference_images maps the detections
back.  No annotations are read here: engine.inference_images scores the detections against a COCO annotation file
(data/evaluation/coco_eval.py)."""
import torch

from ...structures.image_list import to_image_list
from ..transforms import ResizeToTensor, get_size


class StillImageDataset:
    def __init__(self, files, transform=None, loader=None, image_ids=None, min_size=800, max_size=1333, raw=False):
        """raw: the item's image is the loader's uint8 HWC array at its native size, no transform (TEST.BBOX_AUG: the detector builds every
        view itself, DiffusionDet.detect_images_aug); `resized_size`, and with it the orientation sampler, keep the plain transform's sizes.
        files: paths (or whatever `loader` takes); loader(path) -> uint8 HWC RGB (default: Pillow); transform(image, is_current=True)
        -> fp32 [3, oh, ow] (or the device transform's padded [1, 3, ph, pw] with `.image_size`); image_ids default to 0 .. n-1."""
        self.files = list(files)
        self.image_ids = list(range(len(self.files))) if image_ids is None else [int(i) for i in image_ids]
        if len(self.image_ids) != len(self.files):
            raise ValueError("%d image_ids for %d files" % (len(self.image_ids), len(self.files)))
        self.min_size, self.max_size = min_size, max_size
        self.raw = bool(raw)
        self.transform = transform or ResizeToTensor(min_size, max_size)
        self._default_loader = loader is None
        if loader is None:
            from .vid import _pil_loader as loader
        self.loader = loader
        self._sizes = {}

    def __len__(self):
        return len(self.files)

    def original_size(self, idx):
        """(w, h) of the file as it lies on disk; read once (a header read with Pillow when the default loader is in use)"""
        if idx not in self._sizes:
            if self._default_loader:
                from PIL import Image
                with Image.open(self.files[idx]) as im:
                    self._sizes[idx] = (int(im.size[0]), int(im.size[1]))
            elif hasattr(self.loader, "size"):          # a loader that reads headers (data/jpeg.py: DeviceJpegLoader): no decode for a size
                w, h = self.loader.size(self.files[idx])
                self._sizes[idx] = (int(w), int(h))
            else:
                h, w = self.loader(self.files[idx]).shape[:2]
                self._sizes[idx] = (int(w), int(h))
        return self._sizes[idx]

    def resized_size(self, idx):
        """(w, h) the transform will give image idx"""
        oh, ow = get_size(self.original_size(idx), self.min_size, self.max_size)
        return ow, oh

    def __getitem__(self, idx):
        raw = self.loader(self.files[idx])
        h, w = raw.shape[:2]
        self._sizes[idx] = (int(w), int(h))
        if self.raw:
            return raw, self.image_ids[idx], (int(w), int(h))
        img = self.transform(raw, is_current=True)          # every still image chooses its own size
        size = getattr(img, "image_size", None)
        if size is not None:                                 # the device transform pads to a multiple of 32 of the image's own size
            img = img.reshape(img.shape[-3:])[:, :size[0], :size[1]]
        return img, self.image_ids[idx], (int(w), int(h))


def orientation_batches(sizes_wh, batch_size):
    """Indices in batches of at most `batch_size`, wide (w >= h) and tall images in batches of their own, each in the order given: a canvas
    is the largest height by the largest width of its batch, so one tall image among wide ones would pad every image of the batch to a
    square of the long edge."""
    wide = [i for i, (w, h) in enumerate(sizes_wh) if w >= h]
    tall = [i for i, (w, h) in enumerate(sizes_wh) if w < h]
    return [g[a:a + batch_size] for g in (wide, tall) for a in range(0, len(g), batch_size)]


def padding_share(sizes_wh, batches, divisible=32):
    """share of the canvas pixels of `batches` (lists of indices into sizes_wh) that is padding"""
    canvas = real = 0
    for b in batches:
        W = -(-max(sizes_wh[i][0] for i in b) // divisible) * divisible
        H = -(-max(sizes_wh[i][1] for i in b) // divisible) * divisible
        canvas += W * H * len(b)
        real += sum(sizes_wh[i][0] * sizes_wh[i][1] for i in b)
    return 1.0 - real / canvas if canvas else 0.0


class OrientationBatchSampler:
    """batch sampler (an iterable of index lists, as torch.utils.data.DataLoader's `batch_sampler`) over a StillImageDataset or a list of
    (w, h): orientation_batches of the RESIZED sizes"""

    def __init__(self, source, batch_size):
        sizes = [source.resized_size(i) for i in range(len(source))] if hasattr(source, "resized_size") else list(source)
        self.batches = orientation_batches(sizes, batch_size)

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def collate_images(items, size_divisible=32):
    """[(image, id, (w, h))] -> (ImageList on one zero-padded canvas, [id], [(w, h)])"""
    images = [torch.as_tensor(it[0]) for it in items]
    return to_image_list(images, size_divisible), [it[1] for it in items], [tuple(it[2]) for it in items]


def collate_raw(items):
    """[(uint8 HWC image, id, (w, h))] of a raw dataset -> ([image], [id], [(w, h)]): the images stay as they are, each with its own size"""
    return [it[0] for it in items], [it[1] for it in items], [tuple(it[2]) for it in items]


def batches(dataset, batch_size, size_divisible=32, raw=False):
    """the plain loader: collate_images (raw: collate_raw, over a dataset in raw mode) over OrientationBatchSampler, one batch after the other"""
    if raw and not getattr(dataset, "raw", False):
        raise ValueError("batches(raw=True) needs a StillImageDataset(raw=True)")
    for idx in OrientationBatchSampler(dataset, batch_size):
        items = [dataset[i] for i in idx]
        yield collate_raw(items) if raw else collate_images(items, size_divisible)
