"""Split JPEG decode: the entropy (Huffman) stage on the host, everything behind it on the GPU (include/dvid_hip.h, dvid_version >= 11).

  parse(data)                      header only -> JpegInfo; Unsupported for what the split does not take, ValueError for malformed data
  entropy_decode(data_or_path)     -> JpegCoefficients: the int16 coefficients (not dequantised) + the info.  No GPU is touched: this is
                                   what a DataLoader worker returns instead of pixels -- it pickles, and `out=` writes into a caller's
                                   (shared-memory) buffer.  1280 x 720 at 4:2:0 is 2.76 MB of coefficients, as many bytes as its RGB.
  reconstruct(coefs, device)       -> CUDA uint8 [h, w, 3] tensors, Pillow's bits: one pinned staging copy, one upload, two launches.
  decode_many(items, device)       files or bytes -> (tensors, fallbacks): entropy stage in a thread pool (ctypes drops the GIL), one
                                   reconstruct; a file the split does not take is decoded by Pillow on the host and uploaded.
  DeviceJpegLoader(device)         loader(path) for VIDMEGATestDataset / StillImageDataset, with ResizeToTensorDevice behind it.

The result equals np.asarray(PIL.Image.open(f).convert("RGB")) exactly for every file the host stage accepts (libjpeg's default decode is
integer arithmetic throughout: ISLOW IDCT, fancy upsampling, fixed-point colour)."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _lib

PLAN_COLS = 10          # DVID_JPEG_PLAN_COLS
_ERR_CAP = 320


class Unsupported(Exception):
    """a valid JPEG outside what the split decode takes (progressive, CMYK, ...): decode it with Pillow"""


class _Info(C.Structure):          # dvid_jpeg_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hsamp", C.c_int32 * 3), ("vsamp", C.c_int32 * 3),
                ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3), ("reserved", C.c_int32), ("coef_offset", C.c_int64 * 3),
                ("coef_count", C.c_int64), ("quant", (C.c_uint16 * 64) * 3)]


class JpegInfo:
    """What dvid_jpeg_parse reports, as plain Python values (it pickles): width, height, ncomp, hsamp / vsamp / blocks_w / blocks_h /
    coef_offset per component, coef_count, quant uint16 [3, 64] in natural order (rows beyond ncomp are zero)."""
    __slots__ = ("width", "height", "ncomp", "hsamp", "vsamp", "blocks_w", "blocks_h", "coef_offset", "coef_count", "quant")

    def __init__(self, raw):
        n = int(raw.ncomp)
        self.width, self.height, self.ncomp = int(raw.width), int(raw.height), n
        self.hsamp, self.vsamp = tuple(raw.hsamp[:n]), tuple(raw.vsamp[:n])
        self.blocks_w, self.blocks_h = tuple(raw.blocks_w[:n]), tuple(raw.blocks_h[:n])
        self.coef_offset, self.coef_count = tuple(raw.coef_offset[:n]), int(raw.coef_count)
        self.quant = np.ctypeslib.as_array(raw.quant).astype(np.uint16).reshape(3, 64).copy()

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, state):
        for k, v in state.items():
            setattr(self, k, v)

    @property
    def size(self):
        """(w, h)"""
        return self.width, self.height

    def __repr__(self):
        return "JpegInfo(%d x %d, %d component(s), luma %dx%d, %d coefficients)" % (self.width, self.height, self.ncomp, self.hsamp[0], self.vsamp[0],
                                                                                     self.coef_count)


class JpegCoefficients:
    """One file behind the entropy stage: coef int16 [info.coef_count] (a numpy array, possibly a view of the caller's buffer) + info"""
    __slots__ = ("coef", "info")

    def __init__(self, coef, info):
        self.coef, self.info = coef, info

    def __getstate__(self):
        return {"coef": self.coef, "info": self.info}

    def __setstate__(self, state):
        self.coef, self.info = state["coef"], state["info"]


def _bytes_of(data):
    """a contiguous uint8 view of bytes / bytearray / memoryview / ndarray (kept alive by the caller's reference to what is returned)"""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError("jpeg data as an array is uint8 [n], got %s %s" % (data.dtype, data.shape))
        return np.ascontiguousarray(data)
    return np.frombuffer(data, dtype=np.uint8)


def _read(data_or_path):
    if isinstance(data_or_path, (str, os.PathLike)):
        with open(data_or_path, "rb") as f:
            return f.read()
    return data_or_path


def _raise(rc, err, what):
    msg = err.value.decode("utf-8", "replace") or "error %d" % rc
    if what:
        msg = "%s: %s" % (what, msg)
    raise (Unsupported if rc == 3 else ValueError)(msg)          # DVID_ERR_UNSUPPORTED


def parse(data, what=""):
    """The header of a JPEG in memory -> JpegInfo.  Raises Unsupported / ValueError with the library's message (`what`, a path, in front)."""
    buf = _bytes_of(data)
    raw, err = _Info(), C.create_string_buffer(_ERR_CAP)
    rc = _lib.load().dvid_jpeg_parse(buf.ctypes.data, buf.size, C.byref(raw), err, _ERR_CAP)
    if rc:
        _raise(rc, err, what)
    return JpegInfo(raw)


def entropy_decode(data_or_path, out=None):
    """Parse + Huffman-decode one file (a path, or its bytes) -> JpegCoefficients.  out: an int16 numpy array (or writable buffer) of at
    least coef_count elements to decode into; the result's `coef` is then a view of it.  Touches no GPU; safe from any thread or process."""
    what = os.fspath(data_or_path) if isinstance(data_or_path, (str, os.PathLike)) else ""
    buf = _bytes_of(_read(data_or_path))
    info = parse(buf, what)
    if out is None:
        coef = np.empty((info.coef_count,), dtype=np.int16)
    else:
        coef = out if isinstance(out, np.ndarray) else np.frombuffer(out, dtype=np.int16)
        if coef.dtype != np.int16 or coef.ndim != 1 or not coef.flags.c_contiguous or not coef.flags.writeable or coef.size < info.coef_count:
            raise ValueError("%sentropy_decode: `out` is a writable contiguous int16 [>= %d] buffer" % (what and what + ": ", info.coef_count))
        coef = coef[:info.coef_count]
    err = C.create_string_buffer(_ERR_CAP)
    rc = _lib.load().dvid_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef.ctypes.data, coef.size, None, err, _ERR_CAP)
    if rc:
        _raise(rc, err, what)
    return JpegCoefficients(coef, info)


def plan_rows(infos, coef_align=64):
    """(plan int64 [n, PLAN_COLS], total coefficients, total output bytes) for frames laid out one after the other: coefficients at
    multiples of coef_align elements, tables 192 entries apart, pixels back to back"""
    plan = np.zeros((len(infos), PLAN_COLS), dtype=np.int64)
    coef_at = out_at = 0
    for i, info in enumerate(infos):
        row = plan[i]
        row[0:5] = info.width, info.height, info.ncomp, info.hsamp[0], info.vsamp[0]
        for c in range(info.ncomp):
            row[5 + c] = coef_at + info.coef_offset[c]
        row[8], row[9] = 192 * i, out_at
        coef_at += -(-info.coef_count // coef_align) * coef_align
        out_at += info.width * info.height * 3
    return plan, coef_at, out_at


class _Staging:
    """Pinned staging buffers per device, a ring of `depth` per size bucket with the event of each one's last upload (the scheme of
    ResizeToTensorDevice._pinned): a buffer is rewritten only after the copy engine has read it"""

    def __init__(self, depth=4):
        self.depth, self.rings = depth, {}

    def slot(self, device, nbytes):
        import torch
        bucket = 1 << max(16, int(nbytes - 1).bit_length())
        ring = self.rings.setdefault((str(device), bucket), {"slots": [], "next": 0})
        if len(ring["slots"]) < self.depth:
            ring["slots"].append([torch.empty((bucket,), dtype=torch.uint8).pin_memory(), None])
            return ring["slots"][-1]
        slot = ring["slots"][ring["next"]]
        ring["next"] = (ring["next"] + 1) % self.depth
        if slot[1] is not None:
            slot[1].synchronize()
        return slot


_staging = _Staging()


def _reconstruct(infos, fill, device):
    """the staged core: lay n frames out in one pinned buffer, let `fill(c16, starts)` write every frame's coefficients at its start (an
    int16 view of the buffer; starts[i] in elements), add tables and plan, one upload, ops.jpeg_reconstruct_u8"""
    import torch
    from .. import ops
    device = torch.device(device)
    plan, n_coef, _ = plan_rows(infos, coef_align=128)          # 128 int16 = 256 bytes: every frame starts cache-line aligned
    n = len(infos)
    quant_at = n_coef * 2
    plan_at = quant_at + -(-n * 192 * 2 // 256) * 256
    total = plan_at + plan.nbytes
    slot = _staging.slot(device, total)
    host = slot[0].numpy()
    fill(host[:quant_at].view(np.int16), [int(row[5]) for row in plan])
    host[quant_at:quant_at + n * 384].view(np.uint16).reshape(n, 3, 64)[...] = np.stack([info.quant for info in infos])
    host[plan_at:total].view(np.int64).reshape(n, PLAN_COLS)[...] = plan
    with torch.cuda.device(device):
        up = slot[0][:total].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(device))
        return ops.jpeg_reconstruct_u8(up[:quant_at].view(torch.int16), up[quant_at:quant_at + n * 384].view(torch.int16), torch.from_numpy(plan),
                                       plan=up[plan_at:total].view(torch.int64).view(n, PLAN_COLS))


def reconstruct(coefs, device):
    """[JpegCoefficients] -> [CUDA uint8 [h, w, 3]], Pillow's bits.  Coefficients, tables and plan go into ONE pinned staging buffer and up
    in one copy; then ops.jpeg_reconstruct_u8's two launches.  Nothing is synchronised: the tensors are ready in stream order."""
    coefs = list(coefs)
    if not coefs:
        return []
    for c in coefs:
        if c.coef.shape != (c.info.coef_count,) or c.coef.dtype != np.int16:
            raise ValueError("reconstruct: %d coefficients for %r" % (c.coef.size, c.info))

    def fill(c16, starts):
        for start, c in zip(starts, coefs):
            c16[start:start + c.info.coef_count] = c.coef

    return _reconstruct([c.info for c in coefs], fill, device)


def _pil_decode(data_or_path):
    import io
    from PIL import Image
    src = data_or_path if isinstance(data_or_path, (str, os.PathLike)) else io.BytesIO(bytes(data_or_path))
    with Image.open(src) as im:
        return np.asarray(im.convert("RGB"))


def default_threads():
    """the entropy pool's size: this process's share of the CPUs it may run on and of the container's CPU quota, never os.cpu_count()"""
    from ..utils import comm
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    return comm.rank_thread_cap(n, 1, comm.cpu_quota())


_pools = {}


def _pool(threads):
    if threads not in _pools:
        _pools[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="dvid-jpeg")
    return _pools[threads]


def _head_one(item):
    """(bytes, JpegInfo), or (None, Pillow's array) for a file outside the split"""
    what = os.fspath(item) if isinstance(item, (str, os.PathLike)) else ""
    data = _read(item)
    try:
        return data, parse(data, what)
    except Unsupported:
        return None, _pil_decode(item)


def decode_many(items, device, threads=None):
    """Paths or bytes of n JPEG files -> ([CUDA uint8 [h, w, 3]] complete and in order, number of files that took the Pillow fallback).
    Both host passes run in `threads` threads (default_threads() when None): read + parse (a file parse() calls Unsupported is decoded
    by Pillow there), then the entropy stage of every accepted file straight into its place in the pinned staging buffer -- the
    coefficients are written once.  One upload and one reconstruct cover all accepted files; the fallback's arrays are uploaded as they
    are.  A malformed file raises ValueError (with its path)."""
    import torch
    items = list(items)
    threads = default_threads() if threads is None else max(1, int(threads))
    run = map if threads == 1 or len(items) < 2 else _pool(threads).map
    heads = list(run(_head_one, items))
    split = [i for i, (data, _) in enumerate(heads) if data is not None]
    out = [None] * len(items)
    if split:
        names = [os.fspath(items[i]) if isinstance(items[i], (str, os.PathLike)) else "" for i in split]

        def fill(c16, starts):
            def one(k):
                data, info = heads[split[k]]
                try:
                    entropy_decode(data, out=c16[starts[k]:starts[k] + info.coef_count])
                except ValueError as e:
                    raise ValueError("%s: %s" % (names[k], e) if names[k] else str(e)) from None
            list(run(one, range(len(split))))

        for i, t in zip(split, _reconstruct([heads[i][1] for i in split], fill, device)):
            out[i] = t
    fallbacks = 0
    for i, (data, s) in enumerate(heads):
        if data is None:
            out[i] = torch.from_numpy(np.array(s)).to(device)          # a writable copy of Pillow's read-only buffer
            fallbacks += 1
    return out, fallbacks


def _default_fallback(path):
    from .datasets.vid import _pil_loader
    return _pil_loader(path)


class DeviceJpegLoader:
    """loader(path) -> CUDA uint8 [h, w, 3] (Pillow's bits) by the split decode; for a file outside it, the fallback's numpy array, which
    every consumer of a loader already takes.  Plugs into VIDMEGATestDataset(loader=...) / StillImageDataset(loader=...) in front of
    ResizeToTensorDevice, which passes a CUDA tensor through to the resize kernels.  `size(path)` reads the header only.  `fallbacks`
    counts the files that took the fallback.  A malformed file raises ValueError with the path in the message."""

    def __init__(self, device, fallback=None):
        import torch
        self.device = torch.device(device)
        self.fallback = fallback or _default_fallback
        self.fallbacks = 0

    def __call__(self, path):
        try:
            c = entropy_decode(path)
        except Unsupported:
            self.fallbacks += 1
            return self.fallback(path)
        return reconstruct([c], self.device)[0]

    def size(self, path, head=1 << 16):
        """(w, h) from the file's header: the first `head` bytes, the whole file only when the header is longer than that"""
        path = os.fspath(path)
        with open(path, "rb") as f:
            data = f.read(head)
            try:
                return parse(data, path).size
            except Unsupported:
                pass
            except ValueError:
                rest = f.read()
                if not rest:
                    raise
                try:
                    return parse(data + rest, path).size
                except Unsupported:
                    pass
        from PIL import Image
        with Image.open(path) as im:          # the fallback's files: Pillow reads their header
            return int(im.size[0]), int(im.size[1])
