"""The host half of the split JPEG decode (csrc/jpeg_host.cpp, data/jpeg.py) on the CPU: the C ABI, the entropy stage's coefficients
through the numpy restatement of libjpeg's arithmetic (_jpeg_ref.py) against Pillow itself -- equal, not close --, what is refused and
how, damaged files, pickling, and the stand-alone sanitizer program.  No GPU.  Every file is written by Pillow here."""
import io
import os
import pickle
import re
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import _jpeg_ref as R
from conftest import ROOT

from diffusionvid_amd.data import jpeg as J


def test_c_abi_carries_the_jpeg_entries():
    """fails before the split decode exists: the header, _lib.SIGNATURES and the library carry the three symbols, dvid_version() >= 11"""
    from diffusionvid_amd import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvid_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in (("dvid_jpeg_parse", 5), ("dvid_jpeg_entropy_decode", 7), ("dvid_jpeg_reconstruct_u8", 12)):
        decl = re.search(r"\bint %s\(([^;]*?)\);" % name, header, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.dvid_version() >= 11
    assert callable(ops.jpeg_reconstruct_u8) and ops.JPEG_PLAN_COLS == J.PLAN_COLS == int(re.search(r"#define DVID_JPEG_PLAN_COLS (\d+)", header).group(1))
    # the Python mirror of dvid_jpeg_info has the C struct's layout: 16 int32, 4 int64, 192 uint16
    import ctypes
    assert ctypes.sizeof(J._Info) == 16 * 4 + 4 * 8 + 192 * 2 and J._Info.coef_offset.offset == 64 and J._Info.quant.offset == 96


def test_the_host_source_has_no_hip_in_it():
    """the entries initialise no GPU: the file includes no HIP header and names no hip* function (worker processes call it)"""
    src = open(os.path.join(ROOT, "diffusionvid_amd", "csrc", "jpeg_host.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "hip_runtime" not in code and not re.search(r"\bhip[A-Z]\w*\s*\(", code)
    assert "jpeg_host.cpp" in open(os.path.join(ROOT, "diffusionvid_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("k", range(len(R.SIZES)))
def test_coefficients_through_the_reference_equal_pillow(k):
    """every mode of one size: entropy_decode's coefficients, dequantised / transformed / upsampled / converted by _jpeg_ref, EQUAL
    np.asarray(Image.open(..).convert("RGB")); the block grid and the offsets are the contract's"""
    for name, data, want in R.cases()[k * len(R.MODES):(k + 1) * len(R.MODES)]:
        c = J.entropy_decode(data)
        info = c.info
        assert (info.height, info.width) == want.shape[:2] == R.SIZES[k], name
        hmax, vmax = info.hsamp[0], info.vsamp[0]
        at = 0
        for i in range(info.ncomp):
            assert info.blocks_w[i] == -(-info.width // (8 * hmax)) * info.hsamp[i] and info.blocks_h[i] == -(-info.height // (8 * vmax)) * info.vsamp[i], name
            assert info.coef_offset[i] == at, name
            at += info.blocks_w[i] * info.blocks_h[i] * 64
        assert info.coef_count == at == c.coef.size and c.coef.dtype == np.int16, name
        got = R.reconstruct(c.coef, info)
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d pixels differ" % (name, int((got != want).any(-1).sum()))


def test_every_baseline_file_is_accepted_and_the_modes_are_told_apart():
    """no file of the set takes the fallback (so the fallback cannot hide a failure), and the set is what it claims to be"""
    fallbacks, seen = 0, set()
    for name, data, _ in R.cases():
        try:
            info = J.parse(data)
        except J.Unsupported:
            fallbacks += 1
            continue
        seen.add((info.ncomp, info.hsamp[0], info.vsamp[0]))
    assert fallbacks == 0
    assert seen == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert len(R.cases()) == len(R.SIZES) * len(R.MODES)
    names = " ".join(n for n, _, _ in R.cases())
    assert all(s in names for s in ("q30", "q90", "q100", "optimize", "blocks", "rows"))
    assert any(b"\xff\xdd" in d for _, d, _ in R.cases())          # a DRI marker: the restart cases do carry restarts
    # at quality 100 the clamp is exercised: the decoded picture reaches both ends of the range
    assert any("q100" in n and want.min() == 0 and want.max() == 255 for n, _, want in R.cases())


def test_decoding_into_a_callers_buffer_and_from_a_path(tmp_path):
    name, data, _ = R.cases()[14]
    ref = J.entropy_decode(data)
    buf = np.full(ref.info.coef_count + 100, 77, dtype=np.int16)
    c = J.entropy_decode(data, out=buf)
    assert np.shares_memory(c.coef, buf) and np.array_equal(c.coef, ref.coef) and (buf[ref.info.coef_count:] == 77).all()
    shared = bytearray(2 * ref.info.coef_count)          # any writable buffer, as a shared-memory block is
    assert np.array_equal(J.entropy_decode(memoryview(data), out=shared).coef, ref.coef)
    with pytest.raises(ValueError, match="out"):
        J.entropy_decode(data, out=np.empty(ref.info.coef_count - 1, dtype=np.int16))
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    assert np.array_equal(J.entropy_decode(str(path)).coef, ref.coef) and np.array_equal(J.entropy_decode(path).coef, ref.coef)


def test_info_and_coefficients_pickle():
    c = J.entropy_decode(R.cases()[9][1])
    d = pickle.loads(pickle.dumps(c))
    for k in J.JpegInfo.__slots__:
        a, b = getattr(c.info, k), getattr(d.info, k)
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, k
    assert np.array_equal(c.coef, d.coef) and d.info.size == (c.info.width, c.info.height)


def _save(img, mode=None, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_unsupported_files_say_why():
    img = R.picture(24, 40, 5, False)
    with pytest.raises(J.Unsupported, match="progressive"):
        J.parse(_save(img, progressive=True))
    with pytest.raises(J.Unsupported, match="4 components"):
        J.parse(_save(np.dstack([img, img[..., :1]]), "CMYK"))
    with pytest.raises(J.Unsupported, match="progressive"):
        J.entropy_decode(_save(img, progressive=True))
    base = bytearray(_save(img, quality=90, subsampling=2))
    sof = base.index(b"\xff\xc0")
    odd = bytearray(base)
    odd[sof + 11] = 0x12          # luma 1x2: a sampling libjpeg takes and the split does not
    with pytest.raises(J.Unsupported, match="1x2"):
        J.parse(bytes(odd))
    twelve = bytearray(base)
    twelve[sof + 4] = 12
    with pytest.raises(J.Unsupported, match="12-bit"):
        J.parse(bytes(twelve))
    sof1 = bytearray(base)
    sof1[sof + 1] = 0xC1
    with pytest.raises(J.Unsupported, match="SOF1"):
        J.parse(bytes(sof1))
    # three components without a JFIF marker and with ids that say nothing (here 'R', 'G', 'B'): not known to be YCbCr
    app0 = base.index(b"\xff\xe0")
    nojfif = bytearray(base)
    nojfif[app0 + 4:app0 + 8] = b"XXXX"
    for c, cid in enumerate(b"RGB"):
        nojfif[sof + 10 + 3 * c] = nojfif[nojfif.index(b"\xff\xda") + 5 + 2 * c] = cid          # in the frame and in the scan
    with pytest.raises(J.Unsupported, match="YCbCr"):
        J.parse(bytes(nojfif))


def test_malformed_files_are_value_errors_with_the_reason():
    data = bytearray(R.cases()[18][1])
    with pytest.raises(ValueError, match="SOI"):
        J.parse(b"not a jpeg at all")
    with pytest.raises(ValueError, match="truncated scan"):
        J.entropy_decode(bytes(data[:len(data) - 40]))
    dqt = data.index(b"\xff\xdb")
    long_field = bytearray(data)
    long_field[dqt + 2:dqt + 4] = b"\xff\xff"
    with pytest.raises(ValueError, match="length"):
        J.parse(bytes(long_field))
    no_table = bytearray(data)
    dht = no_table.index(b"\xff\xc4")
    no_table[dht + 1] = 0xFE          # the first DHT marker becomes a comment: its table is missing at the scan
    with pytest.raises(ValueError, match="missing"):
        J.parse(bytes(no_table))


def test_truncations_and_corruptions_raise_or_return():
    """every truncation of one small file and 400 fixed-seed single-byte corruptions: each call raises Unsupported / ValueError or returns;
    reaching the end of this test is the assertion (no hang, no crash of the interpreter)"""
    data = next(d for n, d, _ in R.cases() if n.startswith("16x16-420"))
    outcomes = {"ok": 0, "error": 0}

    def run(blob):
        try:
            J.entropy_decode(blob)
            outcomes["ok"] += 1
        except (ValueError, J.Unsupported) as e:
            assert str(e)
            outcomes["error"] += 1

    for n in range(len(data)):
        run(data[:n])
    rng = np.random.default_rng(2024)
    restart = next(d for n, d, _ in R.cases() if n.startswith("37x53") and "blocks" in n)
    for src in (data, restart):
        for _ in range(200):
            blob = bytearray(src)
            blob[int(rng.integers(2, len(blob)))] = int(rng.integers(0, 256))
            run(bytes(blob))
    assert outcomes["error"] >= len(data) - 8 and outcomes["ok"] > 0


def test_entropy_stage_is_thread_safe():
    """the entries keep no state: eight threads decoding different files at once get what one thread gets"""
    from concurrent.futures import ThreadPoolExecutor
    blobs = [d for _, d, _ in R.cases()]
    want = [J.entropy_decode(d).coef for d in blobs]
    with ThreadPoolExecutor(8) as pool:
        for _ in range(3):
            got = list(pool.map(lambda d: J.entropy_decode(d).coef, blobs))
            assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_thread_pool_is_sized_by_the_quota_not_the_machine():
    from diffusionvid_amd.utils import comm
    n = J.default_threads()
    assert 1 <= n <= 32 and n == comm.rank_thread_cap(len(os.sched_getaffinity(0)), 1, comm.cpu_quota())


def test_loader_reads_sizes_from_the_header(tmp_path):
    """DeviceJpegLoader.size: header only (a file cut off behind its first 700 bytes still answers), Pillow for a progressive file, and
    StillImageDataset.original_size goes through it without calling the loader"""
    from diffusionvid_amd.data.datasets.still import StillImageDataset
    img = R.picture(120, 200, 3, False)
    full = _save(img, quality=90)
    (tmp_path / "head.jpg").write_bytes(full[:700])
    (tmp_path / "prog.jpg").write_bytes(_save(img[:50, :70], progressive=True))
    (tmp_path / "bad.jpg").write_bytes(b"\xff\xd8 nothing")
    loader = J.DeviceJpegLoader("cpu")
    assert loader.size(tmp_path / "head.jpg") == (200, 120) and loader.size(str(tmp_path / "prog.jpg")) == (70, 50)
    with pytest.raises(ValueError, match="bad.jpg"):
        loader.size(tmp_path / "bad.jpg")

    class NoDecode(J.DeviceJpegLoader):
        def __call__(self, path):
            raise AssertionError("original_size decoded %s" % path)

    ds = StillImageDataset([str(tmp_path / "head.jpg"), str(tmp_path / "prog.jpg")], loader=NoDecode("cpu"))
    assert ds.original_size(0) == (200, 120) and ds.original_size(1) == (70, 50)


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def test_host_stage_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tools/jpeg_entropy_check.cpp + csrc/jpeg_host.cpp as a program of their own under -fsanitize=address,undefined, over the valid set,
    every truncation of three files and 2000 fixed-seed corruptions: exit 0 and no sanitizer report.  Nothing is loaded into Python."""
    cxx = _compiler()
    assert cxx, "no host C++ compiler (c++, g++, clang++ or $CXX)"
    exe = tmp_path / "jpeg_entropy_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"),
                    os.path.join(ROOT, "diffusionvid_amd", "csrc", "jpeg_host.cpp"), "-o", str(exe)], check=True)
    files = tmp_path / "files"
    files.mkdir()
    cases = R.cases()
    for name, data, _ in cases:
        (files / ("ok_" + name + ".jpg")).write_bytes(data)
    small = [next(d for n, d, _ in cases if n.startswith(p)) for p in ("8x4-444", "16x16-420", "9x17-grey")]
    for i, data in enumerate(small):
        for n in range(len(data)):
            (files / ("cut%d_%04d.jpg" % (i, n))).write_bytes(data[:n])
    rng = np.random.default_rng(7)
    pool = [d for n, d, _ in cases if len(d) < 6000]
    for i in range(2000):
        blob = bytearray(pool[i % len(pool)])
        for _ in range(1 + i % 3):          # one to three damaged bytes, headers included
            blob[int(rng.integers(0, len(blob)))] = int(rng.integers(0, 256))
        (files / ("bad_%04d.jpg" % i)).write_bytes(bytes(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(files)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    m = re.search(r"(\d+) files: (\d+) decoded, (\d+) malformed, (\d+) unsupported, 0 failures", run.stdout)
    assert m and int(m.group(1)) == len(cases) + sum(len(d) for d in small) + 2000 and int(m.group(2)) >= len(cases) and int(m.group(3)) > 500, run.stdout
