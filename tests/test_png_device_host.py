"""CPU tests of PNG results coded on the device (Method.pngEncoder = "device"): the specification tests/png_ref.py against Pillow, zlib's inflate
and an un-filter of this file's own; csrc/png_core.h -- the lines the kernels compile -- through tools/png_core_host_check.cpp under the host
sanitizers; DevicePngFile fed the specification's payloads; and the Stitcher's wiring through a fake engine.  All comparisons are of bytes."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref as ref                     # noqa: E402
import png_cases as K                     # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from test_pyramid_host import PyramidOracleEngine, _Project      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunks(data):
    """-> [(tag, data)] of a PNG, every CRC checked"""
    assert data[:8] == ref.SIGNATURE
    out, at = [], 8
    while at < len(data):
        n = struct.unpack_from(">I", data, at)[0]
        tag, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack_from(">I", data, at + 8 + n)[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        out.append((tag, body)); at += 12 + n
    assert at == len(data)
    return out


def unfilter(filtered, bpp):
    """the PNG specification's reconstruction, byte by byte (independent of png_ref's vector code) -> the raw rows"""
    R, n = filtered.shape[0], filtered.shape[1] - 1
    raw = np.zeros((R, n), np.int64)
    for r in range(R):
        t = int(filtered[r, 0])
        for i in range(n):
            a = int(raw[r, i - bpp]) if i >= bpp else 0
            b = int(raw[r - 1, i]) if r else 0
            c = int(raw[r - 1, i - bpp]) if r and i >= bpp else 0
            if t == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            else:
                pred = (0, a, b, (a + b) // 2)[t]
            raw[r, i] = (int(filtered[r, 1 + i]) + pred) & 255
    return raw.astype(np.uint8)


# ---- 1. the specification itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_the_specifications_files_are_png(case):
    from PIL import Image
    _name, make, S = case
    img = make()
    ch = 1 if img.ndim == 2 else 3
    data = ref.encode(img, S)
    got = np.asarray(Image.open(io.BytesIO(data)))
    assert got.shape == img.shape and np.array_equal(got, img)
    cs = chunks(data)
    n_seg = -(-img.shape[0] // S)
    assert [t for t, _ in cs] == [b"IHDR"] + [b"IDAT"] * (n_seg + 2) + [b"IEND"]
    assert cs[1][1] == b"\x78\x01" and cs[-2][1][:5] == b"\x01\x00\x00\xff\xff"
    z = zlib.decompressobj()
    flat = z.decompress(b"".join(body for tag, body in cs if tag == b"IDAT"))
    assert z.eof and not z.unused_data
    f = ref.filter_rows(img)
    assert flat == f.tobytes()
    assert all(body[0] & 1 == 0 and body[-4:] == b"\x00\x00\xff\xff" for _t, body in cs[2:-2])      # not final; ends on a byte
    if img.size <= 4000:
        assert np.array_equal(unfilter(f, ch), img.reshape(img.shape[0], -1))


def test_every_split_into_bands_gives_the_files_middle():
    rng = np.random.default_rng(3)
    for img, S in ((K.real_crop(70, 90), 16), (K.noise((45, 13, 3), 9), 4), (K.diagonal((33, 40, 3)), 1)):
        R = img.shape[0]
        data = ref.encode(img, S)
        head, tail = ref.head(R, img.shape[1], 1 if img.ndim == 2 else 3), ref.tail(ref.band_adler(img))
        middle = data[len(head):len(data) - len(tail)]
        assert data.startswith(head) and data.endswith(tail) and middle == ref.device_payload(img, S)
        for _ in range(4):
            cuts = sorted(set(int(c) * S for c in rng.integers(1, -(-R // S), 3) if int(c) * S < R))
            edges = [0] + cuts + [R]
            parts, adler = b"", 1
            for r0, r1 in zip(edges[:-1], edges[1:]):
                parts += ref.device_payload(img, S, r0, r1 - r0)
                adler = ref.adler_combine(adler, ref.band_adler(img, r0, r1 - r0), (r1 - r0) * (1 + img[0].size))
            assert parts == middle and adler == ref.band_adler(img), edges


def test_checksum_joins_equal_zlib():
    rng = np.random.default_rng(11)
    for _ in range(200):
        a, b = rng.bytes(int(rng.integers(0, 700))), rng.bytes(int(rng.integers(0, 70000 if _ % 20 == 0 else 700)))
        assert ref.adler_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(a + b)
        assert isa.io.adler_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(a + b)
        assert ref.crc_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
    big = b"\xff" * 200000                                          # sums far beyond one modulus
    assert ref.adler_combine(zlib.adler32(big), zlib.adler32(big[:131071]), 131071) == zlib.adler32(big + big[:131071])


def test_geometry_refusals():
    for kw in (dict(S=0, rows=4, cols=4, ch=1), dict(S=4097, rows=4, cols=4, ch=1), dict(S=16, rows=4, cols=4, ch=2), dict(S=16, rows=0, cols=4, ch=1),
               dict(S=16, rows=4, cols=0, ch=3), dict(S=4096, rows=5000, cols=23302, ch=3)):
        with pytest.raises(ValueError):
            ref.check_geometry(**kw)
    ref.check_geometry(4096, 5000, 23301, 3)                        # 4096 x 69904 x 15 bits: just inside 32 bits
    ref.check_geometry(16, 18649, 16807, 3)


# ---- 2. the case set reaches every filter type, a tie and the byte 128 -----------------------------------------------------------------------------
def test_the_cases_make_the_reference_choose_every_filter():
    seen = set()
    for _name, make, _S in K.CASES:
        seen |= set(ref.filter_rows(make())[:, 0].tolist())
    assert seen == {0, 1, 2, 3, 4}
    assert set(ref.filter_rows(K.real_crop(48, 333))[:, 0].tolist()) == {1, 3, 4}
    assert set(ref.filter_rows(K.h_ramp((20, 70)))[1:, 0].tolist()) == {2}
    assert set(ref.filter_rows(K.none_wins())[:, 0].tolist()) == {0}
    f = ref.filter_rows(K.diagonal((40, 200, 3)))               # Paeth (and Average, where the first pixel is cheaper under it) leave zeros
    assert set(f[1:, 0].tolist()) == {3, 4} and (f[:, 0] == 4).sum() > 30 and not f[1:, 4:].any() and f[1:37, 1].all()
    # a flat row 0: Sub and Paeth both leave the first byte and zeros -- a tie, and the lower type wins
    row = np.full(30, 93, np.uint8)
    cand = ref.candidates(row, np.zeros(30, np.uint8), 1)
    assert ref.cost(cand[1]) == ref.cost(cand[4]) == 93 < min(ref.cost(cand[t]) for t in (0, 2, 3))
    assert ref.filter_rows(K.flat((19, 300)))[0, 0] == 1
    # the byte 128 costs 128, under the filter that wins
    f = ref.filter_rows(K.cost_128())
    assert f[0, 0] == 0 and (f[0, 1:] == 128).sum() == 3 and ref.cost(f[0, 1:]) == 3 * 128 and ref.cost([128]) == 128 and ref.cost([129]) == 127


# ---- 3. compression on real pixels -------------------------------------------------------------------------------------------------------------------
def test_real_strips_code_smaller_than_the_host_writer():
    z = np.load(os.path.join(ROOT, "tests", "golden", "real_full_strips.npz"))
    raw = mine = host = 0
    for k in z.files:
        img = np.ascontiguousarray(z[k][:256])
        rows = np.zeros((img.shape[0], 1 + img.shape[1]), np.uint8)
        rows[:, 1:] = img                                           # filter 0 on every row, as PngBandWriter
        raw += img.size
        host += len(zlib.compress(rows.tobytes(), 1))
        mine += len(ref.device_payload(img, 16)) + len(ref.head(*img.shape, 1)) + len(ref.tail(0)) - len(ref.SIGNATURE)
    print("real strips: device %.3f of the raw bytes, host (filter 0, zlib level 1) %.3f" % (mine / raw, host / raw))
    assert mine < host


# ---- 4. csrc/png_core.h under the host sanitizers ---------------------------------------------------------------------------------------------------
def test_the_core_the_kernels_compile_equals_the_reference(tmp_path):
    src = os.path.join(ROOT, "tools", "png_core_host_check.cpp")
    exe = str(tmp_path / "png_core_host_check")
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    args, imgs = [], []
    for k, (_name, make, S) in enumerate(K.CASES):
        img = make()
        with open(str(tmp_path / ("%d.in" % k)), "wb") as f:
            f.write(struct.pack("<4I", img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, S) + img.tobytes())
        args += [str(tmp_path / ("%d.in" % k)), str(tmp_path / ("%d.out" % k))]
        imgs.append((img, S))
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr                      # the sanitizers, leak detection included, report nothing
    assert "png_core_host_check: %d cases ok" % len(K.CASES) in p.stdout
    for k, (img, S) in enumerate(imgs):
        o = open(str(tmp_path / ("%d.out" % k)), "rb").read()
        R = img.shape[0]
        f = ref.filter_rows(img)
        assert o[:R] == f[:, 0].tobytes(), K.CASES[k][0]
        adler, n = struct.unpack_from("<II", o, R)
        at, got = R + 8, b""
        for _ in range(n):
            m = struct.unpack_from("<I", o, at)[0]
            got += o[at + 4:at + 4 + m]; at += 4 + m
        assert at == len(o) and n == -(-R // S)
        assert adler == ref.band_adler(img, filtered=f), K.CASES[k][0]
        assert got == ref.device_payload(img, S, filtered=f), K.CASES[k][0]


# ---- 5. DevicePngFile ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,S", [((70, 90), 16), ((45, 13, 3), 4), ((33, 40, 3), 1), ((5, 7), 64)])
def test_device_png_file_writes_the_specifications_file(tmp_path, shape, S):
    from PIL import Image
    img = K.noise(shape, 21) >> 3 << 3
    R = shape[0]
    want = ref.encode(img, S)
    rowbytes = 1 + img[0].size
    for band in (S, 2 * S, 3 * S, R + S):
        path = str(tmp_path / "sub" / ("f_%d.png" % band))
        w = isa.DevicePngFile(path, img.shape, S)
        for r0 in range(0, R, band):
            n = min(band, R - r0)
            w.append(np.frombuffer(ref.device_payload(img, S, r0, n), np.uint8), ref.band_adler(img, r0, n), n * rowbytes)
        w.close()
        data = open(path, "rb").read()
        assert data == want and w.bytes_written == len(want), band
    assert np.array_equal(np.asarray(Image.open(path)), img)


def test_device_png_file_refusals_and_abort(tmp_path):
    path = str(tmp_path / "sub" / "r.png")
    for shape, S in (((10, 10, 4), 16), ((10, 10, 2), 16), ((0, 10), 16), ((10, 0, 3), 16), ((10, 10), 0), ((10, 10), 4097), ((5000, 23302, 3), 4096)):
        with pytest.raises(ValueError):
            isa.DevicePngFile(path, shape, S)
    assert not os.path.exists(str(tmp_path / "sub"))                # refused before anything is written
    w = isa.DevicePngFile(path, (10, 10), 16)
    assert os.path.exists(path)
    with pytest.raises(ValueError):                                 # rows are missing
        w.close()
    w.abort()
    assert not os.path.exists(path)
    w.abort()


# ---- 6. the Stitcher ---------------------------------------------------------------------------------------------------------------------------------
class PngOracleEngine(PyramidOracleEngine):
    """PyramidOracleEngine plus canvas_encode_png_bands: the payloads of every band computed by the specification"""

    png_calls = 0
    plain_calls = 0

    def canvas_encode_png_bands(self, h, rows, cols, ch, segment_rows, band_rows):
        self.png_calls += 1
        if band_rows % segment_rows:
            raise ValueError("band_rows")
        img = self.canvas_download(h, rows, cols, ch)
        rgb = np.ascontiguousarray(img[:, :, ::-1]) if ch == 3 else img
        f = ref.filter_rows(rgb)
        for r0 in range(0, rows, band_rows):
            n = min(band_rows, rows - r0)
            yield r0, n, np.frombuffer(ref.device_payload(rgb, segment_rows, r0, n, filtered=f), np.uint8), ref.band_adler(rgb, r0, n, filtered=f)

    def canvas_download_bands(self, *a, **kw):
        self.plain_calls += 1
        return super().canvas_download_bands(*a, **kw)


def test_method_defaults():
    m = isa.Method
    assert (m.pngEncoder, m.pngSegmentRows) == ("host", 16)
    assert isa.Stitcher._ROUTES["device_png"] == "canvas_encode_png_bands"
    sink = lambda *a: None
    sink.device_png = True
    assert isa.Stitcher._routeOf(sink) == "device_png" and isa.Stitcher._routeOf(lambda *a: None) == "plain"
    assert isa.DevicePngFile is isa.io.DevicePngFile


def test_stitcher_writes_one_file_of_the_specifications_bytes(oracle, tmp_path):
    from PIL import Image
    P = _Project(tmp_path)
    eng0, host = P.run(oracle, "host", ext="png", engine=PngOracleEngine)
    assert eng0.png_calls == 0 and eng0.plain_calls == 1            # "host": the pixel bands and PngBandWriter, as before
    assert os.listdir(str(host)) == ["stitching_result_1.png"]
    host_bytes = open(str(host / "stitching_result_1.png"), "rb").read()
    mosaic = np.asarray(Image.open(io.BytesIO(host_bytes)))         # R G B
    assert mosaic.shape == (416, 476, 3)
    assert [t for t, _ in chunks(host_bytes)].count(b"IDAT") >= 1
    for tag, kw, S in (("dev", {}, 16), ("s4", {"pngSegmentRows": 4, "mosaicBandRows": 64}, 4), ("one", {"pngSegmentRows": 32, "mosaicBandRows": 4096}, 32)):
        eng, out = P.run(oracle, tag, ext="png", engine=PngOracleEngine, pngEncoder="device", **kw)
        assert eng.png_calls == 1 and eng.plain_calls == 0
        assert os.listdir(str(out)) == ["stitching_result_1.png"]
        data = open(str(out / "stitching_result_1.png"), "rb").read()
        assert data == ref.encode(mosaic, S), tag
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), mosaic)
    # everything else writes as with "host": other extensions, the whole-mosaic write, a sink of the user's, the pyramid
    for tag, ext, kw in (("tif", "tif", {}), ("whole", "png", {"streamOutput": False}),
                         ("pyr", "tif", {"outputPyramid": True, "pyramidTile": 32, "pyramidLevels": 2})):
        eng, out = P.run(oracle, tag, ext=ext, engine=PngOracleEngine, pngEncoder="device", **kw)
        assert eng.png_calls == 0, tag
    s = isa.Stitcher(); s._engine = eng; s.pngEncoder = "device"
    assert s._devicePng("png") and s._devicePng("PNG") and not s._devicePng("jpg")
    s.mosaicSink = lambda row0, band, full_shape: None
    assert not s._devicePng("png")
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "whole" / "stitching_result_1.png"))), mosaic)


def test_stitcher_refusals_come_before_any_decode(oracle, tmp_path):
    P = _Project(tmp_path)
    said = {}
    for tag, exc, kw in (("eng", NotImplementedError, {"engine": PyramidOracleEngine}), ("value", ValueError, {"pngEncoder": "gpu"}),
                         ("seg0", ValueError, {"pngSegmentRows": 0}), ("seg", ValueError, {"pngSegmentRows": 4097}), ("segf", ValueError, {"pngSegmentRows": 2.5}),
                         ("band", ValueError, {"pngSegmentRows": 24, "mosaicBandRows": 32})):
        kw.setdefault("engine", PngOracleEngine)
        kw.setdefault("pngEncoder", "device")
        with pytest.raises(exc) as e:
            P.run(oracle, tag, ext="png", **kw)
        said[tag] = str(e.value)
        assert P.decodes == 0, tag
        assert not (tmp_path / tag).exists() or not os.listdir(str(tmp_path / tag)), tag
    assert "canvas_encode_png_bands" in said["eng"] and "pngEncoder" in said["value"] and "pngSegmentRows" in said["seg"] and "mosaicBandRows" in said["band"]
    with pytest.raises(ValueError):                                 # an unknown value is refused whatever the output is
        P.run(oracle, "value2", ext="tif", engine=PngOracleEngine, pngEncoder="gpu")
    assert P.decodes == 0
