"""CPU tests of the 16-bit path (vfsms_deep_*): the specification tests/deep_ref.py against brute force, the 16-bit band writers and the
bin table of the mosaic gather under the host sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

from imagestitch_amd.io import TiffBandWriter, NpyBandWriter

import deep_cases as DC
import deep_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against brute force -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DC.KINDS)
def test_window_equals_sorting(kind):
    tiles = DC.tile_set(kind)
    s = np.sort(np.concatenate([t.reshape(-1) for t in tiles]))
    N = len(s)
    for lo_ppm, hi_ppm in DC.PPM_PAIRS:
        lo, hi = int(s[(N - 1) * lo_ppm // 1000000]), int(s[(N - 1) * hi_ppm // 1000000])
        if hi == lo:
            lo, hi = (lo, lo + 1) if lo < 65535 else (hi - 1, hi)
        assert DR.window(tiles, lo_ppm, hi_ppm) == (lo, hi), (kind, lo_ppm, hi_ppm)
    assert DR.window([np.full((2, 2), 65535, np.uint16)], 0, 1000000) == (65534, 65535)
    assert DR.window([np.zeros((2, 2), np.uint16)], 0, 0) == (0, 1)
    for bad in ((-1, 5), (6, 5), (0, 1000001)):
        with pytest.raises(ValueError):
            DR.window(tiles, *bad)


def test_reduce_is_rounded_and_clamped():
    k = np.arange(256)
    assert np.array_equal(DR.reduce((257 * k).astype(np.uint16), 0, 65535), k)
    v = np.arange(65536).astype(np.uint16)
    for lo, hi in ((0, 65535), (7, 8), (100, 4195), (65534, 65535), (2003, 5069)):
        D = hi - lo
        want = [((min(max(int(x), lo), hi) - lo) * 255 + D // 2) // D for x in range(0, 65536, 97)]
        assert DR.reduce(v, lo, hi)[::97].tolist() == want
        out = DR.reduce(v, lo, hi)
        assert out.dtype == np.uint8 and out[lo] == 0 and out[hi] == 255 and out[0] == 0 and out[65535] == 255
    for bad in ((5, 5), (6, 5), (-1, 5), (0, 65536)):
        with pytest.raises(ValueError):
            DR.reduce(v, *bad)


def _mosaic_loop(tiles, yx, rows, cols, mode, feather):
    out = np.zeros((rows, cols), np.uint16)
    for y in range(rows):
        for x in range(cols):
            sw = sp = 0
            for t, (ty, tx) in zip(tiles, yx):
                h, w = t.shape
                r, c = y - ty, x - tx
                if not (0 <= r < h and 0 <= c < w):
                    continue
                if mode == 0:
                    sw, sp = 1, int(t[r, c])
                else:
                    d = min(r + 1, h - r, c + 1, w - c)
                    wg = min(d, feather) if feather > 0 else d
                    sw += wg
                    sp += wg * int(t[r, c])
            if sw:
                out[y, x] = (sp + sw // 2) // sw
    return out


def test_mosaic_equals_a_per_pixel_loop():
    rng = np.random.default_rng(5)
    for trial in range(12):
        rows, cols, n = int(rng.integers(1, 25)), int(rng.integers(1, 25)), int(rng.integers(1, 8))
        tiles, yx = [], []
        for _ in range(n):
            h, w = int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1))
            tiles.append(rng.integers(0, 65536, (h, w)).astype(np.uint16))
            yx.append((int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1))))
        for mode, feather in ((0, 0), (1, 0), (1, 1), (1, 3), (1, 32767)):
            assert np.array_equal(DR.mosaic(tiles, yx, rows, cols, mode, feather), _mosaic_loop(tiles, yx, rows, cols, mode, feather)), (trial, mode, feather)


def test_mosaic_identities_and_overflow():
    rng = np.random.default_rng(6)
    t = rng.integers(0, 65536, (17, 23)).astype(np.uint16)
    for feather in DC.FEATHERS:
        assert np.array_equal(DR.mosaic([t], [(0, 0)], 17, 23, 1, feather), t)
        assert np.array_equal(DR.mosaic([t, t], [(0, 0), (0, 0)], 17, 23, 1, feather), t)
    top = np.full((300, 300), 65535, np.uint16)
    out = DR.mosaic([top] * 6, [(k, 2 * k) for k in range(6)], 320, 320, 1, 0)
    cover = np.zeros((320, 320), bool)
    for k in range(6):
        cover[k:k + 300, 2 * k:2 * k + 300] = True
    assert np.all(out[cover] == 65535) and np.all(out[~cover] == 0)
    with pytest.raises(ValueError):
        DR.mosaic([t], [(1, 0)], 17, 23, 1, 0)
    for name in DC.layouts():                                # the shared layouts are inside their canvases, and every mode has a reference
        assert DC.reference(name, 0, 0).shape == DC.reference(name, 1, 5).shape


# ---- the writers -------------------------------------------------------------------------------------------------------------------------
def _bands(img, band_rows):
    return [(r0, img[r0:r0 + band_rows]) for r0 in range(0, img.shape[0], band_rows)]


@pytest.mark.parametrize("force_big", (False, True))
@pytest.mark.parametrize("band_rows", (1, 7, 45))
def test_tiff_writer_16_bit(tmp_path, band_rows, force_big):
    from PIL import Image
    img = np.random.default_rng(1).integers(0, 65536, (45, 67)).astype(np.uint16)
    path = str(tmp_path / "m.tif")
    w = TiffBandWriter(path, force_big=force_big)
    for r0, band in _bands(img, band_rows):
        w(r0, band, img.shape)
    raw = open(path, "rb").read()
    assert raw[:4] == (b"II\x2b\x00" if force_big else b"II\x2a\x00")
    im = Image.open(path)
    assert im.mode in ("I;16", "I;16L") and im.size == (67, 45)
    assert np.array_equal(np.asarray(im), img)
    # the strips themselves: byte counts in BYTES, little-endian samples, back to back from the header on
    first = 16 if force_big else 8
    assert raw[first:first + img.size * 2] == img.astype("<u2").tobytes()


@pytest.mark.parametrize("band_rows", (1, 7, 45))
def test_npy_writer_16_bit(tmp_path, band_rows):
    img = np.random.default_rng(2).integers(0, 65536, (45, 67)).astype(np.uint16)
    path = str(tmp_path / "m.npy")
    w = NpyBandWriter(path)
    for r0, band in _bands(img, band_rows):
        w(r0, band, img.shape)
    back = np.load(path)
    assert back.dtype == np.uint16 and np.array_equal(back, img)


def _classic_tiff8(img, band_rows):
    """the bytes TiffBandWriter has always written for an 8-bit image (classic TIFF), built here by hand"""
    rows, cols = img.shape[:2]
    ch = img.shape[2] if img.ndim == 3 else 1
    out = bytearray(struct.pack("<2sHI", b"II", 42, 0))
    strips = []
    for r0, band in _bands(img, band_rows):
        if band.ndim == 3:
            band = band[:, :, ::-1]
        strips.append((len(out), band.size))
        out += np.ascontiguousarray(band).tobytes()
    if len(out) & 1:
        out += b"\0"
    n = len(strips)
    off_pos = len(out); out += struct.pack("<%dI" % n, *[o for o, _c in strips])
    cnt_pos = len(out); out += struct.pack("<%dI" % n, *[c for _o, c in strips])
    bps = 8
    if ch == 3:
        bps = len(out); out += struct.pack("<3H", 8, 8, 8) + b"\0\0"
    ifd = len(out)
    tags = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, ch, bps), (259, 3, 1, 1), (262, 3, 1, 2 if ch == 3 else 1),
            (273, 4, n, off_pos if n > 1 else strips[0][0]), (277, 3, 1, ch), (278, 4, 1, min(band_rows, rows)), (279, 4, n, cnt_pos if n > 1 else strips[0][1])]
    out += struct.pack("<H", len(tags))
    for t, ty, c, v in tags:
        out += struct.pack("<HHII", t, ty, c, v)
    out += struct.pack("<I", 0)
    out[4:8] = struct.pack("<I", ifd)
    return bytes(out)


@pytest.mark.parametrize("shape", ((45, 67), (45, 67, 3)))
@pytest.mark.parametrize("band_rows", (7, 45))
def test_8_bit_files_are_what_they_were(tmp_path, shape, band_rows):
    img = np.random.default_rng(3).integers(0, 256, shape).astype(np.uint8)
    path = str(tmp_path / "m8.tif")
    w = TiffBandWriter(path)
    for r0, band in _bands(img, band_rows):
        w(r0, band, img.shape)
    assert open(path, "rb").read() == _classic_tiff8(img, band_rows)
    npy = str(tmp_path / "m8.npy")
    w = NpyBandWriter(npy)
    for r0, band in _bands(img, band_rows):
        w(r0, band, img.shape)
    ref = str(tmp_path / "ref.npy")
    mm = np.lib.format.open_memmap(ref, mode="w+", dtype=np.uint8, shape=img.shape)
    mm[:] = img; mm.flush(); del mm
    assert open(npy, "rb").read() == open(ref, "rb").read()


# ---- the bin table ---------------------------------------------------------------------------------------------------------------------
def test_bin_table_equals_brute_force_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "deep_bins_host_check.cpp")
    exe = str(tmp_path / "deep_bins_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, with nothing preloaded
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr
    assert "blocks ok" in p.stdout, p.stdout
