"""The host half of Method.jpegDecoder = "device" -- the coefficients the library hands to the device (vfsms_jpeg_coefficients), the
specification they go through (tests/jpeg_dec_ref.py) and the routing of the ingest -- without a GPU.  The specification is held to
Pillow's decode byte for byte here; tests/test_jpeg_dec_gpu.py holds the kernel to the specification."""
import io
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import _lib

import jpeg_dec_cases as K
import jpeg_dec_ref as R


@pytest.fixture(scope="module")
def lib():
    if _lib.jpeg_decode(K.jpeg_bytes(np.zeros((16, 16), np.uint8)), False) is None:
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")
    return _lib


def _pillow_gray(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data)); im.draft("L", im.size)
    return np.asarray(im if im.mode == "L" else im.convert("L"))


@pytest.fixture(scope="module")
def decoded(lib):
    """{name: (frame, (h, w, comps) of jpeg_coefficients, planes of the reference, unclamped planes, report)}, once for the module"""
    out = {}
    for name, h, w, nc, data in K.host_set():
        got = lib.jpeg_coefficients(data)
        assert got is not None, name
        frame = R.parse_frame(data)
        coefs, tables = [c for c, _ in got[2]], [q for _, q in got[2]]
        report = {}
        planes = R.decode_planes(coefs, tables, h, w, frame["comps"], report)
        raw = R.decode_planes(coefs, tables, h, w, frame["comps"], unclamped=True)
        out[name] = (frame, got, planes, raw, report)
    return out


def test_reference_on_library_coefficients_equals_pillow(lib, decoded):
    """jpeg_coefficients -> dequantise, jidctint's two passes, + 128, clamp, crop == Pillow's grayscale decode, byte for byte, and on the
    4:2:0 files the chroma planes == those jpeg_read_raw_data hands out (jpeg_decode_raw420) -- the planes k_ingest_420 already takes"""
    for name, h, w, nc, data in K.host_set():
        frame, (gh, gw, comps), planes, _, report = decoded[name]
        assert (gh, gw, len(comps)) == (h, w, nc) == (frame["h"], frame["w"], len(frame["comps"])), name
        print("%s: largest intermediate %d, largest column-pass output %d" % (name, report["intermediate"], report["column_pass"]))
        assert np.array_equal(planes[0], _pillow_gray(data)), name
        if nc == 3:
            Y, Cb, Cr, rh, rw = lib.jpeg_decode_raw420(data)
            assert (rh, rw) == (h, w)
            ch, cw = (h + 1) // 2, (w + 1) // 2
            assert planes[1].shape == (ch, cw)
            assert np.array_equal(planes[0], Y[:h, :w]) and np.array_equal(planes[1], Cb[:ch, :cw]) and np.array_equal(planes[2], Cr[:ch, :cw]), name


def test_reference_reaches_both_clamps(decoded):
    """a condition on the REFERENCE alone: over the set the unclamped samples go below 0 and above 255, and at least 5 % of the samples of
    each bit-noise file are clamped (measured: 6.7 % at quality 100, 50 % at quality 10)"""
    lo = min(int(p.min()) for _, _, _, raw, _ in decoded.values() for p in raw)
    hi = max(int(p.max()) for _, _, _, raw, _ in decoded.values() for p in raw)
    assert lo < 0 and hi > 255, (lo, hi)
    for name in K.BIT_NOISE_FILES:
        raw = decoded[name][3][0]
        share = float(((raw < 0) | (raw > 255)).mean())
        print("%s: %.3f of the samples clamped, range %d .. %d" % (name, share, raw.min(), raw.max()))
        assert share >= 0.05, (name, share)


def test_layout_grid_tables_and_table_precision(lib, decoded):
    """block counts on the iMCU grid, tables in natural order (the file keeps them in zig-zag order), a file with 16-bit tables"""
    for name, h, w, nc, data in K.host_set():
        frame, (_, _, comps), _, _, _ = decoded[name]
        grid = R.block_grid(h, w, frame["comps"])
        for k, (coef, quant) in enumerate(comps):
            assert coef.dtype == np.int16 and quant.dtype == np.uint16 and coef.shape == grid[k] + (64,), (name, k, coef.shape, grid[k])
            assert np.array_equal(quant, frame["tables"][frame["comps"][k][2]]), (name, k)
        if nc == 3:
            pw, ph = (w + 15) & ~15, (h + 15) & ~15
            assert grid == [(ph // 8, pw // 8), (ph // 16, pw // 16), (ph // 16, pw // 16)], (name, grid)      # the raw 4:2:0 layout's planes
        else:
            assert grid == [((h + 7) // 8, (w + 7) // 8)], (name, grid)
    # natural order is not zig-zag order: position 2 of the file's table is natural position 8
    name, h, w, nc, data = K.host_set()[1]
    p = data.index(b"\xff\xdb")
    assert data[p + 4] == 0 and decoded[name][1][2][0][1][8] == data[p + 5 + 2] and decoded[name][1][2][0][1][2] == data[p + 5 + 5]
    for name, h, w, nc, data in (K.host_set()[1], K.host_set()[5]):
        wide = K.sixteen_bit_tables(data)
        assert set(R.parse_frame(wide)["table_bits"].values()) == {16} and set(R.parse_frame(data)["table_bits"].values()) == {8}
        got = lib.jpeg_coefficients(wide)
        assert got is not None and len(got[2]) == nc
        for (c16, q16), (c8, q8) in zip(got[2], decoded[name][1][2]):
            assert np.array_equal(c16, c8) and np.array_equal(q16, q8), name
        assert np.array_equal(_pillow_gray(wide), _pillow_gray(data))


def test_refusals(lib):
    """4:4:4, 4:2:2, CMYK, a 4:2:0 file of four columns, a 12-bit frame and a truncated file: None, the caller takes today's path"""
    for name, _h, _w, data in K.refused_set():
        assert lib.jpeg_coefficients(data) is None, name
    assert lib.jpeg_coefficients(b"\xff\xd8\xff\xd9") is None and lib.jpeg_coefficients(b"not a jpeg") is None


# ---- routing ----------------------------------------------------------------------------------------------------------------------------------
def _recording_engine(oracle, with_dct=True):
    from fakes import NativeJpegEngine

    class Recording(NativeJpegEngine):
        """NativeJpegEngine that writes down which entry saw which file (by size); its device decoder takes what the library's host half
        takes and fills the tiles with the bytes the host decoder yields -- the same bytes, by tests/test_jpeg_dec_gpu.py"""

        def __init__(self, oracle):
            super().__init__(oracle)
            self.dct_seen, self.dct_took, self.jpeg_seen = [], [], []

        def tile_fill_jpeg(self, gray, color, data):
            self.jpeg_seen.append(len(data))
            return super().tile_fill_jpeg(gray, color, data)

    if with_dct:
        def tile_fill_jpeg_dct(self, gray, color, data):
            self.dct_seen.append(len(data))
            if _lib.jpeg_coefficients(data) is None:
                return False
            assert NativeJpegEngine.tile_fill_jpeg(self, gray, color, data)
            self.native.pop()
            self.dct_took.append(len(data))
            return True
        Recording.tile_fill_jpeg_dct = tile_fill_jpeg_dct
    return Recording(oracle)


def test_routing_of_the_decoder_choice(lib, oracle, tmp_path):
    """jpegDecoder "device": tile_fill_jpeg_dct sees every JPEG once; a file it refuses (4:4:4) goes on to tile_fill_jpeg, a file both refuse
    (CMYK) on to `_decode_once`, each once.  "host": the new entry is never called.  An engine without it: NotImplementedError."""
    from PIL import Image
    from imagestitch_amd.synthetic import SyntheticGrid
    from imagestitch_amd import stitcher as ST
    assert isa.Stitcher.jpegDecoder == "host"
    g = SyntheticGrid(2, 2, 256, overlap=0.25)
    files = []
    for k, t in enumerate(g.tiles(threads=1)):
        p = os.path.join(str(tmp_path), "t_%02d.jpg" % k)
        rgb = np.stack([t, t, t], -1)
        if k == 2:
            Image.fromarray(rgb).save(p, quality=93, subsampling=0)             # 4:4:4: the host decoder's
        elif k == 3:
            Image.fromarray(rgb).convert("CMYK").save(p, quality=94)            # CMYK: Pillow's
        else:
            Image.fromarray(t).save(p, quality=92 - k)                          # gray files of different sizes in bytes
        files.append(p)
    sizes = [os.path.getsize(p) for p in files]
    assert len(set(sizes)) == 4
    counts = {"once": []}
    real_once = ST._decode_once

    def once(path, color):
        counts["once"].append(os.path.getsize(path))
        return real_once(path, color)
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod)
    env_old = os.environ.pop("VFSMS_NATIVE_JPEG", None)
    ST._decode_once = once
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod = 1, 0.3, "surf", "fadeInAndFadeOut"
        isa.Stitcher.isColorMode = False
        mosaics = {}
        for decoder in ("device", "host"):
            eng = _recording_engine(oracle)
            s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.direction = 1
            s.jpegDecoder = decoder
            counts["once"] = []
            (status, mosaics[decoder]) = s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)
            assert status == (True, 3) and not eng.live
            if decoder == "device":
                assert sorted(eng.dct_seen) == sorted(sizes) and sorted(eng.dct_took) == sorted(sizes[:2])
                assert sorted(eng.jpeg_seen) == sorted(sizes[2:]) and eng.native == [sizes[2]]
                assert counts["once"] == [sizes[3]]
                assert s._ingestStats["dct"] == 2 and s._ingestStats["native"] == 3 and s._ingestStats["tiles"] == 4
            else:
                assert eng.dct_seen == [] and sorted(eng.jpeg_seen) == sorted(sizes) and counts["once"] == [sizes[3]]
                assert "dct" not in s._ingestStats and s._ingestStats["native"] == 3
        assert np.array_equal(mosaics["device"], mosaics["host"])
        # VFSMS_NATIVE_JPEG=0 still sends everything to Pillow
        os.environ["VFSMS_NATIVE_JPEG"] = "0"
        eng = _recording_engine(oracle)
        s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.direction = 1; s.jpegDecoder = "device"
        counts["once"] = []
        assert s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)[0] == (True, 3)
        assert eng.dct_seen == [] and eng.jpeg_seen == [] and sorted(counts["once"]) == sorted(sizes)
        os.environ.pop("VFSMS_NATIVE_JPEG")
        # an engine without the entry, a value that is no decoder
        s = isa.Stitcher(); s._engine = _recording_engine(oracle, with_dct=False); s.isPrintLog = False; s.direction = 1; s.jpegDecoder = "device"
        with pytest.raises(NotImplementedError):
            s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)
        assert not s._engine.live
        s.jpegDecoder = "gpu"
        with pytest.raises(ValueError):
            s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)
    finally:
        ST._decode_once = real_once
        os.environ.pop("VFSMS_NATIVE_JPEG", None)
        if env_old is not None:
            os.environ["VFSMS_NATIVE_JPEG"] = env_old
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod = old
