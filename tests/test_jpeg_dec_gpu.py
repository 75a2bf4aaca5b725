"""The device half of the JPEG decoder (csrc/jpeg_dec_kernels.hip; Method.jpegDecoder = "device") against its specification,
tests/jpeg_dec_ref.py, byte for byte: the bare operator on coefficients no file produced, vfsms_tile_fill_jpeg_dct on files against Pillow's
two decodes and against vfsms_tile_fill_jpeg, and the Stitcher with the switch on against the Stitcher with it off.
tests/test_jpeg_dec_host.py holds the specification itself to Pillow."""
import io
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid

import ingest_ref
import jpeg_dec_cases as K
import jpeg_dec_ref as R

pytestmark = pytest.mark.gpu

TABLES = (("ones", np.ones(64, np.uint16)), ("q50", R.Q50_LUMA.astype(np.uint16)), ("all255", np.full(64, 255, np.uint16)))
GRIDS = ((1, 1), (3, 5), (9, 33))       # one block; a partial wave (8 blocks a wave); several workgroups (32 blocks each), 297 = 9 * 32 + 9


def _pool(quant):
    """int16 (n, 64): DC only, a single AC term at each of the 64 positions (both signs, alone and on a DC), and the quantised forward DCT
    of random and of 0 / 255 pixel blocks.  Dequantised magnitudes stay within what 8-bit samples produce (<= 2040)."""
    rng = np.random.default_rng(int(quant.sum()))
    blocks = []
    for dc in (-2040, -1000, -1, 0, 1, 7, 1000, 2040):
        b = np.zeros(64, np.int64); b[0] = int(dc / quant[0]); blocks.append(b)
    for p in range(64):
        for sign, dc in ((1, 0), (-1, 0), (1, 300)):
            b = np.zeros(64, np.int64); b[0] = dc // int(quant[0]); b[p] += sign * max(1, 1016 // int(quant[p])); blocks.append(b)
    px = np.concatenate([rng.integers(0, 256, (40, 8, 8)), rng.integers(0, 2, (40, 8, 8)) * 255])
    pool = np.concatenate([np.array(blocks, np.int16), R.forward_dct_quantised(px, quant)])
    return pool


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("table", TABLES, ids=lambda t: t[0])
def test_jpeg_idct_equals_the_reference(engine, table, grid):
    """vfsms_jpeg_idct == idct_plane, exactly; the reference asserts its two conditions on these inputs before the device sees them"""
    name, quant = table
    br, bc = grid
    pool = _pool(quant)
    n = br * bc
    calls = -(-len(pool) // n)                                   # every block of the pool is seen at every grid
    coefs = [np.take(pool, np.arange(k * n, (k + 1) * n) % len(pool), 0).reshape(br, bc, 64) for k in range(calls)]
    report = {}
    wants = [R.idct_plane(c, quant, report=report) for c in coefs]
    print("%s %dx%d: %d calls, largest intermediate %d, largest column-pass output %d" % (name, br, bc, calls, report["intermediate"], report["column_pass"]))
    lo = min(int(R.idct_plane(c, quant, unclamped=True).min()) for c in coefs); hi = max(int(R.idct_plane(c, quant, unclamped=True).max()) for c in coefs)
    assert lo < 0 and hi > 255, (lo, hi)                         # both clamps are reached
    for k, (c, want) in enumerate(zip(coefs, wants)):
        got = engine.jpeg_idct(c, quant)
        assert got.shape == want.shape and np.array_equal(got, want), (name, grid, k, np.argwhere(got != want)[:4].tolist())
    got = engine.jpeg_idct(coefs[0], quant, pitch=bc * 8 + 13)   # rows of a wider array
    assert np.array_equal(got, wants[0])


def _tile_bytes(engine, handle, h, w, ch):
    cv = engine.canvas_create(h, w, ch)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, h, w, ch)
    finally:
        engine.canvas_free(cv)


def _jpeg_or_skip(engine):
    hg0 = engine.tile_reserve(8, 8)
    ok = engine.tile_fill_jpeg(hg0, 0, K.jpeg_bytes(np.zeros((8, 8), np.uint8)))
    if not ok:
        engine.tile_fill(hg0, None)
    engine.tile_free(hg0)
    if not ok:
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")


@pytest.fixture(scope="module")
def file_cases(tmp_path_factory):
    """[(name, h, w, components, bytes, Pillow's grayscale decode, Pillow's B G R decode)], decoded once for the module"""
    from imagestitch_amd import stitcher as ST
    d = tmp_path_factory.mktemp("jpegdct")
    files = [c for c in K.host_set() + K.device_extra_set()] + [(name, h, w, 3, data) for name, w, h, data in ingest_ref.jpeg_set()]
    out = []
    for name, h, w, nc, data in files:
        p = str(d / (name + ".jpg"))
        with open(p, "wb") as f:
            f.write(data)
        out.append((name, h, w, nc, data, ST._imread(p, False), ST._imread(p, True)))
    return out


def test_tile_fill_jpeg_dct_equals_the_two_decodes_and_the_host_path(engine, file_cases):
    """every file -- both tiles, the gray tile alone, the colour tile alone -- through vfsms_tile_fill_jpeg_dct: Pillow's grayscale and colour
    decodes, and the tiles vfsms_tile_fill_jpeg fills from the same bytes.  The four files of ingest_ref.jpeg_set() the path does not
    take (4 columns twice, 3 columns, 1 row) come back False with the tiles still reserved, and vfsms_tile_fill_jpeg fills them."""
    _jpeg_or_skip(engine)
    names = [c[0] for c in file_cases]
    assert "c420_2x5_q90" in names and "c420_200x328_q85" in names and len(names) == 8 + 2 + 39
    refused = []
    for name, h, w, nc, data, want_gray, want_bgr in file_cases:
        assert want_gray.shape == (h, w) and want_bgr.shape == (h, w, 3), name
        takes = nc == 1 or (w >= 5 and h >= 2)
        for which in ("both", "gray", "color"):
            tiles = {}
            for path in ("dct", "host"):
                hg = engine.tile_reserve(h, w) if which != "color" else 0
                hc = engine.tile_reserve_color(h, w, 3) if which != "gray" else 0
                try:
                    if path == "dct":
                        ok = engine.tile_fill_jpeg_dct(hg, hc, data)
                        assert ok == takes, (name, which, ok)
                        if not ok:
                            refused.append(name)
                    if path == "host" or not ok:
                        assert engine.tile_fill_jpeg(hg, hc, data), (name, which, path)
                    tiles[path] = (_tile_bytes(engine, hg, h, w, 1) if hg else None, _tile_bytes(engine, hc, h, w, 3) if hc else None)
                finally:
                    for t in (hg, hc):
                        if t:
                            engine.tile_free(t)
            for path, (gray, bgr) in tiles.items():
                if gray is not None:
                    assert np.array_equal(gray, want_gray), (name, which, path, "gray", int((gray != want_gray).sum()))
                if bgr is not None:
                    assert np.array_equal(bgr, want_bgr), (name, which, path, "colour", int((bgr != want_bgr).any(-1).sum()))
    assert set(refused) == {c[0] for c in file_cases if c[3] == 3 and (c[2] < 5 or c[1] < 2)} and len(set(refused)) == 4, sorted(set(refused))


def test_refused_files_leave_the_tiles_reserved(engine):
    """a file the path does not take: False, and the reserved tiles are still fillable -- by vfsms_tile_fill_jpeg where it takes the file"""
    from PIL import Image
    _jpeg_or_skip(engine)
    for name, h, w, data in K.refused_set():
        hg, hc = engine.tile_reserve(h, w), engine.tile_reserve_color(h, w, 3)
        try:
            assert engine.tile_fill_jpeg_dct(hg, hc, data) is False, name
            if name in ("c444", "c422", "c420_4_columns"):
                assert engine.tile_fill_jpeg(hg, hc, data), name
                im = Image.open(io.BytesIO(data)); im.draft("L", im.size)
                assert np.array_equal(_tile_bytes(engine, hg, h, w, 1), np.asarray(im.convert("L") if im.mode != "L" else im)), name
            else:
                engine.tile_fill_pair(hg, hc, None, 0, 0)
        finally:
            engine.tile_free(hg); engine.tile_free(hc)
    # a file of another size than the tiles: refused as vfsms_tile_fill_jpeg refuses it
    hg = engine.tile_reserve(40, 32)
    try:
        assert engine.tile_fill_jpeg_dct(hg, 0, K.host_set()[0][4]) is False
        engine.tile_fill(hg, None)
    finally:
        engine.tile_free(hg)


@pytest.mark.parametrize("color", (False, True), ids=("gray", "colour"))
def test_stitcher_device_decoder_equals_host_decoder(engine, tmp_path, color):
    """a 3 x 3 grid of 256 x 256 JPEG tiles on disk through imageSetStitchWithMutiple: the mosaic and the offsets under jpegDecoder =
    "device" are those under "host", and all nine tiles went through the device decoder"""
    from PIL import Image
    _jpeg_or_skip(engine)
    g = SyntheticGrid(3, 3, 256, overlap=0.25)
    proj = tmp_path / "demo"; (proj / "1").mkdir(parents=True)
    for k, t in enumerate(g.tiles(threads=2)):
        f = t.astype(np.float32)
        img = np.clip(np.stack([0.6 * f + 30, f, 255 - 0.7 * f], -1), 0, 255).astype(np.uint8) if color else t
        Image.fromarray(img).save(str(proj / "1" / ("1_%02d.jpg" % k)), quality=92)
    names = ("direction", "directIncre", "roiRatio", "isColorMode", "featureMethod", "fuseMethod", "offsetEvaluate")
    old = {n: getattr(isa.Stitcher, n) for n in names}
    runs = {}
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode = 1, 0.3, color
        isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate = "surf", "fadeInAndFadeOut", 3
        for decoder in ("host", "device"):
            st = isa.Stitcher(); st._engine = engine
            assert st.jpegDecoder == "host"
            st.jpegDecoder = decoder
            isa.Stitcher.direction = 1; st.direction = 1
            st.printAndWrite = lambda c: None
            offsets, real = [], st.getStitchByOffset

            def grab(files, offs, offsets=offsets, real=real):
                offsets.append([[int(v) for v in o] for o in offs])
                return real(files, offs)
            st.getStitchByOffset = grab
            out = tmp_path / ("out_" + decoder)
            st.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, st.calculateOffsetForFeatureSearchIncre,
                                         startNum=1, fileExtension="jpg", outputfileExtension="npy")
            runs[decoder] = (np.load(str(out / "stitching_result_1.npy")), offsets, dict(st._ingestStats))
    finally:
        for n, v in old.items():
            setattr(isa.Stitcher, n, v)
    (m_host, off_host, st_host), (m_dev, off_dev, st_dev) = runs["host"], runs["device"]
    assert off_host and len(off_host[0]) == 8 and off_dev == off_host
    assert m_host.shape == m_dev.shape and m_host.ndim == (3 if color else 2) and np.array_equal(m_dev, m_host)
    assert st_dev.get("dct") == 9 and st_dev["native"] == 9 and st_dev["tiles"] == 9
    assert "dct" not in st_host and st_host["native"] == 9
