"""The device entropy decoder (csrc/jpeg_huff_kernels.hip; Method.jpegDecoder = "device-entropy") against its specification,
tests/jpeg_huff_ref.py, byte for byte: the bare operator on every file of tests/jpeg_huff_cases.py, the round bounds, the damaged files,
vfsms_tile_fill_jpeg_huff against vfsms_tile_fill_jpeg and Pillow's two decodes, and the Stitcher with the switch on against the Stitcher
with it off.  tests/test_jpeg_huff_host.py holds the specification itself to libjpeg and Pillow, and the same decoder code on the host."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import _lib
from imagestitch_amd.synthetic import SyntheticGrid

import jpeg_huff_cases as K
import jpeg_huff_ref as H

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, BAD_ARG = _lib.VFSMS_OK, _lib.VFSMS_ERR_UNSUPPORTED, _lib.VFSMS_ERR_BAD_ARG
ONE_SUBSEQUENCE = ("c420_2x5_q90", "flat_8x8", "flat_64x96")


@pytest.fixture(scope="module")
def reference():
    """{name: decode()'s answer}, once for the module"""
    return {name: H.decode(data) for name, h, w, nc, data in K.taken_set()}


def _same(got, want):
    return len(got) == len(want) and all(gc.shape == wc.shape and np.array_equal(gc, wc) and np.array_equal(gq, wq) for (gc, gq), (wc, wq) in zip(got, want))


def test_operator_equals_the_reference(engine, reference):
    """jpeg_entropy_decode(max_rounds = -1) == the sequential decode of the specification on every taken file, the two dense files included;
    the headline file needs repair rounds, so nothing here passes without them"""
    for name, h, w, nc, data in K.taken_set():
        rc, gh, gw, comps, rounds = engine.jpeg_entropy_decode(data, -1)
        assert rc == OK and (gh, gw) == (h, w), (name, rc)
        print("%s: %d rounds" % (name, rounds))
        assert _same(comps, reference[name][2]), name
        if name == K.HEADLINE:
            assert rounds >= 1
        if name in ONE_SUBSEQUENCE:
            assert rounds == 0


def test_operator_without_repair_rounds(engine, reference):
    """max_rounds = 0: the headline file is handed back, the files of one subsequence come back exact"""
    head = [c[4] for c in K.taken_set() if c[0] == K.HEADLINE][0]
    assert engine.jpeg_entropy_decode(head, 0)[0] == UNSUPPORTED
    for name, h, w, nc, data in K.taken_set():
        if name in ONE_SUBSEQUENCE:
            rc, _, _, comps, rounds = engine.jpeg_entropy_decode(data, 0)
            assert rc == OK and rounds == 0 and _same(comps, reference[name][2]), name


def test_default_round_bound_takes_every_texture_and_restart_file(engine, reference):
    """VFSMS_JPEG_HUFF_MAX_ROUNDS: every file but the two dense ones is taken; a dense file may go either way, exact if taken"""
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vfsms.h")).read()
    bound = int(re.search(r"#define VFSMS_JPEG_HUFF_MAX_ROUNDS (\d+)", txt).group(1))
    for name, h, w, nc, data in K.taken_set():
        rc, _, _, comps, rounds = engine.jpeg_entropy_decode(data, bound)
        if name in K.DENSE:
            assert rc in (OK, UNSUPPORTED), (name, rc)
        else:
            assert rc == OK, (name, rc)
        if rc == OK:
            assert rounds <= bound and _same(comps, reference[name][2]), name


def _tile_bytes(engine, handle, h, w, ch):
    cv = engine.canvas_create(h, w, ch)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, h, w, ch)
    finally:
        engine.canvas_free(cv)


def _jpeg_or_skip(engine):
    hg0 = engine.tile_reserve(8, 8)
    ok = engine.tile_fill_jpeg(hg0, 0, K.D.jpeg_bytes(np.zeros((8, 8), np.uint8)))
    if not ok:
        engine.tile_fill(hg0, None)
    engine.tile_free(hg0)
    if not ok:
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")


def test_damaged_files_are_refused_and_leave_the_tiles_reserved(engine):
    """every damaged file: the operator and the fill return the refusal, never a decode; the tiles are still reserved and tile_fill_jpeg
    then fills or refuses them as it does today.  (The same files went through the same decoder code on the host, under sanitizers, first.)"""
    _jpeg_or_skip(engine)
    for name, h, w, data in K.damaged_set():
        assert engine.jpeg_entropy_decode(data, -1)[0] == BAD_ARG, name
        hg, hc = engine.tile_reserve(h, w), engine.tile_reserve_color(h, w, 3)
        try:
            assert engine.tile_fill_jpeg_huff(hg, hc, data) is False, name
            if not engine.tile_fill_jpeg(hg, hc, data):                 # (libjpeg takes a corrupt stream with warnings, or not: its business)
                engine.tile_fill_pair(hg, hc, None, 0, 0)
        finally:
            engine.tile_free(hg); engine.tile_free(hc)


@pytest.fixture(scope="module")
def file_cases(tmp_path_factory):
    """[(name, h, w, components, bytes, Pillow's grayscale decode, Pillow's B G R decode)], decoded once for the module"""
    from imagestitch_amd import stitcher as ST
    d = tmp_path_factory.mktemp("jpeghuff")
    out = []
    for name, h, w, nc, data in K.taken_set():
        p = str(d / (name + ".jpg"))
        with open(p, "wb") as f:
            f.write(data)
        out.append((name, h, w, nc, data, ST._imread(p, False), ST._imread(p, True)))
    return out


def test_tile_fill_jpeg_huff_equals_the_two_decodes_and_the_host_path(engine, file_cases):
    """every taken file -- both tiles, the gray tile alone, the colour tile alone -- through vfsms_tile_fill_jpeg_huff: Pillow's grayscale and
    colour decodes, and the tiles vfsms_tile_fill_jpeg fills from the same bytes.  A dense file the default round bound hands back comes back
    False with the tiles still reserved, and vfsms_tile_fill_jpeg fills them."""
    _jpeg_or_skip(engine)
    for name, h, w, nc, data, want_gray, want_bgr in file_cases:
        for which in ("both", "gray", "color"):
            tiles = {}
            for path in ("huff", "host"):
                hg = engine.tile_reserve(h, w) if which != "color" else 0
                hc = engine.tile_reserve_color(h, w, 3) if which != "gray" else 0
                try:
                    ok = True
                    if path == "huff":
                        ok = engine.tile_fill_jpeg_huff(hg, hc, data)
                        assert ok or name in K.DENSE, (name, which)
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


def test_refused_files_leave_the_tiles_reserved(engine):
    """a file the path does not take: False, and the reserved tiles are still fillable"""
    _jpeg_or_skip(engine)
    for name, h, w, data in K.refused_set():
        assert engine.jpeg_entropy_decode(data, -1)[0] in (UNSUPPORTED, BAD_ARG), name
        hg, hc = engine.tile_reserve(h, w), engine.tile_reserve_color(h, w, 3)
        try:
            assert engine.tile_fill_jpeg_huff(hg, hc, data) is False, name
            if not engine.tile_fill_jpeg(hg, hc, data):
                engine.tile_fill_pair(hg, hc, None, 0, 0)
        finally:
            engine.tile_free(hg); engine.tile_free(hc)
    hg = engine.tile_reserve(40, 32)                                 # a file of another size than the tiles
    try:
        assert engine.tile_fill_jpeg_huff(hg, 0, K.taken_set()[0][4]) is False
        engine.tile_fill(hg, None)
    finally:
        engine.tile_free(hg)


@pytest.mark.parametrize("color", (False, True), ids=("gray", "colour"))
def test_stitcher_device_entropy_equals_host_decoder(engine, tmp_path, color):
    """a 3 x 3 grid of 256 x 256 JPEG tiles on disk through imageSetStitchWithMutiple: the mosaic and the offsets under jpegDecoder =
    "device-entropy" are those under "host", and all nine tiles went through the entropy decoder of the device"""
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
        for decoder in ("host", "device-entropy"):
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
    (m_host, off_host, st_host), (m_dev, off_dev, st_dev) = runs["host"], runs["device-entropy"]
    assert off_host and len(off_host[0]) == 8 and off_dev == off_host
    assert m_host.shape == m_dev.shape and m_host.ndim == (3 if color else 2) and np.array_equal(m_dev, m_host)
    assert st_dev.get("huff") == 9 and st_dev["native"] == 9 and st_dev["tiles"] == 9 and "dct" not in st_dev
    assert "huff" not in st_host and st_host["native"] == 9
