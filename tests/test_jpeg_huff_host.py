"""The entropy decoder of Method.jpegDecoder = "device-entropy" without a GPU: its specification (tests/jpeg_huff_ref.py) against libjpeg's
coefficients and against Pillow's decode, the marker scan of the library (vfsms_jpeg_scan) against the specification's parse, the stand-alone
host program over the code the kernels run (tools/jpeg_huff_host.cpp, csrc/jpeg_huff_core.h) against the specification, and the routing of
the ingest.  tests/test_jpeg_huff_gpu.py holds the kernels to the same specification."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import _lib

import jpeg_dec_ref as R
import jpeg_huff_cases as K
import jpeg_huff_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, BAD_ARG = _lib.VFSMS_ERR_UNSUPPORTED, _lib.VFSMS_ERR_BAD_ARG


@pytest.fixture(scope="module")
def reference():
    """{name: decode()'s answer}, once for the module"""
    return {name: H.decode(data) for name, h, w, nc, data in K.taken_set()}


def _refusal(data):
    """what the specification makes of a file: None (decoded), UNSUPPORTED or BAD_ARG"""
    try:
        H.decode(data)
    except H.Unsupported:
        return UNSUPPORTED
    except H.Damaged:
        return BAD_ARG
    return None


def test_reference_equals_libjpeg_coefficients(reference):
    """the specification == vfsms_jpeg_coefficients (jpeg_read_coefficients) on every taken file: sizes, grids, tables, every coefficient"""
    if _lib.jpeg_coefficients(K.taken_set()[0][4]) is None:
        pytest.skip("no libjpeg.so.8 on this host")
    for name, h, w, nc, data in K.taken_set():
        got, want = _lib.jpeg_coefficients(data), reference[name]
        assert got is not None and got[:2] == want[:2] == (h, w) and len(got[2]) == len(want[2]) == nc, name
        for k, ((gc, gq), (wc, wq)) in enumerate(zip(got[2], want[2])):
            assert gc.shape == wc.shape and np.array_equal(gq, wq), (name, k)
            assert np.array_equal(gc, wc), (name, k, np.argwhere(gc != wc)[:4].tolist())


def test_reference_equals_pillow_decode(reference):
    """through the inverse transform of tests/jpeg_dec_ref.py the specification's coefficients are Pillow's luma plane, byte for byte"""
    from PIL import Image
    for name, h, w, nc, data in K.taken_set():
        _, _, comps = reference[name]
        info = H.parse(data)
        planes = R.decode_planes([c for c, _ in comps], [q for _, q in comps], h, w, [(c[0], c[1], c[2]) for c in info["comps"]])
        im = Image.open(io.BytesIO(data)); im.draft("L", im.size)
        assert np.array_equal(planes[0], np.asarray(im if im.mode == "L" else im.convert("L"))), name


def test_sync_rounds_of_the_cases():
    """the parallel scheme as a model: its fixed point is the sequential decode on every file, and the round counts are those
    VFSMS_JPEG_HUFF_MAX_ROUNDS was chosen from -- at least twice the largest of the files the default bound must take"""
    txt = open(os.path.join(ROOT, "include", "vfsms.h")).read()
    sub_bits = int(re.search(r"#define VFSMS_JPEG_HUFF_SUB_BITS (\d+)", txt).group(1))
    bound = int(re.search(r"#define VFSMS_JPEG_HUFF_MAX_ROUNDS (\d+)", txt).group(1))
    worst = 0
    for name, h, w, nc, data in K.taken_set():
        rounds, nsub, exact = H.sync_rounds(data, sub_bits)
        print("%s: %d rounds of %d possible" % (name, rounds, nsub - 1))
        assert exact and rounds <= max(nsub - 1, 0), name
        if name not in K.DENSE:
            worst = max(worst, rounds)
        if name == K.HEADLINE:
            assert rounds >= 1 and nsub > 1024
    assert bound >= 2 * worst, (bound, worst)
    for name in K.DENSE:                                            # practically sequential: why max_rounds exists
        data = [c[4] for c in K.taken_set() if c[0] == name][0]
        rounds, nsub, _ = H.sync_rounds(data, sub_bits)
        assert rounds >= (nsub - 1) * 3 // 4, (name, rounds, nsub)


def test_jpeg_scan_equals_the_reference_parse():
    """vfsms_jpeg_scan == parse(): header, quantisation and Huffman tables, the unstuffed bytes and the first MCU of every segment, the
    subsequences of every segment"""
    for name, h, w, nc, data in K.taken_set():
        got, want = _lib.jpeg_scan(data), H.parse(data)
        assert isinstance(got, dict), (name, got)
        assert (got["h"], got["w"], got["ncomp"]) == (h, w, nc) and got["grid6"][:2 * nc] == [v for g in want["grid"] for v in g], name
        assert (got["restart_interval"], got["nseg"], got["mcus"], got["blocks_per_mcu"]) == (want["ri"], len(want["segments"]), want["mcus"], want["blocks_per_mcu"]), name
        for k in range(nc):
            assert np.array_equal(got["quant"][k], want["quant"][k]), (name, k)
            for cls in (0, 1):
                counts, values = want["dht"][(cls, want["comps"][k][3 + cls])]
                assert got["dht"][2 * k + cls][0].tolist() == counts and got["dht"][2 * k + cls][1].tolist() == values, (name, k, cls)
        sub0 = 0
        for k, (seg, first, s0) in enumerate(got["segments"]):
            assert seg == want["segments"][k] and first == want["first_mcu"][k] and s0 == sub0, (name, k)
            n = max(1, -(-8 * len(seg) // got["sub_bits"]))
            assert got["subseg"][sub0:sub0 + n].tolist() == [k] * n, (name, k)
            sub0 += n
        assert sub0 == got["nsub"] == len(got["subseg"]) and got["total_bytes"] == len(got["record"]), name


def test_jpeg_scan_refuses_as_the_reference_does():
    """the refused set: VFSMS_ERR_UNSUPPORTED (the truncated file of the dct tests: damaged); the damaged set: VFSMS_ERR_BAD_ARG where the
    markers show it -- the XORed stream scans well, its damage is in the bits"""
    for name, _h, _w, data in K.refused_set():
        want = _refusal(data)
        assert want == (BAD_ARG if name == "truncated" else UNSUPPORTED), (name, want)
        assert _lib.jpeg_scan(data) == want, name
    for name, _h, _w, data in K.damaged_set():
        assert _refusal(data) == BAD_ARG, name
        got = _lib.jpeg_scan(data)
        assert isinstance(got, dict) if name.startswith("xor") else got == BAD_ARG, (name, got)
    assert _lib.jpeg_scan(b"not a jpeg") == UNSUPPORTED and _lib.jpeg_scan(b"\xff\xd8\xff\xd9") == BAD_ARG


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tools/jpeg_huff_host.cpp with csrc/jpeg_host.cpp, the plain build"""
    exe = str(tmp_path_factory.mktemp("jpeghuff") / "jpeg_huff_host")
    csrc = os.path.join(ROOT, "imagestitch_amd", "csrc")
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tools", "jpeg_huff_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"), "-ldl", "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=600)
    return exe


def _run_program(exe, tmp_path, data, *args):
    src, out = str(tmp_path / "in.jpg"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(data)
    if os.path.exists(out):
        os.remove(out)
    p = subprocess.run([exe, src, out] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), p.stdout + p.stderr
    rc = int(re.match(r"rc=(-?\d+)", p.stdout).group(1))
    m = re.search(r"rounds=(\d+)", p.stdout)
    return rc, (open(out, "rb").read() if os.path.exists(out) else None), (int(m.group(1)) if m else None)


def test_host_program_equals_the_reference(host_program, reference, tmp_path):
    """the rounds of the device, run serially over csrc/jpeg_huff_core.h: the reference's bytes on every taken file at max_rounds = -1 (the
    dense files included), the model's round count, a refusal where the rounds are not allowed, and a refusal of every damaged file"""
    for name, h, w, nc, data in K.taken_set():
        rc, got, rounds = _run_program(host_program, tmp_path, data, -1)
        assert rc == 0 and got == H.layout_bytes(reference[name]), name
        assert rounds == H.sync_rounds(data, 1024)[0], name
    head = [c[4] for c in K.taken_set() if c[0] == K.HEADLINE][0]
    assert _run_program(host_program, tmp_path, head, 0)[:2] == (UNSUPPORTED, None)
    rc, got, rounds = _run_program(host_program, tmp_path, head, -1, 256)           # another subsequence size, the same answer
    assert rc == 0 and got == H.layout_bytes(reference[K.HEADLINE]) and rounds == H.sync_rounds(head, 256)[0]
    for name, _h, _w, data in K.damaged_set():
        assert _run_program(host_program, tmp_path, data, -1)[:2] == (BAD_ARG, None), name
    for name, _h, _w, data in K.refused_set():
        assert _run_program(host_program, tmp_path, data, -1)[:2] == (_refusal(data), None), name


# ---- routing ----------------------------------------------------------------------------------------------------------------------------------
def _recording_engine(oracle, with_huff=True):
    from fakes import NativeJpegEngine

    class Recording(NativeJpegEngine):
        """NativeJpegEngine that writes down which entry saw which file (by size); its device decoders take what the library's host halves
        take and fill the tiles with the bytes the host decoder yields -- the same bytes, by tests/test_jpeg_huff_gpu.py"""

        def __init__(self, oracle):
            super().__init__(oracle)
            self.huff_seen, self.huff_took, self.dct_seen, self.dct_took, self.jpeg_seen = [], [], [], [], []

        def tile_fill_jpeg(self, gray, color, data):
            self.jpeg_seen.append(len(data))
            return super().tile_fill_jpeg(gray, color, data)

        def _device(self, seen, took, takes, gray, color, data):
            seen.append(len(data))
            if not takes:
                return False
            assert NativeJpegEngine.tile_fill_jpeg(self, gray, color, data)
            self.native.pop()
            took.append(len(data))
            return True

        def tile_fill_jpeg_dct(self, gray, color, data):
            return self._device(self.dct_seen, self.dct_took, _lib.jpeg_coefficients(data) is not None, gray, color, data)

    if with_huff:
        def tile_fill_jpeg_huff(self, gray, color, data):
            return self._device(self.huff_seen, self.huff_took, isinstance(_lib.jpeg_scan(data), dict), gray, color, data)
        Recording.tile_fill_jpeg_huff = tile_fill_jpeg_huff
    return Recording(oracle)


def test_routing_of_device_entropy(oracle, tmp_path):
    """jpegDecoder "device-entropy": tile_fill_jpeg_huff sees every JPEG once; a file it refuses (progressive) goes on to tile_fill_jpeg_dct,
    one both refuse (4:4:4) to tile_fill_jpeg, one all refuse (CMYK) to `_decode_once`, each once.  "host" and "device" never call the new
    entry.  An engine without it: NotImplementedError before anything is reserved; "gpu" is still no decoder."""
    from PIL import Image
    from imagestitch_amd.synthetic import SyntheticGrid
    from imagestitch_amd import stitcher as ST
    if _lib.jpeg_decode(K.taken_set()[0][4], False) is None:
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")
    assert isa.Stitcher.jpegDecoder == "host"
    g = SyntheticGrid(2, 2, 256, overlap=0.25)
    files = []
    for k, t in enumerate(g.tiles(threads=1)):
        p = os.path.join(str(tmp_path), "t_%02d.jpg" % k)
        rgb = np.stack([t, t, t], -1)
        if k == 1:
            Image.fromarray(t).save(p, quality=91, progressive=True)            # progressive: the dct path's
        elif k == 2:
            Image.fromarray(rgb).save(p, quality=93, subsampling=0)             # 4:4:4: the host decoder's
        elif k == 3:
            Image.fromarray(rgb).convert("CMYK").save(p, quality=94)            # CMYK: Pillow's
        else:
            Image.fromarray(t).save(p, quality=92)
        files.append(p)
    sizes = [os.path.getsize(p) for p in files]
    assert len(set(sizes)) == 4
    counts = {"once": []}
    real_once = ST._decode_once

    def once(path, color):
        counts["once"].append(os.path.getsize(path))
        return real_once(path, color)
    names = ("direction", "directIncre", "roiRatio", "isColorMode", "featureMethod", "fuseMethod")
    old = {n: getattr(isa.Stitcher, n) for n in names}
    env_old = os.environ.pop("VFSMS_NATIVE_JPEG", None)
    ST._decode_once = once
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod = 1, 0.3, "surf", "fadeInAndFadeOut"
        isa.Stitcher.isColorMode = False
        mosaics = {}
        for decoder in ("device-entropy", "device", "host"):
            eng = _recording_engine(oracle)
            s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.direction = 1
            s.jpegDecoder = decoder
            counts["once"] = []
            (status, mosaics[decoder]) = s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)
            assert status == (True, 3) and not eng.live
            assert counts["once"] == [sizes[3]] and s._ingestStats["native"] == 3 and s._ingestStats["tiles"] == 4
            if decoder == "device-entropy":
                assert sorted(eng.huff_seen) == sorted(sizes) and eng.huff_took == [sizes[0]]
                assert sorted(eng.dct_seen) == sorted(sizes[1:]) and eng.dct_took == [sizes[1]]
                assert sorted(eng.jpeg_seen) == sorted(sizes[2:]) and eng.native == [sizes[2]]
                assert s._ingestStats["huff"] == 1 and s._ingestStats["dct"] == 1
            else:
                assert eng.huff_seen == [] and "huff" not in s._ingestStats
                assert sorted(eng.dct_seen) == (sorted(sizes) if decoder == "device" else [])
        assert np.array_equal(mosaics["device-entropy"], mosaics["host"]) and np.array_equal(mosaics["device"], mosaics["host"])
        s = isa.Stitcher(); s._engine = _recording_engine(oracle, with_huff=False); s.isPrintLog = False; s.direction = 1; s.jpegDecoder = "device-entropy"
        with pytest.raises(NotImplementedError):
            s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)
        assert not s._engine.live and s._engine.dct_seen == [] and s._engine.jpeg_seen == []
        s.jpegDecoder = "gpu"
        with pytest.raises(ValueError):
            s.flowStitch(list(files), s.calculateOffsetForFeatureSearchIncre)
    finally:
        ST._decode_once = real_once
        if env_old is not None:
            os.environ["VFSMS_NATIVE_JPEG"] = env_old
        for n, v in old.items():
            setattr(isa.Stitcher, n, v)
