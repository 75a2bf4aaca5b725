"""CPU tests of Method.shadingCorrection: the specification tests/shading_ref.py against Python-loop restatements of its steps, the
measurement that the correction removes a known vignette, and the defaults / refusals of Method and Stitcher on the CPU test doubles."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from fakes import OracleEngine

import shading_ref as SH


# ---- 1. the reference against brute force -----------------------------------------------------------------------------------------
def _brute_profile(T, percentile):
    n = len(T)
    k = (n - 1) * percentile // 100
    out = np.zeros(T[0].shape, np.uint8)
    for idx in np.ndindex(*T[0].shape):
        out[idx] = sorted(int(t[idx]) for t in T)[k]
    return out


def _brute_box(Q, R):
    h, w, ch = Q.shape
    area = (2 * R + 1) ** 2
    out = np.zeros(Q.shape, np.uint16)
    for y in range(h):
        for x in range(w):
            for c in range(ch):
                s = 0
                for dy in range(-R, R + 1):
                    yy = min(max(y + dy, 0), h - 1)
                    for dx in range(-R, R + 1):
                        s += int(Q[yy, min(max(x + dx, 0), w - 1), c])
                assert s + area // 2 < 2 ** 32
                out[y, x, c] = (s + area // 2) // area
    return out


def _brute_gain(Q):
    h, w, ch = Q.shape
    G = np.zeros(Q.shape, np.uint16)
    for c in range(ch):
        m = (sum(int(v) for v in Q[:, :, c].ravel()) + h * w // 2) // (h * w)
        for y in range(h):
            for x in range(w):
                q = int(Q[y, x, c])
                G[y, x, c] = min(65535, (m * 4096 + q // 2) // q) if q > 0 else 4096
    return G


@pytest.mark.parametrize("shape", [(5, 7, 1), (6, 9, 3)])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_reference_steps_equal_their_loop_restatements(shape, n):
    rng = np.random.default_rng(100 * n + shape[2])
    T = [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(n)]
    T[0][0, :3] = 0                                           # ties and a zero corner
    if n > 1:
        T[1][0, :3] = 0
    for pct in (0, 37, 50, 100):
        P = SH.profile(T, pct)
        assert P.dtype == np.uint8 and np.array_equal(P, _brute_profile(T, pct)), pct
        if shape[2] == 1:                                     # 2-D tiles are the same samples
            assert np.array_equal(SH.profile([t[..., 0] for t in T], pct), P[..., 0])
    P = SH.profile(T, 50)
    Q0 = P.astype(np.uint16) << 8
    for R in (1, 3, 12):                                      # 12 exceeds both dimensions
        Q1 = SH.box_pass(Q0, R)
        assert Q1.dtype == np.uint16 and np.array_equal(Q1, _brute_box(Q0, R)), R
        Q2 = SH.smooth(P, R)
        assert np.array_equal(Q2, _brute_box(Q1, R)), R       # two passes, each rounded once
        G = SH.gain(Q2)
        assert G.dtype == np.uint16 and np.array_equal(G, _brute_gain(Q2)), R
        for t in T:
            want = np.array([min(255, (int(p) * int(g) + 2048) >> 12) for p, g in zip(t.ravel(), G.ravel())], np.uint8).reshape(shape)
            assert np.array_equal(SH.apply(t, G), want)
    Qz = np.zeros(shape, np.uint16); Qz[2:, 3:] = 7 << 8
    assert np.array_equal(SH.gain(Qz), _brute_gain(Qz)) and (SH.gain(Qz)[0, 0] == 4096).all()
    Qs = np.full(shape, 255 << 8, np.uint16); Qs[1, 1] = 256
    assert SH.gain(Qs)[1, 1].max() == 65535 and np.array_equal(SH.gain(Qs), _brute_gain(Qs))
    for bad in (lambda: SH.profile(T, 101), lambda: SH.profile(T, -1), lambda: SH.smooth(P, 0), lambda: SH.smooth(P, 128), lambda: SH.profile([], 50)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. the correction does what it is for ----------------------------------------------------------------------------------------
def vignette(h, w, corner=0.65):
    """radial fall-off from 1 at the centre to `corner` at the corners"""
    y, x = np.mgrid[0:h, 0:w]
    r2 = ((y - (h - 1) / 2) ** 2 + (x - (w - 1) / 2) ** 2) / (((h - 1) / 2) ** 2 + ((w - 1) / 2) ** 2)
    return 1.0 - (1.0 - corner) * r2


def vignetted_stack(n=30, size=256, seed=7, grain=40, sigma=2.0):
    """n tiles of size^2: a smooth texture of about `grain` px (a coarse random lattice, bilinearly interpolated) around 150, darkened by
    one common vignette, plus noise of `sigma`"""
    rng = np.random.default_rng(seed)
    V = vignette(size, size)
    m = size // grain + 2
    pos = np.arange(size) / grain
    i0 = pos.astype(int); f = pos - i0
    tiles = []
    for _ in range(n):
        L = rng.uniform(-1, 1, (m, m))
        rows = L[i0] * (1 - f)[:, None] + L[i0 + 1] * f[:, None]
        tex = rows[:, i0] * (1 - f)[None, :] + rows[:, i0 + 1] * f[None, :]
        t = V * (150.0 + 60.0 * tex) + rng.normal(0, sigma, (size, size))
        tiles.append(np.clip(np.rint(t), 0, 255).astype(np.uint8))
    return tiles, V


def residual(G, V):
    f = G.astype(np.float64) / 4096.0 * V
    return float(np.abs(f / f.mean() - 1).max())


# measured with the reference alone on vignetted_stack(): uncorrected max |V / mean(V) - 1| = 0.2634; after the correction
# max |G V / mean(G V) - 1| = 0.1155 (R = 8), 0.1044 (R = 16), 0.1306 (R = 32).  Each bound is halfway between its figure and 0.2634.
MEASURED = {8: 0.1155, 16: 0.1044, 32: 0.1306}
UNCORRECTED = 0.2634


def test_the_correction_removes_a_known_vignette():
    """30 tiles of 256^2 under a radial vignette down to 0.65 at the corners (percentile 50): the residual shading of the corrected tiles,
    dev = max |G V / mean(G V) - 1|, measured 0.1155 / 0.1044 / 0.1306 for R = 8 / 16 / 32 against 0.2634 uncorrected; asserted below
    the midpoint of the two"""
    tiles, V = vignetted_stack()
    raw = float(np.abs(V / V.mean() - 1).max())
    print("uncorrected %.4f" % raw)
    assert abs(raw - UNCORRECTED) < 5e-4
    P = SH.profile(tiles, 50)
    for R, measured in MEASURED.items():
        dev = residual(SH.gain(SH.smooth(P, R)), V)
        print("R = %d: dev %.4f" % (R, dev))
        assert dev < (measured + UNCORRECTED) / 2, (R, dev)


# ---- 3. defaults and refusals -----------------------------------------------------------------------------------------------------
def test_method_defaults():
    m = isa.Method
    assert (m.shadingCorrection, m.shadingPercentile, m.shadingRadius, m.shadingMinTiles, m.shadingGain) == ("none", 50, 32, 8, None)


def _mosaic(oracle, tmp_path, correction, tag):
    from test_host_logic import _write_tiles
    rng = np.random.default_rng(3)
    scene = rng.integers(0, 256, (40, 100)).astype(np.uint8)
    tiles = [np.ascontiguousarray(scene[:, x:x + 40]) for x in (0, 30, 60)]
    files = _write_tiles(tmp_path, tiles, tag)
    s = isa.Stitcher(); s._engine = OracleEngine(oracle); s.isPrintLog = False; s.isColorMode = False
    s.fuseMethod = "fadeInAndFadeOut"
    if correction is not None:
        s.shadingCorrection = correction
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = False
        return s.getStitchByOffset(files, [[0, 30], [0, 30]])
    finally:
        isa.Stitcher.isColorMode = old


def test_stitcher_on_the_cpu_doubles(oracle, tmp_path):
    """an engine without shading_estimate refuses "estimate"; "none" is today's mosaic, byte for byte"""
    with pytest.raises(NotImplementedError):
        _mosaic(oracle, tmp_path, "estimate", "e")
    with pytest.raises(ValueError):
        _mosaic(oracle, tmp_path, "median", "m")
    today = _mosaic(oracle, tmp_path, None, "t")
    assert np.array_equal(_mosaic(oracle, tmp_path, "none", "n"), today)
    assert today.shape == (40, 100) and today.any()


def test_none_keeps_the_golden_mosaics(golden_dir, oracle, tmp_path):
    """the reference's own mosaics (tests/golden/stitch_cases.npz) with shadingCorrection spelled out as "none\""""
    from test_host_logic import _write_tiles, FUSE_NAMES
    g = np.load(os.path.join(golden_dir, "stitch_cases.npz"))
    old = isa.Stitcher.isColorMode
    try:
        for n, (color, fm, _) in enumerate(g["meta"]):
            files = _write_tiles(tmp_path, list(g["s%d_tiles" % n]), "g%d" % n)
            s = isa.Stitcher(); s._engine = OracleEngine(oracle); s.isPrintLog = False
            s.isColorMode = bool(color); isa.Stitcher.isColorMode = bool(color)
            s.fuseMethod = FUSE_NAMES[fm]; s.shadingCorrection = "none"
            res = s.getStitchByOffset(files, [list(map(int, o)) for o in g["s%d_offsets" % n]])
            assert np.array_equal(res, g["s%d_out" % n]), (n, FUSE_NAMES[fm])
    finally:
        isa.Stitcher.isColorMode = old
