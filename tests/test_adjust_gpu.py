"""GPU tests of the global placement (Method.globalAdjust = "ncc"): vfsms_ncc_search_batch equals tests/ncc_search_ref.py bit for bit
(surface and best4) at every path the kernel has -- interior and edge chunks, rows that are no multiple of 16 bytes, negative offsets,
windows that leave the tile, more than one tile of column shifts, sums beyond 32 bits --, GridRegistrar.adjust recovers the true offsets of
a resident grid, and the Stitcher switch turns a wrong path offset into the mosaic of the true ones."""
import functools
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.grid import GridRegistrar
import adjust_cases as AC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (A, B, dx, dy, radius, min_pixels); the specification's answer is computed once per case (expected)"""
    tiles, true = AC.grid("g7")
    P = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(np.array(AC.perturbed(true), np.int64), axis=0)])
    out = {}
    for a, b in AC.EDGES_3X3:                                 # the 12 edges, centred up to 3 px off the truth; w = 200
        out["edge_%d_%d" % (a, b)] = (tiles[a], tiles[b], int(P[b][0] - P[a][0]), int(P[b][1] - P[a][1]), 4, AC.MIN_PIXELS)
    out["radius_1"] = (tiles[0], tiles[1], true[0][0] + 1, true[0][1] - 1, 1, AC.MIN_PIXELS)
    out["radius_16"] = (tiles[0], tiles[5], 3, 150 + 9, 16, AC.MIN_PIXELS)      # four tiles of column shifts, the last one partial
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (200, 420), dtype=np.uint8)
    A203, B203 = np.ascontiguousarray(base[60:157, 150:353]), np.ascontiguousarray(base[1:98, 2:205])   # B's pixel meets A's at (-59, -148)
    out["w203_negative"] = (A203, B203, -60, -150, 4, 0)
    out["w200_negative"] = (tiles[1], tiles[0], -true[0][0] + 2, -true[0][1] - 3, 4, AC.MIN_PIXELS)
    out["window_leaves_the_tile"] = (tiles[0], tiles[1], 160 - 2, 1, 4, 350)    # rows: none to 6 shared; 350 > one row of 200 - |dy + j|
    out["corner_sliver"] = (A203, B203, 95, 200, 4, 0)                           # a few pixels in a corner, most candidates empty
    flat = np.full((50, 70), 17, np.uint8)
    out["flat"] = (flat, flat, 5, -6, 4, 0)
    full = np.full((320, 320), 255, np.uint8)
    out["saturated_320"] = (full, full, 0, 0, 4, 0)                              # Saa = 320 * 320 * 255^2 > 2^32
    sat = rng.integers(250, 256, (320, 320), dtype=np.uint8)
    out["bright_320"] = (sat, np.ascontiguousarray(np.roll(sat, (-1, 2), (0, 1))), 1, -2, 4, 0)   # the same size of sums, not flat
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    A, B, dx, dy, R, mp = cases()[name]
    return AC.spec_rows(A, B, dx, dy, R, mp)


def run(engine, names, radius, min_pixels):
    hs, jobs = [], []
    try:
        for n in names:
            A, B, dx, dy, _R, _mp = cases()[n]
            ha, hb = engine.tile_upload(A), engine.tile_upload(B)
            hs += [ha, hb]
            jobs.append((ha, hb, dx, dy))
        return engine.ncc_search_batch(jobs, radius, min_pixels, want_surface=True)
    finally:
        for h in hs:
            engine.tile_free(h)


def check(names, best, surface):
    for k, n in enumerate(names):
        row, surf = expected(n)
        assert np.array_equal(surface[k], surf), n
        assert best[k].tolist() == row, (n, best[k].tolist(), row)


def test_the_twelve_edges_of_the_grid_in_one_batch(engine):
    names = ["edge_%d_%d" % e for e in AC.EDGES_3X3]
    best, surface = run(engine, names, 4, AC.MIN_PIXELS)
    check(names, best, surface)
    tiles, true = AC.grid("g7")
    P = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(np.array(true, np.int64), axis=0)])
    for k, n in enumerate(names):                            # and the peaks are the truth
        _A, _B, dx, dy, _R, _mp = cases()[n]
        a, b = AC.EDGES_3X3[k]
        assert [dx + best[k, 0], dy + best[k, 1]] == (P[b] - P[a]).tolist()


@pytest.mark.parametrize("name", ["radius_1", "radius_16", "w203_negative", "w200_negative", "window_leaves_the_tile", "corner_sliver", "flat",
                                  "saturated_320", "bright_320"])
def test_single_jobs_equal_the_specification(engine, name):
    _A, _B, _dx, _dy, R, mp = cases()[name]
    best, surface = run(engine, [name], R, mp)
    check([name], best, surface)
    if name == "flat" or name == "saturated_320":
        assert best[0, :3].tolist() == [0, 0, 0] and not surface.any()
    if name == "w203_negative":
        assert best[0, :2].tolist() == [1, 2] and best[0, 2] == isa.Engine.VERIFY_FIXED_ONE
    if name == "window_leaves_the_tile":
        assert (surface[0] == 0).sum() == 4 * 9              # i >= 1 shares at most one row of <= 200 pixels: below min_pixels or empty


def test_a_batch_that_mixes_every_kind_of_job(engine):
    """jobs of different tile shapes in one call; radius 4 and min_pixels 0 for all (the cases' own centres)"""
    names = ["edge_0_5", "w203_negative", "flat", "corner_sliver", "saturated_320", "edge_3_4", "window_leaves_the_tile", "bright_320", "w200_negative"]
    hs, jobs, want = [], [], []
    for n in names:
        A, B, dx, dy, _R, _mp = cases()[n]
        want.append(AC.spec_rows(A, B, dx, dy, 4, 0) if cases()[n][5] != 0 else expected(n))
    best, surface = run(engine, names, 4, 0)
    for k, n in enumerate(names):
        assert np.array_equal(surface[k], want[k][1]), n
        assert best[k].tolist() == want[k][0], n
    best_only = run(engine, names[:3], 4, 0)[0]
    assert np.array_equal(best_only, best[:3])


def test_ncc_search_uploads_two_host_arrays(engine):
    A, B, dx, dy, R, mp = cases()["w203_negative"]
    (i, j), fx, n, surface = engine.ncc_search(A, B, dx, dy, R, mp)
    row, surf = expected("w203_negative")
    assert [i, j, fx, n] == row and np.array_equal(surface, surf)


def test_bad_arguments(engine):
    tiles, _true = AC.grid("g7")
    ha, hb, hc = engine.tile_upload(tiles[0]), engine.tile_upload(tiles[1]), engine.tile_upload(np.zeros((160, 208), np.uint8))
    hcol = engine.tile_upload_color(np.zeros((160, 200, 3), np.uint8))
    try:
        assert engine.ncc_search_batch([], 4, 0).shape == (0, 4)
        for jobs, R in (([(ha, hc, 0, 0)], 4), ([(ha, hb, 0, 0)], 0), ([(ha, hb, 0, 0)], 17), ([(ha, hcol, 0, 0)], 4), ([(ha, 10 ** 9, 0, 0)], 4)):
            with pytest.raises(isa.VfsmsError, match="error -1"):
                engine.ncc_search_batch(jobs, R, 0)
        assert engine.ncc_search_batch([(ha, hb, 120, 0)], 16, 0).shape == (1, 4)      # the engine is fine afterwards
    finally:
        for h in (ha, hb, hc, hcol):
            engine.tile_free(h)


def test_grid_registrar_adjust_recovers_the_truth(engine):
    tiles, true = AC.grid("g7")
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        reg = GridRegistrar(engine)
        got, report = reg.adjust(hs, [t.shape for t in tiles], AC.perturbed(true), radius=AC.RADIUS, threshold=0.5, min_pixels=AC.MIN_PIXELS)
        assert got == true
        assert report["edges"] == 12 and report["measured"] == 12 and report["dropped"] == 0
        table = np.array([[1, dx, dy, 1, 1, 9] for dx, dy in AC.perturbed(true)], np.int32)          # register()'s table works as well
        assert reg.adjust(hs, [t.shape for t in tiles], table, radius=AC.RADIUS, min_pixels=AC.MIN_PIXELS)[0] == true
        with engine_profile(engine) as prof:
            reg.adjust(hs, [t.shape for t in tiles], true, radius=AC.RADIUS, min_pixels=AC.MIN_PIXELS)
        assert prof()["adjust"][1] == 1                      # one launch group under the profile stage "adjust"
    finally:
        for h in hs:
            engine.tile_free(h)


class engine_profile:
    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        self.engine.profile_enable(True)
        self.engine.profile_read(reset=True)
        return lambda: self.stages

    def __exit__(self, *exc):
        self.stages = self.engine.profile_read(reset=True)
        self.engine.profile_enable(False)


class ScriptedStitcher(isa.Stitcher):
    """a Stitcher whose registration method answers from a list of path offsets (a custom method: flowStitch runs pair by pair)"""

    def __init__(self, offsets):
        super().__init__()
        self.script, self.k, self.lines = [list(o) for o in offsets], 0, []
        self.isPrintLog = False
        self.isColorMode = False

    def printAndWrite(self, content):
        self.lines.append(content)

    def scripted(self, images):
        self.k += 1
        return True, list(self.script[self.k - 1])


def test_stitcher_switch_turns_a_wrong_vote_into_the_true_mosaic(engine, tmp_path):
    from PIL import Image
    tiles, true = AC.grid("g7")
    files = []
    for k, t in enumerate(tiles):
        files.append(os.path.join(str(tmp_path), "t%02d.png" % k))
        Image.fromarray(t).save(files[-1])
    wrong = AC.perturbed(true, {4: (2, 0)})                  # one pair wrong by 2 px: every later tile sits 2 rows off

    def mosaic(offsets, switch):
        st = ScriptedStitcher(offsets)
        st._engine = engine
        st.globalAdjust, st.adjustMinPixels = switch, AC.MIN_PIXELS
        (status, _end), img = st.flowStitch(list(files), st.scripted)
        assert status
        return st, np.asarray(img)
    ref_st, ref = mosaic(true, "none")
    st, got = mosaic(wrong, "ncc")
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert "  The adjusted offsetList is " + str(true) in st.lines
    assert st.adjustReport["measured"] == 12
    # "none": no new code runs -- no search, no new log line, the mosaic of the offsets as voted
    class NoSearch:
        def __getattr__(self, name):
            if name == "ncc_search_batch":
                raise AssertionError("globalAdjust = 'none' must not search")
            return getattr(engine, name)
    off = ScriptedStitcher(wrong)
    off._engine = NoSearch()
    (status, _end), plain = off.flowStitch(list(files), off.scripted)
    assert status and not any("adjusted" in ln for ln in off.lines) and len(off.lines) == len(ref_st.lines)
    assert [ln for ln in off.lines if "offsetList" in ln and "rectified" not in ln] == []
    direct = ScriptedStitcher(wrong)
    direct._engine = engine
    assert np.array_equal(np.asarray(plain), np.asarray(direct.getStitchByOffset(list(files), [list(o) for o in wrong])))
