"""GPU tests of Method.failedPairRepair = "stage": vfsms_ncc_wide_batch equals tests/ncc_wide_ref.py bit for bit -- the reduced planes, out8 and
the seed tables, at every path the kernels have --, vfsms_overlap_sums_batch equals verify_ref.sums, GridRegistrar.repair equals
tests/stage_ref.py on a resident grid, and the Stitcher switch keeps one mosaic where a failed pair cut it in two."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.grid import GridRegistrar, split_segments
import adjust_cases as AC
import ncc_wide_ref as W
import stage_cases as SC
import verify_ref

pytestmark = pytest.mark.gpu
FX = verify_ref.FIXED_ONE


def _hip():
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln.split()[-1]]
    return C.CDLL(loaded[0] if loaded else "libamdhip64.so")            # the HIP runtime the library itself runs on


@contextlib.contextmanager
def wrapped(engine, arr, stride, lead):
    """`arr` in device memory with rows `stride` bytes apart, `lead` bytes behind an allocation's start, as a tile of vfsms_tile_wrap"""
    hip = _hip()
    h, w = arr.shape
    padded = np.zeros((h, stride), np.uint8)
    padded[:, :w] = arr
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(padded.size + lead)) == 0
    hd = None
    try:
        assert hip.hipMemcpy(C.c_void_p(buf.value + lead), padded.ctypes.data_as(C.c_void_p), C.c_size_t(padded.size), 1) == 0   # host to device
        hd = engine.tile_wrap(buf.value + lead, h, w, stride)
        yield hd
    finally:
        if hd is not None:
            engine.tile_free(hd)
        assert hip.hipFree(buf) == 0                         # (every call that read the tile has synchronised before it returned)


@contextlib.contextmanager
def resident(engine, keys):
    """{key: handle} of the named tiles, uploaded once"""
    hs = {}
    try:
        for k in keys:
            if k not in hs:
                hs[k] = engine.tile_upload(SC.tile(k))
        yield hs
    finally:
        for h in hs.values():
            engine.tile_free(h)


@functools.lru_cache(maxsize=None)
def odd_pair():
    """97 x 131 and 97 x 203 crops of one random field: rows that are no multiple of 16 bytes; B's pixel meets A's at (-59, -148)"""
    base = np.random.default_rng(9).integers(0, 256, (200, 420), dtype=np.uint8)
    out = {131: (np.ascontiguousarray(base[60:157, 150:281]), np.ascontiguousarray(base[1:98, 2:133])),
           203: (np.ascontiguousarray(base[60:157, 150:353]), np.ascontiguousarray(base[1:98, 2:205]))}
    for a, b in out.values():
        a.setflags(write=False); b.setflags(write=False)
    return out


# ---- the reduced planes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 4, 8])
@pytest.mark.parametrize("which", ["160x200", "97x131", "97x131_wrapped"])
def test_reduced_planes_equal_the_specification(engine, which, f):
    if which == "160x200":
        A, B = AC.grid("g7")[0][0], AC.grid("g7")[0][1]
    else:
        A, B = odd_pair()[131]
    with contextlib.ExitStack() as stack:
        if which.endswith("wrapped"):                        # rows 141 bytes apart behind an odd address: no row of either tile is aligned
            ha, hb = stack.enter_context(wrapped(engine, A, 141, 1)), stack.enter_context(wrapped(engine, B, 141, 3))
        else:
            ha, hb = engine.tile_upload(A), engine.tile_upload(B)
            stack.callback(engine.tile_free, ha); stack.callback(engine.tile_free, hb)
        for dx in range(-7, 9):
            for dy in range(-7, 9):
                Ac, Bc = engine.ncc_wide_reduce_tiles(ha, hb, A.shape, dx, dy, f)
                wa, wb, _Dx, _Dy = W.reduce_pair(A, B, dx, dy, f)
                assert np.array_equal(Ac, wa) and np.array_equal(Bc, wb), (which, f, dx, dy)
    Ac, Bc = engine.ncc_wide_reduce(A, B, -3, 5, f)          # host arrays in
    wa, wb, _Dx, _Dy = W.reduce_pair(A, B, -3, 5, f)
    assert np.array_equal(Ac, wa) and np.array_equal(Bc, wb)


# ---- the wide search ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,K", SC.CONFIGS)
def test_the_fourteen_pairs_in_one_batch(engine, f, K):
    _tiles, true, _classes = SC.grid35()
    disp = SC.displacements(14, 21)
    centres = [(true[k][0] + disp[k][0], true[k][1] + disp[k][1]) for k in range(14)]
    want = [SC.spec_wide(("g35", k), ("g35", k + 1), centres[k][0], centres[k][1], SC.RADIUS, f, K, SC.MIN_PIXELS) for k in range(14)]
    for k, (o8, _s) in enumerate(want):                      # the conditions first, on the specification alone
        assert [centres[k][0] + o8[0], centres[k][1] + o8[1]] == true[k] and round(o8[2] / FX, 4) >= SC.TRUE_SCORE_MIN
    with resident(engine, SC.g35_keys()) as hs:
        jobs = [(hs[("g35", k)], hs[("g35", k + 1)], centres[k][0], centres[k][1]) for k in range(14)]
        out8, seeds = engine.ncc_wide_batch(jobs, SC.RADIUS, f, K, SC.MIN_PIXELS, want_seeds=True)
        only = engine.ncc_wide_batch(jobs, SC.RADIUS, f, K, SC.MIN_PIXELS)
    assert np.array_equal(only, out8)
    for k in range(14):
        assert out8[k].tolist() == want[k][0], (k, out8[k].tolist(), want[k][0])
        assert np.array_equal(seeds[k], want[k][1]), (k, seeds[k].tolist(), want[k][1].tolist())
        assert [centres[k][0] + out8[k, 0], centres[k][1] + out8[k, 1]] == true[k]


def single_cases():
    """name -> (key or array A, B, dx, dy, R, f, K, min_pixels)"""
    _tiles, true, _classes = SC.grid35()
    g7 = AC.grid("g7")[1]
    A203, B203 = odd_pair()[203]
    return {
        "radius_1": (("g35", 0), ("g35", 1), true[0][0] + 1, true[0][1] - 1, 1, 4, 2, SC.MIN_PIXELS),
        "radius_3": (("g35", 0), ("g35", 1), true[0][0] - 2, true[0][1] + 3, 3, 4, 2, SC.MIN_PIXELS),
        "radius_128_leaves_the_tile": (("g35", 0), ("g35", 1), true[0][0], true[0][1], 128, 8, 2, SC.MIN_PIXELS),
        "class_3": (("g35", 3), ("g35", 4), true[3][0] + 13, true[3][1] - 22, 32, 4, 2, SC.MIN_PIXELS),
        "class_4": (("g35", 3), ("g35", 2), -true[2][0] - 9, -true[2][1] + 17, 32, 2, 2, SC.MIN_PIXELS),
        "width_200": (("g7", 0), ("g7", 1), g7[0][0] + 10, g7[0][1] - 11, 12, 4, 2, AC.MIN_PIXELS),
        "width_203": (A203, B203, -59 + 7, -148 - 5, 12, 4, 3, 0),
        "flat": (("flat", 17), ("flat", 17), 190, 3, 32, 4, 2, 0),
        "unrelated": (("g35", 6), ("alt", 7), true[6][0], true[6][1], 32, 4, 2, SC.MIN_PIXELS),
        "blank": (("g35", 3), ("blank", 5), true[3][0], true[3][1], 32, 8, 1, SC.MIN_PIXELS),
        # 66 x 256 = 16896 pixels at the truth; the centre of the coarse level shares 16 x 64 = 1024 blocks < 16896 // 16 and scores 0 there
        "min_pixels_gates_the_coarse_level": (("g35", 0), ("g35", 1), true[0][0], true[0][1], 8, 4, 2, 16896),
    }


def _array(t):
    return SC.tile(t) if isinstance(t, tuple) else t


@functools.lru_cache(maxsize=None)
def single_expected(name):
    A, B, dx, dy, R, f, K, mp = single_cases()[name]
    if isinstance(A, tuple):
        return SC.spec_wide(A, B, dx, dy, R, f, K, mp)
    return W.search(A, B, dx, dy, R, f, K, mp)


@pytest.mark.parametrize("name", ["radius_1", "radius_3", "radius_128_leaves_the_tile", "class_3", "class_4", "width_200", "width_203", "flat",
                                  "unrelated", "blank", "min_pixels_gates_the_coarse_level"])
def test_single_jobs_equal_the_specification(engine, name):
    A, B, dx, dy, R, f, K, mp = single_cases()[name]
    want8, want_seeds = single_expected(name)
    ha, hb = engine.tile_upload(_array(A)), engine.tile_upload(_array(B))
    try:
        out8, seeds = engine.ncc_wide_batch([(ha, hb, dx, dy)], R, f, K, mp, want_seeds=True)
    finally:
        engine.tile_free(ha); engine.tile_free(hb)
    assert out8[0].tolist() == want8, (out8[0].tolist(), want8)
    assert np.array_equal(seeds[0], want_seeds), (seeds[0].tolist(), want_seeds.tolist())
    if name == "flat":
        assert out8[0, :3].tolist() == [0, 0, 0]
    if name == "unrelated":
        assert round(want8[2] / FX, 4) <= SC.UNRELATED_SCORE_MAX
    if name == "blank":
        assert round(want8[2] / FX, 4) <= SC.BLANK_SCORE_MAX
    if name in ("radius_1", "radius_3"):                      # Rc = 1: every seed's fine window is the one around the prediction
        assert out8[0, 7] <= 2 and [abs(int(v)) <= R for v in out8[0, :2]] == [True, True]


def test_jobs_of_two_shapes_in_one_batch(engine):
    _tiles, true, _classes = SC.grid35()
    g7 = AC.grid("g7")[1]
    A203, B203 = odd_pair()[203]
    cases = [(SC.tile(("g35", 0)), SC.tile(("g35", 1)), true[0][0] - 6, true[0][1] + 9), (SC.tile(("g7", 0)), SC.tile(("g7", 1)), g7[0][0] + 10, g7[0][1] - 11),
             (A203, B203, -52, -153), (SC.tile(("g35", 2)), SC.tile(("g35", 3)), true[2][0] + 11, true[2][1] - 4)]
    hs = []
    try:
        jobs = []
        for A, B, dx, dy in cases:
            hs += [engine.tile_upload(A), engine.tile_upload(B)]
            jobs.append((hs[-2], hs[-1], dx, dy))
        out8, seeds = engine.ncc_wide_batch(jobs, 12, 4, 2, 256, want_seeds=True)
    finally:
        for h in hs:
            engine.tile_free(h)
    for k, (A, B, dx, dy) in enumerate(cases):
        want8, want_seeds = W.search(A, B, dx, dy, 12, 4, 2, 256)
        assert out8[k].tolist() == want8 and np.array_equal(seeds[k], want_seeds), k


def test_refusals_leave_the_outputs_untouched(engine):
    tiles = AC.grid("g7")[0]
    ha, hb, hc = engine.tile_upload(tiles[0]), engine.tile_upload(tiles[1]), engine.tile_upload(np.zeros((160, 208), np.uint8))
    hcol = engine.tile_upload_color(np.zeros((160, 200, 3), np.uint8))
    try:
        assert engine.ncc_wide_batch([], 32).shape == (0, 8)
        for job, R, f, K in (((ha, hb, 0, 0), 0, 4, 2), ((ha, hb, 0, 0), 129, 8, 2), ((ha, hb, 0, 0), 32, 3, 2), ((ha, hb, 0, 0), 40, 2, 2),
                             ((ha, hb, 0, 0), 32, 4, 0), ((ha, hb, 0, 0), 32, 4, 5), ((ha, hcol, 0, 0), 32, 4, 2), ((ha, hc, 0, 0), 32, 4, 2)):
            out = np.full((1, 8), -7, np.int32); seeds = np.full((1, 4, 6), -7, np.int32)
            rc = engine.lib.vfsms_ncc_wide_batch(engine.ctx, engine._ncc_jobs([job]), 1, R, f, K, 0, out.ctypes.data_as(C.c_void_p),
                                                 seeds.ctypes.data_as(C.c_void_p), None)
            assert rc == -1 and (out == -7).all() and (seeds == -7).all(), (R, f, K)
            with pytest.raises(isa.VfsmsError, match="error -1"):
                engine.ncc_wide_batch([job], R, f, K, 0)
        assert engine.ncc_wide_batch([(ha, hb, 120, 0)], 32, 4, 2, 0).shape == (1, 8)      # the engine is fine afterwards
    finally:
        for h in (ha, hb, hc, hcol):
            engine.tile_free(h)


# ---- the overlap sums ----------------------------------------------------------------------------------------------------------------------
def test_overlap_sums_equal_the_specification(engine):
    _tiles, true, _classes = SC.grid35()
    A131, B131 = odd_pair()[131]
    with resident(engine, SC.g35_keys()) as hs, wrapped(engine, A131, 141, 1) as wa, wrapped(engine, B131, 141, 3) as wb:
        jobs = [(hs[("g35", k)], hs[("g35", k + 1)], true[k][0], true[k][1]) for k in range(14)]
        jobs += [(hs[("g35", 0)], hs[("g35", 1)], 256, 0), (hs[("g35", 0)], hs[("g35", 1)], 0, -300), (wa, wb, -59, -100), (wa, wb, 3, 0)]
        got = engine.overlap_sums_batch(jobs)
        assert engine.overlap_sums_batch([]).shape == (0, 6)
    want = [verify_ref.sums(SC.tile(("g35", k)), SC.tile(("g35", k + 1)), true[k][0], true[k][1]) for k in range(14)]
    want += [(0,) * 6, (0,) * 6, verify_ref.sums(A131, B131, -59, -100), verify_ref.sums(A131, B131, 3, 0)]
    assert got.dtype == np.int64 and got.tolist() == [list(s) for s in want]


# ---- the registrar ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["turn_measured", "blank_tile_predicted", "foreign_tile_unresolved"])
def test_grid_registrar_repair(engine, name):
    _tiles, true, classes = SC.grid35()
    keys, failed = {"turn_measured": (SC.g35_keys(), [8]), "blank_tile_predicted": (SC.g35_keys({4: ("blank", 5)}), [3, 4]),
                    "foreign_tile_unresolved": (SC.g35_keys({7: ("alt", 7)}), [6, 7])}[name]
    table = SC.truth_table(true, classes, failed)
    want, want_report = SC.ref_repair(keys, table)
    with resident(engine, keys) as hs:
        got, report = GridRegistrar(engine).repair([hs[k] for k in keys], [(256, 256)] * 15, table)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert report == want_report
    if name == "turn_measured":
        assert got[8].tolist() == [1] + true[8] + [2, 0, 0] and report["pairs"][0]["kind"] == "measured"
    if name == "blank_tile_predicted":
        assert report["period"] == 6 and got[3].tolist() == got[4].tolist() == [1, -192, -2, 3, 0, 0]
        assert [e["kind"] for e in report["pairs"]] == ["predicted", "predicted"]
    if name == "foreign_tile_unresolved":
        assert not got[6, 0] and not got[7, 0]
        assert [(a, b) for a, b, _o in split_segments(got)] == [(0, 6), (7, 7), (8, 14)]


def test_repair_runs_under_its_own_profile_stage(engine):
    _tiles, true, _classes = SC.grid35()
    with resident(engine, [("g35", 0), ("g35", 1)]) as hs:
        engine.profile_enable(True)
        try:
            engine.profile_read(reset=True)
            engine.ncc_wide_batch([(hs[("g35", 0)], hs[("g35", 1)], true[0][0], true[0][1])], 32)
            stages = engine.profile_read(reset=True)
        finally:
            engine.profile_enable(False)
    assert stages["repair"][1] == 1 and stages["adjust"][1] == 2     # one sequence: the coarse and the fine search inside it


# ---- the Stitcher ----------------------------------------------------------------------------------------------------------------------------
class ScriptedStitcher(isa.Stitcher):
    """a Stitcher whose registration method answers from a list of path offsets, None for a pair that cannot be registered (a custom
    method: flowStitch runs pair by pair)"""

    def __init__(self, offsets):
        super().__init__()
        self.script, self.k, self.lines = list(offsets), 0, []
        self.isPrintLog = False
        self.isColorMode = False

    def printAndWrite(self, content):
        self.lines.append(content)

    def scripted(self, images):
        self.k += 1
        o = self.script[self.k - 1]
        return (False, [0, 0]) if o is None else (True, list(o))


def test_stitcher_switch_keeps_one_mosaic(engine, tmp_path):
    from PIL import Image
    tiles, true, _classes = SC.grid35()
    files = []
    for k, t in enumerate(tiles):
        files.append(os.path.join(str(tmp_path), "t%02d.png" % k))
        Image.fromarray(t).save(files[-1])
    script = [list(o) for o in true]
    script[8] = None
    ref = ScriptedStitcher(true)
    ref._engine = engine
    (status, _end), want = ref.flowStitch(list(files), ref.scripted)
    assert status
    st = ScriptedStitcher(script)
    st._engine = engine
    st.failedPairRepair = "stage"
    got = st.flowStitchWithMutiple(list(files), st.scripted)
    assert len(got) == 1 and np.array_equal(np.asarray(got[0]), np.asarray(want))
    e = st.repairReport["pairs"][0]
    assert e["pair"] == 8 and e["kind"] == "measured"
    line = "  %s and %s can not be registered: repaired from the stage model (measured, score %.3f)" % (files[8], files[9], e["score"])
    assert line in st.lines and st.lines[st.lines.index(line) + 1] == "  The offset of stitching: dx is %d dy is %d" % tuple(true[8])
    # "none": no new code runs -- the same script gives the two pieces of today

    class NoRepair:
        def __getattr__(self, name):
            if name in ("ncc_wide_batch", "overlap_sums_batch"):
                raise AssertionError("failedPairRepair = 'none' must not search")
            return getattr(engine, name)
    off = ScriptedStitcher(script)
    off._engine = NoRepair()
    pieces = off.flowStitchWithMutiple(list(files), off.scripted)
    assert len(pieces) == 2 and off.repairReport is None
    assert "  %s and %s can not be stitched" % (files[8], files[9]) in off.lines and not any("repaired" in ln for ln in off.lines)
