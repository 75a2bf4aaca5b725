"""CPU tests of Method.focusStack: the specification (tests/focus_ref.py) against naive loops, its ties and flat planes, the quality it
reaches on the synthetic series of tests/focus_cases.py, and the dataset walk (focus.fuse_dataset, Stitcher.imageSetFocusStack) over a
fake engine that answers with the specification."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import focus

import focus_cases as FC
import focus_ref as FR


# ---- the specification against naive loops -------------------------------------------------------------------------------------------
def _naive(planes, R, median):
    n = len(planes); h, w = planes[0].shape[:2]
    cl = lambda v, hi: min(max(v, 0), hi)                     # noqa: E731
    L = []
    for p in planes:
        if p.ndim == 2:
            L.append([[int(p[y, x]) for x in range(w)] for y in range(h)])
        else:
            L.append([[(29 * int(p[y, x, 0]) + 150 * int(p[y, x, 1]) + 77 * int(p[y, x, 2]) + 128) >> 8 for x in range(w)] for y in range(h)])
    M = [[[abs(2 * l[y][x] - l[y][cl(x - 1, w - 1)] - l[y][cl(x + 1, w - 1)]) + abs(2 * l[y][x] - l[cl(y - 1, h - 1)][x] - l[cl(y + 1, h - 1)][x])
           for x in range(w)] for y in range(h)] for l in L]
    S = [sum(sum(r) for r in m) for m in M]
    D = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            best, arg = -1, 0
            for i in range(n):
                f = 0
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        f += M[i][cl(y + dy, h - 1)][cl(x + dx, w - 1)]
                if f > best:
                    best, arg = f, i
            D[y, x] = arg
    if median:
        Dm = D.copy()
        for y in range(h):
            for x in range(w):
                Dm[y, x] = sorted(int(D[cl(y + dy, h - 1), cl(x + dx, w - 1)]) for dy in (-1, 0, 1) for dx in (-1, 0, 1))[4]
        D = Dm
    out = np.zeros_like(planes[0])
    for y in range(h):
        for x in range(w):
            out[y, x] = planes[D[y, x]][y, x]
    return out, D, np.array(S, np.int64)


@pytest.mark.parametrize("median", [0, 1])
@pytest.mark.parametrize("R", [1, 2, 31])
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 7, 3), (9, 4)], ids=lambda s: "x".join(map(str, s)))
def test_specification_equals_naive_loops(shape, R, median):
    rng = np.random.default_rng(sum(shape) + R)
    planes = [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(3)]
    got, want = FR.fuse(planes, R, median), _naive(planes, R, median)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[1].dtype == np.uint8 and got[2].dtype == np.int64
    M = FR.measure(FR.luma(planes[0]))
    assert M.max() <= 1020 and FR.focus(M, R).max() <= 1020 * (2 * R + 1) ** 2 and np.array_equal(FR.scores(planes), want[2])


def test_ties_take_the_lowest_index():
    rng = np.random.default_rng(1)
    one = rng.integers(0, 256, (9, 11, 3)).astype(np.uint8)
    out, D, S = FR.fuse([one, one.copy(), one.copy()], 2, 1)
    assert not D.any() and np.array_equal(out, one) and S[0] == S[1] == S[2]
    planes = [rng.choice(np.array([0, 17, 255], np.uint8), (12, 9)) for _ in range(6)]
    planes[4] = planes[2].copy()
    F = np.stack([FR.focus(FR.measure(FR.luma(p)), 1) for p in planes])
    D = FR.index(planes, 1)
    assert (F[4] == F[2]).all() and not (D == 4).any()
    for i in range(6):
        at = D == i
        assert (F[i][at] == F.max(0)[at]).all() and all((F[j][at] < F[i][at]).all() for j in range(i))
    assert np.array_equal(FR.fuse(planes, 1, 0)[1], D) and np.array_equal(FR.fuse(planes, 1, 1)[1], FR.median3(D))


def test_flat_planes():
    planes = [np.full((6, 8), 10 * k + 3, np.uint8) for k in range(4)]
    out, D, S = FR.fuse(planes, 3, 1)
    assert not FR.focus(FR.measure(FR.luma(planes[2])), 3).any() and not D.any() and not S.any() and np.array_equal(out, planes[0])


def test_the_specification_refuses_what_the_library_refuses():
    p = np.zeros((4, 4), np.uint8)
    for bad in (lambda: FR.fuse([p], 4, 1), lambda: FR.fuse([p] * 65, 4, 1), lambda: FR.fuse([p, np.zeros((4, 5), np.uint8)], 4, 1),
                lambda: FR.fuse([p, np.zeros((4, 4, 3), np.uint8)], 4, 1), lambda: FR.fuse([np.zeros((4, 4, 2), np.uint8)] * 2, 4, 1),
                lambda: FR.fuse([p, p], 0, 1), lambda: FR.fuse([p, p], 32, 1), lambda: FR.fuse([p, p], 4, 2), lambda: FR.fuse([p, p], 4, 1, "voxel"),
                lambda: FR.fuse([p.astype(np.int32)] * 2, 4, 1)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("median", [0, 1])
@pytest.mark.parametrize("R", [2, 4, 8])
@pytest.mark.parametrize("shape", [(48, 80), (96, 160), (64, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("K", [3, 4, 5])
def test_quality_on_the_synthetic_series(K, shape, R, median):
    """the right plane for at least 95 % of the pixels, and a fused mean absolute error of at most one tenth of the best single plane's
    (the specification alone measured at least 0.966, and at most 1.4 grey levels against at least 22)"""
    for kind in ("ramp", "quad"):
        planes, sharp, depth = FC.stack(shape, K, kind, seed=K)
        out, D, _S = FR.fuse(planes, R, median)
        best = min(np.abs(p.astype(np.int32) - sharp).mean() for p in planes)
        assert np.mean(D == depth) >= 0.95, kind
        assert np.abs(out.astype(np.int32) - sharp).mean() <= best / 10, kind


def test_plane_mode_picks_the_largest_score():
    planes, _sharp, _depth = FC.stack((48, 80, 3), 4, "ramp", seed=2)
    out, D, S = FR.fuse(planes, 4, 1, "plane")
    k = int(np.argmax(S))
    assert (D == k).all() and np.array_equal(out, planes[k]) and np.array_equal(S, FR.scores(planes))
    planes[0], planes[2] = planes[k].copy(), planes[k].copy()                         # the largest score three times: the first wins
    out, D, S = FR.fuse(planes, 4, 1, "plane")
    assert S[0] == S[2] == S.max() and not D.any() and np.array_equal(out, planes[0])


# ---- the dataset walk over a fake engine -------------------------------------------------------------------------------------------------
class FakeEngine:
    """tiles are arrays in a dict; focus_stack answers with the specification"""

    def __init__(self):
        self.tiles, self.next, self.uploads, self.calls = {}, 1, 0, []

    def _put(self, img):
        self.tiles[self.next] = np.array(img); self.next += 1; self.uploads += 1
        return self.next - 1

    def tile_upload(self, img):
        assert np.asarray(img).ndim == 2
        return self._put(img)

    def tile_upload_color(self, img):
        assert np.asarray(img).ndim == 3
        return self._put(img)

    def tile_free(self, h):
        del self.tiles[h]

    def focus_stack(self, handles, mode="pixel", radius=4, median=1, want_tile=False):
        self.calls.append((len(handles), mode, radius, median, len(self.tiles)))
        out, D, S = FR.fuse([self.tiles[h] for h in handles], radius, median, mode)
        return (self._put(out) if want_tile else out), D, S


def _series(folder, positions, planes, shape=(24, 40), color=False, ext="png"):
    from PIL import Image
    os.makedirs(str(folder), exist_ok=True)
    stacks = []
    for k in range(positions):
        ps, _sharp, _depth = FC.stack(shape + ((3,) if color else ()), planes, "ramp", seed=10 + k)
        stacks.append(ps)
        for z, p in enumerate(ps):
            Image.fromarray(p[:, :, ::-1] if color else p).save(os.path.join(str(folder), "p%02d_z%d.%s" % (k, z, ext)))
    return stacks


def _stitcher(engine, **settings):
    st = isa.Stitcher(); st._engine = engine
    st.msgs = []
    st.printAndWrite = st.msgs.append
    for k, v in settings.items():
        setattr(st, k, v)
    return st


@pytest.mark.parametrize("color", [False, True], ids=("gray", "colour"))
def test_fuse_dataset_groups_and_names(tmp_path, color):
    from imagestitch_amd.ingest import _imread, _list_images
    stacks = _series(tmp_path / "in", 3, 3, color=color)
    eng = FakeEngine()
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = color
        st = _stitcher(eng, focusStack="pixel", focusRadius=2, focusMedian=0, focusDepthMaps=True)
        files = _list_images(str(tmp_path / "in"), "png")
        written = focus.fuse_dataset(st, files, 3, str(tmp_path / "out"))
    finally:
        isa.Stitcher.isColorMode = old
    assert [os.path.basename(p) for p in written] == ["p00_z0.png", "p01_z0.png", "p02_z0.png"]
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["depth", "p00_z0.png", "p01_z0.png", "p02_z0.png"]
    assert eng.calls == [(3, "pixel", 2, 0, 3)] * 3 and not eng.tiles and eng.uploads == 9      # one position resident at a time, all freed
    for k, path in enumerate(written):
        wout, wD, _wS = FR.fuse(stacks[k], 2, 0)
        assert np.array_equal(_imread(path, color), wout)
        assert np.array_equal(_imread(os.path.join(str(tmp_path / "out"), "depth", "p%02d_z0_depth.png" % k), False), wD)
        assert st.msgs[k] == "  focus stack p%02d_z0: pixels per plane %s" % (k, [int(v) for v in np.bincount(wD.reshape(-1), minlength=3)])
    st2 = _stitcher(FakeEngine(), focusStack="plane")
    focus.fuse_dataset(st2, files[:6], 3, str(tmp_path / "out2"))
    assert sorted(os.listdir(str(tmp_path / "out2"))) == ["p00_z0.png", "p01_z0.png"]            # no depth maps unless asked for
    assert st2.msgs[0].startswith("  focus stack p00_z0: plane ") and "scores [" in st2.msgs[0]


def test_fuse_dataset_refuses_before_a_decode(tmp_path, monkeypatch):
    from PIL import Image
    from imagestitch_amd.ingest import _list_images
    _series(tmp_path / "in", 2, 3)
    files = _list_images(str(tmp_path / "in"), "png")
    decoded = []
    monkeypatch.setattr(focus, "_imread", lambda f, c: decoded.append(f))
    eng = FakeEngine()
    st = _stitcher(eng, focusStack="pixel")
    Image.fromarray(np.zeros((24, 41), np.uint8)).save(str(tmp_path / "odd.png"))
    for bad in (lambda: focus.fuse_dataset(st, files[:5], 3, str(tmp_path / "o")),                # no whole number of positions
                lambda: focus.fuse_dataset(st, files, 1, str(tmp_path / "o")),                    # planes < 2
                lambda: focus.fuse_dataset(st, files, 65, str(tmp_path / "o")),
                lambda: focus.fuse_dataset(st, files[:5] + [str(tmp_path / "odd.png")], 3, str(tmp_path / "o")),   # a plane of another size
                lambda: focus.fuse_dataset(st, files, 3, str(tmp_path / "o"), "jpg"),             # a lossy container
                lambda: focus.fuse_dataset(_stitcher(eng, focusStack="none"), files, 3, str(tmp_path / "o")),
                lambda: focus.fuse_dataset(_stitcher(eng, focusStack="pixel", focusRadius=32), files, 3, str(tmp_path / "o")),
                lambda: focus.fuse_dataset(_stitcher(eng, focusStack="pixel", focusMedian=2), files, 3, str(tmp_path / "o"))):
        with pytest.raises(ValueError):
            bad()
    assert not decoded and not eng.uploads and not os.path.exists(str(tmp_path / "o"))


def test_tiles_are_freed_when_a_decode_fails(tmp_path, monkeypatch):
    from imagestitch_amd.ingest import _imread, _list_images
    _series(tmp_path / "in", 3, 2)
    files = _list_images(str(tmp_path / "in"), "png")

    def decode(f, c):
        if f == files[3]:                                     # the second plane of the second position
            raise OSError("truncated file")
        return _imread(f, c)
    monkeypatch.setattr(focus, "_imread", decode)
    eng = FakeEngine()
    with pytest.raises(OSError):
        focus.fuse_dataset(_stitcher(eng, focusStack="pixel"), files, 2, str(tmp_path / "out"))
    assert not eng.tiles and len(eng.calls) == 1 and os.listdir(str(tmp_path / "out")) == ["p00_z0.png"]

    class Failing(FakeEngine):
        def focus_stack(self, *a, **k):
            raise RuntimeError("device lost")
    eng = Failing()
    monkeypatch.setattr(focus, "_imread", _imread)
    with pytest.raises(RuntimeError):
        focus.fuse_dataset(_stitcher(eng, focusStack="pixel"), files, 2, str(tmp_path / "out3"))
    assert not eng.tiles and eng.uploads == 2


def test_fuse_stack_frees_what_it_uploaded():
    planes, _sharp, _depth = FC.stack((24, 40), 3, "quad", seed=5)
    eng = FakeEngine()
    resident = eng.tile_upload(planes[0])
    out, D, S = focus.fuse_stack(eng, [resident, planes[1], planes[2]], radius=2)
    want = FR.fuse(planes, 2, 1)
    assert all(np.array_equal(a, b) for a, b in zip((out, D, S), want)) and list(eng.tiles) == [resident]
    tile, _D, _S = isa.fuse_stack(eng, planes, mode="plane", want_tile=True)
    assert np.array_equal(eng.tiles[tile], FR.fuse(planes, 4, 1, "plane")[0]) and sorted(eng.tiles) == [resident, tile]
    with pytest.raises(ValueError):
        focus.fuse_stack(eng, planes[:1])
    with pytest.raises(ValueError):
        focus.fuse_stack(eng, planes, mode="none")


def test_image_set_focus_stack(tmp_path):
    """projectAddress/i -> stackedAddress/i, options judged before a file is listed, "none" refused"""
    from imagestitch_amd.ingest import _imread
    stacks = {i: _series(tmp_path / "proj" / str(i), 2, 2) for i in (1, 2)}
    eng = FakeEngine()
    st = _stitcher(eng, focusStack="pixel", focusPlanes=2)
    written = st.imageSetFocusStack(str(tmp_path / "proj"), str(tmp_path / "stacked"), 2, fileExtension="png")
    assert [[os.path.relpath(p, str(tmp_path / "stacked")) for p in w] for w in written] == \
        [[os.path.join(str(i), "p%02d_z0.png" % k) for k in (0, 1)] for i in (1, 2)]
    for i in (1, 2):
        for k in (0, 1):
            assert np.array_equal(_imread(written[i - 1][k], False), FR.fuse(stacks[i][k], 4, 1)[0])
    assert not eng.tiles
    listed = []
    import imagestitch_amd.stitcher as S
    real = S._list_images
    S._list_images = lambda *a: listed.append(a) or real(*a)
    try:
        for settings in ({}, {"focusStack": "none", "focusPlanes": 2}, {"focusStack": "voxel", "focusPlanes": 2}, {"focusStack": "pixel"},
                         {"focusStack": "pixel", "focusPlanes": 65}, {"focusStack": "plane", "focusPlanes": 2, "focusRadius": 0},
                         {"focusStack": "pixel", "focusPlanes": 2, "focusMedian": 3}):
            with pytest.raises(ValueError):
                _stitcher(eng, **settings).imageSetFocusStack(str(tmp_path / "proj"), str(tmp_path / "never"), 2, fileExtension="png")
        assert not listed and not os.path.exists(str(tmp_path / "never"))

        class Bare:
            pass
        with pytest.raises(NotImplementedError):
            _stitcher(Bare(), focusStack="pixel", focusPlanes=2).imageSetFocusStack(str(tmp_path / "proj"), str(tmp_path / "never"), 2, fileExtension="png")
        assert not listed
    finally:
        S._list_images = real


def test_defaults_leave_the_pipeline_untouched():
    """the defaults are "off", and no entry point of the pipeline reads the focus attributes: imageSetStitch* never meets the module"""
    m = isa.Method()
    assert (m.focusStack, m.focusPlanes, m.focusRadius, m.focusMedian, m.focusDepthMaps) == ("none", 1, 4, 1, False)
    import inspect
    for fn in (isa.Stitcher.imageSetStitch, isa.Stitcher.imageSetStitchWithMutiple, isa.Stitcher.flowStitch, isa.Stitcher.flowStitchWithMutiple,
               isa.Stitcher.getStitchByOffset):
        assert "focus" not in inspect.getsource(fn)
    assert {"fuse_stack", "fuse_dataset"} <= set(isa.__all__)
    from imagestitch_amd import _lib
    assert {"vfsms_focus_stack", "vfsms_focus_scores"} <= set(_lib.exported_names())
