"""CPU tests of tests/deep_shading_ref.py, the specification of the 16-bit shading correction: the order statistic against brute force, the
uint32 bound of the box passes at its worst case, the corners of `apply`, and that the correction flattens a vignetted stack over a pedestal."""
import os
import re

import numpy as np
import pytest

import deep_shading_cases as DSC
import deep_shading_ref as DSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["3x5-full-7", "33x131-12bit-64", "3x5-two-64", "1x1-ends-2", "70x257-full-2", "3x5-two-321"])
def test_profile_is_the_order_statistic(name):
    tiles, _ = DSC.tiles(name)
    stack = np.stack(tiles)
    for percentile in (0, 37, 50, 100):
        k = (len(tiles) - 1) * percentile // 100
        want = np.sort(stack, 0)[k]
        got = DSR.profile(tiles, percentile)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (name, percentile)
    assert np.array_equal(DSR.profile(tiles, 0), stack.min(0)) and np.array_equal(DSR.profile(tiles, 100), stack.max(0))


def test_the_box_sums_do_not_wrap_at_the_largest_field():
    """255^2 * 65535 + 32512 < 2^32: a plane of all 65535 at R = 127 stays all 65535 (a wrapped uint32 sum would not)"""
    P = np.full((40, 300), 65535, np.uint16)
    F = DSR.smooth(P, 127, 0)
    assert F.dtype == np.uint16 and (F == 65535).all()
    assert (DSR.smooth(P, 127, 65535) == 0).all()
    assert (DSR.smooth(P, 1, 2000) == 63535).all()


def test_apply_at_its_corners():
    p = np.array([[65535, 0, 1, 40000]], np.uint16)
    G = np.full(p.shape, 65535, np.uint16)
    assert DSR.apply(p, G, 0).tolist() == [[65535, 0, 16, 65535]]                # 1 * 65535 + 2048 >> 12 = 16; the rest clamps
    rng = np.random.default_rng(5)
    t = rng.integers(0, 65536, (9, 11)).astype(np.uint16)
    g = rng.integers(0, 65536, (9, 11)).astype(np.uint16)
    for d in (0, 2000, 40000, 65535):
        out = DSR.apply(t, g, d)
        assert np.array_equal(out[t <= d], t[t <= d])                            # at or below the pedestal: left alone
        one = DSR.apply(t, np.full(t.shape, 4096, np.uint16), d)
        assert np.array_equal(one, t)                                            # a gain of one changes nothing
    # the pedestal at the top of the range: nothing is above it, the field is zero and the gain is one everywhere
    tiles = [rng.integers(0, 65536, (9, 11)).astype(np.uint16) for _ in range(5)]
    G, F, _P = DSR.estimate(tiles, 50, 4, 65535)
    assert (F == 0).all() and (G == 4096).all()
    for a, b in zip(DSR.correct(tiles, 50, 4, 65535), tiles):
        assert np.array_equal(a, b)


def test_the_level_and_the_gain_are_the_rounded_quotients():
    rng = np.random.default_rng(8)
    F = rng.integers(0, 65536, (13, 17)).astype(np.uint16)
    F[3, 4] = 0; F[0, 0] = 1
    M = DSR.level(F)
    assert M == (sum(int(v) for v in F.reshape(-1)) + 110) // 221
    G = DSR.gain(F)
    for (y, x), v in np.ndenumerate(F):
        assert int(G[y, x]) == (4096 if v == 0 else min(65535, (M * 4096 + int(v) // 2) // int(v)))


def test_correction_flattens_a_vignetted_stack_over_its_pedestal():
    """The construction and the figures of the issue: a numpy prototype of the specification gave 0.7799 before and 0.9960 after
    correct(..., 50, 8, d), 0.9962 at R = 4; the bounds are before < 0.80 and after > 0.99."""
    rng = np.random.default_rng(3)
    h, w, N, d = 96, 160, 24, 2000
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = (h - 1) / 2, (w - 1) / 2
    r2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / (cy ** 2 + cx ** 2)
    shade = 1 - 0.35 * r2
    tiles = []
    for _ in range(N):
        scene = np.kron(rng.integers(400, 3000, (12, 20)), np.ones((8, 8), np.int64))
        tiles.append(np.clip(d + shade * scene + rng.integers(0, 12, (h, w)), 0, 65535).astype(np.uint16))

    def ratio(ts):
        m = np.mean([t.astype(np.float64) - d for t in ts], 0)
        return m[:16, :16].mean() / m[h // 2 - 8:h // 2 + 8, w // 2 - 8:w // 2 + 8].mean()
    before = ratio(tiles)
    after = ratio(DSR.correct(tiles, 50, 8, d))
    after4 = ratio(DSR.correct(tiles, 50, 4, d))
    print("flatness: before %.4f, after %.4f (R = 8), %.4f (R = 4)" % (before, after, after4))
    assert before < 0.80 and after > 0.99, (before, after)


def test_arguments_outside_the_specification_are_refused():
    t = np.zeros((4, 4), np.uint16)
    with pytest.raises(ValueError):
        DSR.profile([t.astype(np.uint8)], 50)
    with pytest.raises(ValueError):
        DSR.profile([t], 101)
    with pytest.raises(ValueError):
        DSR.smooth(t, 128, 0)
    with pytest.raises(ValueError):
        DSR.smooth(t, 4, 65536)
    with pytest.raises(ValueError):
        DSR.apply(t, np.zeros((4, 5), np.uint16), 0)
    with pytest.raises(ValueError):
        DSR.apply(t, t, -1)


def test_the_cases_name_the_kernel_staging_limit():
    src = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "deep_shading_kernels.hip")).read()
    assert int(re.search(r"#define DEEP_SHADE_LDS_MAX_N (\d+)", src).group(1)) == DSC.STAGING_LIMIT
    for shape in ("3x5", "33x131"):
        for n in (DSC.STAGING_LIMIT, DSC.STAGING_LIMIT + 1):
            tiles, _ = DSC.tiles("%s-two-%d" % (shape, n))
            assert len(tiles) == n and set(np.unique(np.stack(tiles)).tolist()) == {513, 40000}
