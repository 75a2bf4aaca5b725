"""The cases of the 16-bit shading correction shared by tests/test_deep_shading_host.py and tests/test_deep_shading_gpu.py: tile sets of ONE
shape per set, the parameter combinations each set is run through, and the references (tests/deep_shading_ref.py), computed once."""
import functools

import numpy as np

import deep_cases as DC
import deep_shading_ref as DSR

SHAPES = ((1, 1), (3, 5), (33, 131), (70, 257))              # 33 x 131 = 4323 samples: an odd count, a ragged 8-sample tail, rows no multiple of a dword
SMALL = SHAPES[:2]                                           # the shapes that go through the full cross product of the parameters
KINDS = DC.KINDS
COUNTS = (1, 2, 7, 64)                                       # 7: less than one group of 8 rows of the descent; 64: four groups of 16
STAGING_LIMIT = 320                                          # DEEP_SHADE_LDS_MAX_N of csrc/deep_shading_kernels.hip: up to it the descent runs from LDS
PERCENTILES = (0, 37, 50, 100)
RADII = (1, 4, 127)                                          # 127 exceeds every test tile: replication carries the whole window
PEDESTALS = (0, 2000, 65535)
# every value of every parameter at least once, for the sets that do not go through the whole cross product
COVER = ((0, 1, 0), (37, 4, 2000), (50, 127, 65535), (100, 4, 2000), (50, 1, 2000), (37, 127, 0))


def _tile(kind, rng, h, w):
    """one tile of a data kind of deep_cases.tile_set, drawn anew from rng"""
    if kind == "full":
        t = rng.integers(0, 65536, (h, w))
    elif kind == "12bit":
        t = rng.integers(0, 4096, (h, w))
    elif kind == "constant":
        t = np.full((h, w), 31337)
    elif kind == "two":
        t = rng.choice([513, 40000], (h, w))
    elif kind == "ends":
        t = rng.choice([0, 65535], (h, w))
    else:
        raise KeyError(kind)
    return t.astype(np.uint16)


def _names():
    out = {}
    for h, w in SHAPES:
        for kind in KINDS:
            for n in COUNTS:
                out["%dx%d-%s-%d" % (h, w, kind, n)] = (h, w, kind, n)
    for h, w in ((3, 5), (33, 131)):                         # ties decide every step of the descent, from LDS and from global memory
        for n in (STAGING_LIMIT, STAGING_LIMIT + 1):
            out["%dx%d-two-%d" % (h, w, n)] = (h, w, "two", n)
    return out


SETS = _names()


@functools.lru_cache(maxsize=None)
def tiles(name):
    """the tiles of a set (read-only) and one more tile of the same shape and kind that no call names"""
    h, w, kind, n = SETS[name]
    rng = np.random.default_rng(sorted(SETS).index(name) + 100)
    out = [_tile(kind, rng, h, w) for _ in range(n + 1)]
    for t in out:
        t.setflags(write=False)
    return out[:n], out[n]


def combos(name):
    """the (percentile, radius, pedestal) combinations a set is run through"""
    h, w, _kind, n = SETS[name]
    if (h, w) in SMALL and n <= max(COUNTS):
        return tuple((p, r, d) for p in PERCENTILES for r in RADII for d in PEDESTALS)
    return COVER


@functools.lru_cache(maxsize=None)
def profile(name, percentile):
    P = DSR.profile(tiles(name)[0], percentile)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def reference(name, percentile, radius, pedestal):
    """-> (gain, smooth, profile) of the set, computed once; callers must not write to them"""
    P = profile(name, percentile)
    F = DSR.smooth(P, radius, pedestal)
    G = DSR.gain(F)
    for a in (F, G):
        a.setflags(write=False)
    return G, F, P
