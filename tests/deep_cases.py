"""The cases of the 16-bit path shared by tests/test_deep_host.py (small ones against brute force) and tests/test_deep_gpu.py (the device
against tests/deep_ref.py): tile sets for window / reduce and mosaic layouts."""
import functools

import numpy as np

import deep_ref as DR

PPM_PAIRS = ((0, 1000000), (1000, 999000), (500000, 500000), (0, 0))
SHAPES = ((1, 1), (3, 5), (33, 131), (70, 257), (97, 201))                     # 70 x 257 = 17990 samples: more than one 16384-sample chunk
KINDS = ("full", "12bit", "constant", "two", "ends")
FEATHERS = (0, 1, 5, 32767)


def tile_set(kind, seed=7):
    """one tile of every shape in SHAPES, of a data kind"""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in SHAPES:
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
        out.append(t.astype(np.uint16))
    return out


def _rand(rng, h, w):
    return rng.integers(0, 65536, (h, w)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def layouts():
    """name -> dict(tiles: the distinct arrays, use: per placed tile its index in `tiles`, yx, rows, cols)"""
    rng = np.random.default_rng(11)
    L = {}

    def add(name, tiles, use, yx, rows=None, cols=None):
        rows = rows or max(y + tiles[u].shape[0] for u, (y, x) in zip(use, yx))
        cols = cols or max(x + tiles[u].shape[1] for u, (y, x) in zip(use, yx))
        L[name] = dict(tiles=tiles, use=list(use), yx=[(int(y), int(x)) for y, x in yx], rows=int(rows), cols=int(cols))
    add("single", [_rand(rng, 33, 131)], [0], [(0, 0)])
    add("two_odd", [_rand(rng, 70, 257), _rand(rng, 70, 257)], [0, 1], [(1, 3), (37, 131)], 120, 400)
    add("grid2x2", [_rand(rng, 64, 96) for _ in range(4)], range(4), [(0, 0), (0, 70), (50, 0), (50, 70)])
    yx = [(r * 60 + int(rng.integers(0, 7)), c * 230 + int(rng.integers(0, 7))) for r in range(3) for c in range(3)]
    add("jitter3x3", [_rand(rng, 70, 257) for _ in range(9)], range(9), yx)
    add("inside", [_rand(rng, 97, 201), _rand(rng, 33, 131)], [0, 1], [(0, 0), (20, 30)])
    add("inside_first", [_rand(rng, 33, 131), _rand(rng, 97, 201)], [0, 1], [(20, 30), (0, 0)])
    add("same_position", [_rand(rng, 33, 131), _rand(rng, 33, 131)], [0, 1], [(5, 7), (5, 7)], 45, 150)
    add("same_handle", [_rand(rng, 33, 131)], [0, 0], [(0, 0), (10, 40)])
    add("gap", [_rand(rng, 33, 131), _rand(rng, 33, 131)], [0, 1], [(0, 0), (50, 200)], 90, 340)      # rows 33..49 and 83..89: no tile
    add("mixed", [_rand(rng, h, w) for h, w in SHAPES], range(5), [(40, 250), (0, 0), (10, 2), (30, 100), (1, 150)])
    add("six_over", [_rand(rng, 40, 60) for _ in range(6)], range(6), [(3 * k, 5 * k) for k in range(6)])
    add("all_max", [np.full((40, 60), 65535, np.uint16)], [0] * 6 + [0], [(3 * k, 5 * k) for k in range(6)] + [(30, 70)], 80, 140)
    return L


@functools.lru_cache(maxsize=None)
def reference(name, mode, feather):
    """the whole reference mosaic of a layout, computed once; callers must not write to it"""
    c = layouts()[name]
    out = DR.mosaic([c["tiles"][u] for u in c["use"]], c["yx"], c["rows"], c["cols"], mode, feather)
    out.setflags(write=False)
    return out
