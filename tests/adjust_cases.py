"""Shared inputs of tests/test_adjust_host.py and tests/test_adjust_gpu.py: three small synthetic 3 x 3 grids, the perturbed path
offsets, and an engine whose window search IS the specification (tests/ncc_search_ref.py)."""
import functools

import numpy as np

from imagestitch_amd.synthetic import SyntheticGrid
import ncc_search_ref as S

RADIUS = 4
MIN_PIXELS = 256
# (rows, cols, tile_h, tile_w, overlap, jitter, seed): on each, all 12 side-neighbour edges peak exactly at the true offset
GRIDS = {"g7": (3, 3, 160, 200, 0.25, 4, 7), "g11": (3, 3, 160, 200, 0.25, 4, 11), "g3": (3, 3, 256, 256, 0.2, 6, 3)}
EDGES_3X3 = [(0, 1), (0, 5), (1, 2), (1, 4), (2, 3), (3, 4), (3, 8), (4, 5), (4, 7), (5, 6), (6, 7), (7, 8)]
# errors of three path pairs, up to 3 px; they cancel so that every tile's predicted position -- hence every edge's window centre -- stays
# within 3 px of the truth: tiles 2..4 are off by (3, -2), tiles 7, 8 by (2, -3)
PERTURB = {1: (3, -2), 4: (-3, 2), 6: (2, -3)}


@functools.lru_cache(maxsize=None)
def grid(name):
    """-> (tiles, true path offsets) of GRIDS[name]; computed once and shared: do not write to the arrays"""
    r, c, h, w, ov, jit, seed = GRIDS[name]
    g = SyntheticGrid(r, c, h, w, overlap=ov, jitter=jit, seed=seed)
    tiles = g.tiles(threads=1)
    for t in tiles:
        t.setflags(write=False)
    return tiles, [list(o) for o in g.true_offsets()]


def perturbed(true_offsets, perturb=None):
    out = [list(o) for o in true_offsets]
    for k, (ex, ey) in (PERTURB if perturb is None else perturb).items():
        out[k] = [out[k][0] + ex, out[k][1] + ey]
    return out


@functools.lru_cache(maxsize=None)
def _spec_search(name, a, b, dx, dy, radius, min_pixels):
    tiles, _ = grid(name)
    i, j, fx, surface = S.search(tiles[a], tiles[b], dx, dy, radius, min_pixels)
    surface.setflags(write=False)
    return i, j, fx, S.shared_pixels(tiles[a].shape, dx + i, dy + j), surface


class SpecEngine:
    """Engine.ncc_search_batch answered by the specification; tile handles are indices into grid(name)'s tiles"""

    def __init__(self, name):
        self.name, self.calls = name, 0

    def ncc_search_batch(self, jobs, radius, min_pixels, want_surface=False):
        self.calls += 1
        res = [_spec_search(self.name, int(a), int(b), int(dx), int(dy), int(radius), int(min_pixels)) for a, b, dx, dy in jobs]
        best = np.array([r[:4] for r in res], np.int32).reshape(-1, 4)
        return (best, np.stack([r[4] for r in res])) if want_surface else best


def spec_rows(A, B, dx, dy, radius, min_pixels):
    """(best4 row, surface) of the specification for one job on host arrays"""
    i, j, fx, surface = S.search(A, B, dx, dy, radius, min_pixels)
    return [i, j, fx, S.shared_pixels(A.shape, dx + i, dy + j)], surface
