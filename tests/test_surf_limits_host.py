"""What tests/test_surf_limits_gpu.py assumes about its inputs, asserted from the CPU oracle alone (no GPU), and the registrar's capacity
retry on fakes.

The figures: candidates in the fullest k_nms workgroup of every image (surf_limit_cases.fullest_block against NMS_LOCAL = 192), the
candidate counts C the capacity tests are built around (against SORT_BUCKETS = 1024), and the counts of the retry path."""
import numpy as np
import pytest

import surf_limit_cases as S
from chain_ref import ChainRef
from imagestitch_amd._lib import VFSMS_ERR_CAPACITY, VfsmsError
from imagestitch_amd.grid import GridRegistrar

# name: (C, fullest block, largest group of equal responses) -- measured on the oracle, asserted below
FIGURES = {
    "lattice": (3980, 546, 1344),
    "lattice_width": (1703, 441, 588),
    "lattice_height": (1140, 409, 450),
    "lattice_view": (3988, 546, 1316),
    "lattice_small": (690, 452, 253),
    "lattice_large": (8349, 882, 2745),
    "noise": (274, 56, 1),
    "periodic": (212, 52, 8),
}


def _figures(oracle, name):
    img = S.case_image(name)
    k = S.oracle_detect(name)
    cand = S.candidates(k, S.det_layers(oracle, img))
    _v, ties = np.unique(k["response"], return_counts=True)
    return cand, (len(k), S.fullest_block(cand, img.shape), int(ties.max()))


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_case_figures(oracle, name):
    cand, fig = _figures(oracle, name)
    assert fig == FIGURES[name], (name, fig)
    C, fullest, _ties = fig
    if name.startswith("lattice"):
        assert fullest > 2 * S.NMS_LOCAL, (name, fullest)            # the direct-append branch takes more than half of the fullest block
    else:
        assert fullest < S.NMS_LOCAL, (name, fullest)
    # every candidate sits on a cell its layer evaluates, a middle layer, one keypoint per cell (candidates() asserts the rest)
    assert cand[:, 1].min() >= 1 and cand[:, 1].max() <= S.STOCK[2]


def test_restated_constants_are_the_kernels():
    """fullest_block describes k_nms only while the constants of surf_limit_cases are the #defines of surf_kernels.hip"""
    d = S.kernel_defines()
    assert d == {"NMS_RW": str(S.NMS_RW), "NMS_TW": str(S.NMS_TW), "NMS_TH": "(4 * NMS_RW)", "NMS_LOCAL": str(S.NMS_LOCAL),
                 "SORT_BUCKETS": str(S.SORT_BUCKETS)}, d
    assert S.NMS_TH == 4 * S.NMS_RW


def test_the_view_case_is_a_strided_view():
    v = S.case_image("lattice_view")
    assert v.shape == (200, 320) and not v.flags["C_CONTIGUOUS"] and v.strides == (400, 1)


def test_the_nearest_cell_is_not_always_the_candidates(oracle):
    """interpolate_keypoint accepts offsets up to a whole step, so the nearest cell is a first guess only: on the periodic image and on
    white noise it names other cells than the determinant layers do; the lattice's candidates sit within half a step of their cells"""
    differ = {}
    for name in ("periodic", "noise", "lattice"):
        cells, nearest = S.candidates(S.oracle_detect(name), S.det_layers(oracle, S.case_image(name)), with_nearest=True)
        differ[name] = int((cells != nearest).any(1).sum())
    assert differ["periodic"] > 0 and differ["noise"] > 0 and differ["lattice"] == 0, differ


def test_full_block_next_to_a_partial_one(oracle):
    """block_counts of the width and height cases: layer 3 of octave 0 (margin 17) has two full blocks and a partial third along the axis"""
    for name, axis in (("lattice_width", 3), ("lattice_height", 2)):
        img = S.case_image(name)
        cells = img.shape[axis - 2] - 2 * 17
        size = S.NMS_TW if axis == 3 else S.NMS_TH
        assert cells // size == 2 and 0 < cells % size < size
        bc = S.block_counts(S.candidates(S.oracle_detect(name), S.det_layers(oracle, img)), img.shape)
        got = sorted(key[axis] for key in bc if key[:2] == (0, 3))
        assert got == [0, 1, 2], (name, got)
        assert bc[(0, 3, 0, 0)] > S.NMS_LOCAL and 0 < bc[(0, 3, 0, 2) if axis == 3 else (0, 3, 2, 0)] < bc[(0, 3, 0, 0)]


def test_capacity_cases_sit_where_the_tests_need_them():
    C = {n: len(S.oracle_detect(n)) for n in FIGURES}
    assert C["noise"] < S.SORT_BUCKETS - 1 and C["periodic"] < S.SORT_BUCKETS - 1 and C["lattice_small"] < S.SORT_BUCKETS - 1     # rank sort at capacity C, both sorts at 1023 / 1024
    assert C["lattice"] > S.SORT_BUCKETS                                                                                      # bucket sort at capacity C and C - 1
    for n in FIGURES:                                                                                                         # all fit the operator's default capacity
        h, w = S.case_image(n).shape
        assert C[n] <= h * w // 24 + 4096


def test_batch_strips(oracle):
    """test d: seven distinct strips of eight slots (tile 0's bottom strip is shared), column strips before turn strips, and the lattice
    strip -- the last, 640 x 128 -- holds far more candidates than any other"""
    tiles, jobs = S.batch_tiles(), S.batch_jobs()
    strips = S.strip_table(jobs)
    assert len(strips) == 7 and [s[3:] for s in strips] == [(128, 640)] * 5 + [(640, 128)] * 2
    assert strips[0] == (0, 512, 0, 128, 640) and strips[6] == (2, 0, 0, 640, 128)
    C = [len(oracle.surf_detect(S.strip_pixels(tiles, s))) for s in strips]
    assert C == [2183, 2143, 2412, 2175, 2157, 2232, 3542], C
    assert max(C[:6]) + 1000 < C[6] and C[6] >= S.SORT_BUCKETS and C[6] <= 128 * 640 // 24 + 4096


def test_retry_path_counts(oracle):
    """test e: pair 0's strips are sparse, the strips of pairs 1 and 2 hold more candidates than the capacity learnt from pair 0
    (1.5 x seen + 1024) and fewer than the default capacity the retry falls back to; every pair registers at its first candidate, so the
    chain is two batches: pair 0 alone (slow start), then pairs 1 and 2"""
    tiles = S.retry_tiles()
    log = []
    ref = ChainRef(S.retry_attempts(oracle, tiles, log), [t.shape for t in tiles], 0.2, 1, 16)
    table, d = ref.chain(0, 3, 1)
    assert table.tolist() == [[1, 544, 0, 1, 1, 58], [1, 544, 0, 1, 1, 1780], [1, 544, 0, 1, 1, 1737]] and d == 1
    assert log == [(0, 1, 1), (1, 1, 1), (2, 1, 1)] and ref.stats == dict(attempts=3, batches=2)
    row0 = S.retry_attempts(oracle, tiles)([(0, 1, 1)])[0]
    seen = max(row0[4], row0[5])
    learnt = int(seen * 1.5) + 1024
    C = []
    for p in range(3):
        ra, rb = S._rect(tiles[p].shape, 1, True), S._rect(tiles[p + 1].shape, 1, False)
        C.append((len(oracle.surf_detect(np.ascontiguousarray(tiles[p][ra[0]:ra[0] + ra[2]]))),
                  len(oracle.surf_detect(np.ascontiguousarray(tiles[p + 1][rb[0]:rb[0] + rb[2]])))))
    assert C == [(117, 139), (3533, 3581), (3579, 3595)], C
    assert max(C[0]) <= learnt                                   # the learnt capacity holds pair 0 itself
    assert min(C[1] + C[2]) > learnt, (C, learnt)                # ... and none of the dense strips
    assert max(C[1] + C[2]) <= 128 * 640 // 24 + 4096
    # the image that shows afterwards that no chain left its capacity behind: more candidates than the largest capacity a chain can have
    # learnt (1.5 x the largest strip + 1024), fewer than its own default
    n = len(S.oracle_detect("lattice_large"))
    assert int(max(C[1] + C[2]) * 1.5) + 1024 < n <= 300 * 400 // 24 + 4096
    # the chain over pairs 1 and 2 alone ENDS under a learnt capacity: pair 1 runs alone at the default (slow start), and what it teaches
    # holds pair 2's strips, so the second and last batch neither overflows nor resets anything on its way
    log = []
    ref = ChainRef(S.retry_attempts(oracle, tiles, log), [t.shape for t in tiles], 0.2, 1, 16)
    table12, d = ref.chain(1, 3, 1)
    assert table12.tolist() == table.tolist()[1:] and d == 1 and log == [(1, 1, 1), (2, 1, 1)] and ref.stats == dict(attempts=2, batches=2)
    row1 = S.retry_attempts(oracle, tiles)([(1, 1, 1)])[0]
    learnt12 = int(max(row1[4], row1[5]) * 1.5) + 1024
    assert max(C[2]) <= learnt12 < n, (C, learnt12, n)


# ---- GridRegistrar._surf_batch: only VFSMS_ERR_CAPACITY is an overflow ------------------------------------------------------------------
class _BatchEngine:
    """answers fused batches with rows of 100 keypoints; `fail` (an exception or None) is raised by the first batch that runs under a
    learnt capacity"""

    def __init__(self, fail):
        self.fail, self.calls, self.caps = fail, 0, []

    @staticmethod
    def surf_params(*a, **k):
        return None

    def set_keypoint_capacity(self, n):
        self.caps.append(int(n))

    def attempt_surf_batch(self, jobs, params=None, ratio=0.75, offset_evaluate=3):
        self.calls += 1
        if self.fail is not None and self.caps and self.caps[-1] > 0:
            fail, self.fail = self.fail, None
            raise fail
        out = np.zeros((len(jobs), 8), np.int32)
        out[:] = [1, 7, -3, 5, 100, 100, 10, 0]
        return out


JOB = [(0, 1, 512, 0, 0, 0, 128, 640)]


def _primed(fail):
    eng = _BatchEngine(fail)
    reg = GridRegistrar(eng, roiRatio=0.2)
    reg._surf_batch(JOB)                                          # learns 1.5 x 100 + 1024
    assert reg._kp_cap == 1174 and eng.calls == 1 and eng.caps == []
    return eng, reg


def test_surf_batch_retries_a_capacity_overflow_once():
    eng, reg = _primed(VfsmsError("libvfsms error -2: attempt_surf: strip 0 of 2 exceeded 1174 keypoint candidates", code=VFSMS_ERR_CAPACITY))
    rows = reg._surf_batch(JOB)
    assert rows[0, 0] == 1 and eng.calls == 3                     # the failed batch and its repeat
    assert reg.capacity_retries == 1
    assert eng.caps == [1174, 0, 0] and eng.caps[-1] == 0         # the repeat ran at the library default, which is left in force
    assert reg._kp_cap == 1174                                    # learnt again from the repeat's rows


@pytest.mark.parametrize("fail", [VfsmsError("libvfsms error -3: hip: an illegal memory access was encountered", code=-3),
                                  VfsmsError("libvfsms error -1: attempt_surf: bad arguments", code=-1),
                                  VfsmsError("no code at all"), RuntimeError("the engine's own")],
                         ids=["hip", "bad_arg", "no_code", "runtime_error"])
def test_surf_batch_passes_every_other_error_on(fail):
    eng, reg = _primed(fail)
    with pytest.raises(type(fail)) as caught:
        reg._surf_batch(JOB)
    assert caught.value is fail
    assert eng.calls == 2                                         # nothing was started behind the error
    assert getattr(reg, "capacity_retries", 0) == 0
    assert eng.caps == [1174, 0]                                  # the override was taken back on the way out
    assert reg._kp_cap == 1174                                    # what was learnt stays: the error said nothing about the capacity


def test_vfsms_error_carries_the_return_code():
    assert VfsmsError("x").code is None and VfsmsError("x", code=-2).code == VFSMS_ERR_CAPACITY and str(VfsmsError("x", code=-2)) == "x"
