"""Inputs that drive the SURF candidate path to its fixed-size lists, and the oracle-side arithmetic that proves they do.

Nothing here runs the library: images are built with numpy, and every figure the tests rely on (candidates per k_nms workgroup, candidate
counts C, the counts of the retry grid) comes from the CPU oracle.  tests/test_surf_limits_host.py asserts those figures without a GPU;
tests/test_surf_limits_gpu.py runs the same images through the kernels.

The constants restate the #defines NMS_RW, NMS_TW, NMS_TH, NMS_LOCAL and SORT_BUCKETS of imagestitch_amd/csrc/surf_kernels.hip;
kernel_defines() reads them from the source and tests/test_surf_limits_host.py holds the two together.
"""
import functools
import os
import re

import numpy as np

NMS_RW = 32
NMS_TW = 62
NMS_TH = 4 * NMS_RW
NMS_LOCAL = 192
SORT_BUCKETS = 1024

STOCK = (100.0, 4, 3)          # hessianThreshold, nOctaves, nOctaveLayers of SURF_create()


def kernel_defines():
    """{name: the text behind `#define name`} of the five constants above, from surf_kernels.hip (comments stripped)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "imagestitch_amd", "csrc", "surf_kernels.hip")
    with open(path) as f:
        src = f.read()
    out = {}
    for name in ("NMS_RW", "NMS_TW", "NMS_TH", "NMS_LOCAL", "SORT_BUCKETS"):
        m = re.findall(r"^#define %s[ \t]+(.*?)[ \t]*(?://.*)?$" % name, src, re.M)
        assert len(m) == 1, (name, m)
        out[name] = m[0]
    return out


def _rand_img(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def periodic(seed, shape):
    """A 32 x 32 random block tiled over `shape` (tests/test_candidate_path_gpu.py's _periodic): exact response ties."""
    block = _rand_img(seed, (32, 32))
    return np.ascontiguousarray(np.tile(block, ((shape[0] + 31) // 32, (shape[1] + 31) // 32))[:shape[0], :shape[1]])


def lattice(h, w, period, radius, amp=200, floor=20):
    """uint8 image of Gaussian dots (sigma = radius px, peak amp above floor) on a square lattice of `period` px: a grid, an etch pattern,
    a calibration target.  Separable, so it costs h + w exponentials per lattice line."""
    def line(n):
        x = np.arange(n, dtype=np.float64)[:, None]
        c = np.arange(period / 2.0, n + period, period, dtype=np.float64)[None, :]
        return np.exp(-((x - c) ** 2) / (2.0 * radius * radius)).sum(1)
    img = floor + amp * line(h)[:, None] * line(w)[None, :]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def lattice_over(base, period, radius, amp=120):
    """the dots of lattice() ADDED to `base` (saturating): dense candidates on a texture that stays unique, so that offsets stay decidable"""
    dots = lattice(base.shape[0], base.shape[1], period, radius, amp=amp, floor=0).astype(np.int32)
    return np.clip(base.astype(np.int32) + dots, 0, 255).astype(np.uint8)


# ---- the layer pyramid (oracle/vfsms_oracle.c fast_hessian; surf_kernels.hip LayerPat) ------------------------------------------------
def layer_table(params=STOCK):
    """[(octave, layer in octave, size, step)] in layer-index order: size = (9 + 6 l) << o, step = 1 << o, n_layers + 2 layers per octave"""
    _thr, n_octaves, n_layers = params
    return [(o, l, (9 + 6 * l) << o, 1 << o) for o in range(n_octaves) for l in range(n_layers + 2)]


def layer_margin(tab, li):
    """findMaximaInLayer's margin of layer li, in cells: (size of the layer above / 2) / step + 1"""
    return (tab[li + 1][2] // 2) // tab[li][3] + 1


def det_layers(oracle, img, params=STOCK):
    """{layer index: float32 determinant layer} from the oracle's own layer routine"""
    s = oracle.integral(np.ascontiguousarray(img))
    return {li: oracle.surf_layer(s, size, step)[0] for li, (_o, _l, size, step) in enumerate(layer_table(params))}


def candidates(kps, layers, params=STOCK, with_nearest=False):
    """(octave, layer, i, j) of every detect-only keypoint of the oracle -> int64[n, 4] (layer = 1 .. n_layers inside the octave).

    A candidate of cell (i, j) of a middle layer starts at x = step (j - (size / 2) / step) + (size - 1) / 2, likewise y, and size = the
    layer's; interpolate_keypoint then moves x and y by at most ONE step and size by at most one layer spacing (it accepts |offset| <= 1,
    not 1 / 2).  The nearest cell of the nearest middle layer is therefore a first guess only, and sometimes the neighbour.  The
    candidate's cell is the one among the 27 cells around the guess whose determinant in `layers` (det_layers) IS the keypoint's response
    and whose centre lies within one step and one layer spacing of the keypoint: asserted unique for every keypoint.
    with_nearest: -> (cells, first guesses), for the test that shows the two differ."""
    _thr, n_octaves, n_layers = params
    tab = layer_table(params)
    lpo = n_layers + 2
    out = np.zeros((len(kps), 4), np.int64)
    nearest = np.zeros((len(kps), 4), np.int64)
    for n, k in enumerate(kps):
        o = int(k["octave"])
        step = 1 << o
        ds = 6 << o

        def centre(l, i, j):
            size = tab[o * lpo + l][2]
            return (step * (j - (size // 2) // step) + (size - 1) * 0.5, step * (i - (size // 2) // step) + (size - 1) * 0.5, size)

        l0 = int(np.clip(round((float(k["size"]) / (1 << o) - 9.0) / 6.0), 1, n_layers))
        size0 = tab[o * lpo + l0][2]
        j0 = int(round((float(k["x"]) - (size0 - 1) * 0.5) / step)) + (size0 // 2) // step
        i0 = int(round((float(k["y"]) - (size0 - 1) * 0.5) / step)) + (size0 // 2) // step
        nearest[n] = (o, l0, i0, j0)
        hits = []
        for l in range(max(1, l0 - 1), min(n_layers, l0 + 1) + 1):
            det = layers[o * lpo + l]
            for i in range(i0 - 1, i0 + 2):
                for j in range(j0 - 1, j0 + 2):
                    if not (0 <= i < det.shape[0] and 0 <= j < det.shape[1]) or det[i, j] != k["response"]:
                        continue
                    cx, cy, cs = centre(l, i, j)
                    if abs(float(k["x"]) - cx) <= step and abs(float(k["y"]) - cy) <= step and abs(float(k["size"]) - cs) <= ds:
                        hits.append((o, l, i, j))
        assert len(hits) == 1, ("keypoint %d does not name one cell" % n, k, hits)
        out[n] = hits[0]
    assert len(np.unique(out, axis=0)) == len(out), "two keypoints of one cell"
    return (out, nearest) if with_nearest else out


def block_counts(cand, shape, params=STOCK):
    """{(octave, layer, by, bx): candidates} per k_nms workgroup.

    Restates the tile geometry at the head of k_nms (surf_kernels.hip; its `margin`, `i0`, `j0`, `ia`, `thr`): a workgroup of layer li
    evaluates the rows i0 .. i0 + NMS_TH - 1 with i0 = margin + by * NMS_TH (four waves of NMS_RW rows each) and the columns
    j0 + 1 .. j0 + NMS_TW with j0 = margin - 1 + bx * NMS_TW (lanes 1 .. NMS_TW of a wave; lanes 0 and 63 are halo),
    margin = (size of the layer above / 2) / step + 1.  All candidates of one workgroup go through its one `local[NMS_LOCAL]` list; the
    ones that find it full append to the ROI's list directly."""
    tab = layer_table(params)
    lpo = params[2] + 2
    out = {}
    for o, l, i, j in cand:
        m = layer_margin(tab, int(o) * lpo + int(l))
        assert i >= m and j >= m and i < shape[0] // (1 << o) - m and j < shape[1] // (1 << o) - m, "candidate outside the evaluated cells"
        key = (int(o), int(l), int((i - m) // NMS_TH), int((j - m) // NMS_TW))
        out[key] = out.get(key, 0) + 1
    return out


def fullest_block(cand, shape, params=STOCK):
    """the largest candidate count of one k_nms workgroup (block_counts)"""
    c = block_counts(cand, shape, params)
    return max(c.values()) if c else 0


# ---- the images of the tests ------------------------------------------------------------------------------------------------------------
# name -> image; every lattice case must fill a k_nms workgroup's list (fullest_block > NMS_LOCAL), the noise and periodic cases must not
def case_image(name):
    if name == "lattice":              # 200 x 320: full blocks next to partial ones in both directions on octave 0 (286 x 166 evaluated cells of layer 3)
        return lattice(200, 320, 6, 1.5)
    if name == "lattice_width":        # layer 3 of octave 0 evaluates 166 columns: two full 62-column blocks and a partial one of 42
        return lattice(160, 200, 6, 1.5)
    if name == "lattice_height":       # ... and 266 rows: two full 128-row blocks and a partial one of 10
        return lattice(300, 90, 6, 1.5)
    if name == "lattice_view":         # a column slice of a wider tile: rows are not contiguous
        return lattice(200, 400, 6, 1.5)[:, 400 - 320:]
    if name == "lattice_small":        # few enough candidates for a capacity below SORT_BUCKETS (the rank sort), one full block
        return lattice(170, 100, 6, 1.5)
    if name == "lattice_large":        # more candidates than any capacity the retry chains of test e learn, fewer than the operator's default
        return lattice(300, 400, 6, 1.5)
    if name == "noise":
        return _rand_img(4, (90, 150))
    if name == "periodic":
        return periodic(7, (90, 150))
    raise KeyError(name)


LATTICE_CASES = ("lattice", "lattice_width", "lattice_height", "lattice_view", "lattice_small")


@functools.lru_cache(maxsize=None)
def oracle_detect(name):
    """the oracle's detect-only keypoints of case_image(name): computed once, shared, never modified (read-only array)"""
    from oracle import oracle as O
    k = O.surf_detect(np.ascontiguousarray(case_image(name)))
    k.setflags(write=False)
    return k


# ---- the fused batch of test d: four 640 x 640 tiles of one white-noise field, 64 px of overlap, on the path down, right, up --------------
BATCH_TILE, BATCH_STEP = 640, 576
BATCH_ORIGINS = ((0, 0), (BATCH_STEP, 0), (BATCH_STEP, BATCH_STEP), (0, BATCH_STEP))


@functools.lru_cache(maxsize=None)
def batch_tiles():
    """tiles 0 .. 3; the left 640 x 128 strip of tile 2 carries the dot lattice on top of its texture (far more candidates than any other strip)"""
    field = _rand_img(31, (BATCH_STEP + BATCH_TILE, BATCH_STEP + BATCH_TILE))
    tiles = [np.ascontiguousarray(field[y:y + BATCH_TILE, x:x + BATCH_TILE]) for y, x in BATCH_ORIGINS]
    tiles[2][:, :128] = lattice_over(tiles[2][:, :128], 6, 1.5, amp=200)
    for t in tiles:
        t.setflags(write=False)
    return tuple(tiles)


def _rect(shape, direction, first, ratio=0.2):
    """(y0, x0, h, w) of Method.getROIRegionForIncreMethod, restated (imagestitch_amd.utility.roi_rect; csrc/grid.hip roi_rect)"""
    row, col = shape
    if direction in (1, 3):
        n = int(np.floor(row * ratio)); at_end = (direction == 1) == first
        return (row - n if at_end else 0, 0, n, col)
    n = int(np.floor(col * ratio)); at_end = (direction == 2) == first
    return (0, col - n if at_end else 0, row, n)


def batch_jobs():
    """[(tile a, tile b, direction)] -> jobs as (a, b, ay0, ax0, by0, bx0, h, w) over tile INDICES: two column-strip jobs down and up, one
    turn-strip job, and a fourth job that shares tile 0's bottom strip with the first"""
    out = []
    for a, b, d in ((0, 1, 1), (1, 2, 2), (2, 3, 3), (0, 3, 1)):
        ra, rb = _rect((BATCH_TILE, BATCH_TILE), d, True), _rect((BATCH_TILE, BATCH_TILE), d, False)
        assert ra[2:] == rb[2:]
        out.append((a, b, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]))
    return out


def strip_table(jobs):
    """the distinct strips of a fused batch in the library's order (api.hip shape_order + build_strip_table): jobs in the stable (h, w)
    order, A strip then B strip, a strip listed where it is first used -> [(tile, y0, x0, h, w)]"""
    strips = []
    for j in sorted(jobs, key=lambda j: (j[6], j[7])):
        for s in ((j[0], j[2], j[3], j[6], j[7]), (j[1], j[4], j[5], j[6], j[7])):
            if s not in strips:
                strips.append(s)
    return strips


def strip_pixels(tiles, s):
    t, y0, x0, h, w = s
    return np.ascontiguousarray(tiles[t][y0:y0 + h, x0:x0 + w])


_FEATURE_CACHE = {}            # (shape, pixels, extended) -> the oracle's (keypoints, descriptors): a strip is described once per process


def oracle_row(oracle, a, b, extended=False, ratio=0.75, offset_evaluate=3):
    """the evaluator row [status, dx, dy, votes, nA, nB, nMatches] of strips a, b by the oracle's operator chain (as
    tests/test_gpu_parity.py::test_fused_attempt_equals_operator_chain_and_oracle)"""
    def feats(img):
        key = (img.shape, img.tobytes(), bool(extended))
        if key not in _FEATURE_CACHE:
            _FEATURE_CACHE[key] = oracle.surf_detect_describe(img, extended=extended)
        return _FEATURE_CACHE[key]
    ka, da = feats(a); kb, db = feats(b)
    if len(ka) == 0 or len(kb) == 0:
        return [0, 0, 0, 0, len(ka), len(kb), 0]
    pairs = oracle.bf_l2_ratio_matches(da, db, ratio)
    if len(pairs) == 0:
        return [0, 0, 0, 0, len(ka), len(kb), 0]
    st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, offset_evaluate)
    return [int(st), int(off[0]), int(off[1]), int(votes), len(ka), len(kb), len(pairs)]


# ---- the path of test e: four 640 x 640 tiles in one column, 96 rows of overlap; sparse blobs above, lattice over noise below ----------------
RETRY_TILE, RETRY_STEP = 640, 544


def blob_field(seed, h, w, n):
    """flat 60 plus n Gaussian blobs (sigma 2 .. 5 px, 60 .. 180 grey levels) at random places: few keypoints, every one unique"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 60.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n):
        cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, 5), rng.uniform(60, 180)
        y0, y1, x0, x1 = max(0, int(cy - 20)), min(h, int(cy + 21)), max(0, int(cx - 20)), min(w, int(cx + 21))
        img[y0:y1, x0:x1] += a * np.exp(-((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def retry_tiles():
    """Tile k = rows 544 k .. 544 k + 639 of one field.  The field is sparse down to the row where tile 1's bottom strip begins and dense
    (dot lattice over white noise) from there: pair 0's strips are sparse, the strips of pairs 1 and 2 are dense."""
    H = 3 * RETRY_STEP + RETRY_TILE
    dense_from = RETRY_STEP + RETRY_TILE - 128
    field = blob_field(17, H, RETRY_TILE, 900)
    field[dense_from:] = lattice_over(_rand_img(19, (H - dense_from, RETRY_TILE)), 6, 1.5, amp=200)
    tiles = [np.ascontiguousarray(field[k * RETRY_STEP:k * RETRY_STEP + RETRY_TILE]) for k in range(4)]
    for t in tiles:
        t.setflags(write=False)
    return tuple(tiles)


def retry_attempts(oracle, tiles, log=None):
    """attempts(items) of tests/chain_ref.py over the oracle's operator chain: items [(pair, direction, i)] -> evaluator rows"""
    def attempts(items):
        rows = []
        for p, d, i in items:
            ra, rb = _rect(tiles[p].shape, d, True, i * 0.2), _rect(tiles[p + 1].shape, d, False, i * 0.2)
            a = np.ascontiguousarray(tiles[p][ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]])
            b = np.ascontiguousarray(tiles[p + 1][rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]])
            if log is not None:
                log.append((p, d, i))
            rows.append(oracle_row(oracle, a, b) + [0])
        return rows
    return attempts
