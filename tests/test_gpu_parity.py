"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (imagestitch_amd._lib.Engine ->
libvfsms.so), against the CPU oracle on the same seeded inputs and against the committed golden fixtures.

Bars: bit-exact for integer / index work (integral, keypoint set, match lists, votes, fuse bytes, offsets of
phase correlation) AND for the float32 SURF descriptors / ORB descriptor bytes (every float operation order, sin / cos
included, is replicated: imagestitch_amd/csrc/detmath.h); SURF offsets within +-1 px of Stitcher.py:87."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid

pytestmark = pytest.mark.gpu


def _rand_img(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _kp_fields(k):
    return np.stack([k["x"], k["y"], k["size"], k["response"], k["octave"].astype(np.float32), k["class_id"].astype(np.float32)], 1)


@pytest.fixture(scope="module")
def strips():
    g = SyntheticGrid(2, 2, 640)
    t = g.tiles(threads=1)
    return g, t


def test_integral_bit_exact(engine, oracle):
    for seed, shape in enumerate([(1, 1), (3, 5), (17, 300), (409, 2048), (300, 4200)]):
        img = _rand_img(seed, shape)
        assert np.array_equal(engine.integral(img), oracle.integral(img)), shape
    tile = _rand_img(9, (200, 333))
    view = tile[:, 333 - 66:]                                  # direction-2 ROI: non-contiguous view
    assert np.array_equal(engine.integral(view), oracle.integral(view))


def test_surf_keypoints_bit_exact(engine, oracle, strips):
    g, tiles = strips
    for img in (tiles[0][-128:, :], tiles[1][:, :128], _rand_img(4, (90, 150))):
        a = engine.surf_detect(img)
        b = oracle.surf_detect(np.ascontiguousarray(img))
        assert len(a) == len(b) and len(a) > 50
        assert np.array_equal(_kp_fields(a), _kp_fields(b))


def test_surf_describe_matches_oracle(engine, oracle, strips):
    g, tiles = strips
    for extended in (False, True):
        img = np.ascontiguousarray(tiles[0][-128:, :])
        p = engine.surf_params(extended=extended)
        kxy, desc, kfull = engine.surf_detect_describe(img, p, full=True)
        ko, do = oracle.surf_detect_describe(img, extended=extended)
        assert len(kfull) == len(ko) and desc.shape == do.shape
        assert np.array_equal(_kp_fields(kfull), _kp_fields(ko))
        assert np.array_equal(kfull["angle"], ko["angle"])             # orientation is fully replicated arithmetic
        assert np.array_equal(kxy, np.stack([ko["x"], ko["y"]], 1))
        err = np.abs(desc - do).max(1)
        print("descriptor parity: n=%d exact=%.4f max_abs_err=%.3g" % (len(err), (err == 0).mean(), err.max()))
        assert np.array_equal(desc, do)                                # sin / cos of the window rotation are replicated too (detmath.h)


def test_surf_edge_cases(engine, oracle):
    flat = np.full((64, 200), 90, np.uint8)
    kxy, desc = engine.surf_detect_describe(flat)
    assert len(kxy) == 0 and desc.shape == (0, 64)
    tiny = _rand_img(2, (8, 8))                                        # smaller than the first Haar wavelet
    assert len(engine.surf_detect_describe(tiny)[0]) == 0
    thin = _rand_img(3, (40, 700))                                     # only octave 0 fits
    a = engine.surf_detect_describe(thin, full=True)[2]; b = oracle.surf_detect_describe(thin)[0]
    assert np.array_equal(_kp_fields(a), _kp_fields(b))
    engine.set_keypoint_capacity(16)
    with pytest.raises(isa.VfsmsError):
        engine.surf_detect_describe(_rand_img(5, (128, 128)))
    engine.set_keypoint_capacity(0)


def test_bf_l2_bit_exact(engine, oracle):
    rng = np.random.default_rng(11)
    for nq, nt, dim in [(1, 1, 64), (5, 2, 64), (300, 700, 64), (1500, 1300, 64), (200, 333, 128)]:
        q = rng.normal(size=(nq, dim)).astype(np.float32); t = rng.normal(size=(nt, dim)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True); t /= np.linalg.norm(t, axis=1, keepdims=True)
        if nt > 20:
            t[17] = t[4]; q[0] = t[4]                                  # duplicates: ties -> lower train index
        i1, d1, d2 = engine.bf_l2_knn2(q, t)
        oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
        assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2), (nq, nt, dim)
        assert np.array_equal(engine.bf_l2_ratio_matches(q, t, 0.75), oracle.bf_l2_ratio_matches(q, t, 0.75))
    assert engine.bf_l2_ratio_matches(np.zeros((0, 64), np.float32), np.zeros((4, 64), np.float32)).shape == (0, 2)


def test_bf_l2_mfma_filter_hard_cases(engine, oracle):
    """Descriptors of norm <= 1 go through the MFMA candidate filter + exact verification; the result must stay bit-identical
    to the exhaustive reference arithmetic on inputs built to stress the filter: tight clusters (many near-ties inside the
    filter margin), exact duplicates, zero rows, more trains than one split, and sizes of the 2048-px workload."""
    rng = np.random.default_rng(23)

    def unit(a):
        n = np.linalg.norm(a, axis=1, keepdims=True); n[n == 0] = 1
        return (a / n).astype(np.float32)

    cases = []
    centres = unit(rng.normal(size=(40, 64)))
    t = unit(centres[rng.integers(0, 40, 3000)] + 1e-3 * rng.normal(size=(3000, 64)))       # clusters of radius ~1e-3
    q = unit(centres[rng.integers(0, 40, 2500)] + 1e-3 * rng.normal(size=(2500, 64)))
    cases.append((q, t))
    t2 = unit(rng.normal(size=(5000, 64))); q2 = unit(rng.normal(size=(700, 64)))
    t2[100] = 0; t2[4000] = 0; q2[5] = 0                                                    # zero descriptors (flat patches)
    t2[77] = t2[4100]; t2[78] = t2[4100]; q2[6] = t2[4100]                                  # triple tie at distance 0
    q2[7] = np.float32(0.5) * q2[8]                                                         # norm < 1
    cases.append((q2, t2))
    cases.append((unit(rng.normal(size=(9000, 64))), unit(rng.normal(size=(8300, 64)))))    # ~ the keypoint counts of a 409 x 2048 ROI
    cases.append((unit(rng.normal(size=(130, 64))), unit(rng.normal(size=(33, 64)))))       # one partial second tile
    cases.append((unit(rng.normal(size=(3, 64))), unit(rng.normal(size=(2, 64)))))
    for q, t in cases:
        i1, d1, d2 = engine.bf_l2_knn2(q, t)
        oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
        assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2), (q.shape, t.shape)
        assert np.array_equal(engine.bf_l2_ratio_matches(q, t, 0.75), oracle.bf_l2_ratio_matches(q, t, 0.75))
    # norms > 1 must take the exhaustive kernel and still agree
    q = (3 * rng.normal(size=(400, 64))).astype(np.float32); t = (3 * rng.normal(size=(900, 64))).astype(np.float32)
    i1, d1, d2 = engine.bf_l2_knn2(q, t)
    oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
    assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2)


def test_mode_vote_golden(engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "mode_cases.npz"))
    for i, (ev, st, dx, dy) in enumerate(g["expected"]):
        s, off, _v = engine.mode_offset(g["c%d_kpsA" % i], g["c%d_kpsB" % i], g["c%d_pairs" % i], ev)
        assert (int(s), off[0], off[1]) == (st, dx, dy), i


def test_phase_correlation_offsets_bit_exact(engine, oracle, strips):
    g, tiles = strips
    cases = [(tiles[0][-128:, :], tiles[1][:128, :]), (tiles[0][:, -128:], tiles[2][:, :128]),
             (_rand_img(1, (97, 131)), _rand_img(2, (97, 131))), (_rand_img(3, (625, 64)), _rand_img(4, (625, 64)))]
    a = _rand_img(7, (80, 96)); cases.append((a, np.roll(np.roll(a, 7, 0), -5, 1)))
    for a, b in cases:
        (x, y), r = engine.phase_correlate(a, b)
        (ox, oy), orr = oracle.phase_correlate(np.ascontiguousarray(a), np.ascontiguousarray(b))
        assert abs(x - ox) < 1e-6 and abs(y - oy) < 1e-6 and abs(r - orr) < 1e-9
        # what Stitcher.py:231-232 keeps: int() of the sub-pixel peak.  An exact circular shift (the last case) puts the peak ON an integer to
        # within the rounding of whichever FFT computed the surface (oracle 6.999999999999993, rocFFT 6.99999999999999, the LDS transforms
        # 7.000000000000000): truncation is decided by the last bit there and is compared only where the oracle is 1e-9 away from an integer
        for v, ov in ((y, oy), (x, ox)):
            if abs(ov - round(ov)) > 1e-9:
                assert int(v) == int(ov), (a.shape, (x, y), (ox, oy))
            else:
                assert abs(v - round(ov)) < 1e-9


def test_fuse_fade_golden_bit_exact(engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    for i, (dx, dy, _c) in enumerate(g["meta"]):
        out = engine.fuse_fade_i64(g["f%d_A" % i], g["f%d_B" % i], dx, dy)
        assert np.array_equal(out, g["f%d_out" % i]), i


def test_get_stitch_by_offset_golden_bit_exact(engine, golden_dir, tmp_path):
    """device canvas (u8 + validity) vs the reference's int64/-1 canvas walk, all fuse modes, gray + colour"""
    from test_host_logic import FUSE_NAMES, _write_tiles
    g = np.load(os.path.join(golden_dir, "stitch_cases.npz"))
    for n, (color, fm, _) in enumerate(g["meta"]):
        files = _write_tiles(tmp_path, list(g["s%d_tiles" % n]), "g%d" % n)
        s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False
        s.isColorMode = bool(color); isa.Stitcher.isColorMode = bool(color)
        s.fuseMethod = FUSE_NAMES[fm]
        res = s.getStitchByOffset(files, [list(map(int, o)) for o in g["s%d_offsets" % n]])
        if s.fuseMethod == "trigonometric":
            # the device evaluates sin^2 with its own explicit double-precision routine; the reference's bytes hang on numpy's SIMD sin in
            # the last ulp (wA * a + (1 - wA) * a sits ON an integer when both sides agree): tolerance = one grey level on < 0.1 % of the bytes
            ref = g["s%d_out" % n]
            d = np.abs(res.astype(np.int16) - ref.astype(np.int16))
            assert res.shape == ref.shape and d.max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size, (n, color, int(d.max()), np.count_nonzero(d), d.size)
            continue
        assert np.array_equal(res, g["s%d_out" % n]), (n, FUSE_NAMES[fm], color)
        if s.fuseMethod in ("notFuse", "fadeInAndFadeOut"):
            # streamed write-out (vfsms_canvas_download_rows): the bands of the same mosaic, 7 rows at a time, through NpyBandWriter
            path = os.path.join(str(tmp_path), "mosaic%d.npy" % n)
            s.mosaicSink = isa.NpyBandWriter(path); s.mosaicBandRows = 7
            assert s.getStitchByOffset(files, [list(map(int, o)) for o in g["s%d_offsets" % n]]) is None
            assert np.array_equal(np.load(path), g["s%d_out" % n]), (n, "streamed")
    isa.Stitcher.isColorMode = True


def test_colour_tiles_are_rejected_by_registration(engine):
    """vfsms_tile_upload_ch handles are for the mosaic canvas; the registration entry points take single-channel tiles only."""
    rng = np.random.default_rng(5)
    c = rng.integers(0, 255, (64, 80, 3), dtype=np.uint8)
    hc = engine.tile_upload_color(c)
    hg = engine.tile_upload(np.ascontiguousarray(c[:, :, 0]))
    with pytest.raises(isa.VfsmsError):
        engine.attempt_surf_batch([(hc, hg, 0, 0, 0, 0, 32, 80)])
    engine.tile_free(hc); engine.tile_free(hg)


def test_fused_attempt_equals_operator_chain_and_oracle(engine, oracle, strips):
    g, tiles = strips
    offs, dirs = g.true_offsets(), g.true_directions()
    for k in range(g.n_pairs):
        A, B, d = tiles[k], tiles[k + 1], dirs[k]
        ra = isa.roi_rect(A.shape, d, "first", 0.2); rb = isa.roi_rect(B.shape, d, "second", 0.2)
        ha, hb = engine.tile_upload(A), engine.tile_upload(B)
        row = engine.attempt_surf_batch([(ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])])[0]
        engine.tile_free(ha); engine.tile_free(hb)
        roiA = np.ascontiguousarray(A[ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]])
        roiB = np.ascontiguousarray(B[rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]])
        ka, da = oracle.surf_detect_describe(roiA); kb, db = oracle.surf_detect_describe(roiB)
        pairs = oracle.bf_l2_ratio_matches(da, db, 0.75)
        st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 3)
        assert list(row[:7]) == [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)], (k, row)


def test_stitcher_on_real_strips_within_one_pixel(engine, golden_dir):
    """Stitcher.py:87 is the reference's own ground truth; ROI strips of the real dendriticCrystal tiles."""
    g = np.load(os.path.join(golden_dir, "real_strips.npz"))
    for n, (a, b, direction, H, W, gdx, gdy) in enumerate(g["meta"]):
        ra, rb = g["r%d_roiA" % n], g["r%d_roiB" % n]
        ha, hb = engine.tile_upload(ra), engine.tile_upload(rb)
        row = engine.attempt_surf_batch([(ha, hb, 0, 0, 0, 0, ra.shape[0], ra.shape[1])])[0]
        engine.tile_free(ha); engine.tile_free(hb)
        off = [int(row[1]), int(row[2])]
        if direction == 1: off[0] += H - int(0.2 * H)
        if direction == 3: off[0] -= H - int(0.2 * H)
        if direction == 2: off[1] += W - int(0.2 * W)
        assert row[0] == 1 and abs(off[0] - gdx) <= 1 and abs(off[1] - gdy) <= 1, (a, b, off)


def test_incremental_search_end_to_end_on_synthetic_grid(engine):
    """calculateOffsetForFeatureSearchIncre with the direction rotation across a serpentine turn: offsets
    within +-1 px of the exact ground truth, and the phase path bit-exact vs truth on its own quirk-free case."""
    g = SyntheticGrid(2, 2, 640)
    tiles = g.tiles(threads=1)
    s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False
    s.roiRatio = 0.2; s.direction = 1; s.directIncre = 1; s.featureMethod = "surf"
    for k, truth in enumerate(g.true_offsets()):
        status, off = s.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
        assert status and abs(off[0] - truth[0]) <= 1 and abs(off[1] - truth[1]) <= 1, (k, off, truth)
    assert s.direction == g.true_directions()[-1]


def test_orb_bit_exact_vs_oracle(engine, oracle, strips):
    g, tiles = strips
    for img in (np.ascontiguousarray(tiles[0][-128:, :]), tiles[1][:, :128], _rand_img(8, (150, 200)), np.full((100, 100), 7, np.uint8)):
        kxy, desc, kfull = engine.orb_detect_describe(img, full=True)
        ko, do = oracle.orb_detect_describe(np.ascontiguousarray(img))
        assert len(kfull) == len(ko), (img.shape, len(kfull), len(ko))
        if len(ko) == 0:
            continue
        for f in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(kfull[f], ko[f]), f
        assert np.array_equal(kxy, np.stack([ko["x"], ko["y"]], 1))
        assert np.array_equal(desc, do)                                  # cos / sin of the angle: one explicit algorithm on both sides
    p = engine.orb_params(nfeatures=300, nlevels=4)
    kxy, desc, kfull = engine.orb_detect_describe(np.ascontiguousarray(tiles[0][-128:, :]), p, full=True)
    ko, do = oracle.orb_detect_describe(np.ascontiguousarray(tiles[0][-128:, :]), nfeatures=300, nlevels=4)
    assert np.array_equal(kfull["x"], ko["x"]) and np.array_equal(desc, do)


def test_orb_fused_attempt_and_exact_truth(engine, oracle):
    # ORB keeps keypoints >= 31 px from the ROI border (runByImageBorder), so the shared band must be wider than
    # 62 px inside BOTH strips: 1024-px tiles with 15 % overlap (the 10 % / 640-px grid of the SURF tests is too thin)
    g = SyntheticGrid(2, 2, 1024, overlap=0.15)
    tiles = g.tiles(threads=1)
    for k, (truth, d) in enumerate(zip(g.true_offsets(), g.true_directions())):
        A, B = tiles[k], tiles[k + 1]
        ra = isa.roi_rect(A.shape, d, "first", 0.2); rb = isa.roi_rect(B.shape, d, "second", 0.2)
        ha, hb = engine.tile_upload(A), engine.tile_upload(B)
        row = engine.attempt_orb_batch([(ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])])[0]
        engine.tile_free(ha); engine.tile_free(hb)
        roiA = np.ascontiguousarray(A[ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]])
        roiB = np.ascontiguousarray(B[rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]])
        ka, da = oracle.orb_detect_describe(roiA); kb, db = oracle.orb_detect_describe(roiB)
        pairs, _ = oracle.bf_hamming_matches(da, db)
        st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 3)
        assert list(row[:7]) == [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)], (k, row)
    s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False
    s.roiRatio = 0.2; s.direction = 1; s.directIncre = 1; s.featureMethod = "orb"
    # the cv2 ORB path has neither ratio test nor distance threshold (ImageUtility.py:297-302): every query votes, so a wrong
    # direction collects 3 equal random votes now and then -- the reference's own fragility; 10 votes make the rotation safe
    s.offsetEvaluate = 10
    for k, truth in enumerate(g.true_offsets()):
        status, off = s.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
        assert status and off == truth, (k, off, truth)                  # bit-exact for ORB (north_star)
    a, b = engine.orb_detect_describe(tiles[0])[1], engine.orb_detect_describe(tiles[1])[1]
    assert np.array_equal(engine.bf_hamming_matches(a, b), oracle.bf_hamming_matches(a, b)[0])


def test_demo_strips_iron_and_zirconcl(engine, golden_dir):
    """BASELINE configs[0] / configs[3] on the real micrograph strips: phase-correlation offsets bit-exact against the fixture
    (integer parts as Stitcher.py:231-232 keeps them, sub-pixel peak within 1e-6), and the fused SURF attempt equal to the
    oracle's row (status, offset, votes, keypoint and match counts)."""
    import json
    meta = json.load(open(os.path.join(golden_dir, "demo_strips.json")))["cases"]
    g = np.load(os.path.join(golden_dir, "demo_strips.npz"))
    jobs = []
    for n, c in enumerate(meta):
        a, b = g["d%d_roiA" % n], g["d%d_roiB" % n]
        (x, y), r = engine.phase_correlate(a, b)
        assert [int(y), int(x)] == c["phase_int"], (n, (x, y), c["phase_xy"])
        assert abs(x - c["phase_xy"][0]) < 1e-6 and abs(y - c["phase_xy"][1]) < 1e-6 and abs(r - c["phase_response"]) < 1e-9
        ha, hb = engine.tile_upload(a), engine.tile_upload(b)
        rows = engine.attempt_surf_batch([(ha, hb, 0, 0, 0, 0, a.shape[0], a.shape[1])])
        s = c["surf"]
        assert rows[0].tolist()[:7] == [s["status"], s["offset"][0], s["offset"][1], s["votes"], s["nA"], s["nB"], s["matches"]], (n, rows[0], s)


def test_config0_iron_pair_end_to_end(engine, golden_dir):
    """BASELINE configs[0] through the reference's call surface: Stitcher.calculateOffsetForPhaseCorrleateIncre on the iron
    pair (direction 1, directIncre 0, roiRatio 0.2) returns the reference-as-written offset [1400, 0] that SURVEY 8d derives
    (phase correlation reports b - a and the reference adds it with the feature path's sign), and the SURF path returns
    [1699, 0], within 1 px of the true offset [1699, -1].  The 1936 x 2584 frames are rebuilt around the committed strips:
    both searches succeed at i = 1 and never look outside them."""
    import json
    c = json.load(open(os.path.join(golden_dir, "demo_strips.json")))["cases"][0]
    g = np.load(os.path.join(golden_dir, "demo_strips.npz"))
    H, W = c["shape"]
    A = np.zeros((H, W), np.uint8); B = np.zeros((H, W), np.uint8)
    A[H - g["d0_roiA"].shape[0]:, :] = g["d0_roiA"]; B[:g["d0_roiB"].shape[0], :] = g["d0_roiB"]
    st = isa.Stitcher()
    st._engine = engine
    st.isPrintLog = False
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate)
    try:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio = 1, 0, 0.2
        assert st.calculateOffsetForPhaseCorrleateIncre([A, B]) == (True, [1400, 0])
        isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = "surf", 3
        status, off = st.calculateOffsetForFeatureSearchIncre([A, B])
        assert status and abs(off[0] - 1699) <= 1 and abs(off[1] - (-1)) <= 1, off
    finally:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = old


def test_config4_tile_size_4096_pair(engine, oracle):
    """BASELINE configs[4] tile geometry (4096 x 4096 tiles -> 819 x 4096 strips, ~4x the keypoints of the 2048 case, window classes and
    ticket / capacity paths the 409-row strips never reach): one in-column pair and one turn pair through the grid registrar; offsets
    within 1 px of the synthetic ground truth, and the fused attempt row of the 819 x 4096 strips EQUAL TO THE ORACLE'S chain
    (surf_detect_describe -> bf_l2_ratio_matches -> mode_offset: status, offset, votes, keypoint and match counts), with the keypoints and
    descriptors of the strip themselves bit-identical to the oracle's."""
    from imagestitch_amd.grid import GridRegistrar
    g = SyntheticGrid(2, 2, 4096)
    tiles = g.tiles(threads=4)
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        reg = GridRegistrar(engine, method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1)
        table, _d = reg.register(hs, [t.shape for t in tiles], 1)
        truth = np.array(g.true_offsets())
        assert np.all(table[:, 0] == 1) and np.abs(table[:, 1:3] - truth).max() <= 1, (table, truth)
        ra = isa.roi_rect(tiles[0].shape, 1, "first", 0.2); rb = isa.roi_rect(tiles[1].shape, 1, "second", 0.2)
        assert ra[2:] == (819, 4096)
        row = engine.attempt_surf_batch([(hs[0], hs[1], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])])[0]
        A = np.ascontiguousarray(tiles[0][ra[0]:ra[0] + ra[2]]); B = np.ascontiguousarray(tiles[1][:rb[2]])
        ka, da = oracle.surf_detect_describe(A); kb, db = oracle.surf_detect_describe(B)
        assert len(ka) > 20000 and len(kb) > 20000
        pairs = oracle.bf_l2_ratio_matches(da, db, 0.75)
        st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 3)
        assert row[:7].tolist() == [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)], (row, st, off, votes, len(ka), len(kb), len(pairs))
        full = off[0] + 4096 - int(0.2 * 4096)
        assert st and abs(full - truth[0][0]) <= 1 and abs(off[1] - truth[0][1]) <= 1
        kx, dd, kf = engine.surf_detect_describe(A, full=True)
        assert np.array_equal(_kp_fields(kf), _kp_fields(ka)) and np.array_equal(kf["angle"], ka["angle"]) and np.array_equal(dd, da)
        assert np.array_equal(engine.bf_l2_ratio_matches(da, db, 0.75), pairs)
    finally:
        for h in hs:
            engine.tile_free(h)


def test_config3_zirconcl_phase_incremental(engine, golden_dir):
    """BASELINE configs[3]: zirconCL pairs (1024 x 1280, direction 4, directIncre 0, roiRatio 0.2) through
    Stitcher.calculateOffsetForPhaseCorrleateIncre.  Expected = the fixture's integer phase offsets plus the reference's axis
    correction for direction 4 (Stitcher.py:244-251: dy -= W - int(i * roiRatio * W)); the response gate is 0.15."""
    import json
    cases = json.load(open(os.path.join(golden_dir, "demo_strips.json")))["cases"][1:]
    g = np.load(os.path.join(golden_dir, "demo_strips.npz"))
    st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio)
    try:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio = 4, 0, 0.2
        for n, c in enumerate(cases, start=1):
            H, W = c["shape"]
            ra, rb = g["d%d_roiA" % n], g["d%d_roiB" % n]
            A = np.zeros((H, W), np.uint8); B = np.zeros((H, W), np.uint8)
            A[:, :ra.shape[1]] = ra; B[:, W - rb.shape[1]:] = rb            # direction 4: A's left strip against B's right strip
            assert c["phase_response"] > 0.15
            exp = [c["phase_int"][0], c["phase_int"][1] - (W - int(0.2 * W))]
            assert st.calculateOffsetForPhaseCorrleateIncre([A, B]) == (True, exp), (n, exp)
    finally:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio = old


def test_main_py_driver_end_to_end(engine, tmp_path):
    """The entry point Main.py uses: imageSetStitchWithMutiple(project, output, 1, stitcher.calculateOffsetForFeatureSearchIncre)
    on a folder of tiles (a 3 x 3 serpentine of 768-px synthetic tiles written as PNG).  The batched registration inside
    flowStitch and the pair-by-pair loop must log the same offsets, each within 1 px of the ground truth, and write the
    same mosaic file."""
    from PIL import Image
    g = SyntheticGrid(3, 3, 768, overlap=0.15)
    tiles = g.tiles(threads=2)
    proj = tmp_path / "demo"; (proj / "1").mkdir(parents=True)
    for k, t in enumerate(tiles):
        Image.fromarray(t).save(str(proj / "1" / ("1-%03d.png" % (k + 1))))
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod,
           isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate)
    outs = []
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode = 1, 0.2, False
        isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate = "surf", "fadeInAndFadeOut", 3
        for batched in (True, False):
            st = isa.Stitcher(); st._engine = engine; st.batchRegistration = batched
            isa.Stitcher.direction = 1; st.direction = 1
            msgs = []
            st.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
            out = tmp_path / ("out%d" % batched)
            st.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, st.calculateOffsetForFeatureSearchIncre,
                                         startNum=1, fileExtension="png", outputfileExtension="png")
            offs = [m for m in msgs if "offset of stitching" in m]
            outs.append((offs, np.asarray(Image.open(str(out / "stitching_result_1.png")))))
        assert outs[0][0] == outs[1][0] and len(outs[0][0]) == 8
        assert np.array_equal(outs[0][1], outs[1][1])
        truth = g.true_offsets()
        for line, t in zip(outs[0][0], truth):
            dx, dy = int(line.split("dx is ")[1].split(" ")[0]), int(line.split("dy is ")[1])
            assert abs(dx - t[0]) <= 1 and abs(dy - t[1]) <= 1, (line, t)
        assert outs[0][1].shape[0] > 2 * 768 and outs[0][1].shape[1] > 2 * 768
    finally:
        (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod,
         isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate) = old


def test_dll_mode_parameter_set(engine, oracle, strips):
    """Method.isGPUAvailable = True selects the reference's DLL parameter set (ImageUtility.py:22-40, 265-274, 304-308): SURF
    with extended (128-d) descriptors, whose 2-NN search runs on the exhaustive kernel, and ORB matches cut at
    orbMaxDistance = 30.  Fused attempts must equal the operator chain, and the Hamming cut must equal the oracle's."""
    g, tiles = strips
    ra = isa.roi_rect(tiles[0].shape, 1, "first", 0.2); rb = isa.roi_rect(tiles[1].shape, 1, "second", 0.2)
    A = np.ascontiguousarray(tiles[0][ra[0]:ra[0] + ra[2]]); B = np.ascontiguousarray(tiles[1][:rb[2]])
    ha, hb = engine.tile_upload(tiles[0]), engine.tile_upload(tiles[1])
    job = [(ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])]
    # SURF, extended descriptors
    p = engine.surf_params(100.0, 4, 3, True, False)
    row = engine.attempt_surf_batch(job, p, 0.75, 3)[0]
    ka, da = engine.surf_detect_describe(A, p); kb, db = engine.surf_detect_describe(B, p)
    assert da.shape[1] == 128
    pairs = engine.bf_l2_ratio_matches(da, db, 0.75)
    assert np.array_equal(pairs, oracle.bf_l2_ratio_matches(da, db, 0.75))
    st, off, votes = engine.mode_offset(ka, kb, pairs, 3)
    assert row[:7].tolist() == [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)], (row, st, off, votes)
    # ... and the ORACLE's row for the same parameter set (surfIsExtended = True, ImageUtility.py:22-28): 128-d descriptors bit for bit,
    # the match list and the vote of the whole chain on the CPU
    oka, oda = oracle.surf_detect_describe(A, extended=True); okb, odb = oracle.surf_detect_describe(B, extended=True)
    assert oda.shape[1] == 128 and np.array_equal(da, oda) and np.array_equal(db, odb)
    opairs = oracle.bf_l2_ratio_matches(oda, odb, 0.75)
    ost, ooff, ovotes = oracle.mode_offset(np.stack([oka["x"], oka["y"]], 1), np.stack([okb["x"], okb["y"]], 1), opairs, 3)
    assert row[:7].tolist() == [int(ost), ooff[0], ooff[1], ovotes, len(oka), len(okb), len(opairs)], (row, ost, ooff, ovotes)
    # ORB with the distance threshold of the DLL path
    g2 = SyntheticGrid(2, 1, 1024, overlap=0.15)
    t2 = g2.tiles(threads=1)
    ra = isa.roi_rect(t2[0].shape, 1, "first", 0.2); rb = isa.roi_rect(t2[1].shape, 1, "second", 0.2)
    A = np.ascontiguousarray(t2[0][ra[0]:ra[0] + ra[2]]); B = np.ascontiguousarray(t2[1][:rb[2]])
    ka, da = engine.orb_detect_describe(A); kb, db = engine.orb_detect_describe(B)
    for md in (30, 64, -1):
        gp = engine.bf_hamming_matches(da, db, md)
        op, _od = oracle.bf_hamming_matches(da, db, md)
        assert np.array_equal(gp, op), md
    h0, h1 = engine.tile_upload(t2[0]), engine.tile_upload(t2[1])
    row = engine.attempt_orb_batch([(h0, h1, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])], engine.orb_params(), 30, 3)[0]
    pairs = engine.bf_hamming_matches(da, db, 30)
    st, off, votes = engine.mode_offset(ka, kb, pairs, 3) if len(pairs) else (False, [0, 0], 0)
    assert row[:7].tolist() == [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)], (row, st, off, votes, len(pairs))
    assert 0 < len(pairs) < len(ka)                     # the threshold really cuts
    for h in (ha, hb, h0, h1):
        engine.tile_free(h)


def test_fused_batch_with_featureless_rois(engine, strips):
    """A batch is ragged: ROIs without a single keypoint (flat tiles) sit next to ordinary ones.  Their rows must report zero
    keypoints and no match (Stitcher treats that as "features is None"), and must not disturb their neighbours' rows."""
    g, tiles = strips
    flat = np.full_like(tiles[0], 97)
    ra = isa.roi_rect(tiles[0].shape, 1, "first", 0.2); rb = isa.roi_rect(tiles[1].shape, 1, "second", 0.2)
    hs = [engine.tile_upload(t) for t in (tiles[0], tiles[1], flat)]
    geom = (ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])
    alone = engine.attempt_surf_batch([(hs[0], hs[1]) + geom])[0]
    rows = engine.attempt_surf_batch([(hs[2], hs[1]) + geom, (hs[0], hs[1]) + geom, (hs[0], hs[2]) + geom, (hs[2], hs[2]) + geom])
    assert rows[1].tolist() == alone.tolist() and alone[0] == 1
    assert rows[0][:7].tolist() == [0, 0, 0, 0, 0, int(alone[5]), 0]
    assert rows[2][:7].tolist() == [0, 0, 0, 0, int(alone[4]), 0, 0]
    assert rows[3][:7].tolist() == [0, 0, 0, 0, 0, 0, 0]
    orows = engine.attempt_orb_batch([(hs[2], hs[1]) + geom, (hs[0], hs[2]) + geom, (hs[2], hs[2]) + geom])
    assert orows[:, 0].tolist() == [0, 0, 0] and orows[0][4] == 0 and orows[1][5] == 0 and orows[2][4] == 0 and orows[2][5] == 0
    prow = engine.attempt_phase_batch([(hs[2], hs[2]) + geom])      # identical flat strips: zero spectrum, response 0, no offset
    assert prow.shape == (1, 3) and np.isfinite(prow).all() and prow[0][2] < 0.15
    for h in hs:
        engine.tile_free(h)


def test_full_size_roi_properties(engine):
    """Size-independent properties at the BASELINE geometry (409 x 2048 strips of 2048 x 2048 tiles, ~8.7 k keypoints): keypoints
    come out in KeypointGreater order, descriptors have unit norm, 2-NN distances are ordered and consistent with the descriptors,
    matching a set against itself finds itself at distance 0, and the attempt is symmetric: swapping the tiles with the opposite
    direction negates the offset (+-1 px, the truncation bias of the vote)."""
    g = SyntheticGrid(2, 1, 2048)
    t = g.tiles(threads=2)
    ra = isa.roi_rect(t[0].shape, 1, "first", 0.2); rb = isa.roi_rect(t[1].shape, 1, "second", 0.2)
    A = np.ascontiguousarray(t[0][ra[0]:ra[0] + ra[2]]); B = np.ascontiguousarray(t[1][:rb[2]])
    kxy, da, kf = engine.surf_detect_describe(A, full=True)
    _kb, db = engine.surf_detect_describe(B)
    assert len(kf) > 5000
    r = kf["response"]
    assert np.all(r[:-1] >= r[1:])                                               # response descending (ties broken further down the key)
    tie = r[:-1] == r[1:]
    assert np.all(kf["size"][:-1][tie] >= kf["size"][1:][tie])
    n = np.linalg.norm(da.astype(np.float64), axis=1)
    assert np.all((np.abs(n - 1) < 1e-5) | (n == 0))                             # unit norm (or the zero descriptor of a flat patch)
    i1, d1, d2 = engine.bf_l2_knn2(da, db)
    assert np.all(d1 <= d2) and np.all(i1 >= 0) and np.all(i1 < len(db))
    ref = np.sqrt(((da.astype(np.float64) - db[i1].astype(np.float64)) ** 2).sum(1))
    assert np.abs(ref - d1).max() < 1e-5
    s1, e1, _e2 = engine.bf_l2_knn2(da[:3000], da[:3000])
    nz = n[:3000] > 0
    assert np.all(e1[nz] == 0) and np.all(da[s1[nz]] == da[:3000][nz])          # self match (identical rows may tie on a lower index)
    ha, hb = engine.tile_upload(t[0]), engine.tile_upload(t[1])
    fwd = engine.attempt_surf_batch([(ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])])[0]
    bwd = engine.attempt_surf_batch([(hb, ha, rb[0], rb[1], ra[0], ra[1], ra[2], ra[3])])[0]     # direction 3: B's top against A's bottom
    assert fwd[0] == 1 and bwd[0] == 1
    assert abs(fwd[1] + bwd[1]) <= 1 and abs(fwd[2] + bwd[2]) <= 1, (fwd, bwd)
    engine.tile_free(ha); engine.tile_free(hb)


def test_surf_parameter_variants(engine, oracle, strips):
    """Parameter sets off the default path: upright descriptors (surfIsUpright: no orientation, axis-aligned window, where the
    only non-replicated operation disappears, so descriptors must be bit-exact), a different threshold, and pyramids with other
    octave / layer counts (those take the generic Hessian kernel and other NMS margins)."""
    g, tiles = strips
    img = np.ascontiguousarray(tiles[2][:200, :])
    big = np.ascontiguousarray(tiles[1])                                   # 640 x 640: windows of every class, many cross the border
    for im, kw in ((img, dict(upright=True)), (big, dict(upright=True)), (img, dict(hessian=400.0)), (img, dict(n_octaves=2, n_layers=2)),
                   (big, dict(n_octaves=3, n_layers=4)), (img, dict(n_octaves=4, n_layers=3, extended=True, upright=True))):
        p = engine.surf_params(kw.get("hessian", 100.0), kw.get("n_octaves", 4), kw.get("n_layers", 3), kw.get("extended", False), kw.get("upright", False))
        kxy, desc, kfull = engine.surf_detect_describe(im, p, full=True)
        ko, do = oracle.surf_detect_describe(im, **kw)
        assert len(kfull) == len(ko) and len(ko) > 50, (kw, len(kfull), len(ko))
        assert np.array_equal(_kp_fields(kfull), _kp_fields(ko)), kw
        assert np.array_equal(kfull["angle"], ko["angle"]), kw
        assert np.array_equal(desc, do), kw
    # five octaves would need descriptor windows beyond VFSMS_MAX_WIN (768 px): refused loudly, not computed differently
    with pytest.raises(isa.VfsmsError):
        engine.surf_detect_describe(img, engine.surf_params(100.0, 5, 3, False, False))


def test_keypoint_greater_ties_y_descending(engine, oracle):
    """Equal (response, size, octave) keypoints: upstream's KeypointGreater orders them y DESCENDING, then x ascending.  A tiled
    image plants hundreds of exact ties; kernel and oracle must agree row for row, and the order must be the upstream one."""
    block = np.random.default_rng(5).integers(0, 256, (64, 64), dtype=np.uint8)
    img = np.tile(block, (4, 5))
    a = engine.surf_detect(img); b = oracle.surf_detect(img)
    assert len(a) == len(b) and np.array_equal(_kp_fields(a), _kp_fields(b))
    key = np.stack([a["response"], a["size"], a["octave"].astype(np.float32)], 1)
    same = np.all(key[1:] == key[:-1], 1)
    assert same.sum() > 50
    y0, y1, x0, x1 = a["y"][:-1][same], a["y"][1:][same], a["x"][:-1][same], a["x"][1:][same]
    assert np.all((y0 > y1) | ((y0 == y1) & (x0 < x1))) and np.any(y0 > y1)
    kxy, desc, kf = engine.surf_detect_describe(img, full=True)
    ko, do = oracle.surf_detect_describe(img)
    assert np.array_equal(_kp_fields(kf), _kp_fields(ko)) and np.array_equal(desc, do)


def test_real_dendritic_path_through_grid_registrar(engine, golden_dir):
    """The reference's own ground truth (Stitcher.py:87) around all five serpentine turns of the dendriticCrystal path, 25 pairs:
    1936 x 2584 frames rebuilt around the committed strips (tests/golden/real_path_strips.*), registered through GridRegistrar
    with the direction threaded across the turns (down -> right -> up -> right -> down ...).  Every row must equal the oracle's
    row on the same frames exactly (offset, accepted direction, ROI growth i, votes) and lie within +-1 px of Stitcher.py:87."""
    import json
    from imagestitch_amd.grid import GridRegistrar
    from test_oracle_golden import _rebuild_frames
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    n = 0
    for nb in meta:
        frames = _rebuild_frames(nb, g)
        hs = [engine.tile_upload(f) for f in frames]
        reg = GridRegistrar(engine, method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1)
        table, d_out = reg.register(hs, [f.shape for f in frames], nb["incoming_direction"])
        for h in hs:
            engine.tile_free(h)
        for row, e in zip(table, nb["expected"]):
            assert row[0] == 1, (nb["turn"], e["a"], row)
            assert [int(row[1]), int(row[2])] == e["offset"] and int(row[3]) == e["direction"] and int(row[4]) == e["i"] and int(row[5]) == e["votes"], (nb["turn"], e, row)
            assert abs(int(row[1]) - e["gold"][0]) <= 1 and abs(int(row[2]) - e["gold"][1]) <= 1, (e, row)
            n += 1
        assert d_out == nb["expected"][-1]["direction"]
        # the same neighbourhood pair by pair through the reference's call surface (Stitcher.calculateOffsetForFeatureSearchIncre)
        if nb["turn"] == 30:
            st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
            old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate)
            try:
                isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = 1, 0.2, "surf", 3
                st.direction = nb["incoming_direction"]
                for k, e in enumerate(nb["expected"]):
                    assert st.calculateOffsetForFeatureSearchIncre([frames[k], frames[k + 1]]) == (True, e["offset"]), e
                    assert st.direction == e["direction"]
            finally:
                isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = old
    assert n == 25


def test_enhancement_bit_exact(engine, oracle, strips):
    """cv2.equalizeHist / cv2.createCLAHE(clipLimit, (tileSize, tileSize)).apply as Stitcher.py:269-276 calls them: device bytes equal
    the oracle's on micrograph-like and random images, sizes that are and are not multiples of the CLAHE grid (the extension is
    BORDER_REFLECT_101), a one-grey-level image, other clip limits / grids."""
    g, tiles = strips
    low = (np.random.default_rng(3).normal(110, 12, (203, 317))).clip(0, 255).astype(np.uint8)
    imgs = [tiles[0], np.ascontiguousarray(tiles[1][:409, :]), low, _rand_img(5, (100, 250)), np.full((64, 80), 77, np.uint8), tiles[2][:, 100:357]]
    for img in imgs:
        assert np.array_equal(engine.enhance(img, 1), oracle.equalize_hist(img)), ("equalizeHist", img.shape)
        for clip, ts in ((20.0, 5), (2.0, 8), (40.0, 3), (0.0, 4)):
            assert np.array_equal(engine.enhance(img, 2, clip, ts), oracle.clahe(img, clip, ts)), ("clahe", img.shape, clip, ts)


from imagestitch_amd.synthetic import line_scan as _line_scan  # noqa: E402


def test_full_image_feature_search_resident_cache(engine, oracle):
    """Stitcher.calculateOffsetForFeatureSearch (the method Main.py runs on its four zircon sets, Stitcher.py:260-304) on a line scan
    with a burned-in data bar: whole-tile SURF, tile B's features kept in HBM and reused as tile A's (each tile described once),
    (0, 0) votes of the static bar dropped (ImageUtility.py:158-159).  Every pair must equal the oracle's operator chain on the whole
    tiles (status, offset) and the ground truth within 1 px; with isEnhance (equalizeHist, then CLAHE) the same against the oracle
    chain on the enhanced tiles."""
    tiles, truth = _line_scan()
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.isEnhance,
           isa.Stitcher.isClahe)
    calls = []
    real = engine.features_surf
    try:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = 4, 0, "surf", 3
        for enh, clahe in ((False, False), (True, False), (True, True)):
            isa.Stitcher.isEnhance, isa.Stitcher.isClahe = enh, clahe
            st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
            st.tempImageFeature.isBreak = True
            del calls[:]
            engine.features_surf = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
            pre = (lambda im: im) if not enh else (lambda im: oracle.clahe(im, 20.0, 5)) if clahe else oracle.equalize_hist
            prevB = None
            for k in range(len(tiles) - 1):
                got = st.calculateOffsetForFeatureSearch([tiles[k], tiles[k + 1]])
                ka, da = prevB if prevB is not None else oracle.surf_detect_describe(pre(tiles[k]))
                kb, db = oracle.surf_detect_describe(pre(tiles[k + 1]))
                prevB = (kb, db)
                pairs = oracle.bf_l2_ratio_matches(da, db, 0.75)
                ost, ooff, _v = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 3)
                assert got == ((True, ooff) if ost else (False, "  The two images can not match")), (enh, clahe, k, got, ooff)
                assert got[0] and abs(got[1][0] - truth[k][0]) <= 1 and abs(got[1][1] - truth[k][1]) <= 1, (k, got, truth[k])
            assert len(calls) == len(tiles)                      # the cache: every tile described exactly once
            assert isinstance(st.tempImageFeature.feature, isa.stitcher.ResidentFeatures)
            kxy = np.asarray(st.tempImageFeature.kps)            # reading the cache downloads what detectAndDescribe would have returned
            assert kxy.shape == (len(prevB[0]), 2) and np.array_equal(kxy, np.stack([prevB[0]["x"], prevB[0]["y"]], 1))
            assert np.array_equal(st.tempImageFeature.feature.descriptors(), prevB[1])
            st.releaseTiles()
    finally:
        engine.features_surf = real
        (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.isEnhance,
         isa.Stitcher.isClahe) = old
        isa.Stitcher.tempImageFeature.isBreak = True


def test_incremental_search_with_enhancement(engine, oracle, strips):
    """Method.isEnhance inside the incremental ROI search (Stitcher.py:327-334): fused attempts on equalised / CLAHE'd strips equal
    the oracle chain on the oracle-enhanced strips."""
    g, tiles = strips
    offs, dirs = g.true_offsets(), g.true_directions()
    k = 0
    A, B, d = tiles[k], tiles[k + 1], dirs[k]
    ra = isa.roi_rect(A.shape, d, "first", 0.2); rb = isa.roi_rect(B.shape, d, "second", 0.2)
    ha, hb = engine.tile_upload(A), engine.tile_upload(B)
    roiA = np.ascontiguousarray(A[ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]]); roiB = np.ascontiguousarray(B[rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]])
    for spec, pre in (((1, 0.0, 0), oracle.equalize_hist), ((2, 20.0, 5), lambda im: oracle.clahe(im, 20.0, 5))):
        row = engine.attempt_surf_batch_enhanced([(ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])], None, 0.75, 3, spec)[0]
        ka, da = oracle.surf_detect_describe(pre(roiA)); kb, db = oracle.surf_detect_describe(pre(roiB))
        pairs = oracle.bf_l2_ratio_matches(da, db, 0.75)
        st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 3)
        assert list(row[:7]) == [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)], (spec, row)
    engine.tile_free(ha); engine.tile_free(hb)


def test_fuse_at_production_size_vs_oracle(engine, oracle, tmp_path):
    """fadeInAndFadeOut at the BASELINE tile size: a 2 x 2 serpentine of 2048 x 2048 tiles assembled by Stitcher.getStitchByOffset
    on the device canvas (a 204 x 2048 strip ROI in the column, then whole-tile corner-mode ROIs after the turn) must equal, byte
    for byte, the reference's int64 / -1 canvas walk with the oracle's fuseByFadeInAndFadeOut (tests/fakes.OracleEngine) -- and the
    same with the tiles resident in HBM (the path flowStitch takes after a batched registration)."""
    _fuse_production(engine, oracle, tmp_path, 2048)


def test_fuse_at_config4_tile_size_vs_oracle(engine, oracle, tmp_path):
    """the same at BASELINE configs[4]'s tile size: 4096 x 4096 tiles (819 x 4096 strip ROI, 16 Mpx corner-mode ROIs)."""
    _fuse_production(engine, oracle, tmp_path, 4096)


def _fuse_production(engine, oracle, tmp_path, tile):
    from fakes import OracleEngine
    from test_host_logic import _write_tiles
    g = SyntheticGrid(2, 2, tile, blobs=tile <= 2048)
    tiles = g.tiles(threads=4)
    offs = [list(map(int, o)) for o in g.true_offsets()]
    files = _write_tiles(tmp_path, tiles, "prod")
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = False
        outs = []
        for eng in (engine, OracleEngine(oracle)):
            s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.isColorMode = False
            s.fuseMethod = "fadeInAndFadeOut"
            outs.append(s.getStitchByOffset(files, [list(o) for o in offs]))
        assert outs[0].shape == outs[1].shape and outs[0].shape[0] > 1.85 * tile and np.array_equal(outs[0], outs[1])
        # resident tiles: the handles of a registration phase handed to the fuse
        s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.isColorMode = False; s.fuseMethod = "fadeInAndFadeOut"
        s._resident = {f: (engine.tile_upload(t), t.shape) for f, t in zip(files, tiles)}
        res = s.getStitchByOffset(files, [list(o) for o in offs])
        assert np.array_equal(res, outs[1])
    finally:
        isa.Stitcher.isColorMode = old


def test_zirconcl_surf_attempts_equal_the_oracle(engine, oracle, golden_dir):
    """The fused SURF attempts on the 23 real zirconCL strip pairs (1024 x 256, BASELINE configs[3]'s tiles): every row -- status,
    offset, votes, keypoint and match counts -- equals the oracle chain, whose offsets tests/test_oracle_golden.py pins against phase
    correlation and NCC."""
    from test_oracle_golden import zirconcl_surf_rows
    want = zirconcl_surf_rows(oracle, golden_dir)
    hs = []
    try:
        jobs = []
        for A, B, _r in want:
            ha, hb = engine.tile_upload(A), engine.tile_upload(B)
            hs += [ha, hb]
            jobs.append((ha, hb, 0, 0, 0, 0, A.shape[0], A.shape[1]))
        rows = engine.attempt_surf_batch(jobs, None, 0.75, 3)
        for k, (_A, _B, r) in enumerate(want):
            assert list(rows[k][:7]) == r, (k, list(rows[k][:7]), r)
    finally:
        for h in hs:
            engine.tile_free(h)


def test_ingest_pipeline_reserved_tiles_filled_by_a_slow_decoder(engine):
    """The ingest pipeline (vfsms_tile_reserve / vfsms_tile_fill): the native registrar starts while a slow 'decoder' thread is still
    handing tiles over in path order.  Its speculative batches take only what has arrived (more, smaller batches than with resident
    tiles), the offset table is the same, and a tile whose decoder gives up fails the call instead of hanging it."""
    import threading, time
    g = SyntheticGrid(2, 5, 1024, overlap=0.12)
    tiles = g.tiles(threads=4)
    shapes = [t.shape for t in tiles]
    params = engine.grid_params(method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1, window=48, surf=engine.surf_params())
    res_handles = [engine.tile_upload(t) for t in tiles]
    ref, d_ref, st_ref = engine.pairs_offsets(res_handles, shapes, params)
    for h in res_handles:
        engine.tile_free(h)
    assert ref[:, 0].all()

    handles = [engine.tile_reserve(*s) for s in shapes]
    def decoder(fail_at=None):
        for k, (h, t) in enumerate(zip(handles, tiles)):
            time.sleep(0.05)                                   # several batch times: every batch sees at most the tiles decoded since the last one
            engine.tile_fill(h, None if k == fail_at else t)
    th = threading.Thread(target=decoder); th.start()
    try:
        out, d_out, st = engine.pairs_offsets(handles, shapes, params)
    finally:
        th.join()
        for h in handles:
            engine.tile_free(h)
    assert np.array_equal(out, ref) and d_out == d_ref
    # batches followed the decoder instead of waiting for a window of tiles: with 50 ms between tiles (a batch takes a few) the registrar
    # cannot have gathered the ten tiles in fewer batches than resident tiles need -- >= keeps the check independent of scheduling noise
    assert st[1] >= st_ref[1] and st[0] <= st_ref[0] + 8, (st, st_ref)

    handles = [engine.tile_reserve(*s) for s in shapes]
    th = threading.Thread(target=decoder, kwargs=dict(fail_at=3)); th.start()
    try:
        with pytest.raises(Exception):
            engine.pairs_offsets(handles, shapes, params)
    finally:
        th.join()
        for h in handles:
            engine.tile_free(h)


def test_canvas_assemble_resident_equals_per_tile_calls(engine):
    """vfsms_canvas_assemble_resident (the mosaic walk as one call) == paste + one vfsms_canvas_fuse_tile_resident per tile, byte for
    byte, for both separable blends; a bad mode is refused before anything is enqueued."""
    g = SyntheticGrid(2, 3, 512, overlap=0.12)
    tiles = g.tiles(threads=2)
    offs = [[0, 0]] + [list(map(int, o)) for o in g.true_offsets()]
    shapes = [t.shape for t in tiles]
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, offs)
    handles = [engine.tile_upload(t) for t in tiles]
    try:
        for method in (0, 1):
            geom = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
            for i in range(1, len(tiles)):
                oy, ox = offsetList[i]
                geom.append((oy, ox, max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0]), min(oy + 512, rangeX[i - 1][1]),
                             min(ox + 512, rangeY[i - 1][1]), offs[i][0], offs[i][1], method))
            outs = []
            for one_call in (True, False):
                cv = engine.canvas_create(rows, cols, 1)
                try:
                    if one_call:
                        engine.canvas_assemble_resident(cv, handles, geom)
                    else:
                        engine.canvas_paste_tile(cv, handles[0], geom[0][0], geom[0][1])
                        for i in range(1, len(tiles)):
                            engine.canvas_fuse_tile_resident(cv, handles[i], geom[i][0], geom[i][1], geom[i][2:6], geom[i][6], geom[i][7], method=method)
                    outs.append(engine.canvas_download(cv, rows, cols, 1))
                finally:
                    engine.canvas_free(cv)
            assert np.array_equal(outs[0], outs[1]) and outs[0].any(), method
        cv = engine.canvas_create(rows, cols, 1)
        try:
            with pytest.raises(Exception):
                engine.canvas_assemble_resident(cv, handles[:1], [(0, 0, 0, 0, 0, 0, 0, 0, 5)])
        finally:
            engine.canvas_free(cv)
    finally:
        for h in handles:
            engine.tile_free(h)


def test_orb_at_config2_geometry(engine, oracle):
    """BASELINE configs[2] geometry: 2048 x 2048 tiles, 10 % overlap, ROI strips 409 x 2048, ORB(5000, 1.2, 8, 31, 0, 2, HARRIS, 31, 20)
    with upstream's learned sampling table.  Keypoints + descriptor bytes of a full-size strip equal the oracle's; size-independent
    properties hold (level-major order, per-level quotas, 31 px border in level coordinates, a set matched against itself finds
    itself at Hamming distance 0); the fused attempt row equals the oracle chain and the voted offset equals the integer ground truth
    exactly (north_star's bar for ORB)."""
    g = SyntheticGrid(2, 1, 2048, overlap=0.10)
    t = g.tiles(threads=2)
    truth = g.true_offsets()[0]
    ra = isa.roi_rect(t[0].shape, 1, "first", 0.2); rb = isa.roi_rect(t[1].shape, 1, "second", 0.2)
    assert ra[2:] == (409, 2048)
    A = np.ascontiguousarray(t[0][ra[0]:ra[0] + ra[2]]); B = np.ascontiguousarray(t[1][:rb[2]])
    kxy, da, kf = engine.orb_detect_describe(A, full=True)
    ko, do = oracle.orb_detect_describe(A)
    assert len(kf) == len(ko) > 4000
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(kf[f], ko[f]), f
    assert np.array_equal(da, do)
    assert np.all(np.diff(kf["octave"]) >= 0)
    q = np.bincount(kf["octave"], minlength=8)
    assert q[0] <= 1085 + 64 and q.sum() <= 5000 + 8 * 64
    lx = kf["x"] / (1.2 ** kf["octave"]); ly = kf["y"] / (1.2 ** kf["octave"])
    assert lx.min() >= 30.9 and ly.min() >= 30.9
    self_pairs = engine.bf_hamming_matches(da, da)
    assert len(self_pairs) == len(da)
    assert np.all((da[self_pairs[:, 0]] == da[self_pairs[:, 1]]).all(1))            # distance 0 (ties go to the lower index)
    _kb, db, kfb = engine.orb_detect_describe(B, full=True)
    ha, hb = engine.tile_upload(t[0]), engine.tile_upload(t[1])
    row = engine.attempt_orb_batch([(ha, hb, ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])], engine.orb_params(), -1, 3)[0]
    engine.tile_free(ha); engine.tile_free(hb)
    pairs, _ = oracle.bf_hamming_matches(da, db)
    st, off, votes = oracle.mode_offset(kxy, np.stack([kfb["x"], kfb["y"]], 1), pairs, 3)
    assert list(row[:7]) == [int(st), off[0], off[1], votes, len(da), len(db), len(pairs)], (row, st, off, votes)
    assert st and [off[0] + 2048 - int(0.2 * 2048), off[1]] == truth, (off, truth)


@pytest.mark.gpu
def test_config3_all_zirconcl_pairs_phase(engine, oracle, golden_dir):
    """BASELINE configs[3] in full: the direction-4 ROI strips of all 24 zirconCL tiles (tests/golden/zirconcl_strips.npz), 23 pairs in
    ONE batched launch: truncated offsets equal the oracle's (whose arithmetic tests/phase_numpy.py re-derives independently),
    sub-pixel peak within 1e-6 px, response within 1e-9, and the accept decision (response > 0.15) is the same."""
    import json
    meta = json.load(open(os.path.join(golden_dir, "phase_independent.json")))
    z = np.load(os.path.join(golden_dir, "zirconcl_strips.npz"))
    rows = [r for r in meta["rows"] if r["dataset"] == "zirconCL"]
    assert len(rows) == 23
    H, W = meta["shape"]
    ra, rb = meta["roi_first"], meta["roi_second"]
    tiles = []
    for k in range(24):                                         # frames rebuilt around the two strips of every tile
        T = np.zeros((H, W), np.uint8)
        T[ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]] = z["t%d_first" % k]
        T[rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]] = z["t%d_second" % k]
        tiles.append(T)
    hs = [engine.tile_upload(T) for T in tiles]
    out = engine.attempt_phase_batch([(hs[k], hs[k + 1], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]) for k in range(23)])
    for h in hs:
        engine.tile_free(h)
    for k, r in enumerate(rows):
        (ox, oy), orr = oracle.phase_correlate(z["t%d_first" % k], z["t%d_second" % (k + 1)])
        x, y, resp = out[k]
        assert [int(y), int(x)] == [int(oy), int(ox)] == r["offset_int"], (k, x, y, ox, oy)
        assert abs(x - ox) < 1e-6 and abs(y - oy) < 1e-6 and abs(resp - orr) < 1e-9 and (resp > 0.15) == r["accepted"], (k, x - ox, y - oy, resp - orr)


@pytest.mark.gpu
def test_real_dendritic_path_orb_through_grid_registrar(engine, golden_dir):
    """The ORB leg on the reference's own ground truth: the 25 committed neighbourhood pairs (frames rebuilt around the stored strips)
    through GridRegistrar(method="orb") with offsetEvaluate 3 as the reference has it -- every row equals the oracle's ORB row
    (offset, direction, i, votes; tests/golden/real_path_strips.json `expected_orb`), false accepts included, and the 22 rows the
    oracle puts within +-1 px of Stitcher.py:87 are within +-1 px here too."""
    import json
    from imagestitch_amd.grid import GridRegistrar
    from test_oracle_golden import _rebuild_frames
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    n = 0
    for nb in meta:
        frames = _rebuild_frames(nb, g)
        hs = [engine.tile_upload(f) for f in frames]
        reg = GridRegistrar(engine, method="orb", roiRatio=0.2, offsetEvaluate=3, directIncre=1)
        table, d_out = reg.register(hs, [f.shape for f in frames], nb["incoming_direction"])
        for h in hs:
            engine.tile_free(h)
        for row, e in zip(table, nb["expected_orb"]):
            assert row[0] == 1, (nb["turn"], e["a"], row)
            assert [int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[5])] == e["offset"] + [e["direction"], e["i"], e["votes"]], (nb["turn"], e, row)
            if e["within_one"]:                                # (22 of the 25: see test_orb_real_path_strips_reproduced_by_oracle for the other three)
                assert abs(int(row[1]) - e["gold"][0]) <= 1 and abs(int(row[2]) - e["gold"][1]) <= 1, (e, row)
            n += 1
    assert n == 25


@pytest.mark.gpu
def test_orb_grid_at_offset_evaluate_3_equals_oracle_chain(engine, oracle):
    """configs[2] as it is written -- 2048^2 tiles, 10 % overlap, ORB + Hamming 1-NN + mode vote with offsetEvaluate = 3 -- on a 3 x 3
    serpentine grid.  With every query voting (ImageUtility.py:297-302) a wrong candidate direction now and then collects three equal
    votes and is ACCEPTED; whether cv2's ORB would do the same on these tiles cannot be known here, but the engine must take every
    decision the oracle takes: the whole table (status, offset, direction, i, votes), false accepts included, pair by pair with the
    direction threaded, through the fused native registrar AND through Stitcher.calculateOffsetForFeatureSearchIncre."""
    from imagestitch_amd.grid import GridRegistrar
    from test_oracle_golden import _chain_search, oracle_orb_attempt
    g = SyntheticGrid(3, 3, 2048, overlap=0.10)
    tiles = g.tiles(threads=4)
    hs = [engine.tile_upload(t) for t in tiles]
    reg = GridRegistrar(engine, method="orb", roiRatio=0.2, offsetEvaluate=3, directIncre=1)
    table, d_out = reg.register(hs, [t.shape for t in tiles], 1)
    for h in hs:
        engine.tile_free(h)
    direction, exp = 1, []
    for k in range(len(tiles) - 1):
        st, off, d, i, log = _chain_search(oracle_orb_attempt(oracle, tiles[k], tiles[k + 1]), tiles[k].shape, tiles[k + 1].shape, direction)
        exp.append([int(st), off[0], off[1], d if st else direction, i, log[-1][5] if st else 0])
        if st:
            direction = d
    got = [[int(v) for v in row[:6]] for row in table]
    for k, (a, b) in enumerate(zip(got, exp)):
        if b[0]:
            assert a == b, (k, a, b, g.true_offsets()[k])
        else:
            assert a[0] == 0, (k, a, b)
    # decisions that agree with the ground truth are exact (north_star: bit-exact for ORB); the others are the documented false accepts
    truth = g.true_offsets()
    n_true = sum(1 for k, r in enumerate(exp) if r[0] and [r[1], r[2]] == truth[k])
    assert n_true >= len(exp) - 3, (exp, truth)
    s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False
    s.roiRatio = 0.2; s.direction = 1; s.directIncre = 1; s.featureMethod = "orb"; s.offsetEvaluate = 3
    for k in range(len(tiles) - 1):
        status, off = s.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
        assert (int(status), off if status else None) == (exp[k][0], [exp[k][1], exp[k][2]] if exp[k][0] else None), (k, off, exp[k])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_config2_full_orb_grid_equals_the_oracle_chain(engine, oracle):
    """BASELINE configs[2] at ITS OWN SIZE: the synthetic 10 x 9 grid of 2048^2 tiles (89 pairs, 10 % overlap), ORB(5000, 1.2, 8) +
    BF-Hamming 1-NN + mode vote at the reference's offsetEvaluate = 3 (ImageUtility.py:260, 297-302, 139-178), registered by the native
    registrar in fused batches.  The whole table -- status, offset, direction, i, votes of every pair, the falsely accepted candidates
    included -- must equal the ORACLE's chain (Stitcher.py:316-361 walked pair after pair with the direction threaded).  The oracle's
    attempts are independent of the engine's answer; they are only evaluated ahead on host threads (every pair's first candidate at the
    four directions) so that the walk finishes inside the budget.  `pairs_off_truth` -- decisions that differ from the ground truth: what the
    reference's search does with three equal random votes -- is counted and bounded, the pairs that DO land on the truth are exact."""
    from concurrent.futures import ThreadPoolExecutor
    from imagestitch_amd.grid import GridRegistrar
    from test_oracle_golden import _chain_search, oracle_orb_attempt, pool_size
    g = SyntheticGrid(10, 9, 2048, overlap=0.10)
    tiles = g.tiles(threads=8)
    P = len(tiles) - 1
    hs = [engine.tile_upload(t) for t in tiles]
    reg = GridRegistrar(engine, method="orb", roiRatio=0.2, offsetEvaluate=3, directIncre=1, surfParams=engine.orb_params())
    table, d_out = reg.register(hs, [t.shape for t in tiles], 1)
    for h in hs:
        engine.tile_free(h)
    memo = {}

    def attempt_of(k):
        raw = oracle_orb_attempt(oracle, tiles[k], tiles[k + 1])

        def attempt(d, i):
            if (k, d, i) not in memo:
                memo[(k, d, i)] = raw(d, i)
            return memo[(k, d, i)]
        return attempt
    # every pair's first ring, evaluated ahead in parallel (the C oracle releases the interpreter lock); the walk below decides alone
    jobs = [(k, d, 1) for k in range(P) for d in (1, 2, 3, 4)]
    with ThreadPoolExecutor(max_workers=pool_size()) as ex:
        for key, r in zip(jobs, ex.map(lambda kd: oracle_orb_attempt(oracle, tiles[kd[0]], tiles[kd[0] + 1])(kd[1], kd[2]), jobs)):
            memo[key] = r
    direction, exp = 1, []
    for k in range(P):
        st, off, d, i, log = _chain_search(attempt_of(k), tiles[k].shape, tiles[k + 1].shape, direction)
        exp.append([int(st), off[0], off[1], d if st else direction, i, log[-1][5] if st else 0])
        if st:
            direction = d
    got = [[int(v) for v in row[:6]] for row in table]
    for k, (a, b) in enumerate(zip(got, exp)):
        if b[0]:
            assert a == b, (k, a, b, g.true_offsets()[k])
        else:
            assert a[0] == 0, (k, a, b)
    truth = g.true_offsets()
    off_truth = [k for k, r in enumerate(exp) if not (r[0] and [r[1], r[2]] == [int(truth[k][0]), int(truth[k][1])])]
    print("configs[2]: %d of %d pairs accepted off truth (reference behaviour at 3 votes): %s" % (len(off_truth), P, off_truth))
    assert len(off_truth) <= 30, off_truth


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_headline_surf_grid_equals_the_oracle_chain(engine, oracle):
    """The workload bench.py times, row for row: the synthetic 10 x 9 grid of 2048^2 tiles (89 pairs, 10 % overlap, default seed), SURF +
    BF-L2 2-NN + ratio 0.75 + mode vote at offsetEvaluate = 3, registered by the native registrar with bench.py's window of 48.
      1. The whole table -- status, offset, direction, i, votes of every pair -- equals the ORACLE's chain (Stitcher.py:316-361 walked
         pair after pair with the direction threaded), and every pair lands within 1 px of the synthetic truth.
      2. Every attempt the oracle walk evaluated, the failed candidates included, goes through ONE attempt_surf_batch: its raw row
         (status, offset, votes, keypoint counts of both strips, match count) equals the oracle's.
      3. The path memory and the speculation window never change results: a hint of the true directions, two wrong hints, window 24
         and a registrar that has learned the grid all give the same table.
    The oracle's attempts are evaluated ahead on host threads at the keys the engine's table implies; the walk decides from oracle results
    alone and computes any key it misses on demand."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    from imagestitch_amd.grid import GridRegistrar
    from test_oracle_golden import _chain_search, oracle_surf_attempt, pool_size
    t0 = time.perf_counter()
    g = SyntheticGrid(10, 9, 2048, overlap=0.10)
    tiles = g.tiles(threads=pool_size())
    P = len(tiles) - 1
    assert P == 89
    shapes = [t.shape for t in tiles]
    hs = [engine.tile_upload(t) for t in tiles]

    def registrar(window=48):
        return GridRegistrar(engine, method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1,
                             surfParams=engine.surf_params(), window=window)
    try:
        reg = registrar()
        table, d_out = reg.register(hs, shapes, 1)
        got = [[int(v) for v in row[:6]] for row in table]

        # -- 1. the oracle chain --
        # (one OpenMP thread per oracle call: the attempts themselves run on the pool, on-demand ones included)
        raw = [oracle_surf_attempt(oracle, tiles[k], tiles[k + 1], nthreads=1) for k in range(P)]
        implied, d_in = [], 1
        for k, r in enumerate(got):
            for ring in reg.rings(d_in):
                for (d, i) in ring:
                    implied.append((k, d, i))
                    if r[0] and (d, i) == (r[3], r[4]):
                        break
                else:
                    continue
                break
            d_in = r[3] if r[0] else d_in
        walked = []
        with ThreadPoolExecutor(max_workers=pool_size()) as ex:
            list(ex.map(lambda kdi: raw[kdi[0]](kdi[1], kdi[2]), implied))

            def attempt_of(k):
                def attempt(d, i):
                    if (d, i) not in raw[k].rows:
                        ex.submit(raw[k], d, i).result()
                    walked.append((k, d, i))
                    r = raw[k].rows[(d, i)]
                    return bool(r[0]) and r[4] > 0 and r[5] > 0, [r[1], r[2]], r[3]
                return attempt
            direction, exp = 1, []
            for k in range(P):
                st, off, d, i, log = _chain_search(attempt_of(k), shapes[k], shapes[k + 1], direction)
                exp.append([int(st), off[0], off[1], d if st else direction, i, log[-1][5] if st else 0])
                if st:
                    direction = d
        truth = g.true_offsets()
        for k, b in enumerate(exp):
            assert b[0] == 1 and abs(b[1] - truth[k][0]) <= 1 and abs(b[2] - truth[k][1]) <= 1, (k, b, truth[k])
        for k, (a, b) in enumerate(zip(got, exp)):
            assert a == b, (k, a, b, truth[k])
        assert int(d_out) == direction
        print("headline surf grid: the oracle walk evaluated %d attempts (%d prefetched)" % (len(walked), len(implied)))

        # -- 2. every attempt of the walk in one batch, counts included --
        jobs = []
        for (k, d, i) in walked:
            ra = isa.roi_rect(shapes[k], d, "first", i * 0.2); rb = isa.roi_rect(shapes[k + 1], d, "second", i * 0.2)
            jobs.append((hs[k], hs[k + 1], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]))
        rows = engine.attempt_surf_batch(jobs, engine.surf_params(), 0.75, 3)
        for (k, d, i), row in zip(walked, rows):
            assert row[:7].tolist() == raw[k].rows[(d, i)], (k, d, i, row, raw[k].rows[(d, i)])

        # -- 3. prior and window never change the table --
        true_dirs = [int(v) for v in g.true_directions()]
        assert reg.path_memory is not None
        variants = [("learned path memory", reg, None),
                    ("hint = true directions", registrar(), true_dirs),
                    ("hint = all 1", registrar(), [1] * P),
                    ("hint = true directions shifted by one", registrar(), true_dirs[1:] + true_dirs[:1]),
                    ("window 24", registrar(24), None)]
        for name, r, hint in variants:
            t2, d2 = r.register(hs, shapes, 1, hint=hint)
            assert np.array_equal(t2, table) and int(d2) == int(d_out), name
    finally:
        for h in hs:
            engine.tile_free(h)
    print("headline surf grid: %.1f s" % (time.perf_counter() - t0))


@pytest.mark.gpu
def test_fuse_trigonometric_operator_vs_reference_formula(engine, oracle, golden_dir):
    """ImageFusion.fuseByTrigonometric on the device (vfsms_fuse_trig_i64) against the reference's numpy expression (tests/fakes.py
    restates ImageFusion.py:246-293 line by line) on the 249 fade fixtures -- strip modes both ways round, the four corner cases,
    gray and colour -- and on production-size regions.  Tolerance as written in include/vfsms.h: one grey level on < 0.1 % of the
    bytes (numpy's SIMD sin vs the library's explicit sin, last ulp, where wA a + (1 - wA) a sits on an integer)."""
    from fakes import OracleEngine
    ref = OracleEngine(oracle)
    g = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    nbytes = ndiff = 0
    for i, (dx, dy, _c) in enumerate(g["meta"]):
        A, B = g["f%d_A" % i], g["f%d_B" % i]
        try:
            want = ref.fuse_trig_i64(A, B, dx, dy)
        except IndexError:
            continue                                            # (geometries where the reference's getWeightsMatrix raises)
        got = engine.fuse_trig_i64(A, B, dx, dy)
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        assert d.max() <= 1, (i, int(d.max()))
        nbytes += d.size; ndiff += np.count_nonzero(d)
    rng = np.random.default_rng(3)
    for (r, c, hole) in ((409, 2048, None), (2048, 300, None), (1200, 1500, "tl"), (1500, 1200, "br")):
        A = rng.integers(0, 256, (r, c)).astype(np.int64); B = rng.integers(0, 256, (r, c)).astype(np.int64)
        if hole == "tl": A[:r // 2 + 37, :] = -1; A[:, :c // 2 + 11] = np.where(np.arange(r)[:, None] < r - 90, -1, A[:, :c // 2 + 11])
        if hole == "br": A[r // 3:, c // 4:] = -1
        for dx, dy in ((5, 7), (-5, -7)):
            want = ref.fuse_trig_i64(A, B, dx, dy)
            got = engine.fuse_trig_i64(A, B, dx, dy)
            d = np.abs(got.astype(np.int16) - want.astype(np.int16))
            assert d.max() <= 1, (r, c, hole, int(d.max()))
            nbytes += d.size; ndiff += np.count_nonzero(d)
    assert ndiff <= 1e-3 * nbytes, (ndiff, nbytes)


@pytest.mark.gpu
def test_line_scan_batched_full_image_path(engine, tmp_path):
    """flowStitch over a line scan with caculateOffsetMethod = calculateOffsetForFeatureSearch (Main.py:29-51): the batched path (files ->
    ingest pipeline -> vfsms_features_surf_batch -> vfsms_features_match_offset_batch) must report exactly what the pair-by-pair mirror
    of Stitcher.py:260-304 reports (status, offsets, log lines), with and without CLAHE, and stop behind a pair that cannot be matched."""
    from PIL import Image
    tiles, truth = _line_scan()
    files = []
    for k, t in enumerate(tiles):
        f = os.path.join(str(tmp_path), "scan_%02d.png" % k)
        Image.fromarray(t).save(f); files.append(f)
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.isEnhance,
           isa.Stitcher.isClahe, isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod)
    try:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = 4, 0, "surf", 3
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = False, "notFuse"
        for enh, clahe in ((False, False), (True, True)):
            isa.Stitcher.isEnhance, isa.Stitcher.isClahe = enh, clahe
            seq = isa.Stitcher(); seq._engine = engine; seq.isPrintLog = False
            seq.tempImageFeature.isBreak = True
            want = [seq.calculateOffsetForFeatureSearch([tiles[k], tiles[k + 1]]) for k in range(len(tiles) - 1)]
            seq.releaseTiles()
            st = isa.Stitcher(); st._engine = engine
            msgs = []
            st.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
            got = st._registerBatched(files, st.calculateOffsetForFeatureSearch)
            assert got is not None, "the batched full-image path did not engage"
            status, end, offs, _desc = got
            for h, _s in (st.__dict__.pop("_resident", None) or {}).values():
                engine.tile_free(h)
            assert status and end == len(tiles) - 1 and offs == [w[1] for w in want], (enh, offs, want)
            assert all(w[0] for w in want)
            for k, o in enumerate(offs):
                assert abs(o[0] - truth[k][0]) <= 1 and abs(o[1] - truth[k][1]) <= 1
                assert "  The offset of stitching: dx is %d dy is %d" % (o[0], o[1]) in msgs
        # a tile that cannot be matched (blank) breaks the scan where the pair loop breaks it
        isa.Stitcher.isEnhance = False
        Image.fromarray(np.zeros_like(tiles[0])).save(files[3])
        st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
        status, end, offs, desc = st._registerBatched(files, st.calculateOffsetForFeatureSearch)
        for h, _s in (st.__dict__.pop("_resident", None) or {}).values():
            engine.tile_free(h)
        assert status is False and end == 2 and len(offs) == 2 and "can not be stitched" in desc
    finally:
        (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.isEnhance,
         isa.Stitcher.isClahe, isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod) = old
        isa.Stitcher.tempImageFeature.isBreak = True


@pytest.mark.gpu
def test_timed_mosaic_walk_equals_the_oracle_walk_at_2048(engine, oracle):
    """What `bench.py --method fuse` times -- vfsms_canvas_assemble_resident over resident 2048 x 2048 tiles with the geometry rows
    bench.py builds from Stitcher._layout -- against the reference's int64 / -1 canvas walk (Stitcher.py:434-483) with the oracle's
    fuseByFadeInAndFadeOut: a 3 x 3 serpentine (strip ROIs inside the columns, corner ROIs after both turns, a tile that meets three
    earlier ones), byte for byte."""
    from fakes import OracleEngine
    T = 2048
    g = SyntheticGrid(3, 3, T)
    tiles = g.tiles(threads=4)
    n = len(tiles)
    offs = [[0, 0]] + [list(map(int, o)) for o in g.true_offsets()]
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout([t.shape for t in tiles], offs)
    rois = [None] + [(max(offsetList[i][0], rangeX[i - 1][0]), max(offsetList[i][1], rangeY[i - 1][0]),
                      min(offsetList[i][0] + T, rangeX[i - 1][1]), min(offsetList[i][1] + T, rangeY[i - 1][1])) for i in range(1, n)]
    handles = [engine.tile_upload(t) for t in tiles]
    cv = engine.canvas_create(rows, cols, 1)
    try:
        geom = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
        geom += [(offsetList[i][0], offsetList[i][1]) + tuple(rois[i]) + (offs[i][0], offs[i][1], 0) for i in range(1, n)]
        engine.canvas_assemble_resident(cv, handles, geom)
        got = engine.canvas_download(cv, rows, cols, 1)
    finally:
        engine.canvas_free(cv)
        for h in handles:
            engine.tile_free(h)
    ref = OracleEngine(oracle)
    c = ref.canvas_create(rows, cols, 1)
    ref.canvas_paste(c, tiles[0], offsetList[0][0], offsetList[0][1])
    for i in range(1, n):
        ref.canvas_fuse_tile(c, tiles[i], offsetList[i][0], offsetList[i][1], rois[i], offs[i][0], offs[i][1])
    want = ref.canvas_download(c, rows, cols, 1)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert len({(r[2] - r[0] == T and r[3] - r[1] == T) for r in rois[1:]}) == 2          # both strip and whole-tile (corner) ROIs occurred


def _colour_jpegs(tmp_path, g, tag, quality=92, **kw):
    from PIL import Image
    files = []
    for k, t in enumerate(g.tiles(threads=2)):
        f = t.astype(np.float32)
        rgb = np.clip(np.stack([0.6 * f + 30, f, 255 - 0.7 * f], -1), 0, 255).astype(np.uint8)
        p = os.path.join(str(tmp_path), "%s_%02d.jpg" % (tag, k))
        Image.fromarray(rgb).save(p, quality=quality, **kw)
        files.append(p)
    return files


def _tile_bytes(engine, handle, h, w, ch):
    cv = engine.canvas_create(h, w, ch)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, h, w, ch)
    finally:
        engine.canvas_free(cv)


@pytest.mark.gpu
def test_ingest_pair_fill_equals_the_two_decodes(engine, tmp_path):
    """vfsms_tile_fill_pair (csrc/ingest_kernels.hip): from ONE decode of a JPEG to its Y Cb Cr planes the device writes the gray tile ==
    the file's grayscale decode (cv2.imdecode(..., 0), Stitcher.py:68-69) and the B G R tile == its colour decode (IMREAD_COLOR,
    Stitcher.py:382-403), byte for byte -- 4-byte and 3-byte source pixels, a grayscale file, image areas that are not multiples of 4,
    4:2:0 and 4:4:4 files; giving a pair up fails the call that waits for it."""
    from PIL import Image
    from imagestitch_amd import stitcher as ST
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (41, 57, 3), dtype=np.uint8)
    for (w, h), kw in (((613, 407), dict(quality=90)), ((512, 384), dict(quality=95, subsampling=0)), ((333, 7), dict(quality=70))):
        img = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC))
        p = os.path.join(str(tmp_path), "c_%d.jpg" % w)
        Image.fromarray(img).save(p, **kw)
        want_gray, want_bgr = ST._imread(p, False), ST._imread(p, True)
        ycc = Image.open(p); ycc.draft("YCbCr", ycc.size); ycc = np.ascontiguousarray(np.asarray(ycc))
        assert ycc.shape == (h, w, 3)
        x32 = np.ascontiguousarray(np.concatenate([ycc, np.full((h, w, 1), 255, np.uint8)], 2))
        padded = np.zeros((h, w * 3 + 5), np.uint8); padded[:, :w * 3] = ycc.reshape(h, w * 3)       # a row stride wider than the row
        for src, stride, fmt in ((ycc, w * 3, engine.SRC_YCC24), (x32, w * 4, engine.SRC_YCCX32), (padded, w * 3 + 5, engine.SRC_YCC24)):
            hg, hc = engine.tile_reserve(h, w), engine.tile_reserve_color(h, w, 3)
            try:
                engine.tile_fill_pair(hg, hc, src.ctypes.data, stride, fmt)
                assert np.array_equal(_tile_bytes(engine, hg, h, w, 1), want_gray)
                assert np.array_equal(_tile_bytes(engine, hc, h, w, 3), want_bgr)
            finally:
                engine.tile_free(hg); engine.tile_free(hc)
        # one plane only; a grayscale source replicated into the colour tile
        hc = engine.tile_reserve_color(h, w, 3)
        engine.tile_fill_pair(0, hc, ycc.ctypes.data, w * 3, engine.SRC_YCC24)
        assert np.array_equal(_tile_bytes(engine, hc, h, w, 3), want_bgr)
        engine.tile_free(hc)
        hg, hc = engine.tile_reserve(h, w), engine.tile_reserve_color(h, w, 3)
        engine.tile_fill_pair(hg, hc, want_gray.ctypes.data, w, engine.SRC_GRAY8)
        assert np.array_equal(_tile_bytes(engine, hg, h, w, 1), want_gray)
        assert np.array_equal(_tile_bytes(engine, hc, h, w, 3), np.repeat(want_gray[:, :, None], 3, 2))
        engine.tile_free(hg); engine.tile_free(hc)
    # the decoder's own hand-over (Pillow's pixel block through Arrow, or the array copy) is one of the formats above
    owner, shape, parts = ST._decode_once(p, True)
    hg, hc = engine.tile_reserve(*shape), engine.tile_reserve_color(shape[0], shape[1], 3)
    engine.tile_fill_pair(hg, hc, parts[1], parts[2], parts[3])
    assert np.array_equal(_tile_bytes(engine, hc, shape[0], shape[1], 3), want_bgr)
    engine.tile_free(hg); engine.tile_free(hc)
    # a pair that is given up
    hg, hc = engine.tile_reserve(8, 8), engine.tile_reserve_color(8, 8, 3)
    engine.tile_fill_pair(hg, hc, None, 0, 0)
    cv = engine.canvas_create(8, 8, 3)
    try:
        with pytest.raises(Exception):
            engine.canvas_paste_tile(cv, hc, 0, 0)
    finally:
        engine.canvas_free(cv); engine.tile_free(hg); engine.tile_free(hc)
    with pytest.raises(Exception):
        engine.tile_fill_pair(0, 0, x32.ctypes.data, 4, 2)


@pytest.mark.gpu
def test_tile_fill_jpeg_equals_the_two_decodes(engine, tmp_path):
    """vfsms_tile_fill_jpeg: the FILE'S BYTES in -- libjpeg-turbo inside the library, pinned staging, plane split and colour conversion on the
    device -- the gray tile == the file's grayscale decode (cv2.imdecode(..., 0), Stitcher.py:68-69) and the B G R tile == its colour decode
    (Stitcher.py:382-403), byte for byte: 4:2:0 / 4:4:4 / progressive / grayscale files, areas that are not multiples of 4, one plane at a
    time, many threads at once; a file it refuses (truncated, wrong size, PNG) leaves the tiles RESERVED for another decoder."""
    import io
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from imagestitch_amd import stitcher as ST
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (41, 57, 3), dtype=np.uint8)
    cases = []
    for (w, h), kw in (((613, 407), dict(quality=90)), ((512, 384), dict(quality=95, subsampling=0)), ((333, 7), dict(quality=70)),
                       ((1021, 767), dict(quality=85, progressive=True))):
        img = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC))
        p = os.path.join(str(tmp_path), "j_%d.jpg" % w)
        Image.fromarray(img).save(p, **kw)
        cases.append((p, h, w, ST._imread(p, False), ST._imread(p, True)))
    p = os.path.join(str(tmp_path), "j_gray.jpg")
    Image.fromarray(np.asarray(Image.fromarray(base[:, :, 0]).resize((301, 203), Image.BICUBIC))).save(p, quality=90)
    g = ST._imread(p, False)
    cases.append((p, 203, 301, g, np.repeat(g[:, :, None], 3, 2)))
    hg0, hc0 = engine.tile_reserve(8, 8), engine.tile_reserve_color(8, 8, 3)
    probe = io.BytesIO(); Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(probe, "JPEG")
    if not engine.tile_fill_jpeg(hg0, hc0, probe.getvalue()):
        engine.tile_fill_pair(hg0, hc0, None, 0, 0); engine.tile_free(hg0); engine.tile_free(hc0)
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")
    engine.tile_free(hg0); engine.tile_free(hc0)

    def one(case, which):
        p, h, w, want_gray, want_bgr = case
        data = open(p, "rb").read()
        hg = engine.tile_reserve(h, w) if which != "color" else 0
        hc = engine.tile_reserve_color(h, w, 3) if which != "gray" else 0
        assert engine.tile_fill_jpeg(hg, hc, data)
        return hg, hc
    for case in cases:
        for which in ("both", "gray", "color"):
            hg, hc = one(case, which)
            if hg:
                assert np.array_equal(_tile_bytes(engine, hg, case[1], case[2], 1), case[3]), (case[0], which)
                engine.tile_free(hg)
            if hc:
                assert np.array_equal(_tile_bytes(engine, hc, case[1], case[2], 3), case[4]), (case[0], which)
                engine.tile_free(hc)
    with ThreadPoolExecutor(8) as ex:                          # the decoder pool's use: any thread, concurrently
        got = list(ex.map(lambda k: one(cases[k % len(cases)], "both"), range(24)))
    for k, (hg, hc) in enumerate(got):
        c = cases[k % len(cases)]
        assert np.array_equal(_tile_bytes(engine, hg, c[1], c[2], 1), c[3]) and np.array_equal(_tile_bytes(engine, hc, c[1], c[2], 3), c[4])
        engine.tile_free(hg); engine.tile_free(hc)
    # refused files: the tiles are still reserved, and another decoder's hand-over fills them
    p, h, w, want_gray, want_bgr = cases[0]
    data = open(p, "rb").read()
    png = io.BytesIO(); Image.fromarray(want_bgr[:, :, ::-1]).save(png, "PNG")
    for bad in (data[:len(data) // 2], open(cases[1][0], "rb").read(), png.getvalue()):
        hg, hc = engine.tile_reserve(h, w), engine.tile_reserve_color(h, w, 3)
        assert engine.tile_fill_jpeg(hg, hc, bad) is False
        owner, shape, parts = ST._decode_once(p, True)
        engine.tile_fill_pair(hg, hc, parts[1], parts[2], parts[3])
        assert np.array_equal(_tile_bytes(engine, hg, h, w, 1), want_gray) and np.array_equal(_tile_bytes(engine, hc, h, w, 3), want_bgr)
        engine.tile_free(hg); engine.tile_free(hc)


class _NoIngest:
    """the engine without its ingest entry points: the Stitcher then decodes gray for the pairs and colour for the mosaic, twice per file,
    like the reference"""
    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        if name in ("tile_reserve", "tile_fill_pair", "tile_reserve_color"):
            raise AttributeError(name)
        return getattr(self._e, name)


@pytest.mark.gpu
def test_colour_mode_driver_decodes_each_file_once(engine, tmp_path):
    """Main.py as written (isColorMode = True, Main.py:14) on a folder of colour JPEG tiles through imageSetStitchWithMutiple: the decoder
    runs exactly ONCE per file (counted) -- the registration plane and the mosaic's B G R tile come from the same decode and the colour
    tiles stay in HBM for getStitchByOffset -- and the written mosaic equals, byte for byte, the run that decodes every file twice
    (grayscale for the pairs, colour for the mosaic: Stitcher.py:68-69, 382-403), for fadeInAndFadeOut and for average."""
    from PIL import Image
    from imagestitch_amd import stitcher as ST
    g = SyntheticGrid(3, 3, 768, overlap=0.15)
    proj = tmp_path / "demo"; (proj / "1").mkdir(parents=True)
    files = _colour_jpegs(proj / "1", g, "1")
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod,
           isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate)
    counts = {"once": 0, "imread": 0}
    real_once, real_imread = ST._decode_once, ST._imread

    def once(path, color):
        counts["once"] += 1
        return real_once(path, color)

    def imread(path, color):
        counts["imread"] += 1
        return real_imread(path, color)
    real_native = ST._fill_from_jpeg

    def native(eng, path, hg, hc):                             # the library's own decoder took the file: that is its one decode
        ok = real_native(eng, path, hg, hc)
        counts["once"] += bool(ok)
        return ok
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode = 1, 0.2, True
        isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = "surf", 3
        for fuse in ("fadeInAndFadeOut", "average"):
            isa.Stitcher.fuseMethod = fuse
            outs = []
            for once_only in (True, False):
                st = isa.Stitcher(); st._engine = engine if once_only else _NoIngest(engine)
                isa.Stitcher.direction = 1; st.direction = 1
                msgs = []
                st.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
                out = tmp_path / ("out_%s_%d" % (fuse, once_only))
                counts["once"] = counts["imread"] = 0
                ST._decode_once, ST._imread, ST._fill_from_jpeg = once, imread, native
                os.environ["VFSMS_NATIVE_JPEG"] = "1" if fuse == "fadeInAndFadeOut" else "0"      # either decoder: the library's, Pillow's
                try:
                    st.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, st.calculateOffsetForFeatureSearchIncre,
                                                 startNum=1, fileExtension="jpg", outputfileExtension="png")
                finally:
                    ST._decode_once, ST._imread, ST._fill_from_jpeg = real_once, real_imread, real_native
                    os.environ.pop("VFSMS_NATIVE_JPEG", None)
                if once_only:
                    assert counts == {"once": len(files), "imread": 0}, counts
                else:
                    assert counts["imread"] >= 2 * len(files) - 1, counts
                outs.append(([m for m in msgs if "offset of stitching" in m], np.asarray(Image.open(str(out / "stitching_result_1.png")))))
            assert outs[0][0] == outs[1][0] and len(outs[0][0]) == 8
            assert outs[0][1].ndim == 3 and np.array_equal(outs[0][1], outs[1][1])
            assert outs[0][1].shape[0] > 2 * 768 and outs[0][1][:, :, 0].std() > 5 and not np.array_equal(outs[0][1][:, :, 0], outs[0][1][:, :, 2])
    finally:
        (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod,
         isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate) = old


@pytest.mark.gpu
def test_phase_batch_on_dendritic_crops_against_stitcher_py_87(engine, oracle, golden_dir):
    """The HIP phase correlation (rocFFT batch + the four kernels) on the 25 committed dendriticCrystal strip pairs: every row equals the
    oracle's (integer offsets exact, sub-pixel peak 1e-6, response 1e-9) AND, sign-fixed and axis-corrected as Stitcher.phaseSignFix does,
    lies within 1.5 px of the reference's own offset list (Stitcher.py:87) modulo the padded strip."""
    import json
    from test_oracle_golden import phase87_residual
    d = json.load(open(os.path.join(golden_dir, "dendritic_phase87.json")))["crops"]
    z = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    by_shape = {}
    for r in d:
        by_shape.setdefault(tuple(r["roi"]), []).append(r)
    assert len(by_shape) == 2                                              # 387 x 640 row strips, 640 x 516 column strips
    for shape, rows in by_shape.items():
        hs, jobs = [], []
        try:
            for r in rows:
                ha, hb = engine.tile_upload(np.ascontiguousarray(z[r["key_a"]])), engine.tile_upload(np.ascontiguousarray(z[r["key_b"]]))
                hs += [ha, hb]
                jobs.append((ha, hb, 0, 0, 0, 0, shape[0], shape[1]))
            out = engine.attempt_phase_batch(jobs)                           # one launch for all pairs of a shape
        finally:
            for h in hs:
                engine.tile_free(h)
        for r, (x, y, resp) in zip(rows, out):
            (ox, oy), orr = oracle.phase_correlate(np.ascontiguousarray(z[r["key_a"]]), np.ascontiguousarray(z[r["key_b"]]))
            assert int(x) == int(ox) and int(y) == int(oy) and abs(x - ox) < 1e-6 and abs(y - oy) < 1e-6 and abs(resp - orr) < 1e-9, (r["a"], x, ox, y, oy)
            ry, rx = phase87_residual(r, (x, y))
            assert max(abs(ry), abs(rx)) <= 1.5, (r["a"], ry, rx)
            assert bool(resp > 0.15) == r["accepted"]


@pytest.mark.gpu
def test_line_scan_batched_full_image_path_orb(engine, oracle, tmp_path):
    """The same scans with featureMethod = "orb" (Stitcher.py:260-304 over ImageUtility.py:260, 297-302): the batched whole-tile path
    (N - 1 fused ORB attempts) reports what the pair-by-pair mirror reports -- status, offsets, log lines, the break -- and its first rows
    equal the oracle's chain (ORB of both tiles, BF-Hamming 1-NN, mode vote) on the same tiles."""
    from PIL import Image
    tiles, truth = _line_scan()
    tiles = tiles[:5]
    files = []
    for k, t in enumerate(tiles):
        f = os.path.join(str(tmp_path), "oscan_%02d.png" % k)
        Image.fromarray(t).save(f); files.append(f)
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.isEnhance,
           isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod)
    try:
        isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = 4, 0, "orb", 10
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod, isa.Stitcher.isEnhance = False, "notFuse", False
        seq = isa.Stitcher(); seq._engine = engine; seq.isPrintLog = False
        seq.tempImageFeature.isBreak = True
        want = [seq.calculateOffsetForFeatureSearch([tiles[k], tiles[k + 1]]) for k in range(len(tiles) - 1)]
        seq.releaseTiles()
        st = isa.Stitcher(); st._engine = engine
        msgs = []
        st.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
        got = st._registerBatched(files, st.calculateOffsetForFeatureSearch)
        assert got is not None, "the batched ORB full-image path did not engage"
        status, end, offs, _desc = got
        for h, _s in (st.__dict__.pop("_resident", None) or {}).values():
            engine.tile_free(h)
        assert all(w[0] for w in want) and status and end == len(tiles) - 1 and offs == [w[1] for w in want], (offs, want)
        for k, o in enumerate(offs):
            assert abs(o[0] - truth[k][0]) <= 1 and abs(o[1] - truth[k][1]) <= 1
            assert "  The offset of stitching: dx is %d dy is %d" % (o[0], o[1]) in msgs
        ka, da = oracle.orb_detect_describe(tiles[0]); kb, db = oracle.orb_detect_describe(tiles[1])
        pairs, _ = oracle.bf_hamming_matches(da, db)
        ost, ooff, _votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 10)
        assert ost and list(ooff) == offs[0]
        Image.fromarray(np.zeros_like(tiles[0])).save(files[3])
        st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
        status, end, offs, desc = st._registerBatched(files, st.calculateOffsetForFeatureSearch)
        for h, _s in (st.__dict__.pop("_resident", None) or {}).values():
            engine.tile_free(h)
        assert status is False and end == 2 and len(offs) == 2 and "can not be stitched" in desc
    finally:
        (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.isEnhance,
         isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod) = old
        isa.Stitcher.tempImageFeature.isBreak = True


@pytest.mark.gpu
def test_driver_with_registration_breaks_decodes_once_and_matches_the_pair_loop(engine, tmp_path):
    """imageSetStitchWithMutiple over a folder whose middle tile is blank (two pairs cannot be registered: three segments, Stitcher.py:96-127),
    colour JPEGs: the batched path decodes every file ONCE across both restarts (the tiles behind a break wait in HBM for their segment)
    and writes the files -- names and bytes -- of the pair-by-pair run that decodes gray and colour separately."""
    from PIL import Image
    from imagestitch_amd import stitcher as ST
    g = SyntheticGrid(1, 5, 512, overlap=0.2)
    proj = tmp_path / "brk"; (proj / "1").mkdir(parents=True)
    files = _colour_jpegs(proj / "1", g, "1")
    Image.fromarray(np.full((512, 512, 3), 90, np.uint8)).save(files[2], quality=92)          # nothing to match in tile 2
    old = (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod,
           isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate)
    counts = {"once": 0, "imread": 0}
    real_once, real_imread = ST._decode_once, ST._imread

    def once(path, color):
        counts["once"] += 1
        return real_once(path, color)

    def imread(path, color):
        counts["imread"] += 1
        return real_imread(path, color)
    real_native = ST._fill_from_jpeg

    def native(eng, path, hg, hc):                             # the library's own decoder took the file: that is its one decode
        ok = real_native(eng, path, hg, hc)
        counts["once"] += bool(ok)
        return ok
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode = 1, 0.2, True
        isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate, isa.Stitcher.fuseMethod = "surf", 3, "fadeInAndFadeOut"
        outs = []
        for once_only in (True, False):
            st = isa.Stitcher(); st._engine = engine if once_only else _NoIngest(engine); st.isPrintLog = False
            st.batchRegistration = once_only
            isa.Stitcher.direction = 2; st.direction = 2
            out = tmp_path / ("o%d" % once_only)
            counts["once"] = counts["imread"] = 0
            ST._decode_once, ST._imread, ST._fill_from_jpeg = once, imread, native
            try:
                st.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, st.calculateOffsetForFeatureSearchIncre,
                                             startNum=1, fileExtension="jpg", outputfileExtension="png")
            finally:
                ST._decode_once, ST._imread, ST._fill_from_jpeg = real_once, real_imread, real_native
            if once_only:
                assert counts == {"once": len(files), "imread": 0}, counts
            names = sorted(n for n in os.listdir(str(out)) if n.endswith(".png"))
            outs.append({n: np.asarray(Image.open(str(out / n))) for n in names})
        assert sorted(outs[0]) == sorted(outs[1]) == ["stitching_result_1_1.png", "stitching_result_1_2.png", "stitching_result_1_3.png"], sorted(outs[0])
        for n in outs[0]:
            assert outs[0][n].shape == outs[1][n].shape and np.array_equal(outs[0][n], outs[1][n]), n
        assert outs[0]["stitching_result_1_2.png"].shape[:2] == (512, 512)                    # the blank tile alone
    finally:
        (isa.Stitcher.direction, isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod,
         isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate) = old


@pytest.mark.gpu
def test_rccl_all_gather_at_world_size_1(tmp_path):
    """Row e on hardware: the pair-sharded registration with the REAL collective -- torch.distributed "nccl" (= RCCL), device tensors on
    cuda:0, imagestitch_amd.distributed.make_all_gather -- at world size 1, in a process of its own (tests/rccl_worker.py; the same worker runs
    under torchrun at N = 8).  The sharded table (cold and with a primed path memory) equals GridRegistrar.register's and the ground truth
    within 1 px: RCCL start-up, the device / host tensor hand-over and the one all_gather of the path have run on an MI355X before the first
    8-GPU job does."""
    import json
    import subprocess
    import sys
    out = tmp_path / "rccl.json"
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29537", HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_worker.py")
    p = subprocess.run([sys.executable, worker, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.load(open(out))
    assert r["backend"] == "nccl" and r["world"] == 1 and r["device"] == "cuda:0" and r["gathered_shape"] == [1, 7]
    assert r["rows"] == r["rows_register"] == r["rows_single"] == r["rows_primed"]
    assert len(set(r["direction"])) == 1 and r["repairs"] == 0
    for row, t in zip(r["rows"], r["truth"]):
        assert row[0] == 1 and abs(row[1] - t[0]) <= 1 and abs(row[2] - t[1]) <= 1, (row, t)


@pytest.mark.gpu
def test_full_width_dendritic_strips_surf_and_orb_equal_the_oracle_rows(engine, golden_dir):
    """configs[1] at its real load (tests/golden/real_full_strips.*, tools/capture_golden.py realfull): the UNCROPPED ROI strips of two
    dendriticCrystal pairs -- 004-005, a column pair (387 x 2584, 13.3 k / 13.5 k SURF keypoints), and 015-016, a serpentine turn
    (1936 x 516) -- through vfsms_attempt_surf_batch and vfsms_attempt_orb_batch, both shapes in ONE batch.  Every row equals the
    oracle's attempt row of dendritic_path_oracle*.json ([status, raw dx, raw dy, votes, nA, nB, matches]) and, with the axis
    correction, lands within 1 px of Stitcher.py:87.  (The 25 neighbourhood pairs are 640-px crops with 2.6 k keypoints per strip.)"""
    import json
    meta = json.load(open(os.path.join(golden_dir, "real_full_strips.json")))["pairs"]
    z = np.load(os.path.join(golden_dir, "real_full_strips.npz"))
    hs, jobs = [], []
    for m in meta:
        a, b = z["p%d_a" % m["a"]], z["p%d_b" % m["a"]]
        assert a.shape == b.shape == tuple(m["roi_first"][2:])
        ha, hb = engine.tile_upload(a), engine.tile_upload(b)
        hs += [ha, hb]
        jobs.append((ha, hb, 0, 0, 0, 0, a.shape[0], a.shape[1]))
    engine.set_keypoint_capacity(0)                     # the default: h w / 24 + 4096 candidates per ROI (45 k for these strips)
    srows = engine.attempt_surf_batch(jobs)
    orows = engine.attempt_orb_batch(jobs)
    for m, sr, orr in zip(meta, srows, orows):
        assert sr[:7].tolist() == m["expected_surf"], (m["a"], sr[:7].tolist(), m["expected_surf"])
        assert orr[:7].tolist() == m["expected_orb"], (m["a"], orr[:7].tolist(), m["expected_orb"])
        H, W = m["tile_shape"]
        for row in (sr, orr):
            off = [int(row[1]), int(row[2])]
            if m["direction"] == 1:
                off[0] += H - int(0.2 * H)
            elif m["direction"] == 2:
                off[1] += W - int(0.2 * W)
            assert abs(off[0] - m["gold"][0]) <= 1 and abs(off[1] - m["gold"][1]) <= 1, (m["a"], off, m["gold"])
    for h in hs:
        engine.tile_free(h)


@pytest.mark.gpu
def test_mode_vote_beyond_one_hash_table_equals_the_oracle(engine, oracle):
    """Method.getOffsetByMode (ImageUtility.py:150-170) with MORE votes than one pass of k_scan_mode's LDS table takes (> 5600: configs[4]'s
    819 x 4096 strips leave 6-9 k ratio-test survivors): the votes go through several passes of the table, dealt by a hash of the tuple.  The
    most frequent (dx, dy), ties to the tuple that occurs FIRST in match order, and its count equal the oracle's for planted ties (two
    tuples with the same count in both orders), a dominant mode, all-distinct tuples and zero votes."""
    rng = np.random.default_rng(321)

    def case(n, tuples, counts, shuffle_seed):
        """n matches; tuple t is voted counts[t] times, the rest are distinct tuples"""
        offs = []
        for t, c in zip(tuples, counts):
            offs += [t] * c
        k = 0
        while len(offs) < n:
            offs.append((1000 + k % 4000, -3000 + k // 4000)); k += 1
        offs = np.array(offs, np.int64)
        np.random.default_rng(shuffle_seed).shuffle(offs)
        kb = rng.integers(5000, 9000, (n, 2)).astype(np.float32)
        ka = kb + offs[:, ::-1].astype(np.float32)            # vote = (int(yA - yB), int(xA - xB)): dx = rows, dy = columns
        pairs = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
        return ka, kb, pairs
    cases = [case(9000, [(7, -3), (-12, 40)], [50, 50], 1), case(9000, [(7, -3), (-12, 40)], [50, 50], 2),
             case(20000, [(3, 4)], [6000], 3), case(12000, [], [], 4), case(5601, [(1, 1), (2, 2), (0, 5)], [3, 3, 2], 5),
             case(30000, [(9, 9), (8, 8)], [2, 3], 6)]
    for ci, (ka, kb, pairs) in enumerate(cases):
        for ev in (3, 10):
            got = engine.mode_offset(ka, kb, pairs, ev)
            want = oracle.mode_offset(ka, kb, pairs, ev)
            assert (bool(got[0]), list(got[1]), int(got[2])) == (bool(want[0]), [int(want[1][0]), int(want[1][1])], int(want[2])), (ci, ev, got, want)


@pytest.mark.gpu
def test_descriptor_work_list_one_ticket_per_keypoint_regime(engine, oracle):
    """The descriptor kernels draw their keypoints from k_desc_plan's work list in two regimes: small launches split every window > 256 px
    into 21 tickets (one per output row of the patch), launches with more than 48 large-window keypoints per resident workgroup
    (1280 x 48 = 61440) keep one ticket per keypoint.  The single-ROI entry points the other parity tests use are all in the first
    regime; here 16 whole tiles of 1024 x 1280 go through vfsms_features_surf_batch in ONE fused launch sequence (78 k windows > 64 px: the
    second regime, XCD-affine heads over 16 ROIs, every head owning two of them) and every tile's keypoints and descriptors must be
    bit-identical to the tile described on its own -- and two of them to the oracle."""
    from imagestitch_amd.synthetic import line_scan
    tiles, _truth = line_scan(n=16)
    hs = [engine.tile_upload(t) for t in tiles]
    engine.set_keypoint_capacity(0)
    feats, counts = engine.features_surf_batch(hs)
    try:
        big = 0
        for k, (t, f, n) in enumerate(zip(tiles, feats, counts)):
            kxy, desc = engine.features_download(f, n)
            sxy, sdesc, kf = engine.surf_detect_describe(t, full=True)
            assert n == len(sxy) and np.array_equal(kxy, sxy) and np.array_equal(desc, sdesc), k
            win = np.minimum((21 * (kf["size"] * np.float32(1.2) / np.float32(9.0))).astype(np.int64), 739)
            big += int((win > 64).sum())
            if k in (0, 9):
                ok, od = oracle.surf_detect_describe(t)
                assert len(ok) == n and np.array_equal(desc, od), k
        assert big >= 1280 * 48, big                       # the launch really was in the one-ticket-per-keypoint regime
    finally:
        for f in feats:
            engine.features_free(f)
        for h in hs:
            engine.tile_free(h)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["surf", "orb", "phase"])
def test_projected_shards_reproduce_the_one_gpu_table_on_the_device(engine, method):
    """`bench.py --project-shards` (GridRegistrar.register_projected): the pair-sharded step of 2, 3 and 5 ranks run rank after rank on
    the one device -- cold (no path memory: blind chunk starts + direction stitch-up in assemble) and warm (path memory as the prior:
    hinted starts, speculation plan, repair round when a hint fails) -- gives the table and final direction of the one-GPU walk
    (Stitcher.py:196-217's direction threading), row for row."""
    from imagestitch_amd.grid import GridRegistrar
    g = SyntheticGrid(3, 4, 1024, overlap=0.10)
    tiles = g.tiles(threads=4)
    shapes = [t.shape for t in tiles]
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        one = GridRegistrar(engine, method=method, roiRatio=0.2, offsetEvaluate=3, directIncre=1)
        want, d_want = one.register(hs, shapes, 1)
        assert int(want[:, 0].sum()) >= len(tiles) - 2, want
        for world in (2, 3, 5):
            rp = GridRegistrar(engine, method=method, roiRatio=0.2, offsetEvaluate=3, directIncre=1)
            cold, d_cold, per_rank, _tail = rp.register_projected(hs, shapes, 1, world)
            assert np.array_equal(cold, want) and d_cold == d_want, (method, world, "cold")
            assert sum(q["pairs"] for q in per_rank) == len(tiles) - 1
            warm, d_warm, per_rank, _tail = rp.register_projected(hs, shapes, 1, world)      # path memory of the cold step is the prior now
            assert np.array_equal(warm, want) and d_warm == d_want, (method, world, "warm")
            assert 0 < sum(q["attempts"] for q in per_rank) <= sum(int(r[4]) + 1 for r in want) + world * 8, per_rank
    finally:
        for h in hs:
            engine.tile_free(h)


@pytest.mark.gpu
def test_mosaic_walk_hand_off_is_stable_over_repeated_assemblies(engine):
    """The stats -> weights hand-off of the fuse kernels carries no agent-scope fence since round 6 (slots written and read with
    agent-scope atomics, the ticket orders them): 24 assemblies of the same 3 x 3 mosaic of 2048 x 2048 tiles, alternating with a second
    geometry so that the slots are rewritten with other values in between, give the same canvas bytes every time."""
    import zlib
    T = 2048
    g = SyntheticGrid(3, 3, T)
    tiles = g.tiles(threads=4)
    n = len(tiles)
    handles = [engine.tile_upload(t) for t in tiles]

    def geometry(offs):
        offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout([t.shape for t in tiles], offs)
        rois = [None] + [(max(offsetList[i][0], rangeX[i - 1][0]), max(offsetList[i][1], rangeY[i - 1][0]),
                          min(offsetList[i][0] + T, rangeX[i - 1][1]), min(offsetList[i][1] + T, rangeY[i - 1][1])) for i in range(1, n)]
        geom = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
        geom += [(offsetList[i][0], offsetList[i][1]) + tuple(rois[i]) + (offs[i][0], offs[i][1], 0) for i in range(1, n)]
        return geom, rows, cols
    offs_a = [[0, 0]] + [list(map(int, o)) for o in g.true_offsets()]
    offs_b = [[0, 0]] + [[o[0] + (7 if o[0] > 0 else -7 if o[0] < 0 else 3), o[1] + (5 if k % 2 else -5)] for k, o in enumerate(offs_a[1:])]
    seen = {}
    try:
        for rep in range(24):
            tag, offs = ("a", offs_a) if rep % 2 == 0 else ("b", offs_b)
            geom, rows, cols = geometry(offs)
            cv = engine.canvas_create(rows, cols, 1)
            try:
                engine.canvas_assemble_resident(cv, handles, geom)
                crc = zlib.crc32(engine.canvas_download(cv, rows, cols, 1).tobytes())
            finally:
                engine.canvas_free(cv)
            assert seen.setdefault(tag, crc) == crc, (rep, tag)
    finally:
        for h in handles:
            engine.tile_free(h)
    assert len(seen) == 2 and seen["a"] != seen["b"]


@pytest.mark.gpu
def test_phase_peak_on_the_odd_last_row_or_column(engine, oracle):
    """phasecorr.cpp's fftShift (OpenCV 3.3.1) swaps quadrants of (M >> 1) x (N >> 1): with an odd padded size (5, 15, 25, 45, 75, 625 ...) the
    last row / column lies outside every quadrant and does not move along EITHER axis.  Unrelated small strips put the peak anywhere, so over
    these shapes and seeds it lands on that row or column (or within the 5 x 5 centroid window of it) many times: every one must equal the
    oracle (1e-6 px, 1e-9 response, truncated offsets exact), through the single-pair call and the batched one, in both orientations."""
    from phase_numpy import phase_correlate as np_phase, optimal_dft_size
    shapes = [(5, 7), (7, 5), (15, 9), (9, 15), (25, 27), (27, 25), (45, 75), (75, 45), (13, 40), (40, 13), (5, 5), (3, 9), (9, 3), (25, 64), (64, 25)]
    touched = 0
    for shp in shapes:
        M, N = optimal_dft_size(shp[0]), optimal_dft_size(shp[1])
        for seed in range(6):
            a, b = _rand_img(100 + seed, shp), _rand_img(200 + seed, shp)
            (ox, oy), orr = oracle.phase_correlate(np.ascontiguousarray(a), np.ascontiguousarray(b))
            _xy, _r, (py, px) = np_phase(a, b)
            touched += int((M % 2 == 1 and py + 2 >= M - 1) or (N % 2 == 1 and px + 2 >= N - 1))
            (x, y), r = engine.phase_correlate(a, b)
            assert abs(x - ox) < 1e-6 and abs(y - oy) < 1e-6 and abs(r - orr) < 1e-9, (shp, seed, (x, y, r), (ox, oy, orr), (py, px))
            assert [int(y), int(x)] == [int(oy), int(ox)]
            ha, hb = engine.tile_upload(a), engine.tile_upload(b)
            row = engine.attempt_phase_batch([(ha, hb, 0, 0, 0, 0, shp[0], shp[1])] * 3)
            engine.tile_free(ha); engine.tile_free(hb)
            for q in row:
                assert abs(q[0] - ox) < 1e-6 and abs(q[1] - oy) < 1e-6 and abs(q[2] - orr) < 1e-9, (shp, seed, q, (ox, oy, orr))
    assert touched >= 20, touched


@pytest.mark.gpu
def test_phase_lds_transforms_equal_the_rocfft_path_and_the_oracle_over_strip_shapes(engine, oracle):
    """The hand-written FP64 transforms (csrc/phase_kernels.hip: packed real rows, column kernel with cross power, radix 16 / 9 / 8 / 6 / 10 / 4 /
    3 / 5 / 2 passes) against the rocFFT plans of rounds 2-5 (VFSMS_PHASE_LDS_FFT=0, same process) and the CPU oracle on the strip shapes of the
    datasets and then some: both orientations (tall strips run transposed), 3- and 5-smooth paddings, an odd column length (614 -> 625), tiny
    strips, the config sizes.  1e-9 px between the two device paths, 1e-6 px / 1e-9 response against the oracle (Stitcher.py:230)."""
    shapes = [(409, 2048), (2048, 409), (387, 2584), (2584, 387), (614, 1280), (1280, 614), (204, 1024), (1024, 256), (128, 640), (97, 131), (131, 97),
              (625, 64), (64, 625), (80, 96), (16, 16), (6, 10), (37, 64), (300, 1000), (100, 100), (2, 2), (243, 250), (50, 54), (27, 20), (3, 4)]
    keep = os.environ.get("VFSMS_PHASE_LDS_FFT")
    took_lds = 0
    try:
        for k, shp in enumerate(shapes):
            a = _rand_img(300 + k, shp)
            dy, dx = min(5, shp[0] // 3), -min(9, shp[1] // 3)
            b = np.roll(np.roll(a, dy, 0), dx, 1)
            b = (b.astype(np.int32) + (_rand_img(400 + k, shp) >> 3)).clip(0, 255).astype(np.uint8)
            os.environ["VFSMS_PHASE_LDS_FFT"] = "1"
            took_lds += engine.phase_plan(*shp)["lds_transforms"]
            (x1, y1), r1 = engine.phase_correlate(a, b)
            os.environ["VFSMS_PHASE_LDS_FFT"] = "0"
            assert engine.phase_plan(*shp)["lds_transforms"] == 0
            (x0, y0), r0 = engine.phase_correlate(a, b)
            # relative where the centroid's weight sum is next to zero (a few-pixel strip: the quotient is in the millions of pixels)
            sx, sy = max(1.0, abs(x0)), max(1.0, abs(y0))
            assert abs(x1 - x0) < 1e-8 * sx and abs(y1 - y0) < 1e-8 * sy and abs(r1 - r0) < 1e-12, (shp, (x1, y1, r1), (x0, y0, r0))
            if shp[0] * shp[1] <= 1 << 20:
                (ox, oy), orr = oracle.phase_correlate(np.ascontiguousarray(a), np.ascontiguousarray(b))
                assert abs(x1 - ox) < 1e-6 * sx and abs(y1 - oy) < 1e-6 * sy and abs(r1 - orr) < 1e-9, (shp, (x1, y1, r1), (ox, oy, orr))
    finally:
        if keep is None:
            os.environ.pop("VFSMS_PHASE_LDS_FFT", None)
        else:
            os.environ["VFSMS_PHASE_LDS_FFT"] = keep
    assert took_lds >= len(shapes) - 2, took_lds               # (2, 2) pads to a 2-point row (rocFFT); everything else runs in LDS


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True])
def test_strip_tiles_fused_from_the_rectangle_list_equal_the_statistics_path(engine, colour):
    """Since round 6 the host counts the valid pixels of a fuse ROI from the rectangles placed on the canvas (ImageFusion.py:201's count / size >
    0.65) and blends a strip tile in ONE launch with closed-form ramps; corner tiles keep the statistics kernel.  The same 3 x 3 serpentine mosaic
    (strip ROIs, whole-tile ROIs after the turns, fade and trigonometric operators, negative and positive dx / dy) assembled with the analytic path
    on and off (VFSMS_FUSE_ANALYTIC=0) must be the same bytes, and so must the per-tile calls with their info rows."""
    T = 768
    g = SyntheticGrid(3, 3, T)
    tiles = g.tiles(threads=4)
    if colour:
        tiles = [np.ascontiguousarray(np.stack([t, 255 - t, (t // 2) + 17], -1).astype(np.uint8)) for t in tiles]
    n = len(tiles)
    ch = 3 if colour else 1
    offs = [[0, 0]] + [list(map(int, o)) for o in g.true_offsets()]
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout([t.shape[:2] for t in tiles], offs)
    rois = [None] + [(max(offsetList[i][0], rangeX[i - 1][0]), max(offsetList[i][1], rangeY[i - 1][0]),
                      min(offsetList[i][0] + T, rangeX[i - 1][1]), min(offsetList[i][1] + T, rangeY[i - 1][1])) for i in range(1, n)]
    handles = [(engine.tile_upload_color(t) if colour else engine.tile_upload(t)) for t in tiles]
    keep = os.environ.get("VFSMS_FUSE_ANALYTIC")
    got = {}
    try:
        for method in (0, 1):
            geom = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
            geom += [(offsetList[i][0], offsetList[i][1]) + tuple(rois[i]) + (offs[i][0], offs[i][1], method) for i in range(1, n)]
            for flag in ("1", "0"):
                os.environ["VFSMS_FUSE_ANALYTIC"] = flag
                cv = engine.canvas_create(rows, cols, ch)
                try:
                    engine.canvas_assemble_resident(cv, handles, geom)
                    got[(method, flag)] = engine.canvas_download(cv, rows, cols, ch)
                finally:
                    engine.canvas_free(cv)
            assert np.array_equal(got[(method, "1")], got[(method, "0")]), method
        assert not np.array_equal(got[(0, "1")], got[(1, "1")])
    finally:
        if keep is None:
            os.environ.pop("VFSMS_FUSE_ANALYTIC", None)
        else:
            os.environ["VFSMS_FUSE_ANALYTIC"] = keep
        for h in handles:
            engine.tile_free(h)


@pytest.mark.gpu
def test_random_placements_fused_from_the_rectangle_list_equal_the_statistics_path(engine):
    """The host-side geometry of round 6 (valid count, getWeightsMatrix's rowIndex / colIndex for the four quadrants, the degenerate cases) against
    the statistics kernel on placements no serpentine produces: tiles dropped left of, above, below and across earlier ones (all four `index`
    quadrants, scans from both sides, negative dx / dy), ROI = tile rectangle cut by the bounding box of what lies there (Stitcher.py:446-457)
    or a random sub-rectangle of the tile.  Same bytes, and the same verdict on a degenerate geometry (both raise or neither).
    Path against path only: tests/test_canvas_reference_gpu.py holds these layouts (tests/canvas_cases.random_canvases) to the reference walk."""
    rng = np.random.default_rng(20190158)
    keep = os.environ.get("VFSMS_FUSE_ANALYTIC")
    n_err = n_corner = 0
    try:
        for case in range(40):
            rows, cols = int(rng.integers(500, 900)), int(rng.integers(500, 900))
            ntile = int(rng.integers(3, 8))
            tiles, geom = [], []
            bbox = None
            for k in range(ntile):
                th, tw = int(rng.integers(90, 320)), int(rng.integers(90, 320))
                y0, x0 = int(rng.integers(0, rows - th)), int(rng.integers(0, cols - tw))
                t = rng.integers(0, 256, (th, tw), dtype=np.uint8)
                if case % 5 == 0:
                    t[rng.random((th, tw)) < 0.3] = 0                            # black pixels: the quadrant counts are not the valid areas
                tiles.append(t)
                if bbox is None:
                    geom.append((y0, x0, 0, 0, 0, 0, 0, 0, -1))
                    bbox = [y0, x0, y0 + th, x0 + tw]
                    continue
                if case % 3 == 2:                                                    # any sub-rectangle of the tile
                    ry0 = y0 + int(rng.integers(0, th // 2)); rx0 = x0 + int(rng.integers(0, tw // 2))
                    ry1 = int(rng.integers(ry0 + 2, y0 + th + 1)); rx1 = int(rng.integers(rx0 + 2, x0 + tw + 1))
                else:
                    ry0, rx0, ry1, rx1 = max(y0, bbox[0]), max(x0, bbox[1]), min(y0 + th, bbox[2]), min(x0 + tw, bbox[3])
                if ry1 <= ry0 or rx1 <= rx0:
                    geom.append((y0, x0, 0, 0, 0, 0, 0, 0, -1))
                else:
                    geom.append((y0, x0, ry0, rx0, ry1, rx1, int(rng.integers(-40, 41)), int(rng.integers(-40, 41)), int(rng.integers(0, 2))))
                bbox = [min(bbox[0], y0), min(bbox[1], x0), max(bbox[2], y0 + th), max(bbox[3], x0 + tw)]
            hs = [engine.tile_upload(t) for t in tiles]
            res = {}
            for flag in ("1", "0"):
                os.environ["VFSMS_FUSE_ANALYTIC"] = flag
                cv = engine.canvas_create(rows, cols, 1)
                try:
                    engine.canvas_assemble_resident(cv, hs, geom)
                    try:
                        res[flag] = engine.canvas_download(cv, rows, cols, 1)
                    except isa.VfsmsError as e:
                        assert "degenerate" in str(e)
                        res[flag] = None
                finally:
                    engine.canvas_free(cv)
            for h in hs:
                engine.tile_free(h)
            assert (res["1"] is None) == (res["0"] is None), (case, geom)
            if res["1"] is None:
                n_err += 1
            else:
                assert np.array_equal(res["1"], res["0"]), (case, geom)
            n_corner += sum(1 for g in geom if g[8] >= 0)
    finally:
        if keep is None:
            os.environ.pop("VFSMS_FUSE_ANALYTIC", None)
        else:
            os.environ["VFSMS_FUSE_ANALYTIC"] = keep
    print("random placements: %d fused tiles, %d of 40 canvases with a degenerate geometry" % (n_corner, n_err))
    assert n_corner > 100 and n_err < 30, (n_corner, n_err)
