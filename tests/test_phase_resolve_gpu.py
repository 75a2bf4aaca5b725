"""GPU tests of Stitcher.phaseResolve = "ncc" (csrc/phase_resolve_kernels.hip) against its specification, tests/phase_resolve_ref.py:
rows and candidate tables are integer sums behind a fixed float64 tail and equal the reference exactly; the peak LIST hangs on the
transforms' rounding (the device's differ from pocketfft's by 1e-13 elsewhere in the suite), so every input here is one whose reference
surface shows its top K + 1 peak values, and each peak and its neighbours, a relative 1e-6 apart -- asserted with the reference, never
skipped -- or is exactly zero (a black strip: the transforms of zeros are zeros on any IEEE implementation)."""
import functools
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.grid import GridRegistrar

from phase_cases import resident
import phase_resolve_cases as PC
import phase_resolve_ref as PR

pytestmark = pytest.mark.gpu

K = 2
SHAPES = [(48, 160), (160, 48), (45, 75), (49, 97)]
PLANS = {(48, 160): (1, 0), (160, 48): (1, 1), (45, 75): (0, 0), (49, 97): (1, 0)}      # (LDS transforms, correlated as the transpose)


@functools.lru_cache(maxsize=None)
def batch(shape):
    """the jobs of one strip shape, mixing every CPU case -> [(name, A, B)]: wrapped shifts of both signs, a zero shift (with grey-level
    noise: identical strips make the second peak a matter of rounding), the second-peak case, the refusals"""
    h, w = shape
    jobs = [("shift %r" % (s,),) + PC.cut(h, w, *s) for s in PC.SHIFTS[shape][:4]]
    A, B = PC.cut(h, w, 0, 0)
    jobs.append(("zero shift", A, PC.noisy(B)))
    s = PC.SHIFTS[shape][0]
    jobs.append(("bar",) + PC.bar_pair(h, w, s[0], s[1], 2))
    jobs.append(("disjoint",) + PC.disjoint(h, w))
    jobs.append(("flat",) + PC.flat(h, w))
    return jobs


@functools.lru_cache(maxsize=None)
def reference(shape, min_pixels=PC.MIN_PIXELS):
    out = []
    for name, A, B in (batch(shape) if shape != "production" else [("production",) + PC.production_pair()]):
        R = PR.surface(A, B)
        r = PR.resolve(A, B, K, PC.THRESHOLD, min_pixels, R=R)
        # the condition under which the peak list does not hang on the transform's rounding
        assert PR.peak_gap_ok(R, K) or not R.any(), (shape, name)
        out.append(r)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_equals_the_reference(engine, shape):
    plan = engine.phase_plan(*shape)
    assert (plan["lds_transforms"], plan["transposed"]) == PLANS[shape]
    strips = batch(shape)
    assert len(strips) >= 6
    ref = reference(shape)
    handles, jobs = resident(engine, strips)
    try:
        rows, cands, pk = engine.attempt_phase_resolve_batch(jobs, K, PC.THRESHOLD, PC.MIN_PIXELS)
    finally:
        for hd in handles:
            engine.tile_free(hd)
    for k, ((name, _A, _B), r) in enumerate(zip(strips, ref)):
        assert pk[k].tolist() == r["peaks"].tolist(), (shape, name)
        assert cands[k].tolist() == r["cands"].tolist(), (shape, name)
        assert rows[k].tolist() == r["row"].tolist(), (shape, name)
    # what the cases are about, on the device's own rows
    for k, s in enumerate(PC.SHIFTS[shape][:4]):
        assert rows[k, :3].tolist() == [1, s[0], s[1]]
    assert rows[4, :3].tolist() == [1, 0, 0]
    s = PC.SHIFTS[shape][0]
    assert pk[5, 0].tolist() == [0, 0] and rows[5, :3].tolist() == [1, s[0], s[1]] and 4 <= rows[5, 6] < 8
    assert rows[6, 0] == 0 and rows[7].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]


def test_production_strip_pair(engine):
    """one 409 x 2048 pair: the LDS configuration of the headline grid (432 x 2048), a shift wrapped on both axes"""
    plan = engine.phase_plan(409, 2048)
    assert (plan["lds_transforms"], plan["M"], plan["N"]) == (1, 432, 2048)
    A, B = PC.production_pair()
    r = reference("production", 4096)[0]
    assert r["row"][:3].tolist() == [1, 300, -1500] and r["peaks"][0].tolist() == [300, 548]
    handles, jobs = resident(engine, [("production", A, B)])
    try:
        rows, cands, pk = engine.attempt_phase_resolve_batch(jobs, K, PC.THRESHOLD, 4096)
    finally:
        for hd in handles:
            engine.tile_free(hd)
    assert pk[0].tolist() == r["peaks"].tolist() and cands[0].tolist() == r["cands"].tolist() and rows[0].tolist() == r["row"].tolist()


def test_mixed_shapes_and_peak_counts_in_one_batch(engine):
    """jobs of every shape in one call come back in the caller's order; K = 1 and K = 8 tables"""
    strips = [batch(s)[k] for k in (1, 5) for s in SHAPES]
    handles, jobs = resident(engine, strips)
    try:
        for kk in (1, 8):
            rows, cands, pk = engine.attempt_phase_resolve_batch(jobs, kk, PC.THRESHOLD, PC.MIN_PIXELS)
            for k, (_n, A, B) in enumerate(strips):
                r = PR.resolve(A, B, kk, PC.THRESHOLD, PC.MIN_PIXELS)
                assert rows[k].tolist() == r["row"].tolist() and pk[k, 0].tolist() == r["peaks"][0].tolist()
                if kk == 1:
                    assert cands[k].tolist() == r["cands"].tolist()
    finally:
        for hd in handles:
            engine.tile_free(hd)


def test_host_strips_equal_the_batch(engine):
    for shape in SHAPES:
        for (name, A, B), r in zip(batch(shape), reference(shape)):
            row, cands, pk = engine.phase_resolve(A, B, K, PC.THRESHOLD, PC.MIN_PIXELS)
            assert (row.tolist(), cands.tolist(), pk.tolist()) == (r["row"].tolist(), r["cands"].tolist(), r["peaks"].tolist()), (shape, name)


def test_arguments(engine):
    A, B = PC.cut(48, 160, 5, -7)
    for bad in (dict(peaks=0), dict(peaks=9), dict(threshold=1.5), dict(threshold=float("nan")), dict(min_pixels=-1)):
        with pytest.raises(isa.VfsmsError):
            engine.phase_resolve(A, B, **bad)
        with pytest.raises(isa.VfsmsError):
            engine.attempt_phase_resolve_batch([], **bad)
        with pytest.raises(isa.VfsmsError):
            engine.set_phase_resolver("ncc", **bad)
    with pytest.raises(isa.VfsmsError):
        engine.set_phase_resolver(2)
    assert engine.attempt_phase_resolve_batch([], 2)[0].shape == (0, 8)


@functools.lru_cache(maxsize=None)
def cpu_chain():
    from test_phase_resolve_host import reference_chain
    tiles, offsets, dirs = PC.grid_tiles()
    out, d_out, _st = reference_chain(tiles)
    assert out[:, 1:3].tolist() == offsets
    return tiles, out, d_out


def test_pairs_offsets_with_the_resolver_equal_the_cpu_chain(engine):
    tiles, want, d_want = cpu_chain()
    handles = [engine.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    try:
        p = engine.grid_params(method="phase", roiRatio=0.2, directIncre=1, window=8)
        off, _d, _s = engine.pairs_offsets(handles, shapes, p, stop_on_fail=True)                 # resolver off: the reference's reading, as before
        engine.set_phase_resolver("ncc", 2, 0.5, 4096)
        try:
            out, d_out, _st = engine.pairs_offsets(handles, shapes, p, stop_on_fail=True)
        finally:
            engine.set_phase_resolver("none")
        again, _d2, _s2 = engine.pairs_offsets(handles, shapes, p, stop_on_fail=True)
        assert out.tolist() == want.tolist() and d_out == d_want
        assert again.tolist() == off.tolist() and off.tolist() != out.tolist()
        for native in (True, False):
            reg = GridRegistrar(engine, method="phase", roiRatio=0.2, window=8, phaseResolve="ncc")
            reg.native = native
            table, d = reg.register(handles, shapes, 1, stop_on_fail=True)
            assert table.tolist() == want.tolist() and d == d_want
    finally:
        for hd in handles:
            engine.tile_free(hd)


def test_stitcher_pair_by_pair_and_batched(engine, tmp_path):
    from PIL import Image
    tiles, want, _d = cpu_chain()
    files = []
    for k, t in enumerate(tiles):
        f = os.path.join(str(tmp_path), "g_%02d.png" % k)
        Image.fromarray(t).save(f); files.append(f)

    def stitcher():
        st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
        st.isColorMode, st.roiRatio, st.direction, st.directIncre = False, 0.2, 1, 1
        st.phaseResolve = "ncc"
        return st
    st = stitcher()
    pairwise = [st.calculateOffsetForPhaseCorrleateIncre([tiles[k], tiles[k + 1]]) for k in range(len(tiles) - 1)]
    assert pairwise == [(True, o) for o in want[:, 1:3].tolist()] and st.direction == 1
    st = stitcher()
    st.phaseSignFix = True                                       # not consulted with the resolver on
    status, end, offsets, _desc = st._registerBatched(files, st.calculateOffsetForPhaseCorrleateIncre)
    assert status and end == len(tiles) - 1 and offsets == want[:, 1:3].tolist()
