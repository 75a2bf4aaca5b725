"""GPU tests of the hand-written FP64 transforms of csrc/phase_kernels.hip (packed real rows, the column kernel with the cross power, nine
butterflies as first and as later passes, the tiled spectrum layout, the __umulhi divisions, the transposed orientation, chunked batches)
against two float64 references that share no code with them or with each other: tests/phase_numpy.py (pocketfft) and the CPU oracle.
The cases, the bounds and where the bounds come from are in tests/phase_cases.py; test_phase_cases_host.py checks on the CPU everything
about them that concerns the references alone.

1. every length the LDS path can run (136 row half-lengths, 86 column lengths), a planted pair held to both references at 100 times the
   references' own disagreement, an unrelated pair held to the reference's four largest peaks;
2. peaks placed on the corners and edges of the surface (the clamped 5 x 5 window), through the LDS path, rocFFT and the batch entry;
3. all-black strips give exactly ((N / 2, M / 2), 0.0);
4. batches whose jobs all differ, both orientations in one call, under every chunk size, bit-identical to the single calls;
5. the workgroup geometries the environment can ask for, bit-identical to the default one;
6. one-row and one-column strips."""
import contextlib
import math
import os

import numpy as np
import pytest

import phase_cases as C

pytestmark = pytest.mark.gpu

KNOBS = ("VFSMS_PHASE_LDS_FFT", "VFSMS_PHASE_CHUNK", "VFSMS_PHASE_C", "VFSMS_PHASE_ROWPTS", "VFSMS_PHASE_TDIV", "VFSMS_PHASE_TCOL")


@contextlib.contextmanager
def knobs(**values):
    """the phase path's environment knobs (read with getenv on every call) for the length of a block: VFSMS_PHASE_<name> = value, None = unset"""
    keep = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for name, v in values.items():
            assert "VFSMS_PHASE_" + name in KNOBS
            if v is not None:
                os.environ["VFSMS_PHASE_" + name] = str(v)
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def correlate(engine, a, b):
    (x, y), r = engine.phase_correlate(a, b)
    return (x, y, r)


def batch_rows(engine, strips, resolve=None):
    """the strips as resident tiles (odd corners, strides that are no multiple of 16) through attempt_phase_batch, or with resolve = K through
    attempt_phase_resolve_batch"""
    handles, jobs = C.resident(engine, strips)
    try:
        if resolve is None:
            return engine.attempt_phase_batch(jobs)
        return engine.attempt_phase_resolve_batch(jobs, resolve, C.RESOLVE_THRESHOLD, C.RESOLVE_MIN_PIXELS)
    finally:
        for hd in handles:
            engine.tile_free(hd)


# ---- 1. the length sweep -------------------------------------------------------------------------------------------------------------
def test_every_length_takes_the_lds_transforms(engine):
    with knobs():
        rows = [engine.phase_plan(*s) for s in C.row_shapes()]
        cols = [engine.phase_plan(*s) for s in C.col_shapes()]
    assert all(p["lds_transforms"] == 1 and p["transposed"] == 0 for p in rows + cols)
    halves, lengths = sorted({p["N"] // 2 for p in rows}), sorted({p["M"] for p in cols})
    assert halves == C.ROW_HALF_LENGTHS and len(halves) == 136
    assert lengths == C.COL_LENGTHS and len(lengths) == 86
    # the restated host rule the accounting of test_phase_cases_host.py stands on answers as the library does
    for s, p in zip(C.sweep_shapes(), rows + cols):
        assert p == C.own_shape(*s), s


@pytest.mark.parametrize("group", [n for n, _s in C.sweep_groups()])
def test_length_sweep(engine, oracle, group):
    shapes = dict(C.sweep_groups())[group]
    took_part = 0
    with knobs():
        for s in shapes:
            plan = engine.phase_plan(*s)
            assert (plan["lds_transforms"], plan["transposed"]) == (1, 0), s
            a, b = C.planted_pair(s)
            n, o, _pos = C.planted_refs(s, oracle)
            C.hold(correlate(engine, a, b), n, o, ("planted", s))
            pk, clear = C.unrelated_ref(s)
            if clear:
                a, b = C.unrelated_pair(s)
                _row, _cands, got = engine.phase_resolve(a, b, C.PEAKS, C.RESOLVE_THRESHOLD, C.RESOLVE_MIN_PIXELS)
                assert got.tolist() == [list(p) for p in pk], ("unrelated", s)
                took_part += 1
    print("%s: %d shapes, %d unrelated pairs took part; largest device deviation so far %r" % (group, len(shapes), took_part, C.worst))
    assert took_part >= (1.0 - C.MAX_DROPPED) * len(shapes) - 1


# ---- 2. peaks placed at the border ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.BORDER_SHAPES)
def test_peaks_on_the_border_of_the_surface(engine, oracle, shape):
    cases = C.border_cases(shape)
    with knobs():
        lds = engine.phase_plan(*shape)["lds_transforms"]
        assert lds == int(shape != (25, 27))                     # odd by odd: rocFFT either way
        single = [correlate(engine, a, b) for _t, a, b in cases]
        batch = batch_rows(engine, [(str(t), a, b) for t, a, b in cases])
    with knobs(LDS_FFT=0):
        assert engine.phase_plan(*shape)["lds_transforms"] == 0
        rocfft = [correlate(engine, a, b) for _t, a, b in cases]
    for k, (t, _a, _b) in enumerate(cases):
        n, o, pos = C.border_refs(shape, k, oracle)
        assert pos == t
        C.hold(single[k], n, o, ("single", shape, t))
        C.hold(rocfft[k], n, o, ("rocfft", shape, t))
        C.hold(tuple(batch[k]), n, o, ("batch", shape, t))
        if lds:
            assert tuple(batch[k]) == single[k], (shape, t)      # the same kernels and geometry behind both entries
    print("border %r: largest device deviation so far %r" % (shape, C.worst))


# ---- 3. degenerate strips ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.DEGENERATE_SHAPES)
def test_black_strips_give_exactly_the_centre_and_no_response(engine, shape):
    want = C.degenerate_result(shape)
    pairs = C.degenerate_pairs(shape)
    with knobs():
        assert engine.phase_plan(*shape)["lds_transforms"] == 1
        for name, a, b in pairs:
            assert correlate(engine, a, b) == want, (shape, name, "lds")
        rows = batch_rows(engine, pairs)
        assert [tuple(r) for r in rows.tolist()] == [want] * len(pairs), (shape, "batch")
    with knobs(LDS_FFT=0):
        assert engine.phase_plan(*shape)["lds_transforms"] == 0
        for name, a, b in pairs:
            assert correlate(engine, a, b) == want, (shape, name, "rocfft")


@pytest.mark.parametrize("shape", C.CONSTANT_SHAPES)
def test_constant_strips_return_finite_numbers(engine, shape):
    """Only that: a constant non-zero strip is not a defined input.  Where a side equals its padded size the spectrum has exact zeros, and
    P |P| / (|P|^2 + eps) normalises their rounding noise to unit magnitude: on 15 x 20 strips of 255 phase_numpy answers x = 9.0 and the
    oracle 6.0 (test_phase_cases_host.py::test_constant_strips_are_not_a_defined_input), so no reference can pin the device."""
    a = np.full(shape, 255, np.uint8)
    for lds in (1, 0):
        with knobs(LDS_FFT=lds):
            assert all(math.isfinite(v) for v in correlate(engine, a, a))
            assert all(math.isfinite(v) for v in correlate(engine, a, np.full(shape, 7, np.uint8)))
    with knobs():
        assert np.isfinite(batch_rows(engine, [("constant", a, a)] * 2)).all()


# ---- 4. batches whose jobs differ ----------------------------------------------------------------------------------------------------
_single = {}


def single_calls(engine, strips):
    """engine.phase_correlate of every strip pair as host arrays, default knobs, once per pair"""
    out = []
    with knobs():
        for name, a, b in strips:
            if name not in _single:
                _single[name] = correlate(engine, a, b)
            out.append(_single[name])
    return np.array(out)


def test_mixed_batch_under_every_chunk_size(engine, oracle):
    with knobs():
        assert [engine.phase_plan(*s)["transposed"] for s in C.BATCH_SHAPES] == [0, 1]
        assert all(engine.phase_plan(*s)["lds_transforms"] == 1 for s in C.BATCH_SHAPES)
    strips = C.mixed_batch()
    want = single_calls(engine, strips)
    assert len({tuple(r) for r in want.tolist()}) == len(strips)                 # every job has an answer of its own
    for k, (name, a, b) in enumerate(strips):
        n, o, _pos = C.refs(("batch", name), a, b, oracle)
        C.hold(tuple(want[k]), n, o, ("single", name))
    for chunk in C.CHUNKS:
        with knobs(CHUNK=chunk):
            rows = batch_rows(engine, strips)
        assert np.array_equal(rows, want), (chunk, rows, want)                   # bit-identical, in the caller's order


def test_resolve_batch_under_every_chunk_size(engine):
    """the peak sink reuses the surface planes chunk after chunk, in both orientations"""
    strips, ref = C.mixed_batch(), C.mixed_batch_resolved()
    assert all(ok for _r, ok in ref)
    for chunk in C.CHUNKS:
        with knobs(CHUNK=chunk):
            rows, cands, pk = batch_rows(engine, strips, resolve=C.BATCH_K)
        for k, (r, _ok) in enumerate(ref):
            assert pk[k].tolist() == r["peaks"].tolist(), (chunk, strips[k][0])
            assert cands[k].tolist() == r["cands"].tolist(), (chunk, strips[k][0])
            assert rows[k].tolist() == r["row"].tolist(), (chunk, strips[k][0])


def test_seventy_different_jobs_run_in_three_chunks(engine, oracle):
    strips = C.batch_strips(C.BATCH_SHAPES[1], C.MANY)
    assert len(strips) == 70
    want = single_calls(engine, strips)
    assert len({tuple(r) for r in want.tolist()}) == 70
    for k, (name, a, b) in enumerate(strips):
        n, o, _pos = C.refs(("batch", name), a, b, oracle)
        C.hold(tuple(want[k]), n, o, ("single", name))
    with knobs():
        rows = batch_rows(engine, strips)
    assert np.array_equal(rows, want)
    with knobs(LDS_FFT=0):                                                       # rocFFT plans of 32 + 32 + 6 (a plan of 6)
        assert engine.phase_plan(*C.BATCH_SHAPES[1])["lds_transforms"] == 0
        rows = batch_rows(engine, strips)
    for q, w in zip(rows, want):
        sx, sy = max(1.0, abs(w[0])), max(1.0, abs(w[1]))
        assert abs(q[0] - w[0]) < 1e-8 * sx and abs(q[1] - w[1]) < 1e-8 * sy and abs(q[2] - w[2]) < 1e-12, (q, w)


# ---- 5. workgroup geometry -----------------------------------------------------------------------------------------------------------
_default_geometry = {}


def default_geometry(engine, oracle):
    """plan and result of every geometry shape, and the mixed batch's rows, under the default geometry (held to the references here)"""
    if not _default_geometry:
        with knobs():
            for s in C.GEOMETRY_SHAPES:
                a, b = C.geometry_pair(s)
                got = correlate(engine, a, b)
                n, o, _pos = C.refs(("geometry", s), a, b, oracle)
                C.hold(got, n, o, ("geometry", s))
                _default_geometry[s] = (engine.phase_plan(*s), got)
            _default_geometry["batch"] = batch_rows(engine, C.mixed_batch())
    return _default_geometry


@pytest.mark.parametrize("knob,value", C.GEOMETRY_SETTINGS)
def test_results_do_not_depend_on_the_workgroup_geometry(engine, oracle, knob, value):
    """A transform's arithmetic does not depend on which thread or workgroup carries it, and `better` is a total order: bit identity."""
    default = default_geometry(engine, oracle)
    ran, skipped = [], []
    with knobs(**{knob[len("VFSMS_PHASE_"):]: value}):
        for s in C.GEOMETRY_SHAPES:
            plan = engine.phase_plan(*s)
            assert plan == C.geometry_restated(s, knob, value), (s, plan)
            if not C.geometry_takes(plan, default[s][0]):
                skipped.append(s)                                # clamped back by the host (or off the LDS path)
                continue
            got = correlate(engine, *C.geometry_pair(s))
            assert got == default[s][1], (knob, value, s, plan, got, default[s][1])
            ran.append(s)
        batch_takes = [C.geometry_takes(engine.phase_plan(*s), C.own_shape(*s)) for s in C.BATCH_SHAPES]
        if any(batch_takes):
            assert np.array_equal(batch_rows(engine, C.mixed_batch()), default["batch"]), (knob, value)
    print("%s=%s: ran on %d shapes, clamped back on %d %r; the mixed batch %s" % (knob, value, len(ran), len(skipped), skipped,
                                                                                "ran" if any(batch_takes) else "was clamped back"))
    if (knob, value) not in (("VFSMS_PHASE_TDIV", "16"), ("VFSMS_PHASE_TCOL", "64")):      # those two the host always clamps back
        assert len(ran) >= 9 and (any(batch_takes) or (knob, value) == ("VFSMS_PHASE_ROWPTS", "4096"))      # 16 rows of 40 points either way


# ---- 6. one-row and one-column strips ------------------------------------------------------------------------------------------------
def test_one_row_and_one_column_strips(engine, oracle):
    """rocFFT and unshift2's half-swap branch: a 1 x n or n x 1 surface swaps its two halves"""
    with knobs():
        for s in C.VECTOR_SHAPES:
            assert engine.phase_plan(*s)["lds_transforms"] == 0
            a, b = C.vector_pair(s)
            n, o, _pos = C.vector_refs(s, oracle)
            C.hold(correlate(engine, a, b), n, o, ("vector", s))
