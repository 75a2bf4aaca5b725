"""GPU tests (-m gpu) of the strip table of a fused SURF or ORB batch (csrc/api.hip: build_strip_table): a strip that several slots of one batch
name -- the turn of the serpentine path (pair p in direction 1 next to pair p + 1 in direction 3), the same job twice, a job whose A strip
is another job's B strip, one buffer behind two tile handles -- is detected and described once and read by every job that uses it.  Every
row of such a batch must equal the row of the same job evaluated alone in its own call, plain and with equalised / CLAHE'd strips, and
with VFSMS_OVERLAP=1 (the batch cut in two parts on two streams).  VFSMS_STRIP_DEDUP=0 restores one strip per slot: the bench grid's
offset table must not change with it.  The environment switches are read once per process, so those settings run in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                  # run as a child process: python tests/test_strip_dedup_gpu.py ...
    sys.path.insert(0, ROOT)

import imagestitch_amd as isa                             # noqa: E402
from imagestitch_amd.synthetic import SyntheticGrid       # noqa: E402

pytestmark = pytest.mark.gpu
SPECS = [(0, 0.0, 0), (1, 0.0, 0), (2, 20.0, 5)]         # plain, equalizeHist, CLAHE(clipLimit 20, 5 x 5 tiles)


def _tiles():
    return SyntheticGrid(2, 2, 640).tiles(threads=1)


def _job(hs, shapes, p, d, i=1, a=None, b=None):
    """(tile_a, tile_b, ay0, ax0, by0, bx0, h, w) of pair p (tiles a, b: p, p + 1 by default) in direction d at searchRatio 0.2 i"""
    a = p if a is None else a
    b = p + 1 if b is None else b
    ra = isa.roi_rect(shapes[a], d, "first", 0.2 * i); rb = isa.roi_rect(shapes[b], d, "second", 0.2 * i)
    return (hs[a], hs[b], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])


def _batches(hs, shapes):
    """batches of jobs that repeat strips, by name"""
    turn = [_job(hs, shapes, 0, 1), _job(hs, shapes, 1, 3)]          # pair 0's B strip (top of tile 1) is pair 1's A strip
    same = _job(hs, shapes, 1, 2)
    # job X = (1, 2) in direction 1: A = bottom of tile 1; job Y = (0, 1) in direction 3: B = bottom of tile 1
    a_is_b = [_job(hs, shapes, 1, 1), _job(hs, shapes, 0, 3)]
    r = isa.roi_rect(shapes[2], 1, "first", 0.2)
    self_pair = (hs[2], hs[2], r[0], r[1], r[0], r[1], r[2], r[3])              # one strip on both sides of a job
    mixed = turn + a_is_b + [same, _job(hs, shapes, 2, 4), _job(hs, shapes, 0, 2), same, _job(hs, shapes, 0, 1, 2), _job(hs, shapes, 1, 3, 2),
                             self_pair, turn[1]]
    return dict(turn=turn, same_twice=[same, same], a_is_b=a_is_b, self_pair=[self_pair], mixed=mixed)


def _attempt(engine, jobs, spec):
    if spec[0] == 0:
        return engine.attempt_surf_batch(jobs)
    return engine.attempt_surf_batch_enhanced(jobs, None, 0.75, 3, spec)


def _rows_of(engine, tiles, spec, names=None, attempt=_attempt):
    shapes = [t.shape for t in tiles]
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        bs = _batches(hs, shapes)
        return {k: attempt(engine, v, spec).tolist() for k, v in bs.items() if names is None or k in names}, \
               {k: [attempt(engine, [j], spec)[0].tolist() for j in v] for k, v in bs.items() if names is None or k in names}
    finally:
        for h in hs:
            engine.tile_free(h)


@pytest.mark.parametrize("spec", SPECS, ids=["plain", "equalize", "clahe"])
def test_repeated_strips_give_the_rows_of_jobs_alone(engine, spec):
    batched, alone = _rows_of(engine, _tiles(), spec)
    for name in batched:
        assert batched[name] == alone[name], (name, spec)
    assert any(r[0] == 1 for r in alone["mixed"]) and all(r[4] > 0 and r[5] > 0 for r in alone["mixed"])


def _attempt_orb(engine, jobs, spec):
    return engine.attempt_orb_batch(jobs)


def test_orb_repeated_strips_give_the_rows_of_jobs_alone(engine):
    """vfsms_attempt_orb_batch reads the same strip table: every row of the named batches equals the job alone, and a strip per slot
    (VFSMS_STRIP_DEDUP=0, child process) gives the same rows"""
    batched, alone = _rows_of(engine, _tiles(), SPECS[0], attempt=_attempt_orb)
    for name in batched:
        assert batched[name] == alone[name], name
    assert any(r[0] == 1 for r in alone["mixed"]) and all(r[4] > 0 and r[5] > 0 for r in alone["mixed"])
    assert _child(["orb"], dict(VFSMS_STRIP_DEDUP="0"), 300) == batched


def test_one_buffer_behind_two_handles(engine):
    """vfsms_tile_wrap gives one device buffer two handles: the strip is keyed by its address, and the rows stay those of the jobs alone"""
    import ctypes as C
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln.split()[-1]]
    hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")            # the HIP runtime the library itself runs on
    tiles = _tiles()[:2]
    h, w = tiles[0].shape
    bufs = []
    try:
        for t in tiles:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(h * w)) == 0
            bufs.append(p)
            src = np.ascontiguousarray(t)
            assert hip.hipMemcpy(p, src.ctypes.data_as(C.c_void_p), C.c_size_t(h * w), 1) == 0       # hipMemcpyHostToDevice
        hs = [engine.tile_wrap(bufs[0].value, h, w, w), engine.tile_wrap(bufs[1].value, h, w, w), engine.tile_wrap(bufs[1].value, h, w, w)]
        shapes = [(h, w)] * 3
        try:
            jobs = [_job(hs, shapes, 0, 1), _job(hs, shapes, 0, 1, b=2), _job(hs, shapes, 0, 3, a=2, b=0), _job(hs, shapes, 0, 3, a=1, b=0)]
            rows = engine.attempt_surf_batch(jobs).tolist()
            alone = [engine.attempt_surf_batch([j])[0].tolist() for j in jobs]
            assert rows == alone
            assert rows[0] == rows[1] and rows[2] == rows[3] and rows[0][0] == 1
        finally:
            for x in hs:
                engine.tile_free(x)
            engine.sync()
    finally:
        for p in bufs:
            hip.hipFree(p)


def _child(args, env, timeout):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_overlap_parts_read_shared_strips(engine):
    """VFSMS_OVERLAP=1 cuts a batch of 12 or more jobs in two parts; a strip belongs to the first part that uses it, so part 1's jobs read
    part-0 strips.  Every row equals the job's row alone (computed here, one stream)."""
    _, alone = _rows_of(engine, _tiles(), SPECS[0], names=("mixed",))
    for pct in ("30", "70"):
        got = _child(["batch"], dict(VFSMS_OVERLAP="1", VFSMS_OVERLAP_PCT=pct), 300)
        assert got["mixed"] == alone["mixed"], pct


@pytest.mark.timeout(900)
def test_bench_grid_table_with_and_without_the_strip_table(tmp_path):
    """The bench grid (10 x 9 tiles of 2048^2, SURF, roiRatio 0.2) registered cold and then with the learned path memory, once with the
    strip table and once with a strip per slot (VFSMS_STRIP_DEDUP=0): the offset tables, directions and attempt / batch counts are equal."""
    g = SyntheticGrid(10, 9, 2048)
    path = str(tmp_path / "tiles.npy")
    np.save(path, np.stack(list(g.tiles(processes=8))))                # spawned workers: this process holds a GPU context
    on = _child(["grid", path], dict(VFSMS_STRIP_DEDUP="1"), 400)
    off = _child(["grid", path], dict(VFSMS_STRIP_DEDUP="0"), 400)
    assert on == off
    assert on["warm"]["batches"] < on["cold"]["batches"] and len(on["warm"]["table"]) == g.n_tiles - 1


def _main(argv):
    from imagestitch_amd.grid import GridRegistrar
    eng = isa.Engine(0)
    if argv[0] == "batch":
        batched, _ = _rows_of(eng, _tiles(), SPECS[0], names=("mixed",))
        out = batched
    elif argv[0] == "orb":
        out, _ = _rows_of(eng, _tiles(), SPECS[0], attempt=_attempt_orb)
    else:
        tiles = np.load(argv[1], mmap_mode="r")
        hs = [eng.tile_upload(np.ascontiguousarray(t)) for t in tiles]
        shapes = [t.shape for t in tiles]
        reg = GridRegistrar(eng, method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1, surfParams=eng.surf_params())
        out = {}
        for leg in ("cold", "warm"):                         # the second call plans with the path memory the first one left
            a0, b0 = reg.stats["attempts"], reg.stats["batches"]
            table, d_out = reg.register(hs, shapes, 1)
            out[leg] = dict(table=[[int(v) for v in r[:6]] for r in table], direction=int(d_out),
                            attempts=reg.stats["attempts"] - a0, batches=reg.stats["batches"] - b0)
        for h in hs:
            eng.tile_free(h)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    _main(sys.argv[1:])
