"""GPU tests (``-m gpu``) of the droplet shapes gathered on the device (chs_shapes / chs_batch_shapes,
chsimpy_amd/csrc/chs_shapes.hip).

Reference: the numpy model ``shapes.shape_table`` on the field as downloaded with ``get_U`` -- the exact values the
device holds, also for fp32 -- with the label image of ``scipy.ndimage.label`` renumbered by ascending `first`
(tests/test_components_host.py: reference), which tests/test_shapes_host.py holds against plain loops.  Every cell is an
integer and every accumulation an integer add: every comparison is for equality of words, shape table, component table
and labels.

The sizes are the smallest at which each path of the sweep can still go wrong: one workgroup, one below / equal to / one
above a tile, more than two tiles a side; 513 for the 64-bit sums; the two sizes just above the cache bound for the
streamed loads."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, shapes
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import log_line, make
import test_gpu_components as tgc
import test_gpu_spectrum as tgs
import test_components_host as cchost
import test_morphology_host as mh
import test_shapes_host as host

pytestmark = pytest.mark.gpu

T = host.T
TILE = cchost.tile_from_header()
SIDES = host.SIDES
engine_of = tgc.engine_of


def dev_look(eng, t, conn, side, labels=True, delx=None):
    words, tab, cctab, lab = eng.shapes_look(t, conn, components.side_code(side), labels)
    assert words.dtype == np.int64 and tab.dtype == np.int64 and tab.shape == (int(words[0]), shapes.CHS_SH_COLS)
    co = components.Components(words[:components.CHS_CC_WORDS], eng.N, t, conn, side, table=cctab, labels=lab, delx=delx)
    return shapes.Shapes(words, tab, co)


def model_of(Ud, t, conn, side):
    """(words, shape table, component table, labels) of the downloaded field: scipy's labelling, the numpy model's table."""
    X = host.fg_of(Ud, t, side)
    labels, cctab = cchost.reference(X, conn)
    table = shapes.shape_table(Ud, t, conn, side, labels=labels)
    return shapes.summary_of(table, components.summary_of(cctab, X.shape[0]), conn), table, cctab, labels


def check(sh, Ud, t, what=''):
    """A device look against the model on the downloaded field: words, both tables, the labels where fetched."""
    words, table, cctab, labels = model_of(Ud, t, sh.connectivity, sh.side)
    assert np.array_equal(sh.table, table), (what, np.argwhere(sh.table != table)[:8])
    assert np.array_equal(sh.words, words), (what, sh.words, words)
    assert np.array_equal(sh.components.table, cctab), what
    if sh.components.labels is not None:
        assert np.array_equal(sh.components.labels, labels), what
    return sh


class Looker:
    """Looks at fields on one engine, each uploaded once and compared as downloaded."""

    def __init__(self, eng):
        self.eng, self.U, self.Ud = eng, None, None

    def __call__(self, U, t, conn, side, what=''):
        if self.U is not U:
            self.eng.set_U(U)
            self.U, self.Ud = U, self.eng.get_U()
        return check(dev_look(self.eng, t, conn, side), self.Ud, t, f"{what} {conn} {side}")


# ---------------------------------------------------------------------------
# 1. sizes and patterns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", cchost.tile_sizes(TILE))
def test_patterns_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    look = Looker(eng)
    for name, U, _ in cchost.patterns(N, TILE):
        for conn in (4, 8):
            for side in SIDES:
                look(U, T, conn, side, f"{name} N={N}")
    for name, U, t, _ in mh.hand_made(N):                # the threshold, NaN and one-ulp fields
        for conn in (4, 8):
            for side in SIDES:
                look(U, t, conn, side, f"{name} N={N}")
    s.close(fetch_U=False)


def test_patterns_on_the_device_fp32(gpu):
    N = max(TILE) + 1
    s, eng = engine_of(N, 'chirp', 'float32')
    look = Looker(eng)
    for name, U, _ in cchost.patterns(N, TILE):
        for conn in (4, 8):
            for side in SIDES:
                look(U, T, conn, side, f"{name} fp32")
    s.close(fetch_U=False)


def test_more_components_in_a_tile_than_slots(gpu):
    """A checkerboard at connectivity 4: 2048 one-pixel components in every full tile, more than any slot count that fits
    in LDS -- most contributions go straight to the table."""
    N = 2 * max(TILE) + 2
    s, eng = engine_of(N, 'chirp')
    ii, jj = np.indices((N, N))
    sh = Looker(eng)(mh.field_of((ii + jj) % 2 == 0), T, 4, 'below', 'checkerboard')
    assert sh.count == N * N // 2 and np.all(sh.area == 1) and np.all(sh.perimeter == 4) and sh.total_holes == 0
    assert np.array_equal(sh.si, sh.first // N) and np.array_equal(sh.sj, sh.first % N)
    s.close(fetch_U=False)


@pytest.mark.parametrize("N,pattern", [(130, 'serpentine'), (129, 'stripes')])
def test_one_component_fed_by_every_workgroup(gpu, N, pattern):
    """A serpentine one pixel wide that passes through every tile is one component to which every workgroup adds by
    global atomics; stripes are components fed by a column of workgroups each."""
    s, eng = engine_of(N, 'chirp')
    ii, jj = np.indices((N, N))
    X = host.serpentine(N) if pattern == 'serpentine' else jj % 2 == 0
    look = Looker(eng)
    for conn in (4, 8):
        sh = look(mh.field_of(X), T, conn, 'below', pattern)
        if pattern == 'serpentine':
            assert sh.count == 1 and sh.area[0] == int(X.sum()) and sh.holes[0] == 0 and sh.quads[0] == 0
        else:
            assert sh.count == (N + 1) // 2 and np.all(sh.area == N) and np.all(sh.pairs_v == N - 1)
        look(mh.field_of(X), T, conn, 'above', pattern)
    s.close(fetch_U=False)


def test_sums_beyond_32_bits(gpu):
    """All foreground at N = 513: one component, sii = N sum i^2 = 2.3e10 -- the smallest size astride the tiles at which a
    32-bit accumulation anywhere in the sweep shows."""
    N = 513
    s, eng = engine_of(N, 'chirp')
    sh = Looker(eng)(np.full((N, N), mh.FG), T, 4, 'below', 'full 513')
    sq = (N - 1) * N * (2 * N - 1) // 6
    assert sh.count == 1 and sh.sii[0] == sh.sjj[0] == N * sq > 2 ** 34 and sh.sij[0] == (N * (N - 1) // 2) ** 2 > 2 ** 34
    assert sh.su_fix[0] == N * N * int(mh.FG * 2.0 ** 30) > 2 ** 45 and sh.wall[0] == 4 * N
    assert np.array_equal(sh.centroid[0], [256.0, 256.0]) and sh.orientation[0] == 0.0 and abs(sh.aspect[0] - 1) < 1e-12
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random fields: every engine and element type, N that is no multiple of a 16-byte load
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine,dtype", tgc.RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in tgc.RANDOM_CASES])
def test_random_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    rng = np.random.default_rng(13 * N + len(engine))
    look = Looker(eng)
    for density in (0.35, 0.6):
        U = host.special_field(N, rng)
        U = np.where(np.isfinite(U) & (np.abs(U) < 1), np.where(rng.random((N, N)) < density, 0.5 * U, 0.5 + 0.5 * U), U)
        U[rng.integers(0, N, 3), rng.integers(0, N, 3)] = T
        for conn in (4, 8):
            for side in SIDES:
                sh = look(U, T, conn, side, f"N={N} {engine} {dtype} {density}")
                assert sh.count > 0
        assert np.isnan(look.Ud).sum() == np.isnan(U).sum() > 0 and np.count_nonzero(look.Ud == T) >= 1
        assert look(U, T, 4, 'above').n_outside.sum() >= np.isnan(U).sum()
    assert eng.shapes_ms() >= 0.0 and eng.components_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field, and the invariants across three looks of the same handle
# ---------------------------------------------------------------------------
def test_an_evolved_field_and_the_invariants(gpu):
    N, steps = 256, 2000
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    t = s.params.threshold
    Ud = s._engine.get_U()
    mo = s.morphology()
    for conn in (4, 8):
        for side in SIDES:
            sh = check(s.shapes(connectivity=conn, side=side, labels=True), Ud, t, f"evolved {conn} {side}")
            assert sh.threshold == t and sh.N == N and sh.delx == sol.delx and sh.count >= 1 and 0 < sh.area.sum() < N * N
            other = s.components(connectivity=host.OTHER[conn], side='above' if side == 'below' else 'below', table=False)
            assert sh.total_holes == other.inner, (conn, side)
            if side == 'below':
                host.check_invariants(sh, mo, other.inner, f"evolved {conn}")
            assert np.array_equal(sh.radius_eq, np.sqrt(sh.area / np.pi) * sol.delx)
            assert np.all(sh.n_outside == 0) and np.all((sh.mean_u > 0) & (sh.mean_u < 1))
            if side == 'below':
                assert np.all(sh.mean_u < t + 2.0 ** -30)
        # (one phase is the connected matrix, the other one the droplets in its holes)
        assert sh.count > 100 and sh.inner_round > 100
        log_line(f"shapes: evolved N={N} after {steps} steps, connectivity {conn}: {sh.count} components above, "
                 f"{sh.total_holes} holes, shapes {s._engine.shapes_ms():.4f} ms, components {s._engine.components_ms():.4f} ms")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. the streamed loads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", [(4097, 'float64'), (5793, 'float32')])
def test_streamed_loads(gpu, N, dtype):
    """Just above the cache bound (tests/test_gpu_looks_large.py): k_sh_sweep<T, true>.  The model by its vectorised path,
    the labels from scipy.  The foreground is made of 6 x 6 blocks, a fifth of them: droplets of some size, their number
    and the host's work small."""
    s = chsimpy_amd.Solver(make(N, 2, 'auto', dtype=dtype))
    eng = s._get_engine()
    assert 2 * N * N * (8 if dtype == 'float64' else 4) > 256 << 20
    rng = np.random.default_rng(N)
    blocks = np.repeat(np.repeat(rng.random((N // 6 + 1, N // 6 + 1)) < 0.2, 6, axis=0), 6, axis=1)[:N, :N]
    U = np.where(blocks, 0.1 + 0.3 * rng.random((N, N), dtype=np.float32), 0.8)
    U[rng.integers(0, N, 16), rng.integers(0, N, 16)] = T
    U[N // 3, N - 2], U[5, 7], U[N - 1, 0] = np.nan, -np.inf, -9.0
    eng.set_U(U)
    Ud = eng.get_U()
    sh = check(dev_look(eng, T, 4, 'below', labels=False), Ud, T, f"streamed N={N} {dtype}")
    assert sh.count > 10000 and sh.area.max() > 36 and sh.n_outside.sum() == 2
    log_line(f"shapes, large: N={N} {dtype} streamed: shapes {eng.shapes_ms():.3f} ms, components {eng.components_ms():.3f} ms")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 5. coupling with the components look, state, errors
# ---------------------------------------------------------------------------
def test_coupling_with_the_components_look(gpu):
    N = 100
    s, eng = engine_of(N, 'chirp')
    rng = np.random.default_rng(5)
    U = host.special_field(N, rng)
    eng.set_U(U)
    Ud = eng.get_U()
    code = components.side_code('above')
    words = eng.shapes(T, 8, code)
    # after shapes, the component table and the labels are those of that look
    _, table, cctab, labels = model_of(Ud, T, 8, 'above')
    assert np.array_equal(eng.components_table(), cctab) and np.array_equal(eng.components_labels(), labels)
    assert np.array_equal(eng.shapes_table(), table)                      # (fetched behind the label kernel)
    assert np.array_equal(words[:7], eng.components(T, 8, code))
    # a later components look with other arguments leaves the shapes table fetchable and unchanged
    other = eng.components(0.3, 4, components.side_code('below'))
    assert int(other[0]) != int(words[0])
    assert np.array_equal(eng.shapes_table(), table)
    assert np.array_equal(eng.components_table(), cchost.reference(host.fg_of(Ud, 0.3, 'below'), 4)[1])
    # two looks give the same bits
    a, b = dev_look(eng, T, 4, 'below'), dev_look(eng, T, 4, 'below')
    assert np.array_equal(a.words, b.words) and np.array_equal(a.table, b.table)
    s.close(fetch_U=False)


def test_errors_are_those_of_components(gpu):
    s = tgs.solver(128, 4, 'fast')
    eng = s._get_engine()
    out = np.zeros(_lib.CHS_SH_WORDS, dtype=np.int64)
    cco = np.zeros(_lib.CHS_CC_WORDS, dtype=np.int64)
    tab = np.zeros((128 * 128, _lib.CHS_SH_COLS), dtype=np.int64)
    ms = np.zeros(1)
    o, c, tb = _lib._i64ptr(out), _lib._i64ptr(cco), _lib._i64ptr(tab)

    def both(*args):
        """The code of chs_shapes, which must be that of chs_components with the same arguments."""
        rs = gpu.chs_shapes(eng._h, *args, o)
        assert rs == gpu.chs_components(eng._h, *args, c)
        return rs

    assert both(0.5, 4, 0) == _lib.CHS_ESTATE                                               # no field yet
    assert gpu.chs_shapes_table(eng._h, 0, tb) == _lib.CHS_ESTATE                           # no look yet
    assert gpu.chs_shapes_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    with pytest.raises(AssertionError):
        s.shapes()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert both(bad, 4, 0) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    for conn in (0, 6, -4, 16):
        assert both(0.5, conn, 0) == _lib.CHS_EINVAL
        assert 'connectivity' in gpu.chs_last_error().decode()
    for side in (2, -1):
        assert both(0.5, 4, side) == _lib.CHS_EINVAL
    assert both(float('nan'), 5, 2) == _lib.CHS_EINVAL and 'finite' in gpu.chs_last_error().decode()   # the same order
    assert gpu.chs_shapes(eng._h, 0.5, 4, 0, None) == _lib.CHS_EINVAL == gpu.chs_components(eng._h, 0.5, 4, 0, None)
    assert gpu.chs_shapes(eng._h, float('nan'), 4, 0, None) == _lib.CHS_EINVAL and 'null' in gpu.chs_last_error().decode()
    assert gpu.chs_shapes(None, 0.5, 4, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_shapes_table(None, 0, tb) == _lib.CHS_EINVAL
    assert gpu.chs_shapes_last_ms(eng._h, None) == _lib.CHS_EINVAL and gpu.chs_shapes_last_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_shapes_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE                 # none of them was a look
    assert gpu.chs_shapes_table(eng._h, 0, tb) == _lib.CHS_ESTATE
    t = float(np.median(eng.get_U()))
    assert gpu.chs_shapes(eng._h, t, 4, 0, o) == _lib.CHS_OK
    C = int(out[0])
    assert C > 0 and gpu.chs_shapes_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for rows in (C - 1, C + 1, -1):
        assert gpu.chs_shapes_table(eng._h, rows, tb) == _lib.CHS_EINVAL
    assert gpu.chs_shapes_table(eng._h, C, None) == _lib.CHS_EINVAL
    assert gpu.chs_shapes(eng._h, float('inf'), 4, 0, o) == _lib.CHS_EINVAL                  # a refused call leaves the look
    assert gpu.chs_shapes_table(eng._h, C, tb) == _lib.CHS_OK
    assert int(tab[:C, 1].sum()) == int(out[1]) == int(out[shapes.CHS_SH_SUM_AREA])
    with pytest.raises(ValueError):
        s.shapes(connectivity=5)
    with pytest.raises(ValueError):
        s.shapes(side='left')
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_shapes(b._h, 0, 0.5, 4, 0, o) == _lib.CHS_ESTATE == gpu.chs_batch_components(b._h, 0, 0.5, 4, 0, c)
    assert gpu.chs_batch_shapes_table(b._h, 0, tb) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, 65536):
        assert gpu.chs_batch_shapes(b._h, member, 0.5, 4, 0, o) == _lib.CHS_EINVAL, member
    for args in ((float('nan'), 4, 0), (0.5, 5, 0), (0.5, 8, 3)):
        assert gpu.chs_batch_shapes(b._h, 1, *args, o) == _lib.CHS_EINVAL == gpu.chs_batch_components(b._h, 1, *args, c)
    assert gpu.chs_batch_shapes(b._h, 1, 0.5, 8, 1, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_shapes(None, 1, 0.5, 8, 1, o) == _lib.CHS_EINVAL and gpu.chs_batch_shapes_table(None, 0, tb) == _lib.CHS_EINVAL
    assert gpu.chs_batch_shapes_table(b._h, 0, tb) == _lib.CHS_ESTATE                        # none of them was a look
    assert gpu.chs_batch_shapes(b._h, 1, 0.5, 8, 1, o) == _lib.CHS_OK
    C = int(out[0])
    assert gpu.chs_batch_shapes_table(b._h, C + 1, tb) == _lib.CHS_EINVAL and gpu.chs_batch_shapes_table(b._h, C, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_shapes_table(b._h, C, tb) == _lib.CHS_OK
    assert int(tab[:C, 1].sum()) == out[1] == int((~(bs.solvers[1]._engine.get_U() < 0.5)).sum())
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 6. the run does not notice
# ---------------------------------------------------------------------------
OBSERVED = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]
assert sorted(c[1] for c in OBSERVED) == ['chirp', 'fast']


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVED, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVED])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with shapes() between them against the same calls with get_U() between them: all nine record columns, the
    state and the final field, bit for bit."""
    got, Ug = tgs._observed_run(N, engine, calls, lambda s: s.shapes(connectivity=8), seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert np.array_equal(Ug, Ur)


# ---------------------------------------------------------------------------
# 7. batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_batch_equals_the_single_solver(gpu, N, engine):
    B = 3
    ps = tgs._members(N, B, 100)
    for p in ps:
        p.engine = engine
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    fields = [s._engine.get_U() for s in bs.solvers]
    ts = [float(np.median(f)) for f in fields]             # a two-phase picture of every member
    shs = bs.shapes(threshold=ts, connectivity=8, labels=True)
    assert len(shs) == B and [sh.threshold for sh in shs] == ts
    single, eng = engine_of(N, engine)
    for m in range(B):
        check(shs[m], fields[m], ts[m], f"member {m}")
        eng.set_U(fields[m])
        one = dev_look(eng, ts[m], 8, 'below')
        assert np.array_equal(one.words, shs[m].words) and np.array_equal(one.table, shs[m].table), m
        assert np.array_equal(one.components.table, shs[m].components.table), m
        again = bs.shapes(m, threshold=ts, connectivity=8)                       # member = m
        assert np.array_equal(again.table, shs[m].table) and again.components.labels is None
        through = bs.solvers[m].shapes(ts[m], connectivity=8)                    # through the member's Solver
        assert np.array_equal(through.words, shs[m].words) and np.array_equal(through.table, shs[m].table)
        assert shs[m].count > 1 and shs[m].delx == bs.solvers[m].solution.delx
    single.close(fetch_U=False)
    assert not np.array_equal(shs[0].words, shs[1].words)
    bs.close(fetch_U=False)
