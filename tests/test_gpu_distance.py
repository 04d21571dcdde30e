"""GPU tests (``-m gpu``) of the exact Euclidean distance transform of the thresholded field on the device
(chs_distance / chs_batch_distance, chsimpy_amd/csrc/chs_distance.hip).

Reference: ``np.rint(scipy.ndimage.distance_transform_edt(X) ** 2)`` on the foreground of the field as downloaded with
``get_U`` -- the exact values the device holds, also for fp32 -- and CHS_DT_INF by the definition where the grid has no
background (tests/test_distance_host.py: reference, check_look).  Everything is integer: every comparison is for
equality of summary, histogram and map.

``B, C`` are the rows of a band of the vertical pass and the pixels of a wavefront pass of the horizontal one
(``_lib.distance_tile()``); the pattern sizes are the smallest at which each phase can still go wrong."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, distance, experiment as ex
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_distance_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
TILE = host.tile_from_source()        # (the library's own is checked against it below)
SIDES = host.SIDES


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, side, hist=True, map=True):
    words, hi, d2 = eng.distance_look(t, components.side_code(side), hist, map)
    return distance.Distance(words, eng.N, t, side, hist=hi, d2=d2)


def fg_of(Ud, t, side):
    X = np.nan_to_num(Ud, nan=np.inf) < t
    return X if side == 'below' else ~X


# ---------------------------------------------------------------------------
# 1. patterns
# ---------------------------------------------------------------------------
def test_the_tile_is_the_sources(gpu):
    assert _lib.distance_tile() == TILE


def _pattern_look(eng, check_upload=False):
    def look(U, t, side):
        if look.U is not U:
            eng.set_U(U)
            look.U = U
            if check_upload:
                assert np.array_equal(eng.get_U() < t, U < t)
        return dev_look(eng, t, side)
    look.U = None
    return look


@pytest.mark.parametrize("N", host.tile_sizes(TILE))
def test_patterns_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    look = _pattern_look(eng)
    for name, U, want in host.patterns(N, TILE):
        host.check_pattern(look, name, U, want, N)
    for name, U, t, _ in mh.hand_made(N):               # the threshold, NaN and one-ulp fields, on both sides
        for side in SIDES:
            host.check_look(look(U, t, side), fg_of(U, t, side), f"{name} N={N} {side}")
    s.close(fetch_U=False)


def test_patterns_on_the_device_fp32(gpu):
    N = TILE[0] + 1                                      # (no multiple of four: the element loads; two bands)
    s, eng = engine_of(N, 'chirp', 'float32')
    look = _pattern_look(eng, check_upload=True)
    for name, U, want in host.patterns(N, TILE):
        host.check_pattern(look, name, U, want, N)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random fields: every load path, engine and element type
# ---------------------------------------------------------------------------
RANDOM_CASES = [(8, 'chirp', 'float64'), (100, 'chirp', 'float32'), (129, 'chirp', 'float32'), (512, 'fast', 'float32'),
                (513, 'chirp', 'float64'), (100, 'direct', 'float64')]


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    rng = np.random.default_rng(13 * N + len(engine))
    for density in (0.3, 0.6, 0.95):
        U = mh.field_of(rng.random((N, N)) < density)
        k = max(2, N // 16)
        U[rng.integers(0, N, k), rng.integers(0, N, k)] = T     # a few pixels at the threshold: background below
        eng.set_U(U)
        Ud = eng.get_U()
        assert np.array_equal(Ud == T, U == T)
        for side in SIDES:
            di = dev_look(eng, T, side)
            host.check_look(di, fg_of(Ud, T, side), f"N={N} {engine} {dtype} {density} {side}")
            assert 0 < di.fg < N * N and di.ninf == 0 and di.d2max >= 1
    assert eng.distance_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the other looks of the same handle
# ---------------------------------------------------------------------------
def test_an_evolved_field_against_scipy_and_the_other_looks(gpu):
    """After 40 steps at N = 512 fp64 on the fast engine, thresholded at the field's median: the device equals scipy;
    FG is the morphology's n_A and the components' area; D2 > 0 is the foreground."""
    N, steps = 512, 40
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    for side in SIDES:
        di = s.distance(t, side=side, map=True)
        X = fg_of(U, t, side)
        host.check_look(di, X, f"evolved N={N} {side}")
        assert np.array_equal(di.d2 > 0, X) and di.threshold == t and di.N == N and di.delx == sol.delx
        assert di.fg == s.components(t, side=side, table=False).area
        assert di.r_max_phys == di.r_max * sol.delx and 0 < di.quantile(0.5) <= di.quantile(0.9) <= di.r_max
    below = s.distance(t)                                # the defaults: the histogram, no map
    assert below.d2 is None and below.hist is not None and below.fg == s.morphology(t).n_A and 0 < below.fg < N * N
    bare = s.distance(t, hist=False)
    assert bare.hist is None and np.array_equal(bare.words, below.words)
    own = s.distance()                                   # params.threshold
    assert own.threshold == s.params.threshold and own.fg == s.morphology().n_A
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. determinism; a look changes nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_two_looks_give_the_same_bits(gpu, N, engine):
    s = tgs.solver(N, 8, engine)
    s.prepare()
    s.solve_or_resume(4)
    t = float(np.median(s._engine.get_U()))
    a, b = s.distance(t, map=True), s.distance(t, map=True)
    assert a.fg > 1 and np.array_equal(a.words, b.words) and np.array_equal(a.hist, b.hist) and np.array_equal(a.d2, b.d2)
    s.close(fetch_U=False)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with distance() on both sides between them against the same calls with get_U() between them: all nine
    record columns, the state and the final field, bit for bit."""
    assert {c[1] for c in OBSERVE_CASES} == {'fast', 'chirp'}

    def look(s):
        s.distance(map=True)
        s.distance(side='above')
    got, Ug = tgs._observed_run(N, engine, calls, look, seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert got[-1][0].shape[0] == 1 + sum(calls) - (1 if seed is None else 0)
    assert np.array_equal(Ug, Ur)


# ---------------------------------------------------------------------------
# 5. batches
# ---------------------------------------------------------------------------
def _same(a, b):
    return (np.array_equal(a.words, b.words) and np.array_equal(a.hist, b.hist)
            and (a.d2 is None or b.d2 is None or np.array_equal(a.d2, b.d2)))


@pytest.mark.parametrize("N,engine", [(256, 'fast'), (136, 'chirp')])
def test_batch_equals_the_single_solvers_and_leaves_the_members_alone(gpu, N, engine):
    B = 3
    ps = tgs._members(N, B, 100)                         # (three members with their own A0, A1 and seed)
    for m, p in enumerate(ps):
        p.threshold = p.XXX + 1e-3 * (m - 1)             # ... and their own threshold
    ts = [p.threshold for p in ps]
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    dis = bs.distance(map=True)                          # every member at its own threshold
    assert len(dis) == B and [di.threshold for di in dis] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    for m in range(B):
        host.check_look(dis[m], fields[m] < ts[m], f"member {m}")
        assert _same(bs.distance(m, map=True), dis[m]), m                       # member = m
        assert _same(bs.solvers[m].distance(map=True), dis[m]), m               # through the member's Solver
        assert 0 < dis[m].fg < N * N
    assert not np.array_equal(dis[0].words, dis[1].words)
    same = bs.distance(threshold=ts[1], side='above')                            # one threshold for all
    for m in range(B):
        host.check_look(same[m], ~(fields[m] < ts[1]), f"member {m} above")
    assert _same(bs.distance(2, threshold=ts), dis[2])
    with pytest.raises(ValueError):
        bs.distance(threshold=[0.5])
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert _same(s.distance(map=True), dis[m]), m
        s.close(fetch_U=False)
    ref = BatchSolver(ps)                                # the members' next call without the looks
    ref.prepare()
    ref.solve_or_resume(20)
    ref.solve_or_resume(5)
    plain = tgs._batch_snap(ref)
    ref.close(fetch_U=False)
    for m in range(B):
        assert np.array_equal(looked[m][0], plain[m][0]) and np.array_equal(looked[m][1], plain[m][1]), m
        assert looked[m][2] == plain[m][2], m


# ---------------------------------------------------------------------------
# 5b. experiment
# ---------------------------------------------------------------------------
def same_values(got, want):
    """Parsed csv values against computed ones: equal, or NaN on both sides."""
    return len(got) == len(want) and all(g == w or (g != g and w != w) for g, w in zip(got, want))


class ModelSolver:
    """What experiment._widths_of asks of a Solver, answered by the numpy model on a field."""

    def __init__(self, U, threshold):
        self.U, self.threshold = U, threshold

    def distance(self, side='below'):
        return host.model_look(self.U, self.threshold, side)


def test_experiment_widths_batch_equals_member_path(gpu, tmp_path, capsys):
    """`-N 136 -R 4 -n 80 --widths` one by one and with `--batch 2` write identical -widths.csv, their -results.csv is
    byte for byte that of a run without the flag, and without the flag no such file appears.  Every row is what
    experiment._widths_of gives from the numpy model on the member's exported final field (the floats are written with
    repr: the parsed values are compared exactly)."""
    base = ['-N', '136', '-R', '4', '-n', '80']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--concurrent', '1', '--widths', '--export-csv', 'U', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '2', '--widths', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    one, batch = open(tmp_path / 'one-widths.csv').read(), open(tmp_path / 'batch-widths.csv').read()
    assert one == batch
    lines = one.splitlines()
    assert lines[0] == ','.join(ex.WIDTHS_COLS) and len(lines) == 5
    ints = [c in ex.MEASUREMENTS[3].int_cols for c in ex.WIDTHS_COLS]
    assert ex.MEASUREMENTS[3].key == 'widths' and sum(ints) == 7
    for i, ln in enumerate(lines[1:]):
        f = ln.split(',')
        assert all(('.' not in v and 'e' not in v) == k or v == 'nan' for v, k in zip(f, ints)), ln
        got = [int(v) if k else float(v) for v, k in zip(f, ints)]
        U = np.loadtxt(tmp_path / f'one-run{i}.solution.U.csv', delimiter=',')
        assert U.shape == (136, 136) and got[0] == i and got[1] == chsimpy_amd.Parameters().threshold
        want = (i,) + ex._widths_of(ModelSolver(U, got[1]))
        assert same_values(got, want), (i, got, want)
        assert got[2] + got[8] == 136 * 136 and 0 < got[2] < 136 * 136 and got[3] >= 1.0      # both sides are there
    assert not (tmp_path / 'plain-widths.csv').exists()
    plain = open(tmp_path / 'plain-results.csv', 'rb').read()
    assert plain == open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    nb = _lib.distance_bins(N)
    out = np.zeros(_lib.CHS_DT_WORDS, dtype=np.int64)
    hist = np.zeros(nb + 1, dtype=np.int64)
    d2 = np.zeros((N, N), dtype=np.int32)
    ms = np.zeros(1)
    o, h, d = _lib._i64ptr(out), _lib._i64ptr(hist), _lib._i32ptr(d2)
    assert gpu.chs_distance(eng._h, 0.5, 0, o) == _lib.CHS_ESTATE                            # no field yet
    for call in (lambda: gpu.chs_distance_hist(eng._h, nb, h), lambda: gpu.chs_distance_map(eng._h, d),
                 lambda: gpu.chs_distance_last_ms(eng._h, _lib._dptr(ms))):
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.distance()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert gpu.chs_distance(eng._h, bad, 0, o) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    for side in (2, -1):
        assert gpu.chs_distance(eng._h, 0.5, side, o) == _lib.CHS_EINVAL
        assert 'side' in gpu.chs_last_error().decode()
    assert gpu.chs_distance(eng._h, 0.5, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_distance(None, 0.5, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_distance_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_distance_map(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_distance_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_distance_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE               # none of them was a look
    assert gpu.chs_distance_map(eng._h, d) == _lib.CHS_ESTATE and gpu.chs_distance_hist(eng._h, nb, h) == _lib.CHS_ESTATE
    t = float(np.median(eng.get_U()))
    assert gpu.chs_distance(eng._h, t, 0, o) == _lib.CHS_OK
    assert out[0] > 0 and gpu.chs_distance_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for bins in (nb - 1, nb + 1, 0, -1):
        assert gpu.chs_distance_hist(eng._h, bins, h) == _lib.CHS_EINVAL
        assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_distance_hist(eng._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_distance_map(eng._h, None) == _lib.CHS_EINVAL
    hist[nb] = -7
    assert gpu.chs_distance_hist(eng._h, nb, h) == _lib.CHS_OK and gpu.chs_distance_map(eng._h, d) == _lib.CHS_OK
    assert hist[nb] == -7 and int(hist[:nb].sum()) == int(out[0]) == int((d2 > 0).sum())
    with pytest.raises(ValueError):
        s.distance(side='left')
    with pytest.raises(_lib.EngineError):
        s.distance(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_distance(b._h, 0, 0.5, 0, o) == _lib.CHS_ESTATE                     # no fields yet
    assert gpu.chs_batch_distance_hist(b._h, nb, h) == _lib.CHS_ESTATE
    assert gpu.chs_batch_distance_map(b._h, d) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, -2, 65536):
        assert gpu.chs_batch_distance(b._h, member, 0.5, 0, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_distance(b._h, 1, float('nan'), 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance(b._h, 1, 0.5, 3, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance(b._h, 1, 0.5, 1, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance(None, 1, 0.5, 1, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance_map(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance_hist(b._h, nb, h) == _lib.CHS_ESTATE                       # none of them was a look
    assert gpu.chs_batch_distance(b._h, 1, 0.5, 1, o) == _lib.CHS_OK
    assert gpu.chs_batch_distance_hist(b._h, nb + 1, h) == _lib.CHS_EINVAL
    assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_batch_distance_hist(b._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance_map(b._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_distance_hist(b._h, nb, h) == _lib.CHS_OK and gpu.chs_batch_distance_map(b._h, d) == _lib.CHS_OK
    assert out[0] == int((~(bs.solvers[1]._engine.get_U() < 0.5)).sum()) == int((d2 > 0).sum())
    bs.close(fetch_U=False)
