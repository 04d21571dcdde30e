"""GPU tests (``-m gpu``) of the local thickness of the thresholded field on the device (chs_thickness /
chs_batch_thickness, chsimpy_amd/csrc/chs_thickness.hip).

Reference: the numpy model of chsimpy_amd/thickness.py applied to the field as downloaded with ``get_U`` -- the exact
values the device holds, also for fp32 -- which tests/test_thickness_host.py holds to a brute-force painter over all
centres.  Everything is integer: map, histogram and words are compared for equality.

The pattern sizes: N = 8 (one tile of everything), 65 (two 64-row bands of the distance look, discs across every tile
border) and 100 (no multiple of four: element loads)."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, distance, thickness
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_thickness_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
SIDES = host.SIDES


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, side, max_work=None):
    code = components.side_code(side)
    (words, hi, t2), (dwords, dhi, d2) = eng.thickness_look(t, code, True, True, max_work)
    di = distance.Distance(dwords, eng.N, t, side, hist=dhi, d2=d2)
    return thickness.Thickness(words, eng.N, t, side, hist=hi, t2=t2, distance=di)


def same(a, b):
    return (np.array_equal(a.words, b.words) and np.array_equal(a.hist, b.hist) and np.array_equal(a.t2, b.t2)
            and np.array_equal(a.distance.words, b.distance.words) and np.array_equal(a.distance.hist, b.distance.hist)
            and np.array_equal(a.distance.d2, b.distance.d2))


def check(got, Ud, t, side, what):
    """A device look against the model on the downloaded field; the definition's invariants on top."""
    want = thickness.model_look(Ud, t, side)
    assert np.array_equal(got.t2, want.t2), what
    assert np.array_equal(got.words, want.words), (what, got.words, want.words)
    assert np.array_equal(got.hist, want.hist), what
    assert np.array_equal(got.distance.d2, want.distance.d2) and np.array_equal(got.distance.words, want.distance.words), what
    host.check_invariants(got.t2, got.kept, got.work, got.distance.d2, what)
    return want


# ---------------------------------------------------------------------------
# 1. patterns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 65, 100])
def test_patterns_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    most = 16 * _lib.thickness_work_default(N)          # (one background pixel in a full grid is what the limit is for)
    for name, X in host.patterns(N):
        eng.set_U(mh.field_of(X))
        Ud = eng.get_U()
        for side in SIDES:
            want = check(dev_look(eng, T, side, most), Ud, T, side, f"{name} N={N} {side}")
            assert want.fg == int((X if side == 'below' else ~X).sum())
    for name, U, t, _ in mh.hand_made(N):               # the threshold, NaN and one-ulp fields, on both sides
        eng.set_U(U)
        Ud = eng.get_U()
        for side in SIDES:
            check(dev_look(eng, t, side, most), Ud, t, side, f"{name} N={N} {side}")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random fields: engines and element types
# ---------------------------------------------------------------------------
RANDOM_CASES = [(8, 'chirp', 'float64'), (100, 'direct', 'float64'), (129, 'chirp', 'float32'), (128, 'fast', 'float32')]


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    rng = np.random.default_rng(17 * N + len(engine))
    for density in (0.3, 0.6, 0.95):
        U = mh.field_of(rng.random((N, N)) < density)
        k = max(2, N // 16)
        U[rng.integers(0, N, k), rng.integers(0, N, k)] = T     # a few pixels at the threshold: background below
        eng.set_U(U)
        Ud = eng.get_U()
        assert np.array_equal(Ud == T, U == T)
        for side in SIDES:
            th = dev_look(eng, T, side)
            check(th, Ud, T, side, f"N={N} {engine} {dtype} {density} {side}")
            assert 0 < th.fg < N * N and th.ninf == 0 and th.t2max >= 1 and 1 <= th.kept <= th.fg
    assert eng.thickness_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the other looks of the same handle
# ---------------------------------------------------------------------------
def test_an_evolved_field_against_the_model_and_the_other_looks(gpu):
    """After 40 steps at N = 512 fp64 on the fast engine, thresholded at the field's median: the device equals the model
    under the default work limit; the distance look inside is the handle's distance look; FG is the components' area."""
    N, steps = 512, 40
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    for side in SIDES:
        th = s.thickness(t, side=side, map=True)         # max_work=None: the default
        check(th, U, t, side, f"evolved N={N} {side}")
        assert th.work <= _lib.thickness_work_default(N) and th.work_per_pixel < 1024
        di = s.distance(t, side=side, map=True)
        assert np.array_equal(th.distance.words, di.words) and np.array_equal(th.distance.hist, di.hist)
        assert np.array_equal(th.distance.d2, di.d2)
        assert th.fg == s.components(t, side=side, table=False).area and th.delx == sol.delx and th.N == N
        assert 0 < th.quantile(0.5) <= th.quantile(0.9) <= th.r_max
        assert th.mean_thickness_phys == th.mean_thickness * sol.delx and th.r_max == di.r_max
    below = s.thickness(t)                               # the defaults: the histogram, no map
    assert below.t2 is None and below.hist is not None and below.distance.d2 is None and 0 < below.fg < N * N
    bare = s.thickness(t, hist=False)
    assert bare.hist is None and np.array_equal(bare.words, below.words)
    own = s.thickness()                                  # params.threshold
    assert own.threshold == s.params.threshold and own.fg == s.morphology().n_A
    assert s._engine.thickness_ms() >= s._engine.distance_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. the work limit
# ---------------------------------------------------------------------------
def test_the_work_limit(gpu):
    N = 32
    s, eng = engine_of(N, 'chirp')
    nb = _lib.distance_bins(N)
    out = np.zeros(_lib.CHS_TH_WORDS, dtype=np.int64)
    t2, d2 = np.zeros((N, N), dtype=np.int32), np.zeros((N, N), dtype=np.int32)
    o, tp, dp = _lib._i64ptr(out), _lib._i32ptr(t2), _lib._i32ptr(d2)
    other = mh.field_of(np.random.default_rng(1).random((N, N)) < 0.6)
    eng.set_U(other)
    first = dev_look(eng, T, 'below')                    # a good look of another field
    X = np.ones((N, N), dtype=bool)
    X[N // 3, N // 2 + 1] = False
    U = mh.field_of(X)
    eng.set_U(U)
    want = thickness.model_look(U, T)
    work, default = want.work, _lib.thickness_work_default(N)
    assert 0 < work - 1 and work <= 16 * default
    assert gpu.chs_thickness(eng._h, T, 0, work - 1, o) == _lib.CHS_ELIMIT                  # refused
    msg = gpu.chs_last_error().decode()
    assert str(work) in msg and str(work - 1) in msg
    assert out[_lib.CHS_TH_WORK] == work and out[_lib.CHS_TH_KEPT] == want.kept and not out[:5].any()
    assert gpu.chs_thickness_map(eng._h, tp) == _lib.CHS_ESTATE
    assert gpu.chs_thickness_hist(eng._h, nb, _lib._i64ptr(np.zeros(nb, dtype=np.int64))) == _lib.CHS_ESTATE
    assert gpu.chs_distance_map(eng._h, dp) == _lib.CHS_OK                                  # the distance look is complete
    assert np.array_equal(d2, want.distance.d2) and not np.array_equal(d2, first.distance.d2)
    with pytest.raises(_lib.ThicknessLimitError) as e:
        s.thickness(T, max_work=work - 1)
    assert (e.value.work, e.value.limit) == (work, work - 1) and isinstance(e.value, _lib.EngineError)
    got = dev_look(eng, T, 'below', work)                # exactly enough: the next good look works
    check(got, U, T, 'below', "max_work = WORK")
    assert got.work == work
    for bad in (16 * default + 1, -1, -(1 << 62)):       # out of range: the previous look stays
        assert gpu.chs_thickness(eng._h, T, 0, bad, o) == _lib.CHS_EINVAL, bad
        assert 'max_work' in gpu.chs_last_error().decode()
        assert gpu.chs_thickness_map(eng._h, tp) == _lib.CHS_OK and np.array_equal(t2, want.t2)
    assert gpu.chs_thickness(eng._h, T, 0, 16 * default, o) == _lib.CHS_OK and np.array_equal(out, want.words)
    assert gpu.chs_thickness(eng._h, T, 0, 0, o) == _lib.CHS_OK and np.array_equal(out, want.words)   # 0: the default
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 5. determinism; a look changes nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_two_looks_give_the_same_bits(gpu, N, engine):
    s = tgs.solver(N, 8, engine)
    s.prepare()
    s.solve_or_resume(4)
    t = float(np.median(s._engine.get_U()))
    a, b = s.thickness(t, map=True), s.thickness(t, map=True)
    assert a.fg > 1 and same(a, b)
    s.close(fetch_U=False)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with thickness() on both sides between them against the same calls with get_U() between them: all nine
    record columns, the state and the final field, bit for bit."""
    assert {c[1] for c in OBSERVE_CASES} == {'fast', 'chirp'}

    def look(s):
        t = float(np.median(s._engine.get_U()))
        s.thickness(t, map=True)
        s.thickness(side='above')
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
# 6. batches
# ---------------------------------------------------------------------------
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
    ths = bs.thickness(map=True)                         # every member at its own threshold
    assert len(ths) == B and [th.threshold for th in ths] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    for m in range(B):
        check(ths[m], fields[m], ts[m], 'below', f"member {m}")
        assert same(bs.thickness(m, map=True), ths[m]), m                       # member = m
        assert same(bs.solvers[m].thickness(map=True), ths[m]), m               # through the member's Solver
        assert 0 < ths[m].fg < N * N
    assert not np.array_equal(ths[0].words, ths[1].words)
    above = bs.thickness(threshold=ts[1], side='above', map=True)                # one threshold for all
    for m in range(B):
        check(above[m], fields[m], ts[1], 'above', f"member {m} above")
    assert bs._batch.thickness_ms() >= 0.0
    with pytest.raises(ValueError):
        bs.thickness(threshold=[0.5])
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert same(s.thickness(map=True), ths[m]), m
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
# 7. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    nb = _lib.distance_bins(N)
    out = np.zeros(_lib.CHS_TH_WORDS, dtype=np.int64)
    hist = np.zeros(nb + 1, dtype=np.int64)
    t2 = np.zeros((N, N), dtype=np.int32)
    ms = np.zeros(1)
    o, h, d = _lib._i64ptr(out), _lib._i64ptr(hist), _lib._i32ptr(t2)
    assert gpu.chs_thickness(eng._h, 0.5, 0, 0, o) == _lib.CHS_ESTATE                        # no field yet
    for call in (lambda: gpu.chs_thickness_hist(eng._h, nb, h), lambda: gpu.chs_thickness_map(eng._h, d),
                 lambda: gpu.chs_thickness_last_ms(eng._h, _lib._dptr(ms))):
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.thickness()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert gpu.chs_thickness(eng._h, bad, 0, 0, o) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    for side in (2, -1):
        assert gpu.chs_thickness(eng._h, 0.5, side, 0, o) == _lib.CHS_EINVAL
        assert 'side' in gpu.chs_last_error().decode()
    assert gpu.chs_thickness(eng._h, 0.5, 0, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_thickness(None, 0.5, 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_thickness_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_thickness_map(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_thickness_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_thickness_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE              # none of them was a look
    assert gpu.chs_thickness_map(eng._h, d) == _lib.CHS_ESTATE and gpu.chs_thickness_hist(eng._h, nb, h) == _lib.CHS_ESTATE
    t = float(np.median(eng.get_U()))
    assert gpu.chs_thickness(eng._h, t, 0, 0, o) == _lib.CHS_OK
    assert out[0] > 0 and gpu.chs_thickness_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for bins in (nb - 1, nb + 1, 0, -1):
        assert gpu.chs_thickness_hist(eng._h, bins, h) == _lib.CHS_EINVAL
        assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_thickness_hist(eng._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_thickness_map(eng._h, None) == _lib.CHS_EINVAL
    hist[nb] = -7
    assert gpu.chs_thickness_hist(eng._h, nb, h) == _lib.CHS_OK and gpu.chs_thickness_map(eng._h, d) == _lib.CHS_OK
    assert hist[nb] == -7 and int(hist[:nb].sum()) == int(out[0]) == int((t2 > 0).sum())
    with pytest.raises(ValueError):
        s.thickness(side='left')
    with pytest.raises(_lib.EngineError):
        s.thickness(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_thickness(b._h, 0, 0.5, 0, 0, o) == _lib.CHS_ESTATE                 # no fields yet
    assert gpu.chs_batch_thickness_hist(b._h, nb, h) == _lib.CHS_ESTATE
    assert gpu.chs_batch_thickness_map(b._h, d) == _lib.CHS_ESTATE
    assert gpu.chs_batch_thickness_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, -2, 65536):
        assert gpu.chs_batch_thickness(b._h, member, 0.5, 0, 0, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_thickness(b._h, 1, float('nan'), 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness(b._h, 1, 0.5, 3, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness(b._h, 1, 0.5, 1, -1, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness(b._h, 1, 0.5, 1, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness(None, 1, 0.5, 1, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness_map(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness_last_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness_hist(b._h, nb, h) == _lib.CHS_ESTATE                      # none of them was a look
    assert gpu.chs_batch_thickness(b._h, 1, 0.5, 1, 0, o) == _lib.CHS_OK
    assert gpu.chs_batch_thickness_hist(b._h, nb + 1, h) == _lib.CHS_EINVAL
    assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_batch_thickness_hist(b._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness_map(b._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_thickness_hist(b._h, nb, h) == _lib.CHS_OK and gpu.chs_batch_thickness_map(b._h, d) == _lib.CHS_OK
    assert out[0] == int((~(bs.solvers[1]._engine.get_U() < 0.5)).sum()) == int((t2 > 0).sum())
    bs.close(fetch_U=False)
