"""GPU tests (``-m gpu``) of the skeleton look on the device (chs_skeleton / chs_batch_skeleton,
chsimpy_amd/csrc/chs_skeleton.hip).

Reference: the packed numpy model of chsimpy_amd/skeleton.py applied to the field as downloaded with ``get_U`` -- the exact
values the device holds, also for fp32 -- which tests/test_skeleton_host.py holds to a per-pixel implementation of the
definition.  Everything is integer: plane, words and histogram are compared for equality, with no tolerance.

The sizes: N = 8 (one word a row, one workgroup), 63, 64, 65 (a full word, and one pixel in a second word), 129 (three words,
the last one partial), 200 (the chirp engine; several workgroups) and 256 (the fast engine), each in fp64 and fp32 and
on both sides."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, skeleton
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_skeleton_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
SIDES = host.SIDES


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, side, max_subiters=None):
    words, hi, plane = eng.skeleton_look(t, components.side_code(side), True, True, max_subiters)
    return skeleton.Skeleton(words, eng.N, t, side, hist=hi, plane=plane)


def same(a, b):
    return np.array_equal(a.words, b.words) and np.array_equal(a.hist, b.hist) and np.array_equal(a.plane, b.plane)


def check(got, Ud, t, side, what, max_subiters=None):
    """A device look against the model on the downloaded field."""
    want = skeleton.model_look(Ud, t, side, max_subiters=max_subiters)
    assert np.array_equal(got.plane, want.plane), what
    assert np.array_equal(got.words, want.words), (what, got.words, want.words)
    assert np.array_equal(got.hist, want.hist), what
    return want


# ---------------------------------------------------------------------------
# 1. patterns and random masks: sizes, engines, element types, both sides
# ---------------------------------------------------------------------------
CASES = [(N, engine, dtype) for N, engine in ((8, 'direct'), (63, 'direct'), (64, 'direct'), (65, 'direct'), (129, 'direct'),
                                             (200, 'chirp'), (256, 'fast')) for dtype in ('float64', 'float32')]


@pytest.mark.parametrize("N,engine,dtype", CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_patterns_and_random_masks(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    for name, X in host.patterns(N) + host.random_masks(N):
        eng.set_U(mh.field_of(X))
        Ud = eng.get_U()
        for side in SIDES:
            want = check(dev_look(eng, T, side), Ud, T, side, f"{name} N={N} {side}")
            assert want.fg == int((X if side == 'below' else ~X).sum())
            if side == 'below':                                    # ... and the per-pixel rule itself
                S, last = host.reference(f"{name} {N}", X)
                assert np.array_equal(want.mask(), S) and want.subiters == last, name
    assert eng.skeleton_ms() >= eng.skeleton_thin_ms() >= 0.0
    s.close(fetch_U=False)


def test_the_threshold_and_nan_conventions(gpu):
    N = 65
    s, eng = engine_of(N, 'direct')
    for name, U, t, _ in mh.hand_made(N):                          # the threshold, NaN and one-ulp fields, on both sides
        eng.set_U(U)
        Ud = eng.get_U()
        for side in SIDES:
            check(dev_look(eng, t, side), Ud, t, side, f"{name} {side}")
    s.close(fetch_U=False)


def test_carries_across_word_and_row_boundaries(gpu):
    """A diagonal line through (63, 63) - (64, 64) and a column pair at 63 | 64 stay as they are; the full grid at N = 65
    has a partial last word and takes 130 sub-iterations: more than four chunks of the host."""
    N = 65
    s, eng = engine_of(N, 'direct')
    pats = dict(host.patterns(N))
    for name in ('diagonal through 63-64', 'diagonal', 'antidiagonal'):
        eng.set_U(mh.field_of(pats[name]))
        sk = dev_look(eng, T, 'below')
        assert np.array_equal(sk.mask(), pats[name]) and sk.subiters == 0 and sk.ends == 2, name
        assert sk.diagonal == sk.pixels - 1 and sk.axial == 0
    eng.set_U(mh.field_of(pats['columns 63-64']))
    sk = dev_look(eng, T, 'below')
    S, last = host.reference('columns 63-64 65', pats['columns 63-64'])
    assert np.array_equal(sk.mask(), S) and sk.subiters == last and sk.euler8 == 1
    eng.set_U(mh.field_of(pats['full']))
    sk = dev_look(eng, T, 'below')
    assert sk.subiters + 4 == 130 and sk.ninf == sk.pixels and sk.fg == N * N and sk.euler8 == 1
    check(sk, eng.get_U(), T, 'below', 'full 65')
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. evolved fields; the other looks of the same handle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [512, 4096])
def test_an_evolved_field_against_the_model_and_the_other_looks(gpu, N):
    """After 40 steps, fp64 on the fast engine, thresholded at the field's median: the device equals the packed model under
    the default limit; EULER8 is the morphology look's and FG the distance look's on the same handle.  At N = 512 the model
    starts from the downloaded field, on both sides.  At N = 4096 (a row of the plane is exactly one wavefront of words)
    the side below alone is looked at, and the packed model is fed the D2 of a distance look on the same handle: the
    numpy distance transform alone takes seconds there, tests/test_gpu_distance.py holds D2 to it, and here
    ``D2 > 0`` is held to ``U < t`` of the downloaded field, so the mask is tied to the field; this case does not check
    the distance half on its own."""
    steps = 40
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    for side in (SIDES if N == 512 else SIDES[:1]):
        sk = s.skeleton(t, side=side, map=True)                # max_subiters=None: the default
        di = s.distance(t, side=side, map=N > 512)
        if N == 512:
            check(sk, U, t, side, f"evolved N={N} {side}")
        else:                                                  # the packed model on the distance look's own D2 (held to its
            assert np.array_equal(di.d2 > 0, U < t)            # numpy model in tests/test_gpu_distance.py, seconds at this N)
            words, hist, plane = skeleton.skeleton_of(di.d2)
            assert np.array_equal(sk.plane, plane) and np.array_equal(sk.words, words) and np.array_equal(sk.hist, hist)
        assert sk.fg == di.fg and 0 < sk.pixels < sk.fg and sk.d2max <= di.d2max and sk.ninf == 0
        if side == 'below':
            assert sk.euler8 == s.morphology(t).euler8
        assert sk.delx == sol.delx and sk.N == N and sk.limit == _lib.skeleton_subiters_default(N)
        assert 1 <= sk.quantile(0.5) <= sk.quantile(0.9) <= sk.r_max and sk.length_phys == sk.length * sol.delx
    if N == 512:
        below = s.skeleton(t)                                  # the defaults: the histogram, no plane
        assert below.plane is None and below.mask() is None and below.hist is not None and 0 < below.fg < N * N
        bare = s.skeleton(t, hist=False)
        assert bare.hist is None and np.array_equal(bare.words, below.words)
        own = s.skeleton()                                     # params.threshold
        assert own.threshold == s.params.threshold and own.fg == s.morphology().n_A
        assert s._engine.skeleton_ms() >= s._engine.distance_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. the limit
# ---------------------------------------------------------------------------
def test_the_limit(gpu):
    N = 65
    s, eng = engine_of(N, 'direct')
    nb = _lib.distance_bins(N)
    out = np.zeros(_lib.CHS_SK_WORDS, dtype=np.int64)
    plane = np.zeros((N, 2), dtype=np.uint64)
    d2 = np.zeros((N, N), dtype=np.int32)
    o, pp, dp = _lib._i64ptr(out), plane.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)), _lib._i32ptr(d2)
    other = mh.field_of(np.random.default_rng(1).random((N, N)) < 0.6)
    eng.set_U(other)
    first = dev_look(eng, T, 'below')                    # a good look of another field
    U = mh.field_of(np.ones((N, N), dtype=bool))
    eng.set_U(U)
    assert gpu.chs_skeleton(eng._h, T, 0, 16, o) == _lib.CHS_ELIMIT                         # refused
    msg = gpu.chs_last_error().decode()
    assert 'sub-iteration 16' in msg and 'max_subiters = 16' in msg
    assert out[_lib.CHS_SK_SUBITERS] == 16 and out[_lib.CHS_SK_LIMIT] == 16 and not out[:15].any()
    assert gpu.chs_skeleton_plane(eng._h, pp) == _lib.CHS_ESTATE
    assert gpu.chs_skeleton_hist(eng._h, nb, _lib._i64ptr(np.zeros(nb, dtype=np.int64))) == _lib.CHS_ESTATE
    assert gpu.chs_distance_map(eng._h, dp) == _lib.CHS_OK                                  # the distance look is complete
    assert (d2 == skeleton.CHS_DT_INF).all()
    with pytest.raises(_lib.SkeletonLimitError) as e:
        s.skeleton(T, max_subiters=16)
    assert (e.value.subiters, e.value.limit) == (16, 16) and isinstance(e.value, _lib.EngineError)
    with pytest.raises(_lib.SkeletonLimitError) as e:
        s.skeleton(T, max_subiters=129)                  # the last deletion is in sub-iteration 126: three quiet ones
    assert (e.value.subiters, e.value.limit) == (126, 129)
    got = dev_look(eng, T, 'below', 130)                 # exactly enough
    check(got, U, T, 'below', "max_subiters = 130", 130)
    assert (got.subiters, got.limit) == (126, 130)
    want = skeleton.model_look(U, T)
    default = _lib.skeleton_subiters_default(N)
    for bad in (16 * default + 1, -1, -(1 << 62)):       # out of range: the previous look stays
        assert gpu.chs_skeleton(eng._h, T, 0, bad, o) == _lib.CHS_EINVAL, bad
        assert 'max_subiters' in gpu.chs_last_error().decode()
        assert gpu.chs_skeleton_plane(eng._h, pp) == _lib.CHS_OK and np.array_equal(plane, want.plane)
    for limit in (16 * default, 0):                      # 0: the default
        assert gpu.chs_skeleton(eng._h, T, 0, limit, o) == _lib.CHS_OK
        assert np.array_equal(out[:16], want.words[:16]) and out[_lib.CHS_SK_LIMIT] == (limit or default)
    check(dev_look(eng, T, 'below'), U, T, 'below', 'the same handle with the default')
    assert not np.array_equal(first.plane, want.plane)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. determinism; a look changes nothing
# ---------------------------------------------------------------------------
def test_two_looks_give_the_same_bits(gpu):
    s = tgs.solver(128, 8, 'fast')
    s.prepare()
    s.solve_or_resume(4)
    t = float(np.median(s._engine.get_U()))
    a, b = s.skeleton(t, map=True), s.skeleton(t, map=True)
    assert a.fg > 1 and same(a, b)
    s.close(fetch_U=False)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with skeleton() on both sides between them against the same calls with get_U() between them: all nine record
    columns, the state and the final field, bit for bit."""
    assert {c[1] for c in OBSERVE_CASES} == {'fast', 'chirp'}

    def look(s):
        t = float(np.median(s._engine.get_U()))
        s.skeleton(t, map=True)
        s.skeleton(side='above')
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
# 5. batches; the pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(256, 'fast'), (136, 'chirp')])
def test_batch_equals_the_single_solvers(gpu, N, engine):
    B = 3
    ps = tgs._members(N, B, 100)                         # (three members with their own A0, A1 and seed)
    for m, p in enumerate(ps):
        p.threshold = p.XXX + 1e-3 * (m - 1)             # ... and their own threshold
    ts = [p.threshold for p in ps]
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    sks = bs.skeleton(map=True)                          # every member at its own threshold
    assert len(sks) == B and [sk.threshold for sk in sks] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    for m in range(B):
        check(sks[m], fields[m], ts[m], 'below', f"member {m}")
        assert same(bs.skeleton(m, map=True), sks[m]), m                         # member = m
        assert same(bs.solvers[m].skeleton(map=True), sks[m]), m                 # through the member's Solver
        assert 0 < sks[m].pixels < sks[m].fg < N * N
    assert not np.array_equal(sks[0].words, sks[1].words)
    above = bs.skeleton(threshold=ts[1], side='above', map=True)                 # one threshold for all
    for m in range(B):
        check(above[m], fields[m], ts[1], 'above', f"member {m} above")
    assert bs._batch.skeleton_ms() >= bs._batch.skeleton_thin_ms() >= 0.0
    with pytest.raises(ValueError):
        bs.skeleton(threshold=[0.5])
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert same(s.skeleton(map=True), sks[m]), m
        s.close(fetch_U=False)


def test_a_rearmed_handle_has_no_skeleton_result(gpu):
    N = 128
    _lib.pool_clear()
    s = tgs.solver(N, 4, 'fast')
    s.prepare()
    assert s.skeleton(map=True).pixels > 0
    s._engine.close()                                    # parked
    assert _lib.pool_count() == 1
    s2 = tgs.solver(N, 4, 'fast')
    eng = s2._get_engine()
    assert _lib.pool_count() == 0                        # ... and taken
    nb = _lib.distance_bins(N)
    ms = np.zeros(1)
    plane = np.zeros((N, 2), dtype=np.uint64)
    assert gpu.chs_skeleton_plane(eng._h, plane.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64))) == _lib.CHS_ESTATE
    assert gpu.chs_skeleton_hist(eng._h, nb, _lib._i64ptr(np.zeros(nb, dtype=np.int64))) == _lib.CHS_ESTATE
    assert gpu.chs_skeleton_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    assert gpu.chs_skeleton_thin_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    s2.prepare()
    U = eng.get_U()
    check(s2.skeleton(map=True), U, s2.params.threshold, 'below', 're-armed')
    s2.close(fetch_U=False)
    _lib.pool_clear()


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    nb = _lib.distance_bins(N)
    out = np.zeros(_lib.CHS_SK_WORDS, dtype=np.int64)
    hist = np.zeros(nb + 1, dtype=np.int64)
    plane = np.zeros((N, 2), dtype=np.uint64)
    ms = np.zeros(1)
    o, h, d = _lib._i64ptr(out), _lib._i64ptr(hist), plane.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64))
    assert gpu.chs_skeleton(eng._h, 0.5, 0, 0, o) == _lib.CHS_ESTATE                         # no field yet
    for call in (lambda: gpu.chs_skeleton_hist(eng._h, nb, h), lambda: gpu.chs_skeleton_plane(eng._h, d),
                 lambda: gpu.chs_skeleton_last_ms(eng._h, _lib._dptr(ms)), lambda: gpu.chs_skeleton_thin_ms(eng._h, _lib._dptr(ms))):
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.skeleton()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert gpu.chs_skeleton(eng._h, bad, 0, 0, o) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    for side in (2, -1):
        assert gpu.chs_skeleton(eng._h, 0.5, side, 0, o) == _lib.CHS_EINVAL
        assert 'side' in gpu.chs_last_error().decode()
    assert gpu.chs_skeleton(eng._h, 0.5, 0, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton(None, 0.5, 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton_plane(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton_thin_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE               # none of them was a look
    assert gpu.chs_skeleton_plane(eng._h, d) == _lib.CHS_ESTATE and gpu.chs_skeleton_hist(eng._h, nb, h) == _lib.CHS_ESTATE
    t = float(np.median(eng.get_U()))
    assert gpu.chs_skeleton(eng._h, t, 0, 0, o) == _lib.CHS_OK
    assert out[0] > 0 and gpu.chs_skeleton_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    assert gpu.chs_skeleton_thin_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for bins in (nb - 1, nb + 1, 0, -1):
        assert gpu.chs_skeleton_hist(eng._h, bins, h) == _lib.CHS_EINVAL
        assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_skeleton_hist(eng._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_skeleton_plane(eng._h, None) == _lib.CHS_EINVAL
    hist[nb] = -7
    assert gpu.chs_skeleton_hist(eng._h, nb, h) == _lib.CHS_OK and gpu.chs_skeleton_plane(eng._h, d) == _lib.CHS_OK
    assert hist[nb] == -7 and int(hist[:nb].sum()) == int(out[skeleton.CHS_SK_PIXELS]) == skeleton.popcount(plane)
    with pytest.raises(ValueError):
        s.skeleton(side='left')
    with pytest.raises(_lib.EngineError):
        s.skeleton(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_skeleton(b._h, 0, 0.5, 0, 0, o) == _lib.CHS_ESTATE                  # no fields yet
    assert gpu.chs_batch_skeleton_hist(b._h, nb, h) == _lib.CHS_ESTATE
    assert gpu.chs_batch_skeleton_plane(b._h, d) == _lib.CHS_ESTATE
    assert gpu.chs_batch_skeleton_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    assert gpu.chs_batch_skeleton_thin_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, -2, 65536):
        assert gpu.chs_batch_skeleton(b._h, member, 0.5, 0, 0, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_skeleton(b._h, 1, float('nan'), 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton(b._h, 1, 0.5, 3, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton(b._h, 1, 0.5, 1, -1, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton(b._h, 1, 0.5, 1, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton(None, 1, 0.5, 1, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_plane(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_last_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_thin_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_hist(b._h, nb, h) == _lib.CHS_ESTATE                       # none of them was a look
    assert gpu.chs_batch_skeleton(b._h, 1, 0.5, 1, 0, o) == _lib.CHS_OK
    assert gpu.chs_batch_skeleton_hist(b._h, nb + 1, h) == _lib.CHS_EINVAL
    assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_batch_skeleton_hist(b._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_plane(b._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_skeleton_hist(b._h, nb, h) == _lib.CHS_OK and gpu.chs_batch_skeleton_plane(b._h, d) == _lib.CHS_OK
    assert out[0] == int((~(bs.solvers[1]._engine.get_U() < 0.5)).sum()) and out[1] == skeleton.popcount(plane)
    bs.close(fetch_U=False)
