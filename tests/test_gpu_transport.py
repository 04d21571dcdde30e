"""GPU tests (``-m gpu``) of the transport look on the device (chs_transport / chs_batch_transport,
chsimpy_amd/csrc/chs_transport.hip).

The definition (include/chs_hip.h: chs_transport).  The active pixels are those of the 4-connected components of the phase
whose bounding box touches both the source wall and the opposite one.  Two 4-adjacent active pixels share a bond of
conductance 1; an active pixel on the source wall has a bond of conductance 2 to the face at c = 1, one on the target wall a
bond of conductance 2 to the face at c = 0.  F_in = sum over the source wall of 2 (1 - c), F_out = sum over the target wall
of 2 c, cut[k] the flux through the face between depth k-1 and k.  With r = b - A c evaluated from the returned c,
|F_out - F*|, |F_in - F*| and |cut[k] - F_out| are at most |r|_1.  A look succeeds only if RES1 <= tol min(F_in, F_out) for the
true residual.

What a device look is held to (tests/test_transport_host.py: check_solution; the field is the one downloaded with
``get_U``, the exact values the device holds, also for fp32):
* the integer words equal the numpy model's exactly;
* from the fetched map r is recomputed in numpy: the reported RES1 agrees with it to rounding(ACTIVE, N) = eps (73 ACTIVE +
  2 N^2) and RESINF to 72 eps.  Derivation: r_p is at most six terms whose magnitudes add up to at most 12 (b_p = 2, a
  diagonal of at most 6 times |c| <= 1, four neighbours), so any order of evaluation, fused or not, is within 6 u 12 = 36 eps
  of the exact r_p (u = eps / 2) and two evaluations within 72 eps; over ACTIVE pixels 72 eps ACTIVE, plus eps ACTIVE for the
  rounding of the two sums of non-negative terms (|r|_1 < 1).  A flux or a cut is a sum of at most N terms of magnitude at
  most 2: any two orders agree within 2 N u 2 N = 2 eps N^2;
* acceptance holds on the recomputed values: RES1 <= tol min(F_in, F_out) + rounding;
* flux: |F_out - F_ref| <= RES1_device + RES1_ref + rounding, F_ref and RES1_ref from scipy's spsolve on the host;
* conservation: every cut[k], and F_in, lies within RES1 + rounding of F_out;
* closed forms hold within RES1 + rounding;
* the map is not compared with the numpy model bit for bit -- the summation order is the kernel's own -- but held to the
  certificate above and to equality between two device looks.

The pattern sizes: N = 8 (one partial tile), 65 (2 x 2 tiles of 64 x 64, the second a single pixel wide) and 130 (3 x 3
tiles: a tile with eight neighbours).  The one-pixel serpentine needs as many iterations as it has pixels, N^2 / 2: at N =
130 that is above the default limit of 48 N + 64, and the look gets max_iters = 2 L there."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, transport
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_geodesic_host as gh
import test_morphology_host as mh
import test_transport_host as host

pytestmark = pytest.mark.gpu

T = host.T
SIDES = ('below', 'above')
SOURCES = host.SOURCES
W = transport


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, side, source, tol=W.TOL_DEFAULT, max_iters=None):
    words, vals, pr, cm = eng.transport_look(t, components.side_code(side), source, tol, True, True, max_iters)
    return transport.Transport(words, vals, eng.N, t, side, source, profile=pr, c=cm)


def check(got, X, source, what, tol=W.TOL_DEFAULT, limit=None, closed=None):
    host.check_solution(X, source, got.C, got.words, got.vals, got.profile, what, tol=tol, limit=limit, closed=closed)


def same_bits(a, b):
    return (np.array_equal(a.words, b.words) and a.vals.tobytes() == b.vals.tobytes() and a.profile.tobytes() == b.profile.tobytes()
            and a.C.tobytes() == b.C.tobytes())


# ---------------------------------------------------------------------------
# 1. patterns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sources", [(0, 1), (2, 3)], ids=['rows', 'columns'])
@pytest.mark.parametrize("N", [8, 65, 130])
def test_patterns_on_the_device(gpu, N, sources):
    s, eng = engine_of(N, 'chirp')
    default = _lib.transport_iters_default(N)
    assert default == transport.iters_default(N)
    names, most = set(), 0
    for name, X0, closed in host.patterns(N):
        names.add(name)
        for source in sources:
            X = host.oriented(X0, source)
            L = int(X.sum())
            limit = 2 * L if name == 'serpentine' and 2 * L > default else None
            for side in SIDES:
                eng.set_U(mh.field_of(X if side == 'below' else ~X))    # the same foreground on either side
                assert np.array_equal(components.foreground(eng.get_U(), T, side), X)
                got = dev_look(eng, T, side, source, max_iters=limit)
                check(got, X, source, f"{name} N={N} {side} source={source}", limit=limit, closed=closed)
                assert got.side == side and got.fg == L and got.percolates == (closed != 0.0)
                most = max(most, got.iters)
                if name == 'serpentine':
                    assert got.iters >= L - 1 and got.active == L       # a path of L unknowns: no fewer iterations
    assert names == {'full', 'channels', 'serpentine', 'comb', 'plate', 'no span', 'empty', 'beside'}
    assert (most > default) == (N == 130)
    for name, U, t, _ in mh.hand_made(N):                               # the threshold, NaN and one-ulp fields, on both sides
        eng.set_U(U)
        Ud = eng.get_U()
        for side in SIDES:
            X = components.foreground(Ud, t, side)
            check(dev_look(eng, t, side, sources[0]), X, sources[0], f"{name} N={N} {side} source={sources[0]}")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random masks: engines and element types
# ---------------------------------------------------------------------------
RANDOM_CASES = [(100, 'direct', 'float64'), (129, 'direct', 'float32'), (100, 'chirp', 'float32'), (129, 'chirp', 'float64'),
                (128, 'fast', 'float64'), (128, 'fast', 'float32')]     # (the fast engine has no N = 100 or 129)


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_masks(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    masks = gh.random_masks(N, 4)
    spans = set()
    for seed, X, perc in masks:
        U = mh.field_of(X)
        k = max(2, N // 16)
        rng = np.random.default_rng(seed)
        ii, jj = rng.integers(0, N, k), rng.integers(0, N, k)
        U[ii, jj] = np.where(X[ii, jj], np.nextafter(np.float32(T), np.float32(0)), T)   # at the threshold: background
        eng.set_U(U)
        assert np.array_equal(components.foreground(eng.get_U(), T, 'below'), X)
        for source in SOURCES:
            got = dev_look(eng, T, 'below', source)
            check(got, X, source, f"N={N} {engine} {dtype} seed={seed} source={source}")
            if source == 0:
                assert got.percolates == perc
                spans.add(got.percolates)
                again = dev_look(eng, T, 'below', source)
                assert same_bits(again, got)
        eng.set_U(mh.field_of(~X))
        check(dev_look(eng, T, 'above', 1), X, 1, f"N={N} {engine} {dtype} seed={seed} above")
    assert spans == {True, False}                                       # a spanning and a non-spanning mask
    assert eng.transport_ms() >= eng.transport_solve_ms() >= 0.0
    s.close(fetch_U=False)


@pytest.mark.parametrize("tol", [1e-2, 1e-9])
def test_the_tolerance_is_the_callers(gpu, tol):
    N = 100
    s, eng = engine_of(N, 'chirp')
    _, X, _ = gh.random_masks(N, 4)[0]
    eng.set_U(mh.field_of(X))
    got = dev_look(eng, T, 'below', 0, tol=tol)
    check(got, X, 0, f"tol={tol}", tol=tol)
    ref = dev_look(eng, T, 'below', 0)
    assert (got.iters < ref.iters) == (tol > W.TOL_DEFAULT) and got.tol == tol
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the components of the same handle
# ---------------------------------------------------------------------------
EVOLVED = dict(seed=2024, steps=4000, side='below', sources=('top', 'left'))


def test_an_evolved_field(gpu):
    """N = 128 on the fast engine, thresholded at its median.  At the median a phase rarely spans at connectivity 4: the
    seed and the step count were searched with the oracle on the CPU (seeds 2023 .. 2034 at 1500 to 6000 steps) for a
    field whose phase below the median spans from top to bottom and from left to right, and keeps doing so when the
    threshold moves by 1e-6: seed 2024 after 4000 steps, 5234 of 8192 pixels active.  Asserted here on the device's own
    field."""
    N, steps, side = 128, EVOLVED['steps'], EVOLVED['side']
    s = tgs.solver(N, steps + 1, 'fast', seed=EVOLVED['seed'])
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    X = components.foreground(U, t, side)
    cc = s.components(t, connectivity=4, side=side, table=True)
    for source in EVOLVED['sources']:
        code = transport.source_code(source)
        assert transport.System(X, code).active.any(), source            # it spans
        got = s.transport(t, side=side, source=source, map=True)
        check(got, X, code, f"evolved source={source}")
        again = s.transport(t, side=side, source=source, map=True)      # two looks: the same bits
        assert same_bits(again, got) and again.iters == got.iters and again.checks == got.checks
        assert got.cc_count == cc.count and got.fg == cc.area
        lo, hi = (cc.bbox[:, 0], cc.bbox[:, 1]) if code < 2 else (cc.bbox[:, 2], cc.bbox[:, 3])
        span = (lo == 0) & (hi == N - 1)
        assert got.cc_spanning == int(span.sum()) and got.active == int(cc.areas[span].sum(dtype=np.int64))
        assert got.percolates and got.tortuosity_factor >= 1.0 and 0.0 < got.deff < got.porosity
        assert got.limit == _lib.transport_iters_default(N) and got.delx == sol.delx and got.deff_bound <= 1e-6 * got.deff
        bare = s.transport(t, side=side, source=source, profile=False)
        assert bare.profile is None and bare.C is None and np.array_equal(bare.words, got.words) and bare.vals.tobytes() == got.vals.tobytes()
    assert np.array_equal(s._engine.components_table(), cc.table)       # the components look of the handle: the same
    assert s._engine.transport_ms() >= s._engine.transport_solve_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. the limit
# ---------------------------------------------------------------------------
def test_the_iteration_limit(gpu):
    N = 65
    s, eng = engine_of(N, 'chirp')
    words = np.zeros(_lib.CHS_TRN_WORDS, dtype=np.int64)
    vals = np.ones(_lib.CHS_TRN_VALS)
    cm = np.zeros((N, N))
    pr = np.zeros((N + 1, 3))
    wp, vp, cp, pp = _lib._i64ptr(words), _lib._dptr(vals), _lib._dptr(cm), _lib._dptr(pr)
    other = host.comb(N)
    eng.set_U(mh.field_of(other))
    first = dev_look(eng, T, 'below', 0)                                # a good look of another field
    X = host.serpentine(N)
    L = int(X.sum())
    default = _lib.transport_iters_default(N)
    assert 16 < L <= default
    eng.set_U(mh.field_of(X))
    assert gpu.chs_transport(eng._h, T, 0, 0, 1e-6, 16, wp, vp) == _lib.CHS_ELIMIT            # refused
    msg = gpu.chs_last_error().decode()
    assert 'ITERS = 16' in msg and 'max_iters = 16' in msg
    assert words[W.CHS_TRN_ITERS] == 16 and words[W.CHS_TRN_LIMIT] == 16 and not words[:W.CHS_TRN_ITERS].any()
    assert words[W.CHS_TRN_CHECKS] == 0 and not vals.any()
    assert gpu.chs_transport_map(eng._h, cp) == _lib.CHS_ESTATE                              # no look
    assert gpu.chs_transport_profile(eng._h, pp) == _lib.CHS_ESTATE
    assert gpu.chs_transport_last_ms(eng._h, _lib._dptr(np.zeros(1))) == _lib.CHS_ESTATE
    assert gpu.chs_transport_solve_ms(eng._h, _lib._dptr(np.zeros(1))) == _lib.CHS_ESTATE
    labels, table = components.label(mh.field_of(X), T, 4)                                  # the components look is intact
    tab, lab = np.zeros(table.shape, dtype=np.int32), np.zeros((N, N), dtype=np.int32)
    assert gpu.chs_components_table(eng._h, table.shape[0], _lib._i32ptr(tab)) == _lib.CHS_OK and np.array_equal(tab, table)
    assert gpu.chs_components_labels(eng._h, _lib._i32ptr(lab)) == _lib.CHS_OK and np.array_equal(lab, labels)
    with pytest.raises(_lib.TransportLimitError) as e:
        s.transport(T, max_iters=16)
    assert (e.value.iters, e.value.limit) == (16, 16) and isinstance(e.value, _lib.EngineError)
    got = dev_look(eng, T, 'below', 0)                                  # the default limit: a good look
    check(got, X, 0, "the default limit", closed=1.0 / L)
    assert L - 1 <= got.iters <= default and got.C.tobytes() != first.C.tobytes()
    for bad in (16 * default + 1, -1, -(1 << 62)):                      # out of range: the previous look stays
        assert gpu.chs_transport(eng._h, T, 0, 0, 1e-6, bad, wp, vp) == _lib.CHS_EINVAL, bad
        assert 'max_iters' in gpu.chs_last_error().decode()
        assert gpu.chs_transport_map(eng._h, cp) == _lib.CHS_OK and cm.tobytes() == got.C.tobytes()
    for bad in (0.0, 1e-13, 0.02, float('nan'), -1e-6, float('inf')):
        assert gpu.chs_transport(eng._h, T, 0, 0, bad, 0, wp, vp) == _lib.CHS_EINVAL, bad
        assert 'tol' in gpu.chs_last_error().decode()
        assert gpu.chs_transport_map(eng._h, cp) == _lib.CHS_OK and cm.tobytes() == got.C.tobytes()
    assert gpu.chs_transport(eng._h, T, 0, 0, 1e-6, 16 * default, wp, vp) == _lib.CHS_OK and words[W.CHS_TRN_LIMIT] == 16 * default
    assert gpu.chs_transport(eng._h, T, 0, 0, 1e-6, 0, wp, vp) == _lib.CHS_OK and words[W.CHS_TRN_LIMIT] == default    # 0: the default
    assert np.array_equal(words, got.words) and vals.tobytes() == got.vals.tobytes()
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 5. a look between calls does not change the run; batches; a re-armed engine
# ---------------------------------------------------------------------------
OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with transport looks between them -- a refused one among them -- against the same calls with get_U() between
    them: all nine record columns, the state and the final field, bit for bit.  The threshold is the field's 0.75
    quantile: three quarters of a young field span."""
    assert {c[1] for c in OBSERVE_CASES} == {'fast', 'chirp'}
    refused, solved = [], []

    def look(s):
        t = float(np.quantile(s._engine.get_U(), 0.75))
        try:
            s.transport(t, max_iters=1)
        except _lib.TransportLimitError as e:
            refused.append((e.iters, e.limit))
        solved.append(s.transport(t, map=True).iters)
        s.transport(side='above', source='right')
    got, Ug = tgs._observed_run(N, engine, calls, look, seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    assert refused and set(refused) == {(1, 1)} and max(solved) > 1
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert np.array_equal(Ug, Ur)


def test_batch_equals_the_single_solvers(gpu):
    N, B = 128, 3
    ps = tgs._members(N, B, 100)
    bs = BatchSolver(ps)
    bs.prepare()
    bs.solve_or_resume(20)
    fields = [s._engine.get_U() for s in bs.solvers]
    ts = [float(np.quantile(U, 0.7 + 0.02 * m)) for m, U in enumerate(fields)]
    looks = bs.transport(threshold=ts, source='left', map=True)        # every member at its own threshold
    assert len(looks) == B and [g.threshold for g in looks] == ts
    assert bs._batch.transport_map().tobytes() == looks[B - 1].C.tobytes()   # the one buffer set: the last member's snapshot
    assert bs._batch.transport_profile().tobytes() == looks[B - 1].profile.tobytes()
    for m in range(B):
        X = components.foreground(fields[m], ts[m], 'below')
        check(looks[m], X, 2, f"member {m}")
        one = bs.transport(m, threshold=ts, source='left', map=True)
        assert same_bits(one, looks[m])
        assert looks[m].percolates and 0 < looks[m].fg < N * N
    assert not np.array_equal(looks[0].words, looks[1].words)
    assert bs._batch.transport_ms() >= bs._batch.transport_solve_ms() >= 0.0
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                                         # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        one = s.transport(ts[m], source='left', map=True)
        assert same_bits(one, looks[m]), m
        s.close(fetch_U=False)
    ref = BatchSolver(ps)                                              # the members' next call without the looks
    ref.prepare()
    ref.solve_or_resume(20)
    ref.solve_or_resume(5)
    plain = tgs._batch_snap(ref)
    ref.close(fetch_U=False)
    for m in range(B):
        assert np.array_equal(looked[m][0], plain[m][0]) and np.array_equal(looked[m][1], plain[m][1]), m
        assert looked[m][2] == plain[m][2], m


def test_a_run_on_a_rearmed_engine_equals_a_fresh_one(gpu):
    """An engine that solved a transport problem, was parked and is taken again: no transport result, and its run is the
    run of an engine created with the pool empty, bit for bit."""
    N = 128

    def run(s):
        s.prepare()
        s.solve_or_resume(12)
        st = s._engine.get_state()
        return s.solution.timedata.data().copy(), s._engine.get_U(), (st.delt, st.time_delta_sum, st.computed_steps, st.stop_reason)

    _lib.pool_clear()
    s = tgs.solver(N, 1000, 'fast')
    want = run(s)
    s.close(fetch_U=False)
    _lib.pool_clear()
    s = tgs.solver(N, 1000, 'fast', seed=77)
    s.prepare()
    s.solve_or_resume(5)
    assert s.transport(float(np.quantile(s._engine.get_U(), 0.75)), map=True).iters > 1
    s._engine.close()                                                   # parked
    assert _lib.pool_count() == 1
    s2 = tgs.solver(N, 1000, 'fast')
    eng = s2._get_engine()
    assert _lib.pool_count() == 0                                       # ... and taken
    ms = np.zeros(1)
    assert gpu.chs_transport_map(eng._h, _lib._dptr(np.zeros((N, N)))) == _lib.CHS_ESTATE
    assert gpu.chs_transport_profile(eng._h, _lib._dptr(np.zeros((N + 1, 3)))) == _lib.CHS_ESTATE
    assert gpu.chs_transport_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    assert gpu.chs_transport_solve_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    got = run(s2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    X = components.foreground(got[1], s2.params.threshold, 'below')
    check(s2.transport(map=True), X, 0, 're-armed')
    s2.close(fetch_U=False)
    _lib.pool_clear()


# ---------------------------------------------------------------------------
# 6. arguments and states
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    words = np.zeros(_lib.CHS_TRN_WORDS, dtype=np.int64)
    vals = np.zeros(_lib.CHS_TRN_VALS + 1)
    pr = np.zeros((N + 2, 3))
    cm = np.zeros((N, N))
    ms = np.zeros(1)
    w, v, pp, d = _lib._i64ptr(words), _lib._dptr(vals), _lib._dptr(pr), _lib._dptr(cm)
    fetches = (lambda: gpu.chs_transport_profile(eng._h, pp), lambda: gpu.chs_transport_map(eng._h, d),
               lambda: gpu.chs_transport_last_ms(eng._h, _lib._dptr(ms)), lambda: gpu.chs_transport_solve_ms(eng._h, _lib._dptr(ms)))
    assert gpu.chs_transport(eng._h, 0.5, 0, 0, 1e-6, 0, w, v) == _lib.CHS_ESTATE            # no field yet
    assert gpu.chs_transport(eng._h, 0.5, 0, 4, 1e-6, 0, w, v) == _lib.CHS_EINVAL            # ... but the arguments first
    for call in fetches:
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.transport()
    s.prepare()
    # a doubly-wrong call gives the error of the first in the order: null, threshold, side, source, tol, max_iters
    order = [('null', dict(w=None)), ('null', dict(v=None)), ('finite', dict(t=float('nan'))), ('side', dict(side=2)), ('source', dict(source=4)),
             ('tol', dict(tol=0.5)), ('max_iters', dict(limit=-1))]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw = dict(w=w, v=v, t=0.5, side=0, source=0, tol=1e-6, limit=0)
            kw.update(order[a][1])
            kw.update(order[b][1])
            assert gpu.chs_transport(eng._h, kw['t'], kw['side'], kw['source'], kw['tol'], kw['limit'], kw['w'], kw['v']) == _lib.CHS_EINVAL
            assert order[a][0] in gpu.chs_last_error().decode(), (order[a][0], order[b][0])
    assert gpu.chs_transport(eng._h, 0.5, 0, 0, 1e-6, 0, w, None) == _lib.CHS_EINVAL and 'null' in gpu.chs_last_error().decode()
    for bad in (float('inf'), -float('inf')):
        assert gpu.chs_transport(eng._h, bad, 0, 0, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    for side in (2, -1):
        assert gpu.chs_transport(eng._h, 0.5, side, 0, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    for source in (4, -1):
        assert gpu.chs_transport(eng._h, 0.5, 0, source, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_transport(None, 0.5, 0, 0, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_transport_profile(None, pp) == _lib.CHS_EINVAL and gpu.chs_transport_map(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_transport_last_ms(eng._h, None) == _lib.CHS_EINVAL and gpu.chs_transport_solve_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    for call in fetches:
        assert call() == _lib.CHS_ESTATE                                                    # none of them was a look
    t = float(np.quantile(eng.get_U(), 0.75))
    cc = s.components(t, connectivity=4)
    vals[_lib.CHS_TRN_VALS] = -7.0
    pr[N + 1] = -7.0
    assert gpu.chs_transport(eng._h, t, 0, 0, 1e-6, 0, w, v) == _lib.CHS_OK
    assert words[W.CHS_TRN_FG] == cc.area and words[W.CHS_TRN_CC_COUNT] == cc.count and words[W.CHS_TRN_ACTIVE] > 0
    assert gpu.chs_transport_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    was = ms[0]
    assert gpu.chs_transport_map(eng._h, d) == _lib.CHS_OK and gpu.chs_transport_profile(eng._h, pp) == _lib.CHS_OK
    assert vals[_lib.CHS_TRN_VALS] == -7.0 and np.all(pr[N + 1] == -7.0)                     # nothing beyond the arrays
    assert pr[0, 0] == vals[W.CHS_TRN_F_IN] and pr[N, 0] == vals[W.CHS_TRN_F_OUT] and int(pr[:N, 2].sum()) == words[W.CHS_TRN_ACTIVE]
    assert int((cm >= 0).sum()) == words[W.CHS_TRN_ACTIVE] and int((cm != -1.0).sum()) == words[W.CHS_TRN_FG]
    kept = cm.copy()
    for args in ((float('nan'), 0, 0, 1e-6, 0), (t, 3, 0, 1e-6, 0), (t, 0, 7, 1e-6, 0), (t, 0, 0, 1.0, 0), (t, 0, 0, 1e-6, -5)):
        assert gpu.chs_transport(eng._h, *args, w, v) == _lib.CHS_EINVAL                     # rejected: the last look stays,
        assert gpu.chs_transport_map(eng._h, d) == _lib.CHS_OK and cm.tobytes() == kept.tobytes()   # snapshot and time
        assert gpu.chs_transport_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] == was
        assert np.array_equal(eng.components_table(), cc.table)                      # ... and the components look too
    assert gpu.chs_transport_profile(eng._h, None) == _lib.CHS_EINVAL and gpu.chs_transport_map(eng._h, None) == _lib.CHS_EINVAL
    with pytest.raises(ValueError):
        s.transport(source='middle')
    with pytest.raises(ValueError):
        s.transport(side='beside')
    with pytest.raises(_lib.EngineError):
        s.transport(float('nan'))
    with pytest.raises(_lib.EngineError):
        s.transport(tol=0.5)
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_transport(b._h, 0, 0.5, 0, 0, 1e-6, 0, w, v) == _lib.CHS_ESTATE      # no fields yet
    assert gpu.chs_batch_transport_map(b._h, d) == _lib.CHS_ESTATE and gpu.chs_batch_transport_profile(b._h, pp) == _lib.CHS_ESTATE
    assert gpu.chs_batch_transport_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    assert gpu.chs_batch_transport_solve_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, 65536):
        assert gpu.chs_batch_transport(b._h, member, 0.5, 0, 0, 1e-6, 0, w, v) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_transport(b._h, 1, float('nan'), 0, 0, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport(b._h, 1, 0.5, 0, 5, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport(b._h, 1, 0.5, 0, 0, 0.0, 0, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport(b._h, 1, 0.5, 0, 0, 1e-6, -1, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport(b._h, 1, 0.5, 0, 0, 1e-6, 0, None, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport(None, 1, 0.5, 0, 0, 1e-6, 0, w, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport_map(None, d) == _lib.CHS_EINVAL and gpu.chs_batch_transport_profile(None, pp) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport_last_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_transport_map(b._h, d) == _lib.CHS_ESTATE                            # none of them was a look
    U1 = bs.solvers[1]._engine.get_U()
    assert gpu.chs_batch_transport(b._h, 1, 0.5, 1, 3, 1e-6, 0, w, v) == _lib.CHS_OK
    assert gpu.chs_batch_transport_map(b._h, d) == _lib.CHS_OK and gpu.chs_batch_transport_profile(b._h, pp) == _lib.CHS_OK
    assert words[W.CHS_TRN_FG] == int((~(U1 < 0.5)).sum()) == int((cm != -1.0).sum())
    bs.close(fetch_U=False)
