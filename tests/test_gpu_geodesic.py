"""GPU tests (``-m gpu``) of the geodesic look on the device (chs_geodesic / chs_batch_geodesic,
chsimpy_amd/csrc/chs_geodesic.hip).

The definition (include/chs_hip.h: chs_geodesic).  Foreground, ``side`` and ``connectivity`` are those of chs_components,
with no wrap-around.  ``source`` is one of four walls: 0 is row 0, 1 is row N-1, 2 is column 0, 3 is column N-1; the target
is the opposite wall; the depth k of a pixel is its distance from the source wall along that axis.  A path moves from a
foreground pixel to a foreground neighbour: at connectivity 4 an axial step costs 1 (UNIT = 1), at connectivity 8 an axial
step costs 3 and a diagonal step 4 (UNIT = 3), a diagonal step needing only its two end pixels to be foreground.  G[p] is
-1 for background, 0 for a foreground pixel on the source wall, otherwise the smallest cost of a path from any such pixel
to p, CHS_GEO_INF for a foreground pixel that no path reaches.  Bin d of the histogram (4N bins) counts the reached pixels
with G // UNIT == d, the last bin everything beyond; the profile holds, per depth, the foreground pixels, the reached
pixels and the sum of G over them.

Reference: the numpy model of chsimpy_amd/geodesic.py applied to the mask of the field as downloaded with ``get_U`` --
the exact values the device holds, also for fp32 -- which tests/test_geodesic_host.py holds to a heap Dijkstra and to
scipy.  Everything is integer: map, histogram, profile and the 15 unique words are compared for equality.  ROUNDS is
checked as 1 <= ROUNDS <= rounds_bound (the synchronous tile model), and as 0 when SOURCES == 0.

The pattern sizes: N = 8 (one tile), 65 (2 x 2 tiles, the second a single pixel wide) and 130 (3 x 3 tiles: a tile with
eight neighbours)."""
import functools

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, geodesic
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_geodesic_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
SIDES, CONNS, SOURCES = host.SIDES, host.CONNS, host.SOURCES
W = geodesic


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, conn, side, source, max_rounds=None):
    words, hi, pr, g = eng.geodesic_look(t, conn, components.side_code(side), source, True, True, True, max_rounds)
    return geodesic.Geodesic(words, eng.N, t, conn, side, source, hist=hi, profile=pr, g=g)


_KEEP = {}


@functools.lru_cache(maxsize=None)
def _reference(key, conn, source):
    """(G, words, hist, profile, rounds_bound) of a mask, once per mask and arguments."""
    X = _KEEP[key]
    N = X.shape[0]
    G = geodesic.relax(X, conn, source)
    labels, table = components.label(mh.field_of(X), T, conn)
    holds = np.unique(labels[X & (geodesic.depth_of(N, source) == 0)]).size
    words, hist, profile = geodesic.stats_of(G, conn, source, cc_count=table.shape[0], cc_reached=holds)
    return G, words, hist, profile, geodesic.rounds_bound(X, conn, source)


def check(got, X, conn, source, what, limit=None):
    """A device look against the model of the mask X."""
    key = (X.shape[0], X.tobytes())
    _KEEP[key] = X
    G, words, hist, profile, bound = _reference(key, conn, source)
    assert np.array_equal(got.G, G), what
    assert got.limit == (geodesic.rounds_default(X.shape[0]) if limit is None else limit), what
    assert np.array_equal(got.words[W.UNIQUE[:-1]], words[W.UNIQUE[:-1]]), (what, got.words, words)
    assert np.array_equal(got.hist, hist), what
    assert np.array_equal(got.profile, profile), what
    if got.sources == 0:
        assert got.rounds == 0, what
    else:
        assert 1 <= got.rounds <= bound <= got.limit, (what, got.rounds, bound)
    return bound


# ---------------------------------------------------------------------------
# 1. patterns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sources", [(0, 1), (2, 3)], ids=['rows', 'columns'])
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("N", [8, 65, 130])
def test_patterns_on_the_device(gpu, N, conn, sources):
    s, eng = engine_of(N, 'chirp')
    names = [name for name, _ in host.patterns(N)]
    assert {'full', 'empty', 'no sources', 'serpentine', 'spiral', 'comb', 'islands'} <= set(names)
    assert ('staircase' in names) == ('staircase back' in names) == (N == 130)
    most = 0
    for name, X in host.patterns(N):
        for side in SIDES:
            eng.set_U(mh.field_of(X if side == 'below' else ~X))       # the same foreground on either side
            assert np.array_equal(components.foreground(eng.get_U(), T, side), X)
            for source in sources:
                got = dev_look(eng, T, conn, side, source)
                most = max(most, check(got, X, conn, source, f"{name} N={N} conn={conn} {side} source={source}"))
                assert got.side == side and got.fg == int(X.sum())
    assert most > (16 if N == 130 else 1)                               # the serpentines: tiles re-activated many times
    for name, U, t, _ in mh.hand_made(N):                               # the threshold, NaN and one-ulp fields, on both sides
        eng.set_U(U)
        Ud = eng.get_U()
        for side in SIDES:
            X = components.foreground(Ud, t, side)
            for source in sources[::-1][:1] + sources[:1]:
                check(dev_look(eng, t, conn, side, source), X, conn, source, f"{name} N={N} conn={conn} {side} source={source}")
    s.close(fetch_U=False)


def test_the_corner_hand_over(gpu):
    """The staircases at N = 130: the corridor crosses from tile (0, 0) to tile (1, 1) by the diagonal step
    (63,63)-(64,64) alone -- and, back, from tile (0, 1) to tile (1, 0) by (63,64)-(64,63) -- so the pixels behind are
    reached only if a changed corner pixel wakes the diagonal tile."""
    N = 130
    s, eng = engine_of(N, 'chirp')
    for back in (False, True):
        X = host.staircase(N, back)
        a, b = (64, 63) if back else (63, 64)
        eng.set_U(mh.field_of(X))
        got = dev_look(eng, T, 8, 'below', 0)
        check(got, X, 8, 0, f"staircase back={back}")
        assert got.G[63, a] == 3 * 63 and got.G[64, b] == 3 * 63 + 4 and got.G[N - 1, b] == 3 * (N - 2) + 4
        assert got.percolates and got.reached == got.fg == N and got.gmin_target_pos == b and got.rounds >= 2
        four = dev_look(eng, T, 4, 'below', 0)
        check(four, X, 4, 0, f"staircase back={back} at connectivity 4")
        assert four.reached == 64 and not four.percolates and four.isolated == N - 64
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random masks: engines and element types
# ---------------------------------------------------------------------------
RANDOM_CASES = [(100, 'direct', 'float64'), (129, 'direct', 'float32'), (100, 'chirp', 'float32'), (129, 'chirp', 'float64'),
                (128, 'fast', 'float64'), (128, 'fast', 'float32')]     # (the fast engine has no N = 100 or 129)


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_masks(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    for conn in CONNS:
        masks = host.random_masks(N, conn)
        assert {perc for _, _, perc in masks} == {True, False}, (N, conn)    # a percolating and a non-percolating one
        for seed, X, perc in masks:
            U = mh.field_of(X)
            k = max(2, N // 16)
            rng = np.random.default_rng(seed)
            ii, jj = rng.integers(0, N, k), rng.integers(0, N, k)
            U[ii, jj] = np.where(X[ii, jj], np.nextafter(np.float32(T), np.float32(0)), T)   # at the threshold: background
            eng.set_U(U)
            assert np.array_equal(components.foreground(eng.get_U(), T, 'below'), X)
            for source in SOURCES:
                got = dev_look(eng, T, conn, 'below', source)
                check(got, X, conn, source, f"N={N} {engine} {dtype} conn={conn} seed={seed} source={source}")
                if source == 0:
                    assert got.percolates == perc
            eng.set_U(mh.field_of(~X))
            check(dev_look(eng, T, conn, 'above', 1), X, conn, 1, f"N={N} {engine} {dtype} conn={conn} seed={seed} above")
    assert eng.geodesic_ms() >= eng.geodesic_relax_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the components of the same handle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("source", ['top', 'left'])
@pytest.mark.parametrize("conn", CONNS)
def test_an_evolved_field_against_the_model_and_the_components(gpu, conn, source):
    """After 40 steps at N = 512 fp64 on the fast engine, thresholded at the field's median: the device equals the model
    under the default limit; REACHED is the area of the components that touch the source wall; percolation is what their
    bounding boxes say; the tortuosity is at least 1 (0.9428 in the chamfer metric)."""
    N, steps = 512, 40
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    X = components.foreground(U, t, 'below')
    code = geodesic.source_code(source)
    got = s.geodesic(t, connectivity=conn, source=source, map=True)        # max_rounds=None: the default
    G = geodesic.relax(X, conn, code)
    words, hist, profile = geodesic.stats_of(G, conn, code)
    assert np.array_equal(got.G, G)
    assert np.array_equal(got.words[:W.CHS_GEO_UNIT + 1], words[:W.CHS_GEO_UNIT + 1]), (got.words, words)
    assert np.array_equal(got.hist, hist) and np.array_equal(got.profile, profile)
    assert got.limit == geodesic.rounds_default(N) == _lib.geodesic_rounds_default(N)
    assert 1 <= got.rounds <= geodesic.rounds_bound(X, conn, code) <= got.limit
    cc = s.components(t, connectivity=conn, table=True)
    lo, hi = (cc.bbox[:, 0], cc.bbox[:, 1]) if code < 2 else (cc.bbox[:, 2], cc.bbox[:, 3])
    touch = lo == 0
    assert got.cc_count == cc.count and got.cc_reached == int(touch.sum()) and got.fg == cc.area
    assert got.reached == int(cc.areas[touch].sum(dtype=np.int64))
    assert got.percolates == bool((touch & (hi == N - 1)).any())
    if got.percolates:
        assert got.tortuosity >= (1.0 if conn == 4 else geodesic.CHAMFER_BOUNDS[0]) and got.mean_tortuosity >= got.tortuosity
    assert 0 < got.sources < N and 0 < got.accessible_fraction <= 1.0 and got.delx == sol.delx
    cdf = got.depth_cdf()
    assert np.all(np.diff(cdf) >= 0) and cdf[-1] == got.accessible_fraction
    again = s.geodesic(t, connectivity=conn, source=source, map=True)      # two looks: the same bits
    assert np.array_equal(again.G, got.G) and np.array_equal(again.words[W.UNIQUE], got.words[W.UNIQUE])
    assert np.array_equal(again.hist, got.hist) and np.array_equal(again.profile, got.profile)
    bare = s.geodesic(t, connectivity=conn, source=source, hist=False, profile=False)
    assert bare.hist is None and bare.profile is None and bare.G is None and np.array_equal(bare.words[W.UNIQUE], got.words[W.UNIQUE])
    assert s._engine.geodesic_ms() >= s._engine.geodesic_relax_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. the round limit
# ---------------------------------------------------------------------------
def test_the_round_limit(gpu):
    N = 130
    s, eng = engine_of(N, 'chirp')
    nb = _lib.geodesic_bins(N)
    out = np.zeros(_lib.CHS_GEO_WORDS, dtype=np.int64)
    gm = np.zeros((N, N), dtype=np.int32)
    o, gp = _lib._i64ptr(out), _lib._i32ptr(gm)
    other = host.comb(N)
    eng.set_U(mh.field_of(other))
    first = dev_look(eng, T, 4, 'below', 0)                             # a good look of another field
    X = host.serpentine(N)
    eng.set_U(mh.field_of(X))
    bound = geodesic.rounds_bound(X, 4, 0)
    assert 16 < bound <= geodesic.rounds_default(N)
    assert gpu.chs_geodesic(eng._h, T, 4, 0, 0, 16, o) == _lib.CHS_ELIMIT                    # refused
    msg = gpu.chs_last_error().decode()
    assert 'ROUNDS = 16' in msg and 'max_rounds = 16' in msg
    assert out[_lib.CHS_GEO_ROUNDS] == 16 and out[_lib.CHS_GEO_LIMIT] == 16 and not out[:_lib.CHS_GEO_ROUNDS].any()
    assert gpu.chs_geodesic_map(eng._h, gp) == _lib.CHS_ESTATE                              # no look
    assert gpu.chs_geodesic_hist(eng._h, nb, _lib._i64ptr(np.zeros(nb, dtype=np.int64))) == _lib.CHS_ESTATE
    assert gpu.chs_geodesic_profile(eng._h, _lib._i64ptr(np.zeros((N, 3), dtype=np.int64))) == _lib.CHS_ESTATE
    assert gpu.chs_geodesic_last_ms(eng._h, _lib._dptr(np.zeros(1))) == _lib.CHS_ESTATE
    labels, table = components.label(mh.field_of(X), T, 4)                                  # the components look is intact
    tab, lab = np.zeros(table.shape, dtype=np.int32), np.zeros((N, N), dtype=np.int32)
    assert gpu.chs_components_table(eng._h, table.shape[0], _lib._i32ptr(tab)) == _lib.CHS_OK and np.array_equal(tab, table)
    assert gpu.chs_components_labels(eng._h, _lib._i32ptr(lab)) == _lib.CHS_OK and np.array_equal(lab, labels)
    with pytest.raises(_lib.GeodesicLimitError) as e:
        s.geodesic(T, connectivity=4, max_rounds=16)
    assert (e.value.rounds, e.value.limit) == (16, 16) and isinstance(e.value, _lib.EngineError)
    got = dev_look(eng, T, 4, 'below', 0, bound)                        # the bound is enough: the next good look works
    check(got, X, 4, 0, "max_rounds = rounds_bound", limit=bound)
    assert not np.array_equal(got.G, first.G)
    default = _lib.geodesic_rounds_default(N)
    for bad in (16 * default + 1, -1, -(1 << 62)):                      # out of range: the previous look stays
        assert gpu.chs_geodesic(eng._h, T, 4, 0, 0, bad, o) == _lib.CHS_EINVAL, bad
        assert 'max_rounds' in gpu.chs_last_error().decode()
        assert gpu.chs_geodesic_map(eng._h, gp) == _lib.CHS_OK and np.array_equal(gm, got.G)
    assert gpu.chs_geodesic(eng._h, T, 4, 0, 0, 16 * default, o) == _lib.CHS_OK and out[_lib.CHS_GEO_LIMIT] == 16 * default
    assert gpu.chs_geodesic(eng._h, T, 4, 0, 0, 0, o) == _lib.CHS_OK and out[_lib.CHS_GEO_LIMIT] == default    # 0: the default
    assert np.array_equal(out[W.UNIQUE[:-1]], got.words[W.UNIQUE[:-1]])
    s.close(fetch_U=False)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with geodesic looks between them -- a refused one among them -- against the same calls with get_U() between
    them: all nine record columns, the state and the final field, bit for bit."""
    assert {c[1] for c in OBSERVE_CASES} == {'fast', 'chirp'}
    refused = []

    def look(s):
        t = float(np.median(s._engine.get_U()))
        try:
            s.geodesic(t, connectivity=4, max_rounds=1)
        except _lib.GeodesicLimitError as e:
            refused.append((e.rounds, e.limit))
        s.geodesic(t, map=True)
        s.geodesic(side='above', source='right')
    got, Ug = tgs._observed_run(N, engine, calls, look, seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    assert refused and set(refused) == {(1, 1)}
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert np.array_equal(Ug, Ur)


# ---------------------------------------------------------------------------
# 5. batches
# ---------------------------------------------------------------------------
def test_batch_equals_the_single_solvers(gpu):
    N, B = 128, 3
    ps = tgs._members(N, B, 100)
    for m, p in enumerate(ps):
        p.threshold = p.XXX + 1e-3 * (m - 1)
    ts = [p.threshold for p in ps]
    bs = BatchSolver(ps)
    bs.prepare()
    bs.solve_or_resume(20)
    looks = bs.geodesic(connectivity=4, source='left', map=True)      # every member at its own threshold
    assert len(looks) == B and [g.threshold for g in looks] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    assert np.array_equal(bs._batch.geodesic_map(), looks[B - 1].G)    # the one buffer set: the last member's snapshot
    assert np.array_equal(bs._batch.geodesic_hist(), looks[B - 1].hist) and np.array_equal(bs._batch.geodesic_profile(), looks[B - 1].profile)
    for m in range(B):
        X = components.foreground(fields[m], ts[m], 'below')
        check(looks[m], X, 4, 2, f"member {m}")
        one = bs.geodesic(m, connectivity=4, source='left', map=True)
        assert np.array_equal(one.G, looks[m].G) and np.array_equal(one.words[W.UNIQUE], looks[m].words[W.UNIQUE])
        assert 0 < looks[m].fg < N * N
    assert not np.array_equal(looks[0].words, looks[1].words)
    assert bs._batch.geodesic_ms() >= 0.0
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                                         # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        one = s.geodesic(connectivity=4, source='left', map=True)
        assert np.array_equal(one.G, looks[m].G) and np.array_equal(one.words[W.UNIQUE], looks[m].words[W.UNIQUE]), m
        assert np.array_equal(one.hist, looks[m].hist) and np.array_equal(one.profile, looks[m].profile), m
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


# ---------------------------------------------------------------------------
# 6. arguments and states
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    nb = _lib.geodesic_bins(N)
    out = np.zeros(_lib.CHS_GEO_WORDS, dtype=np.int64)
    hist = np.zeros(nb + 1, dtype=np.int64)
    prof = np.zeros((N, 3), dtype=np.int64)
    gm = np.zeros((N, N), dtype=np.int32)
    ms = np.zeros(1)
    o, h, pp, d = _lib._i64ptr(out), _lib._i64ptr(hist), _lib._i64ptr(prof), _lib._i32ptr(gm)
    fetches = (lambda: gpu.chs_geodesic_hist(eng._h, nb, h), lambda: gpu.chs_geodesic_profile(eng._h, pp),
               lambda: gpu.chs_geodesic_map(eng._h, d), lambda: gpu.chs_geodesic_last_ms(eng._h, _lib._dptr(ms)),
               lambda: gpu.chs_geodesic_relax_ms(eng._h, _lib._dptr(ms)))
    assert gpu.chs_geodesic(eng._h, 0.5, 8, 0, 0, 0, o) == _lib.CHS_ESTATE                   # no field yet
    assert gpu.chs_geodesic(eng._h, 0.5, 8, 0, 4, 0, o) == _lib.CHS_EINVAL                   # ... but the arguments first
    for call in fetches:
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.geodesic()
    s.prepare()
    # a doubly-wrong call gives the error of the components look's order: null, threshold, connectivity, side -- then
    # source, max_rounds
    order = [('null', dict(out=None)), ('finite', dict(t=float('nan'))), ('connectivity', dict(conn=6)), ('side', dict(side=2)),
             ('source', dict(source=4)), ('max_rounds', dict(limit=-1))]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw = dict(out=o, t=0.5, conn=8, side=0, source=0, limit=0)
            kw.update(order[a][1])
            kw.update(order[b][1])
            assert gpu.chs_geodesic(eng._h, kw['t'], kw['conn'], kw['side'], kw['source'], kw['limit'], kw['out']) == _lib.CHS_EINVAL
            assert order[a][0] in gpu.chs_last_error().decode(), (order[a][0], order[b][0])
    for bad in (float('inf'), -float('inf')):
        assert gpu.chs_geodesic(eng._h, bad, 8, 0, 0, 0, o) == _lib.CHS_EINVAL
    for conn in (0, 6, -4):
        assert gpu.chs_geodesic(eng._h, 0.5, conn, 0, 0, 0, o) == _lib.CHS_EINVAL
    for source in (4, -1):
        assert gpu.chs_geodesic(eng._h, 0.5, 8, 0, source, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_geodesic(None, 0.5, 8, 0, 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_geodesic_hist(None, nb, h) == _lib.CHS_EINVAL and gpu.chs_geodesic_profile(None, pp) == _lib.CHS_EINVAL
    assert gpu.chs_geodesic_map(None, d) == _lib.CHS_EINVAL and gpu.chs_geodesic_last_ms(eng._h, None) == _lib.CHS_EINVAL
    for call in fetches:
        assert call() == _lib.CHS_ESTATE                                                    # none of them was a look
    t = float(np.median(eng.get_U()))
    cc = s.components(t, connectivity=8)
    assert gpu.chs_geodesic(eng._h, t, 8, 0, 0, 0, o) == _lib.CHS_OK
    assert out[0] == cc.area and out[W.CHS_GEO_CC_COUNT] == cc.count
    assert gpu.chs_geodesic_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    was = ms[0]
    assert gpu.chs_geodesic_map(eng._h, d) == _lib.CHS_OK
    kept = gm.copy()
    for args in ((float('nan'), 8, 0, 0, 0), (t, 5, 0, 0, 0), (t, 8, 3, 0, 0), (t, 8, 0, 7, 0), (t, 8, 0, 0, -5)):
        assert gpu.chs_geodesic(eng._h, *args, o) == _lib.CHS_EINVAL                         # rejected: the last look stays,
        assert gpu.chs_geodesic_map(eng._h, d) == _lib.CHS_OK and np.array_equal(gm, kept)   # snapshot and time
        assert gpu.chs_geodesic_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] == was
        assert np.array_equal(eng.components_table(), cc.table)                      # ... and the components look too
    for bins in (nb - 1, nb + 1, 0, -1):
        assert gpu.chs_geodesic_hist(eng._h, bins, h) == _lib.CHS_EINVAL
        assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_geodesic_hist(eng._h, nb, None) == _lib.CHS_EINVAL and gpu.chs_geodesic_profile(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_geodesic_map(eng._h, None) == _lib.CHS_EINVAL
    hist[nb] = -7
    assert gpu.chs_geodesic_hist(eng._h, nb, h) == _lib.CHS_OK and gpu.chs_geodesic_profile(eng._h, pp) == _lib.CHS_OK
    assert hist[nb] == -7 and int(hist[:nb].sum()) == int(out[W.CHS_GEO_REACHED]) == int(prof[:, 1].sum())
    assert int(prof[:, 0].sum()) == int(out[0]) == int((gm >= 0).sum())
    with pytest.raises(ValueError):
        s.geodesic(source='middle')
    with pytest.raises(ValueError):
        s.geodesic(connectivity=6)
    with pytest.raises(_lib.EngineError):
        s.geodesic(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_geodesic(b._h, 0, 0.5, 8, 0, 0, 0, o) == _lib.CHS_ESTATE             # no fields yet
    assert gpu.chs_batch_geodesic_hist(b._h, nb, h) == _lib.CHS_ESTATE and gpu.chs_batch_geodesic_map(b._h, d) == _lib.CHS_ESTATE
    assert gpu.chs_batch_geodesic_profile(b._h, pp) == _lib.CHS_ESTATE
    assert gpu.chs_batch_geodesic_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, 65536):
        assert gpu.chs_batch_geodesic(b._h, member, 0.5, 8, 0, 0, 0, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_geodesic(b._h, 1, float('nan'), 8, 0, 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic(b._h, 1, 0.5, 8, 0, 5, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic(b._h, 1, 0.5, 8, 0, 0, -1, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic(b._h, 1, 0.5, 8, 0, 0, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic(None, 1, 0.5, 8, 0, 0, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic_hist(None, nb, h) == _lib.CHS_EINVAL and gpu.chs_batch_geodesic_map(None, d) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic_last_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_geodesic_hist(b._h, nb, h) == _lib.CHS_ESTATE                       # none of them was a look
    assert gpu.chs_batch_geodesic(b._h, 1, 0.5, 8, 1, 3, 0, o) == _lib.CHS_OK
    assert gpu.chs_batch_geodesic_hist(b._h, nb + 1, h) == _lib.CHS_EINVAL and f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_batch_geodesic_hist(b._h, nb, h) == _lib.CHS_OK and gpu.chs_batch_geodesic_map(b._h, d) == _lib.CHS_OK
    assert out[0] == int((~(bs.solvers[1]._engine.get_U() < 0.5)).sum()) == int((gm >= 0).sum())
    bs.close(fetch_U=False)
