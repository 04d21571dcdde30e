"""GPU tests (``-m gpu``) of the two-point correlation of the thresholded field on the device (chs_two_point /
chs_batch_two_point, chsimpy_amd/csrc/chs_two_point.hip).

The definition (include/chs_hip.h: chs_two_point): phase 0 is ``(double)U < t`` (a NaN pixel and a pixel equal to t are
not phase 0), phase 1 its complement inside the grid; ``c[p][dy][dx + rmax]`` counts the positions (i, j) for which (i, j)
and (i + dy, j + dx) are both inside the grid and both of phase p, for ``0 <= dy <= rmax, |dx| <= rmax``, without
wrap-around; ``pairs(dy, dx) = (N - dy)(N - |dx|)``.

Reference: the numpy model ``two_point.pair_counts`` (tests/test_two_point_host.py holds it against the definition
written out and against closed forms) on the field as downloaded with ``get_U`` -- the exact values the device holds,
also for fp32.  Everything is integer: every comparison is for equality of the 8 words and of the whole count table.

``W, H, LANES`` are the pixels of a row in one word, the rows of a band of the pair kernel and the lanes of its workgroup
(``_lib.two_point_tile()``), ``CHUNK`` the pixels of a row that one workgroup owns."""
import types

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, chords, two_point as tp
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import log_line, make
import test_gpu_spectrum as tgs
import test_gpu_looks_large as large
import test_two_point_host as host

pytestmark = pytest.mark.gpu
big = large.big                       # the streamed handles of tests/test_gpu_looks_large.py, one per size for this module

T, FG, BG = host.T, host.FG, host.BG
W, H, LANES = 32, 64, 256             # (the library's own is checked against it below)
CHUNK = _lib.CHS_TP_CHUNK
SIZES = [(8, 1), (8, 7), (31, 30), (32, 31), (33, 32), (63, 62), (64, 63), (65, 64), (129, 65), (130, 33), (257, 256),
         (H + 1, min(H + 1, tp.max_r(H + 1))), (2 * H - 1, min(H + 1, tp.max_r(2 * H - 1)))]


def engine_of(N, engine='chirp', dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, rmax):
    words, c = eng.two_point_look(t, rmax, True)
    return tp.TwoPoint(words, eng.N, t, rmax, counts=c)


def check(two, want, what):
    """The look `two` holds exactly the table `want` and its summary."""
    assert two.counts.dtype == np.int64 and two.counts.shape == want.shape, what
    assert np.array_equal(two.counts, want), (what, np.argwhere(two.counts != want)[:8])
    assert np.array_equal(two.words, tp.summary_of(want)), (what, two.words, tp.summary_of(want))


def test_the_tile_is_the_sources(gpu):
    assert _lib.two_point_tile() == (W, H, LANES) == _lib.Engine.two_point_tile()
    assert CHUNK == 2048 and (H + 1, H) in SIZES and (2 * H - 1, H + 1) in SIZES   # (dy crosses a band: rmax >= H)


# ---------------------------------------------------------------------------
# 1. sizes: random fields, both element types
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ['float64', 'float32'])
@pytest.mark.parametrize("N,rmax", SIZES, ids=[f"N{n}-r{r}" for n, r in SIZES])
def test_sizes(gpu, N, rmax, dtype):
    s, eng = engine_of(N, 'chirp', dtype)
    for fraction in (0.1, 0.5):
        U = host.random_field(N, fraction, 7 * N + rmax)
        eng.set_U(U)
        Ud = eng.get_U()
        assert np.array_equal(Ud == T, U == T) and np.array_equal(np.isnan(Ud), np.isnan(U))
        two = dev_look(eng, T, rmax)
        check(two, tp.pair_counts(Ud, T, rmax), f"N={N} rmax={rmax} {dtype} {fraction}")
        assert 0 < two.n('below') < N * N
    assert eng.two_point_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. patterns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,rmax", [(8, 7), (33, 32), (65, 64), (130, 65)])
def test_closed_forms_on_the_device(gpu, N, rmax):
    s, eng = engine_of(N)
    names = []
    for name, U, want in host.closed_forms(N, rmax):
        eng.set_U(U)
        check(dev_look(eng, T, rmax), want, f"{name} N={N}")
        names.append(name)
    assert {'all-phase-0', 'all-phase-1', 'checkerboard', 'stripes-2', 'stripes-6', 'single-pixel-0-0'} <= set(names)
    s.close(fetch_U=False)


def _pixels(N, at):
    U = np.full((N, N), BG)
    for i, j in at:
        U[i, j] = FG
    return U


@pytest.mark.parametrize("N", [33, 65, 130])
def test_pixels_at_the_word_borders_and_the_last_band(gpu, N):
    """Two phase-0 pixels straddling columns 31|32 and 63|64; a pixel in column N - 1 (the zeroed bits behind it); a row
    of phase 0 at i = N - 1 (the last, partial band).  Phase 0 in closed form, both phases against the model."""
    rmax = tp.max_r(N) if N < 100 else 70
    s, eng = engine_of(N)
    cases = [('31|32', [(3, 31), (3, 32)]), ('last column', [(N // 2, N - 1)]), ('last column and first', [(5, N - 1), (6, 0)])]
    if N > 64:
        cases.append(('63|64', [(N - 2, 63), (N - 1, 64)]))
    for name, at in cases:
        U = _pixels(N, at)
        eng.set_U(U)
        two = dev_look(eng, T, rmax)
        want0 = np.zeros((rmax + 1, 2 * rmax + 1), dtype=np.int64)
        want0[0, rmax] = len(at)
        for (i, j) in at:
            for (k, l) in at:
                dy, dx = k - i, l - j
                if (dy, dx) != (0, 0) and 0 <= dy <= rmax and abs(dx) <= rmax:
                    want0[dy, dx + rmax] += 1
        assert np.array_equal(two.counts[0], want0), (name, N, np.argwhere(two.counts[0] != want0)[:5])
        check(two, tp.pair_counts(U, T, rmax), f"{name} N={N}")
    U = np.full((N, N), BG)
    U[N - 1, :] = FG
    eng.set_U(U)
    two = dev_look(eng, T, rmax)
    want0 = np.zeros((rmax + 1, 2 * rmax + 1), dtype=np.int64)
    want0[0] = N - np.abs(np.arange(-rmax, rmax + 1))
    assert np.array_equal(two.counts[0], want0)
    check(two, tp.pair_counts(U, T, rmax), f"last row N={N}")
    s.close(fetch_U=False)


@pytest.mark.parametrize("N,dtype", [(CHUNK + 1, 'float32'), (CHUNK + 34, 'float64')])
def test_across_the_chunk_border(gpu, N, dtype):
    """N = CHUNK + 1 and CHUNK + 34: a second workgroup per band owns one pixel, or a word and two bits; partners up to
    rmax = 40 lie across the border between them on either side."""
    rmax = 40
    s, eng = engine_of(N, 'chirp', dtype)
    U = host.random_field(N, 0.5, N)
    U[:, CHUNK - 2:CHUNK + 2] = FG                       # both sides of the border hold phase 0 ...
    U[::3, CHUNK] = BG                                   # ... with gaps
    eng.set_U(U)
    Ud = eng.get_U()
    check(dev_look(eng, T, rmax), tp.pair_counts(Ud, T, rmax), f"N={N} {dtype}")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the other looks of the same handle
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def evolved(gpu):
    """N = 1024 fp64 after 300 steps of the default parameters."""
    N, steps = 1024, 300
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    yield types.SimpleNamespace(s=s, N=N, U=U, t=t, want=tp.pair_counts(U, t, 64))
    s.close(fetch_U=False)


def test_an_evolved_field(evolved):
    s, N, t = evolved.s, evolved.N, evolved.t
    two = s.two_point(t)
    check(two, evolved.want, f"evolved N={N}")
    assert two.rmax == 64 and two.N == N and two.threshold == t and two.delx == s.solution.delx
    assert 0 < two.n('below') < N * N
    z = two.first_zero('below')
    log_line(f"two-point: evolved N={N} after 300 steps: first zero of the autocovariance {z}, look "
             f"{s._engine.two_point_ms():.3f} ms")
    bare = s.two_point(t, counts=False)
    assert bare.counts is None and np.array_equal(bare.words, two.words)
    own = s.two_point(rmax=3)                            # params.threshold
    assert own.threshold == s.params.threshold and own.rmax == 3 and own.n('below') == s.morphology().n_A
    with pytest.raises(ValueError):
        s.two_point(t, rmax=257)


def test_identities_with_the_other_looks(evolved):
    s, N, t = evolved.s, evolved.N, evolved.t
    two = s.two_point(t)
    co = s.chords(t)
    mo = s.morphology(t)
    assert two.n('below') == mo.n_A == co.n('below') and two.n('above') == co.n('above')
    rmax = two.rmax
    for p, phase in enumerate(chords.PHASES):
        # neighbours within a line = pixels - chords of the phase along that line
        for d, name in (('rows', 'adj_rows_'), ('cols', 'adj_cols_')):
            assert two.word(name + phase) == two.n(phase) - (co.count(phase, d) + co.cut(phase, d)), (phase, d)
        # the lineal path needs every pixel between the two ends: its integer numerator at r is at most c at distance r - 1
        for d in ('rows', 'cols'):
            n = co.hist[p, chords.direction_code(d)].sum(axis=0)            # n(c): the chords of length c, both classes
            line = two.counts[p, 0, rmax:] if d == 'rows' else two.counts[p, :, rmax]
            for r in range(1, rmax + 2):
                num = sum(int(n[c]) * (c - r + 1) for c in range(r, N + 1) if n[c])   # the segments of r pixels that fit
                assert num / (N * (N - r + 1)) == co.lineal_path(phase, d)[r - 1]
                assert num <= int(line[r - 1]), (phase, d, r)
                if r <= 2:
                    assert num == int(line[r - 1]), (phase, d, r)


# ---------------------------------------------------------------------------
# 4. look behaviour
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_two_looks_give_the_same_bits_and_another_rmax_resizes(gpu, N, engine):
    s = tgs.solver(N, 8, engine)
    s.prepare()
    s.solve_or_resume(4)
    U = s._engine.get_U()
    t = float(np.median(U))
    a, b = s.two_point(t, rmax=40), s.two_point(t, rmax=40)
    assert np.array_equal(a.words, b.words) and np.array_equal(a.counts, b.counts)
    for rmax in (7, 99, 40):                             # smaller, larger, back
        two = s.two_point(t, rmax=rmax)
        check(two, tp.pair_counts(U, t, rmax), f"N={N} rmax={rmax}")
        assert s._engine.two_point_counts().shape == (2, rmax + 1, 2 * rmax + 1)
    assert np.array_equal(two.counts, a.counts)
    s.close(fetch_U=False)


def test_errors_and_a_rejected_call_leaves_the_last_look(gpu):
    N = 65
    s = tgs.solver(N, 4, 'chirp')
    eng = s._get_engine()
    out = np.zeros(_lib.CHS_TP_WORDS, dtype=np.int64)
    n = _lib.two_point_size(N, 10)
    buf = np.zeros(n + 1, dtype=np.int64)
    ms = np.zeros(1)
    o, c = _lib._i64ptr(out), _lib._i64ptr(buf)
    assert gpu.chs_two_point(eng._h, 0.5, 10, o) == _lib.CHS_ESTATE                          # no field yet
    assert gpu.chs_two_point_counts(eng._h, n, c) == _lib.CHS_ESTATE                         # no look yet
    assert gpu.chs_two_point_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    with pytest.raises(AssertionError):
        s.two_point()
    s.prepare()
    eng.set_U(host.random_field(N, 0.5, 9))
    Ud = eng.get_U()
    assert gpu.chs_two_point(eng._h, 0.5, 0, o) == _lib.CHS_EINVAL and 'rmax' in gpu.chs_last_error().decode()
    assert gpu.chs_two_point_counts(eng._h, n, c) == _lib.CHS_ESTATE                         # none of them was a look
    assert gpu.chs_two_point(eng._h, T, 10, o) == _lib.CHS_OK
    want = tp.pair_counts(Ud, T, 10)
    assert np.array_equal(out, tp.summary_of(want))
    assert gpu.chs_two_point_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    t0 = ms[0]
    for rmax in (0, -1, tp.max_r(N) + 1, 257):                                               # rejected: rmax ...
        assert gpu.chs_two_point(eng._h, T, rmax, o) == _lib.CHS_EINVAL
        assert 'rmax' in gpu.chs_last_error().decode()
    for bad in (float('nan'), float('inf'), -float('inf')):                                  # ... the threshold ...
        assert gpu.chs_two_point(eng._h, bad, 10, o) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_two_point(eng._h, float('nan'), 0, o) == _lib.CHS_EINVAL                  # doubly wrong: the threshold first
    assert 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_two_point(eng._h, T, 10, None) == _lib.CHS_EINVAL                         # ... a null argument
    for wrong in (n - 1, n + 1, 0, -1, _lib.two_point_size(N, 11)):
        assert gpu.chs_two_point_counts(eng._h, wrong, c) == _lib.CHS_EINVAL
        assert f"expected {n}" in gpu.chs_last_error().decode()
    assert gpu.chs_two_point_counts(eng._h, n, None) == _lib.CHS_EINVAL
    buf[n] = -7                                                                              # the last look and its time are in place
    assert gpu.chs_two_point_counts(eng._h, n, c) == _lib.CHS_OK and buf[n] == -7
    assert np.array_equal(buf[:n].reshape(want.shape), want)
    assert gpu.chs_two_point_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] == t0
    assert gpu.chs_two_point_last_ms(eng._h, None) == _lib.CHS_EINVAL
    with pytest.raises(_lib.EngineError):
        s.two_point(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    n = _lib.two_point_size(128, 5)
    buf = np.zeros(n, dtype=np.int64)
    c = _lib._i64ptr(buf)
    assert gpu.chs_batch_two_point(b._h, 0, 0.5, 5, o) == _lib.CHS_ESTATE                    # no fields yet
    assert gpu.chs_batch_two_point_counts(b._h, n, c) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, 65536):
        assert gpu.chs_batch_two_point(b._h, member, 0.5, 5, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_two_point(b._h, 1, 0.5, 128, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_two_point_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    U1 = b.get_U(1)
    t = float(np.median(U1))
    assert gpu.chs_batch_two_point(b._h, 1, t, 5, o) == _lib.CHS_OK
    assert gpu.chs_batch_two_point_counts(b._h, n + 1, c) == _lib.CHS_EINVAL
    assert f"expected {n}" in gpu.chs_last_error().decode()
    assert gpu.chs_batch_two_point_counts(b._h, n, c) == _lib.CHS_OK
    assert np.array_equal(buf.reshape(2, 6, 11), tp.pair_counts(U1, t, 5))
    assert gpu.chs_batch_two_point_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    bs.close(fetch_U=False)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with two_point() between them against the same calls with get_U() between them: all nine record columns, the
    state and the final field, bit for bit."""
    assert {(c[0], c[1]) for c in OBSERVE_CASES} == {(128, 'fast'), (100, 'chirp')}

    def look(s):
        s.two_point()
        s.two_point(rmax=5, counts=False)
    got, Ug = tgs._observed_run(N, engine, calls, look, seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert np.array_equal(Ug, Ur)


# ---------------------------------------------------------------------------
# 5. batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (136, 'chirp')])
def test_batch_equals_a_single_handle_holding_the_same_field(gpu, N, engine):
    B, rmax = 3, 33
    ps = tgs._members(N, B, 100)
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(10)
    fields = [s._engine.get_U() for s in bs.solvers]
    ts = [float(np.median(U)) for U in fields]
    twos = bs.two_point(threshold=ts, rmax=rmax)
    assert len(twos) == B and [two.threshold for two in twos] == ts
    single, eng = engine_of(N, 'chirp' if engine == 'chirp' else 'fast')
    for m in range(B):
        check(twos[m], tp.pair_counts(fields[m], ts[m], rmax), f"member {m}")
        eng.set_U(fields[m])
        assert np.array_equal(eng.get_U(), fields[m])
        one = dev_look(eng, ts[m], rmax)
        assert np.array_equal(one.words, twos[m].words) and np.array_equal(one.counts, twos[m].counts), m
        again = bs.two_point(m, threshold=ts, rmax=rmax)
        assert np.array_equal(again.counts, twos[m].counts), m
        assert bs._batch.two_point_ms() >= 0.0
    assert not np.array_equal(twos[0].counts, twos[1].counts)
    assert bs.two_point(0, counts=False).rmax == 64 and bs.two_point(0, counts=False).counts is None
    single.close(fetch_U=False)
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 6. the streamed loads
# ---------------------------------------------------------------------------
def test_the_streamed_sizes_lie_above_the_cache_bound():
    bound = large.cache_bound_from_source()
    for N, dtype, _ in large.STREAMED:
        assert 2 * N * N * large.ESZ[dtype] > bound, (N, dtype)
    assert [c[:2] for c in large.STREAMED] == [(4097, 'float64'), (4098, 'float64'), (5793, 'float32'), (5796, 'float32')]


def test_streamed_two_point(big):
    """k_tp_mask<T, true>: rmax = 2 against the definition written out with slices on the downloaded field."""
    two = dev_look(big.eng, T, 2)
    check(two, tp.pair_counts_slices(big.Ud, T, 2), big.what)
    assert two.n('below') == int(big.below.sum())
    log_line(f"two-point, large: {big.what}: rmax 2 {big.eng.two_point_ms():.3f} ms")

