"""GPU tests (``-m gpu``) of the sub-pixel interface look on the device (chs_contour / chs_batch_contour,
chsimpy_amd/csrc/chs_contour.hip).

The definition: include/chs_hip.h, chs_contour (the docstring of chsimpy_amd/contour.py repeats it).

Reference: the numpy model ``contour.contour_model`` (tests/test_contour_host.py holds it against the definition read
out cell by cell and against closed forms) on the field as downloaded with ``get_U`` -- the exact values the device
holds, also for fp32.

* The 16 words and both histograms are integers: equality.
* The map: the per-cell arithmetic is compiled without contraction and the device's fp64 division and square root are
  correctly rounded, so ``ell`` and ``kappa`` of every cell are the model's bit for bit (`check_map`; a NaN is compared as
  a NaN).  That makes r = 0 below.
* The six sums: the terms are the model's, so the only difference is the order of the additions.  The device adds at
  most E terms one after the other and joins the results by trees D deep (``_lib.contour_sum_terms``, DESIGN.md section
  3j), the reference is the ``numpy.longdouble`` sum of the same terms: ``|dev - ref| <= (E - 1 + D + r) 2^-53 sum|term|``,
  r = 0.

``TW x TH`` is the cell tile of a workgroup (``_lib.contour_tile()``)."""
import types

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, contour as ct
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import log_line, make
import test_gpu_spectrum as tgs
import test_gpu_looks_large as large
import test_contour_host as host

pytestmark = pytest.mark.gpu
big = large.big                       # the streamed handles of tests/test_gpu_looks_large.py, one per size for this module

T = host.T
TW, TH = 64, 16                       # (the library's own is checked against it below)
SIZES = sorted({8, 9, 33, 63, 64, 65, 66, 129, 130, TW, TW + 1, 2 * TW - 1, 2 * TW + 1, TH, TH + 1, 2 * TH - 1, 2 * TH + 1})
R_MAP = 0                             # roundings inside a term that the device and the model do not share: the map is bitwise


def engine_of(N, engine='chirp', dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, bins=64, kmax=1.0, map=True):
    words, sums, hist, mp = eng.contour_look(t, bins, kmax, True, map)
    return ct.Contour(words, sums, eng.N, t, bins, kmax, hist=hist, map=mp)


def check_map(c, m, what):
    assert c.ell_map.dtype == np.float64 and c.ell_map.shape == m.ell.shape, what
    bad = np.argwhere(c.ell_map.view(np.int64) != m.ell.view(np.int64))
    assert len(bad) == 0, (what, 'ell', bad[:5])
    assert np.array_equal(np.isnan(c.kappa_map), np.isnan(m.kappa)), (what, 'the curvature cells')
    k = ~np.isnan(m.kappa)
    bad = np.argwhere(k & (np.where(k, c.kappa_map, 0.0).view(np.int64) != np.where(k, m.kappa, 0.0).view(np.int64)))
    assert len(bad) == 0, (what, 'kappa', bad[:5], c.kappa_map[tuple(bad[0])], m.kappa[tuple(bad[0])])


def check_sums(c, m, what):
    E, D = _lib.contour_sum_terms(c.N)
    for k, name in enumerate(ct.SUMS):
        terms = m.terms[name]
        ref, mag = terms.sum(dtype=np.longdouble), np.abs(terms).sum(dtype=np.longdouble)
        err, bound = abs(np.longdouble(c.sums[k]) - ref), (E - 1 + D + R_MAP) * 2.0 ** -53 * mag
        assert err <= bound, (what, name, float(err), float(bound), c.sums[k], float(ref))


def check(c, m, what, map=True):
    """The look `c` holds the words, the histograms, the map and, within their bound, the sums of the model `m`."""
    assert c.words.dtype == np.int64 and np.array_equal(c.words, m.words), (what, dict(zip(ct.WORDS, zip(c.words, m.words))))
    assert np.array_equal(np.stack((c.hist, c.hist_length)), m.hist), (what, np.argwhere(np.stack((c.hist, c.hist_length)) != m.hist)[:5])
    if map:
        check_map(c, m, what)
    check_sums(c, m, what)


def test_the_tile_is_the_sources(gpu):
    assert _lib.contour_tile()[:2] == (TW, TH) == host.tile_from_source()[:2]
    assert {TW, TW + 1, 2 * TW + 1, TH + 1, 2 * TH - 1} <= set(SIZES) and min(SIZES) == 8


# ---------------------------------------------------------------------------
# 1. sizes: random fields, both element types
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ['float64', 'float32'])
@pytest.mark.parametrize("N", SIZES)
def test_sizes(gpu, N, dtype):
    s, eng = engine_of(N, 'chirp', dtype)
    for fraction in (0.2, 0.5):
        eng.set_U(host.smooth_field(N, 11 * N + 1, fraction))
        Ud = eng.get_U()
        m = ct.contour_model(Ud, T, 64, 4.0)
        c = dev_look(eng, T, 64, 4.0)
        check(c, m, f"N={N} {dtype} {fraction}")
        assert 0 < c.word('n_below') < N * N and c.word('segments') > 0 and (N < 16 or c.word('cells_curv') > 0)
    assert eng.contour_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. closed forms, special values
# ---------------------------------------------------------------------------
def test_closed_forms_on_the_device(gpu):
    N = 33
    s, eng = engine_of(N)
    ramp = np.tile(np.arange(N) / 4, (N, 1))
    for field, want in ((ramp, (0.0, N - 1.0)), (ramp.T.copy(), (N - 1.0, 0.0))):
        eng.set_U(field)
        c = dev_look(eng, 3.3)
        check(c, ct.contour_model(field, 3.3), 'ramp')
        assert c.length == N - 1 and (c.sum('txx'), c.sum('tyy')) == want and c.sum('txy') == 0.0
        assert np.all(c.kappa_map[~np.isnan(c.kappa_map)] == 0.0) and c.word('cells_curv') == N - 3
        assert c.sum('k1') == c.sum('ka') == c.sum('k2') == 0.0
    i, j = np.indices((N, N))
    board = host.mh.field_of((i + j) % 2 == 0)
    eng.set_U(board)
    c = dev_look(eng, T)
    check(c, ct.contour_model(board, T), 'checkerboard')
    assert c.word('saddles') == (N - 1) ** 2 and c.word('cells_curv') == 0 and c.word('segments') == 2 * (N - 1) ** 2
    for v, below in ((host.FG, N * N), (host.BG, 0)):
        eng.set_U(np.full((N, N), v))
        c = dev_look(eng, T)
        want = np.zeros(ct.CHS_CT_WORDS, dtype=np.int64)
        want[ct.CHS_CT_N_BELOW] = below
        assert np.array_equal(c.words, want) and not c.sums.any() and not c.hist.any() and not c.hist_length.any()
        assert not c.ell_map.any() and np.isnan(c.kappa_map).all()
    s.close(fetch_U=False)

    N, c0, R = 129, 64.25, 40
    s, eng = engine_of(N)
    U = host.paraboloid(N, c0)
    eng.set_U(U)
    c = dev_look(eng, float(R * R), 64, 0.05)
    check(c, ct.contour_model(U, float(R * R), 64, 0.05), 'paraboloid')
    ii, jj = np.nonzero(~np.isnan(c.kappa_map))
    rho = np.hypot(ii + 0.5 - c0, jj + 0.5 - c0)
    assert len(ii) == c.word('cells_curv') == c.word('cells_one') + c.word('cells_two') > 200
    assert np.max(np.abs(c.kappa_map[ii, jj] * rho - 1.0)) <= 4 * 2.0 ** -52
    rel = c.length / (2 * np.pi * R) - 1.0
    assert -(1 / 8 + 1 / 12) / R ** 2 <= rel <= 0.0, rel
    assert abs(c.sum('k1') / (2 * np.pi) - 1.0) <= 1e-3
    assert c.word('saddles') == c.word('ends') == 0
    log_line(f"contour: paraboloid R={R} N={N}: length / (2 pi R) - 1 = {rel:.3e}, K1 / (2 pi) - 1 = "
             f"{c.sum('k1') / (2 * np.pi) - 1:.3e}, pixel ratio {c.pixel_ratio:.4f}")
    s.close(fetch_U=False)


@pytest.mark.parametrize("dtype", ['float64', 'float32'])
def test_special_values_at_the_tile_corners_and_in_the_halo(gpu, dtype):
    """N = 130: 3 x 9 tiles.  NaN, +inf, -inf and pixels equal to t at the corners of the tiles, in the halo rows and
    columns on either side of their borders and on the grid's outermost lines."""
    N = 130
    s, eng = engine_of(N, 'chirp', dtype)
    U = host.smooth_field(N, 77)
    vals = (np.nan, np.inf, -np.inf, T)
    k = 0
    for i in (0, 1, TH - 1, TH, TH + 1, TH + 2, 2 * TH - 1, 2 * TH, 8 * TH, 8 * TH + 1, N - 2, N - 1):
        for j in (0, 1, TW - 1, TW, TW + 1, TW + 2, 2 * TW - 1, 2 * TW, 2 * TW + 1, N - 1):
            if (i * 7 + j) % 3 == 0:
                U[i, j] = vals[k % 4]
                k += 1
    assert k > 30
    eng.set_U(U)
    Ud = eng.get_U()
    assert np.array_equal(np.isnan(Ud), np.isnan(U)) and np.array_equal(np.isinf(Ud), np.isinf(U)) and np.array_equal(Ud == T, U == T)
    m = ct.contour_model(Ud, T, 32, 3.0)
    c = dev_look(eng, T, 32, 3.0)
    check(c, m, f"special {dtype}")
    assert c.word('n_nonfinite') == np.count_nonzero(~np.isfinite(U)) > 20
    assert c.word('cells_bad') == np.count_nonzero(m.cells.bad) > 50
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the other looks of the same handle
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def evolved(gpu):
    """N = 256 fp64 after 300 steps of the default parameters."""
    N, steps = 256, 300
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    yield types.SimpleNamespace(s=s, N=N, U=U, t=t)
    s.close(fetch_U=False)


def test_an_evolved_field(evolved):
    s, N, t = evolved.s, evolved.N, evolved.t
    m = ct.contour_model(evolved.U, t, 64, 1.0)
    c = s.contour(t, map=True)
    check(c, m, f"evolved N={N}")
    assert c.N == N and c.threshold == t and c.delx == s.solution.delx and (c.bins, c.kmax) == (64, 1.0)
    assert 1.0 < c.pixel_ratio < 1.5 and c.word('cells_bad') == 0 and c.word('cells_curv') > 100
    o = c.orientation()
    log_line(f"contour: evolved N={N} after 300 steps: S_V {c.S_V:.5f}, pixel ratio {c.pixel_ratio:.4f}, mean curvature "
             f"{c.mean_curvature:.4e}, rms {c.rms_curvature:.4e}, anisotropy {o.anisotropy:.3e}, under/over "
             f"{c.word('hist_under')}/{c.word('hist_over')}, look {s._engine.contour_ms():.3f} ms")
    bare = s.contour(t, hist=False)
    assert bare.hist is None and bare.ell_map is None and np.array_equal(bare.words, c.words)
    assert bare.sums.tobytes() == c.sums.tobytes()
    own = s.contour()                                      # params.threshold
    assert own.threshold == s.params.threshold and own.word('n_below') == s.morphology().n_A


def test_identities_with_the_other_looks(evolved):
    s, N, t = evolved.s, evolved.N, evolved.t
    c = s.contour(t)
    mo = s.morphology(t)
    two = s.two_point(t, rmax=1)
    assert c.word('vertices_rows') + c.word('vertices_cols') == mo.perimeter_inner
    assert c.word('vertices_rows') == N * (N - 1) - two.word('adj_rows_below') - two.word('adj_rows_above')
    assert c.word('vertices_cols') == N * (N - 1) - two.word('adj_cols_below') - two.word('adj_cols_above')
    assert c.word('n_below') == mo.n_A == two.n('below') and c.word('n_nonfinite') == 0


# ---------------------------------------------------------------------------
# 4. look behaviour
# ---------------------------------------------------------------------------
def test_looks_give_the_same_bits(gpu):
    N = 130
    U = host.smooth_field(N, 5)
    s, eng = engine_of(N)
    eng.set_U(U)
    looks = [dev_look(eng, T, 64, 4.0, map=False) for _ in range(3)]
    s2, eng2 = engine_of(N)
    eng2.set_U(U)
    looks.append(dev_look(eng2, T, 64, 4.0, map=False))
    assert looks[0].sums.all()                             # (a noise field: none of the six is zero)
    for c in looks[1:]:
        assert c.sums.tobytes() == looks[0].sums.tobytes() and np.array_equal(c.words, looks[0].words)
        assert np.array_equal(c.hist, looks[0].hist) and np.array_equal(c.hist_length, looks[0].hist_length)
    s.close(fetch_U=False)
    s2.close(fetch_U=False)


def test_bins_kmax_and_the_map_that_goes_with_its_look(gpu):
    N = 65
    s, eng = engine_of(N)
    eng.set_U(host.smooth_field(N, 9))
    Ud = eng.get_U()
    for bins, kmax in ((1, 2.0), (1024, 2.0), (64, 1e-3), (7, 0.3)):
        m = ct.contour_model(Ud, T, bins, kmax)
        c = dev_look(eng, T, bins, kmax)
        check(c, m, f"bins {bins} kmax {kmax}")
        assert eng.contour_hist().shape == (2, bins)
        if kmax == 1e-3:
            assert c.word('hist_under') > 0 < c.word('hist_over')
    # a look with the map, then one with other bins and without it: the map went with its look
    c = dev_look(eng, T, 16, 2.0, map=True)
    assert eng.contour_map().shape == (2, N - 1, N - 1)
    d = dev_look(eng, T, 33, 2.0, map=False)
    check(d, ct.contour_model(Ud, T, 33, 2.0), 'after a map', map=False)
    assert d.sums.tobytes() == c.sums.tobytes() and eng.contour_hist().shape == (2, 33)
    with pytest.raises(AssertionError, match='without the map'):
        eng.contour_map()
    with pytest.raises(_lib.EngineError, match='expected 33'):
        eng.contour_hist(16)
    e = dev_look(eng, T, 16, 2.0, map=True)                # and back
    check(e, ct.contour_model(Ud, T, 16, 2.0), 'a map again')
    s.close(fetch_U=False)


def test_errors_and_a_rejected_call_leaves_the_last_look(gpu):
    N = 65
    s = tgs.solver(N, 4, 'chirp')
    eng = s._get_engine()
    words, sums, ms = np.zeros(16, dtype=np.int64), np.zeros(6), np.zeros(1)
    hist = np.zeros(2 * 64 + 1, dtype=np.int64)
    o, f, h = _lib._i64ptr(words), _lib._dptr(sums), _lib._i64ptr(hist)
    assert gpu.chs_contour(eng._h, 0.5, 64, 1.0, 0, o, f) == _lib.CHS_ESTATE                 # no field yet
    assert gpu.chs_contour_hist(eng._h, 64, h) == _lib.CHS_ESTATE                            # no look yet
    assert gpu.chs_contour_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    with pytest.raises(AssertionError):
        s.contour()
    s.prepare()
    eng.set_U(host.smooth_field(N, 3))
    Ud = eng.get_U()
    assert gpu.chs_contour(eng._h, T, 0, 1.0, 0, o, f) == _lib.CHS_EINVAL and 'bins' in gpu.chs_last_error().decode()
    assert gpu.chs_contour_hist(eng._h, 64, h) == _lib.CHS_ESTATE                            # that was no look
    assert gpu.chs_contour(eng._h, T, 64, 1.0, 0, o, f) == _lib.CHS_OK
    m = ct.contour_model(Ud, T, 64, 1.0)
    assert np.array_equal(words, m.words)
    assert gpu.chs_contour_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    t0, w0, s0 = ms[0], words.copy(), sums.copy()
    for bins in (0, -1, 1025):                                                               # rejected: bins ...
        assert gpu.chs_contour(eng._h, T, bins, 1.0, 0, o, f) == _lib.CHS_EINVAL and 'bins' in gpu.chs_last_error().decode()
    for kmax in (0.0, -1.0, float('nan'), float('inf')):                                     # ... kmax ...
        assert gpu.chs_contour(eng._h, T, 64, kmax, 0, o, f) == _lib.CHS_EINVAL and 'kmax' in gpu.chs_last_error().decode()
    for bad in (float('nan'), float('inf'), -float('inf')):                                  # ... the threshold ...
        assert gpu.chs_contour(eng._h, bad, 64, 1.0, 0, o, f) == _lib.CHS_EINVAL and 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_contour(eng._h, T, 64, 1.0, 0, None, f) == _lib.CHS_EINVAL                # ... a null argument
    assert gpu.chs_contour(eng._h, T, 64, 1.0, 0, o, None) == _lib.CHS_EINVAL
    assert np.array_equal(words, w0) and sums.tobytes() == s0.tobytes()
    for wrong in (63, 65, 0, -1):
        assert gpu.chs_contour_hist(eng._h, wrong, h) == _lib.CHS_EINVAL and 'expected 64' in gpu.chs_last_error().decode()
    assert gpu.chs_contour_hist(eng._h, 64, None) == _lib.CHS_EINVAL
    assert gpu.chs_contour_map(eng._h, 2 * (N - 1) ** 2, f) == _lib.CHS_ESTATE               # a look without the map
    hist[-1] = -7                                                                            # the last look and its time are in place
    assert gpu.chs_contour_hist(eng._h, 64, h) == _lib.CHS_OK and hist[-1] == -7
    assert np.array_equal(hist[:-1].reshape(2, 64), m.hist)
    assert gpu.chs_contour_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] == t0
    assert gpu.chs_contour_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_contour(eng._h, T, 64, 1.0, 1, o, f) == _lib.CHS_OK
    mp = np.zeros(2 * (N - 1) ** 2 + 1)
    assert gpu.chs_contour_map(eng._h, mp.size, _lib._dptr(mp)) == _lib.CHS_EINVAL and f"expected {mp.size - 1}" in gpu.chs_last_error().decode()
    assert gpu.chs_contour_map(eng._h, mp.size - 1, _lib._dptr(mp)) == _lib.CHS_OK
    assert np.array_equal(mp[:(N - 1) ** 2].reshape(N - 1, N - 1), m.ell)
    with pytest.raises(_lib.EngineError):
        s.contour(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_contour(b._h, 0, 0.5, 64, 1.0, 0, o, f) == _lib.CHS_ESTATE          # no fields yet
    assert gpu.chs_batch_contour_hist(b._h, 64, h) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, 65536):
        assert gpu.chs_batch_contour(b._h, member, 0.5, 64, 1.0, 0, o, f) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_contour(b._h, 1, 0.5, 0, 1.0, 0, o, f) == _lib.CHS_EINVAL
    assert gpu.chs_batch_contour_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    U1 = b.get_U(1)
    t = float(np.median(U1))
    assert gpu.chs_batch_contour(b._h, 1, t, 64, 50.0, 0, o, f) == _lib.CHS_OK
    m = ct.contour_model(U1, t, 64, 50.0)
    assert np.array_equal(words, m.words)
    assert gpu.chs_batch_contour_hist(b._h, 63, h) == _lib.CHS_EINVAL and 'expected 64' in gpu.chs_last_error().decode()
    assert gpu.chs_batch_contour_hist(b._h, 64, h) == _lib.CHS_OK and np.array_equal(hist[:-1].reshape(2, 64), m.hist)
    assert gpu.chs_batch_contour_map(b._h, 2 * 127 ** 2, f) == _lib.CHS_ESTATE
    assert gpu.chs_batch_contour_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    bs.close(fetch_U=False)


def _looks(s):
    s.contour()
    s.contour(bins=5, kmax=0.25, hist=False, map=True)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] == 128 and not c[4]]


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with contour() between them against the same calls with get_U() between them: all nine record columns, the
    state and the final field, bit for bit."""
    assert [(c[0], c[1]) for c in OBSERVE_CASES] == [(128, 'fast')]
    got, Ug = tgs._observed_run(N, engine, calls, _looks, seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert np.array_equal(Ug, Ur)


def test_a_look_at_a_member_does_not_change_the_batch(gpu):
    def run(look):
        bs = BatchSolver(tgs._members(128, 3, 100))
        bs.prepare()
        bs.solve_or_resume(20)
        look(bs)
        bs.solve_or_resume(20)
        out = tgs._batch_snap(bs)
        bs.close(fetch_U=False)
        return out
    got, ref = run(lambda bs: _looks(bs.solvers[1])), run(lambda bs: None)
    for m in range(3):
        assert got[m][0].tobytes() == ref[m][0].tobytes() and got[m][1].tobytes() == ref[m][1].tobytes(), m
        assert got[m][2] == ref[m][2], m


# ---------------------------------------------------------------------------
# 5. batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (136, 'chirp')])
def test_batch_equals_a_single_handle_holding_the_same_field(gpu, N, engine):
    B = 3
    bs = BatchSolver(tgs._members(N, B, 100))
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(10)
    fields = [s._engine.get_U() for s in bs.solvers]
    ts = [float(np.median(U)) for U in fields]
    cs = bs.contour(threshold=ts, bins=32, kmax=50.0, map=True)
    assert len(cs) == B and [c.threshold for c in cs] == ts
    single, eng = engine_of(N, 'chirp' if engine == 'chirp' else 'fast')
    for m in range(B):
        check(cs[m], ct.contour_model(fields[m], ts[m], 32, 50.0), f"member {m}")
        eng.set_U(fields[m])
        assert np.array_equal(eng.get_U(), fields[m])
        one = dev_look(eng, ts[m], 32, 50.0)
        assert np.array_equal(one.words, cs[m].words) and one.sums.tobytes() == cs[m].sums.tobytes(), m
        assert np.array_equal(one.hist, cs[m].hist) and np.array_equal(one.hist_length, cs[m].hist_length), m
        again = bs.contour(m, threshold=ts, bins=32, kmax=50.0)
        assert again.sums.tobytes() == cs[m].sums.tobytes() and again.ell_map is None, m
        assert bs._batch.contour_ms() >= 0.0
    assert not np.array_equal(cs[0].words, cs[1].words)
    single.close(fetch_U=False)
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 6. the streamed loads
# ---------------------------------------------------------------------------
def test_streamed_contour(big):
    """k_ct_cells<T, V, true> at N = 4097, 4098 (fp64) and 5793, 5796 (fp32): words, histograms and sums against the model
    of the downloaded field; the map at the two sizes with element loads."""
    with_map = big.V == 1
    m = ct.contour_model(big.Ud, T, 64, 8.0)
    c = dev_look(big.eng, T, 64, 8.0, map=with_map)
    check(c, m, big.what, map=with_map)
    assert c.word('n_below') == int(big.below.sum()) and c.word('n_nonfinite') == 1 and c.word('cells_bad') > 0
    log_line(f"contour, large: {big.what}: {big.eng.contour_ms():.3f} ms (map {with_map}), {c.word('segments')} segments")
