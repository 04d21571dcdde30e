"""GPU tests (``-m gpu``) of the five looks at the field where production runs them and the other look tests stop:

* above the cache bound (``chs_grid_exceeds_cache``: 2 N^2 esz > 256 MiB), where every look's first kernel is the
  instantiation with non-temporal loads -- k_spec_bins, k_morph_quads, k_cc_tile, k_dt_mask <T, V, true> for two element
  types and two load widths, k_ch_mask <T, true> for two element types (DESIGN.md section 3g lists them with the test that
  runs each).  The direct engine takes any N; the four sizes are the smallest that reach each instantiation;
* the distance transform and the chord lengths at N = 4096 and 2049, against references that hold at any N
  (tests/test_distance_host.py: reference_exact; the numpy model of the chords), and the radius bins beyond the
  workgroup's LDS histogram of k_dt_stats, which need a distance of DT_LBINS pixels.

A streamed kernel's whole output is the thresholded mask, so the sharp checks are pixel-wise equalities against ``get_U``
of the same handle.  Everything but the structure factor is integer and compared for equality; the structure factor has
the derived bound of tests/test_gpu_spectrum.py with the transform error measured by ``Engine.dctn`` against scipy
(profiles/looks_large_sizes.txt)."""
import math
import os
import re
import types

import numpy as np
import pytest
from scipy import fft as sfft

import chsimpy_amd
from chsimpy_amd import _build, _lib, chords, components, distance, morphology
from gpu_helpers import log_line, make
import test_gpu_spectrum as tgs
import test_chords_host as chost
import test_components_host as cchost
import test_distance_host as dhost
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = mh.T
SIDES = dhost.SIDES
MIB = 1 << 20
ESZ = {'float64': 8, 'float32': 4}
# the smallest N that reaches each streamed instantiation: (N, element type, pixels per load)
STREAMED = [(4097, 'float64', 1), (4098, 'float64', 2), (5793, 'float32', 1), (5796, 'float32', 4)]
FULL_DISTANCE = {(4098, 'float64'), (5796, 'float32')}     # the whole map, words and histogram against reference_exact
FULL_COMPONENTS = {(4097, 'float64'), (5793, 'float32')}   # table and labels against scipy's labelling
# max |Engine.dctn(X) - scipy.fft.dctn(X)| / max |scipy.fft.dctn(X)| of the direct engine on the centred test field X, as
# measured on the MI355X (profiles/looks_large_sizes.txt); the structure factor's tau is five times that
# (on the field itself, whose largest coefficient is the constant mode N * mean(U), the same absolute error reads 1.7e-14
# ... 3.6e-8: no measure of what the bins of the centred field can move by)
DCTN_MEASURED = {(4097, 'float64'): 5.57e-13, (4098, 'float64'): 4.84e-13, (5793, 'float32'): 2.51e-5, (5796, 'float32'): 2.73e-5}


def cache_bound_from_source():
    """The byte count of chs_grid_exceeds_cache (chs_common.h), read from its text."""
    src = open(os.path.join(_build.CSRC, 'chs_common.h')).read()
    m = re.search(r'chs_grid_exceeds_cache\(size_t N, size_t elem_bytes\)\s*\{\s*return 2 \* N \* N \* elem_bytes > '
                  r'\(\(size_t\)(\d+) << (\d+)\);', src)
    assert m, "chs_grid_exceeds_cache is not what this module was written for"
    return int(m.group(1)) << int(m.group(2))


def lbins_from_source():
    src = open(os.path.join(_build.CSRC, 'chs_distance.hip')).read()
    return int(re.search(r'#define\s+DT_LBINS\s+(\d+)\b', src).group(1))


def below_of(Ud, t):
    return np.nan_to_num(Ud, nan=np.inf) < t


def side_of(below, side):
    return below if side == 'below' else ~below


def distance_raw(eng, t, side, map=True):
    return eng.distance_look(t, components.side_code(side), True, map)


def test_the_sizes_lie_on_their_side_of_the_cache_bound():
    """Every streamed size is above the bound the kernels' launchers use, the largest size of the other look tests
    (N = 4096 fp64) is exactly at it, which is not above: a change of the bound makes this test say so."""
    bound = cache_bound_from_source()
    assert bound == 256 * MIB
    for N, dtype, V in STREAMED:
        assert 2 * N * N * ESZ[dtype] > 256 * MIB, (N, dtype)
        n0 = N - (16 // ESZ[dtype] if V > 1 else 1)      # the size before it with this load width
        assert 2 * n0 * n0 * ESZ[dtype] <= 256 * MIB, (N, dtype)                       # (the smallest such N)
        assert (N % (16 // ESZ[dtype]) == 0) == (V > 1), (N, dtype)                    # (16-byte rows or not)
    assert 2 * 4096 * 4096 * 8 == 256 * MIB
    assert 2 * 4096 * 4096 * 4 < 2 * 5792 * 5792 * 4 <= 256 * MIB


# ---------------------------------------------------------------------------
# B. the streamed instantiations
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module', params=STREAMED, ids=[f"N{c[0]}-{c[1]}" for c in STREAMED])
def big(request, gpu):
    """One direct engine per size with a random two-level field, a few pixels exactly at the threshold and one NaN,
    uploaded once; what the device holds (``get_U``) and its mask below the threshold go with it."""
    N, dtype, V = request.param
    s = chsimpy_amd.Solver(make(N, 2, 'auto', dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == 'direct'
    assert 2 * N * N * ESZ[dtype] > 256 * MIB
    rng = np.random.default_rng(N)
    U = mh.field_of(rng.random((N, N)) < 0.6)
    at = (rng.integers(0, N, 24), rng.integers(0, N, 24))
    U[at] = T                                            # at the threshold: not below it
    nan_at = (N // 3, N - 2)
    U[nan_at] = np.nan                                   # NaN: not below it either
    eng.set_U(U)
    Ud = eng.get_U()
    assert np.array_equal(Ud == T, U == T) and np.isnan(Ud[nan_at]) and int(np.isnan(Ud).sum()) == 1
    below = below_of(Ud, T)
    assert np.array_equal(below, np.nan_to_num(U, nan=np.inf) < T) and not below[at].any() and not below[nan_at]
    yield types.SimpleNamespace(N=N, dtype=dtype, V=V, eng=eng, U=U, Ud=Ud, below=below, nan_at=nan_at,
                                what=f"N={N} {dtype} streamed")
    s.close(fetch_U=False)


def test_streamed_distance(big):
    """k_dt_mask<T, V, true>: D2 > 0 is the foreground on both sides; fg and ninf of the summary; at one size per element
    type the whole map, the words and the histogram of the side below against the index-based reference."""
    N, eng = big.N, big.eng
    for side in SIDES:
        X = side_of(big.below, side)
        words, hist, d2 = distance_raw(eng, T, side)
        assert d2.dtype == np.int32 and np.array_equal(d2 > 0, X), (big.what, side)
        assert words[distance.CHS_DT_FG] == int(X.sum()) == int(hist.sum()) and words[distance.CHS_DT_NINF] == 0
        assert 0 < words[distance.CHS_DT_FG] < N * N
        if side == 'below' and (N, big.dtype) in FULL_DISTANCE:
            di = types.SimpleNamespace(words=words, hist=hist, d2=d2)
            dhost.check_against(di, dhost.reference_exact(X), f"{big.what} {side}")
    log_line(f"looks, large: {big.what}: distance {eng.distance_ms():.3f} ms")


def test_streamed_components(big):
    """k_cc_tile<T, V, true>: labels >= 0 is the foreground on both sides; at one size per element type summary, table
    and labels of the side below against scipy's labelling."""
    N, eng = big.N, big.eng
    for side in SIDES:
        X = side_of(big.below, side)
        words, tab, lab = eng.components_look(T, 4, components.side_code(side), True, True)
        assert lab.dtype == np.int32 and np.array_equal(lab >= 0, X), (big.what, side)
        co = components.Components(words, N, T, 4, side, table=tab, labels=lab)
        assert co.area == int(X.sum()) and co.count > 1000
        if side == 'below' and (N, big.dtype) in FULL_COMPONENTS:
            cchost.check_look(co, X, 4, f"{big.what} {side}")
    log_line(f"looks, large: {big.what}: components {eng.components_ms():.3f} ms")


def test_streamed_morphology(big):
    """k_morph_quads<T, V, true>: the seven words against the numpy model on the downloaded field."""
    words = big.eng.morphology(T)
    want = morphology.quad_counts(big.Ud, T)
    assert words.dtype == np.int64 and np.array_equal(words, want), (big.what, words, want)
    assert morphology.Morphology(words, big.N, T).n_A == int(big.below.sum())
    log_line(f"looks, large: {big.what}: morphology {big.eng.morphology_ms():.3f} ms")


def test_streamed_chords(big):
    """k_ch_mask<T, true>: the eight histograms against the numpy model on the downloaded field, the 24 words against
    the summary of them."""
    words, hist = big.eng.chords_look(T, True)
    want = chords.chord_histograms(big.Ud, T)
    assert hist.dtype == np.int64 and hist.shape == want.shape
    assert np.array_equal(hist, want), (big.what, np.argwhere(hist != want)[:5])
    assert words.dtype == np.int64 and np.array_equal(words, chords.summary_of(want)), big.what
    log_line(f"looks, large: {big.what}: chords {big.eng.chords_ms():.3f} ms")


def dctn_error(eng, X):
    """max |Engine.dctn(X) - scipy.fft.dctn(X)| / max |scipy.fft.dctn(X)|."""
    ref = sfft.dctn(X, norm='ortho', workers=max(1, min(8, os.cpu_count() or 1)))
    return float(np.max(np.abs(eng.dctn(X) - ref)) / np.max(np.abs(ref)))


def test_streamed_structure_factor(big):
    """k_spec_bins<T, V, true>: the field without its NaN pixel (a NaN would be the whole spectrum), against scipy with
    the derived bound of tests/test_gpu_spectrum.py.  tau is five times the error of the engine's transform measured
    through Engine.dctn on the centred field (DCTN_MEASURED), never anything taken from the structure factor."""
    N, eng = big.N, big.eng
    measured = DCTN_MEASURED[(N, big.dtype)]
    clean = big.U.copy()
    clean[big.nan_at] = mh.BG
    eng.set_U(clean)
    try:
        Ud = eng.get_U()
        err = dctn_error(eng, Ud - Ud.mean())
        log_line(f"looks, large: {big.what}: dctn error on the centred field {err:.3e} (recorded {measured})")
        ssum = eng.structure_factor()
        ms = eng.structure_factor_ms()
        log_line(f"looks, large: {big.what}: structure factor {ms[0]:.3f} + {ms[1]:.3f} + {ms[2]:.3f} ms")
        tgs.check(ssum, Ud, 5 * measured, big.what)
    finally:
        eng.set_U(big.U)                                 # the other tests of this size look at the field with its NaN


def test_streamed_looks_agree_with_each_other(big):
    """The identities of test_the_five_looks_in_turn_do_not_disturb_each_other: the area of the chords, the morphology,
    the distance transform and the components is one number, and so is the perimeter of chords and morphology."""
    N, eng = big.N, big.eng
    mo = morphology.Morphology(eng.morphology(T), N, T)
    cc = components.Components(eng.components(T, 4, _lib.CHS_CC_BELOW), N, T, 4, 'below')
    dw = eng.distance(T, _lib.CHS_CC_BELOW)
    ch = chords.Chords(eng.chords(T), N, T)
    assert ch.n('below') == mo.n_A == int(dw[distance.CHS_DT_FG]) == cc.area == int(big.below.sum())
    assert ch.n('above') == N * N - mo.n_A and int(dw[distance.CHS_DT_NINF]) == 0
    assert ch.perimeter('below') == mo.perimeter
    assert int(mo.words[1:6].sum()) + int(mo.words[0]) == (N + 1) ** 2


# ---------------------------------------------------------------------------
# C. distance and chords at the sizes they are used at
# ---------------------------------------------------------------------------
def test_an_evolved_field_at_4096(gpu):
    """N = 4096 fp64 on the fast engine (cached loads, 64 bands, 64 words a line) after 4 steps from the default start
    field, thresholded at the field's median: the distance transform of both sides against the index-based reference --
    map, words, histogram -- the chords against the model, and the identities of the two evolved-field tests at N = 512
    that need no further reference."""
    N, steps = 4096, 4
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    below = below_of(U, t)
    co = s.chords(t)
    hist = chords.chord_histograms(U, t)
    assert np.array_equal(co.hist, hist) and np.array_equal(co.words, chords.summary_of(hist))
    assert co.threshold == t and co.N == N and co.delx == sol.delx
    mo = s.morphology(t)
    assert co.perimeter('below') == mo.perimeter and co.n('below') == mo.n_A == int(below.sum())
    assert 0 < co.n('below') < N * N
    for side in SIDES:
        X = side_of(below, side)
        di = s.distance(t, side=side, map=True)
        dhost.check_against(di, dhost.reference_exact(X), f"evolved N={N} {side}")
        assert np.array_equal(di.d2 > 0, X) and di.threshold == t and di.N == N and di.delx == sol.delx
        assert di.fg == s.components(t, side=side, table=False).area == co.n(side) and di.d2max >= 1
        assert di.r_max_phys == di.r_max * sol.delx and 0 < di.quantile(0.5) <= di.quantile(0.9) <= di.r_max
        i, j = di.argmax
        h = math.isqrt(di.d2max - 1)                     # every pixel nearer than r_max is the phase's: |offset| <= h
        for d, at in (('rows', j), ('cols', i)):
            assert min(at, h) + min(N - 1 - at, h) + 1 <= co.max_all(side, d), (side, d)
            assert 1 <= co.quantile(0.5, side, d) <= co.quantile(0.9, side, d) <= co.max(side, d) <= co.max_all(side, d)
        assert co.lineal_path(side, 'rows')[0] == co.n(side) / (N * N) == co.lineal_path(side, 'cols')[0]
    log_line(f"looks, large: evolved N={N} fp64 fast: distance {s._engine.distance_ms():.3f} ms, chords "
             f"{s._engine.chords_ms():.3f} ms")
    s.close(fetch_U=False)


def test_a_random_field_at_2049_fp32(gpu):
    """N = 2049 fp32 on the chirp engine: element loads, 33 bands and 33 words a line, the last of one row / one bit.  A
    random field at density 0.6: the distance transform of both sides against the index-based reference, the chords
    against the model."""
    N = 2049
    s = chsimpy_amd.Solver(make(N, 2, 'chirp', dtype='float32'))
    eng = s._get_engine()
    assert eng.engine == 'chirp'
    rng = np.random.default_rng(N)
    U = mh.field_of(rng.random((N, N)) < 0.6)
    U[rng.integers(0, N, 16), rng.integers(0, N, 16)] = T
    eng.set_U(U)
    Ud = eng.get_U()
    assert np.array_equal(Ud == T, U == T)
    below = below_of(Ud, T)
    for side in SIDES:
        X = side_of(below, side)
        words, hist, d2 = distance_raw(eng, T, side)
        dhost.check_against(types.SimpleNamespace(words=words, hist=hist, d2=d2), dhost.reference_exact(X), f"N={N} {side}")
        assert 0 < words[0] < N * N and words[4] == 0
    words, hist = eng.chords_look(T, True)
    want = chords.chord_histograms(Ud, T)
    assert np.array_equal(hist, want) and np.array_equal(words, chords.summary_of(want))
    log_line(f"looks, large: random N={N} fp32 chirp: distance {eng.distance_ms():.3f} ms, chords {eng.chords_ms():.3f} ms")
    s.close(fetch_U=False)


FAR = [(4096, 'fast'), (4098, 'direct')]


@pytest.mark.parametrize("N,engine", FAR, ids=[f"N{c[0]}-{c[1]}" for c in FAR])
def test_the_far_radius_bins(gpu, N, engine):
    """All foreground but the pixel (0, 0), then but three pixels: D2 is the closed form min_k (i-i_k)^2 + (j-j_k)^2, and
    the radius bins from DT_LBINS on -- which k_dt_stats adds straight to the global histogram, and which only a distance
    of DT_LBINS pixels reaches -- hold pixels, by the reference alone.  N = 4096: cached loads; N = 4098: streamed."""
    lbins = lbins_from_source()
    s = chsimpy_amd.Solver(make(N, 2, 'auto'))
    eng = s._get_engine()
    assert eng.engine == engine and (2 * N * N * 8 > 256 * MIB) == (engine == 'direct')
    # (three pixels near one corner: their bisectors cut the whole grid, and the far corner stays beyond DT_LBINS pixels)
    for background in (((0, 0),), ((0, 0), (40, 3), (5, 70))):
        D2 = dhost.closed_form(N, background)
        want = distance.histogram_of(D2)                 # (distance.radius_bins of the closed form, counted)
        assert len(want) == distance.bin_count(N) > lbins
        far_bins, far_pixels = int(np.count_nonzero(want[lbins:])), int(want[lbins:].sum())
        assert far_bins > 0 and far_pixels > 0, (N, background)
        X = np.ones((N, N), dtype=bool)
        for i, j in background:
            X[i, j] = False
        eng.set_U(mh.field_of(X))
        words, hist, d2 = distance_raw(eng, T, 'below')
        assert np.array_equal(d2, D2), (N, background, np.argwhere(d2 != D2)[:5])
        assert np.array_equal(hist, want), (N, background, np.flatnonzero(hist != want)[:5])
        assert np.array_equal(hist[lbins:], want[lbins:]) and int(hist[lbins:].sum()) == far_pixels
        assert np.array_equal(words, distance.summary_of(D2))
        if len(background) == 1:
            assert words.tolist() == [N * N - 1, 2 * (N - 1) ** 2, N * N - 1, 2 * N * sum(k * k for k in range(N)), 0]
            assert hist[-1] >= 1 and far_bins > 1000
        log_line(f"looks, large: far bins N={N} {engine}, {len(background)} background pixels: {far_bins} bins from "
                 f"{lbins} on hold {far_pixels} pixels; distance {eng.distance_ms():.3f} ms")
    s.close(fetch_U=False)


def test_chord_patterns_at_4098(gpu):
    """The hand-made patterns of the chords at N = 4098 fp64 on the direct engine: 65 words a line, the last of two
    bits, streamed loads.  Every pattern against its closed form, which is all eight histograms (both directions are
    given), and the words against their summary; one pattern of each kind against the model as well."""
    N = 4098
    tile = chost.tile_from_source()
    assert -(-N // tile[0]) == 65 and N % tile[0] == 2
    s = chsimpy_amd.Solver(make(N, 2, 'auto'))
    eng = s._get_engine()
    assert eng.engine == 'direct'
    names = []
    for name, U, want in chost.patterns(N, tile):
        eng.set_U(U)
        words, hist = eng.chords_look(T, True)
        assert set(want) == {chost.ROWS, chost.COLS}
        for d, lines in want.items():
            exp = chost.expected_of(N, lines)
            assert np.array_equal(hist[:, d], exp), (name, chords.DIRECTIONS[d], np.argwhere(hist[:, d] != exp)[:5])
        assert np.array_equal(words, chords.summary_of(hist)), name
        if name in ('checkerboard', 'six-words-from-bit-10-along-cols'):
            chost.check_look(chords.Chords(words, N, T, hist=hist), U < T, f"{name} N={N}")
        names.append(name)
    assert 'six-words-from-bit-10-along-rows' in names and 'three-words-from-bit-30-along-cols' in names
    assert 'long-chords-along-cols' in names and 'all-phase-0' in names
    s.close(fetch_U=False)
