"""CPU tests of the contour look's host side (chsimpy_amd/contour.py) and of the entry points of the library that need
no device.

The definition (include/chs_hip.h: chs_contour; the docstring of chsimpy_amd/contour.py repeats it): the marching-squares
contour of ``U = t`` with linearly interpolated vertices, saddles cutting off every below corner on its own, the length
and the orientation tensor segment by segment, the curvature of the level set from a 4 x 4 stencil at every crossed
cell that is no saddle, lengths summed in fixed point.

``contour.cells`` (vectorised: the model the GPU tests compare with) is held against ``contour.cells_loop`` (the
definition read out cell by cell in Python floats) bit for bit, and both against closed forms."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from chsimpy_amd import _build, _lib, contour as ct, morphology
import test_morphology_host as mh

FG, BG, T = mh.FG, mh.BG, mh.T
SIZES = [2, 3, 4, 5, 8, 33]
CELL_ARRAYS = ('code', 'l', 'txx', 'txy', 'tyy', 'ell', 'kappa', 'crossed', 'saddle', 'curv', 'wall', 'bad')


def smooth_field(N, seed, fraction=0.5):
    """A field with values spread over [0, 1] around the threshold T: white noise, so that every code occurs."""
    rng = np.random.default_rng(seed)
    U = T + (rng.random((N, N)) - fraction) * 0.5
    return U


def special_field(N, seed):
    """`smooth_field` with pixels equal to T, NaN, +inf and -inf among them."""
    rng = np.random.default_rng(seed)
    U = smooth_field(N, seed)
    k = max(1, N // 4)
    for v in (T, np.nan, np.inf, -np.inf):
        U[rng.integers(0, N, k), rng.integers(0, N, k)] = v
    return U


def fields(N):
    out = [('smooth-0.5', smooth_field(N, N)), ('smooth-0.2', smooth_field(N, N + 1, 0.2)), ('special', special_field(N, N + 2))]
    out.append(('two-level', mh.field_of(np.random.default_rng(N + 3).random((N, N)) < 0.5)))
    return out


def same(a, b):
    return np.array_equal(a, b, equal_nan=(np.asarray(a).dtype.kind == 'f'))


def check_identities(m, N, what):
    """The self-checks of the look (include/chs_hip.h) on a model's results, and the constructor that repeats them."""
    w = {name: int(v) for name, v in zip(ct.WORDS, m.words)}
    assert w['segments'] == w['cells_one'] + w['cells_two'] + 2 * w['saddles'], what
    assert 2 * w['segments'] == 2 * (w['vertices_rows'] + w['vertices_cols']) - w['ends'], what
    assert w['cells_curv'] + w['cells_wall'] + w['cells_bad'] == w['cells_one'] + w['cells_two'], what
    assert int(m.hist[0].sum()) + w['hist_under'] + w['hist_over'] == w['cells_curv'], what
    assert int(m.hist[1].sum()) <= w['l_curv_fix'], what
    if w['hist_under'] + w['hist_over'] == 0:
        assert int(m.hist[1].sum()) == w['l_curv_fix'], what
    txx, tyy = float(m.sums[ct.CHS_CT_TXX]), float(m.sums[ct.CHS_CT_TYY])
    if math.isfinite(txx + tyy):
        # (the model's sums are added in long double: what is left are the 4 roundings of a term and fix()'s cut)
        assert abs(txx + tyy - w['l_fix'] / ct.FIX) <= 8 * 2.0 ** -53 * (txx + tyy) + w['segments'] * 2.0 ** -30, what
    c = ct.Contour(m.words, m.sums, N, m.cells.threshold, m.bins, m.kmax, hist=m.hist, map=np.stack((m.ell, m.kappa)))
    assert c.word('segments') == w['segments'] and c.length == w['l_fix'] / ct.FIX
    return c


@pytest.mark.parametrize("N", SIZES)
def test_the_vectorised_model_is_the_loop(N):
    for name, U in fields(N):
        a, b = ct.cells(U, T), ct.cells_loop(U, T)
        for k in CELL_ARRAYS:
            assert same(getattr(a, k), getattr(b, k)), (N, name, k)
        ma, mb = ct.model_of(a, 16, 0.75), ct.model_of(b, 16, 0.75)
        assert np.array_equal(ma.words, mb.words) and same(ma.sums, mb.sums) and np.array_equal(ma.hist, mb.hist)
        check_identities(ma, N, f"{name} N={N}")
        q = morphology.Morphology(morphology.quad_counts(U, T), N, T)
        assert ma.words[ct.CHS_CT_VERTICES_ROWS] + ma.words[ct.CHS_CT_VERTICES_COLS] == q.perimeter_inner, (N, name)
        assert ma.words[ct.CHS_CT_N_BELOW] == q.n_A, (N, name)
        assert ma.words[ct.CHS_CT_N_NONFINITE] == np.count_nonzero(~np.isfinite(U))
        assert np.all(a.ell[~a.crossed] == 0.0) and np.all(a.ell[a.crossed & ~a.saddle] <= math.sqrt(2.0))
        assert np.array_equal(np.isnan(a.kappa), ~a.curv)
    if N >= 8:
        sp = ct.cells(special_field(N, N + 2), T)
        assert sp.bad.any() or N < 33                       # (the non-finite pixels reach a stencil)


def test_every_code_and_its_segments():
    """A 2 x 2 field per code: the segments of `SEGMENTS`, vertices at 1/4 from the below pixel."""
    lo, hi = T - 0.25, T + 0.75                            # s = 0.25 / 1.0
    for code in range(16):
        U = np.array([[lo if code & 1 else hi, lo if code & 2 else hi], [lo if code & 4 else hi, lo if code & 8 else hi]])
        cl = ct.cells(U, T)
        m = ct.model_of(cl)
        assert cl.code[0, 0] == code
        segs = ct.SEGMENTS[code]
        assert m.words[ct.CHS_CT_SEGMENTS] == len(segs)
        assert m.words[ct.CHS_CT_SADDLES] == (code in (6, 9))
        a, b, c, d = U.ravel() < T
        f = lambda p, q: 0.25 if p else 0.75               # the vertex lies at 1/4 from the below pixel
        pos = {'T': (f(a, b), 0.0), 'B': (f(c, d), 1.0), 'L': (0.0, f(a, c)), 'R': (1.0, f(b, d))}
        for k, name in enumerate(segs):
            (px, py), (qx, qy) = pos[name[0]], pos[name[1]]
            dx, dy = qx - px, qy - py
            ll = math.sqrt(dx * dx + dy * dy)
            assert cl.l[k, 0, 0] == ll, (code, name)
            assert cl.txx[k, 0, 0] == dx * dx / ll and cl.txy[k, 0, 0] == dx * dy / ll and cl.tyy[k, 0, 0] == dy * dy / ll
        check_identities(m, 2, f"code {code}")
        if code in (6, 9):                                 # both below corners cut off: two short segments
            assert cl.ell[0, 0] == 2 * math.sqrt(0.125)


def test_a_ramp():
    N = 33
    U = np.tile(np.arange(N) / 4, (N, 1))
    for field, want in ((U, (0.0, N - 1.0)), (U.T.copy(), (N - 1.0, 0.0))):
        m = ct.contour_model(field, 3.3)
        c = check_identities(m, N, 'ramp')
        assert c.length == N - 1 and c.word('l_fix') == (N - 1) << 30
        assert (c.sum('txx'), c.sum('tyy')) == want and c.sum('txy') == 0.0
        assert np.all(m.kappa[m.cells.curv] == 0.0) and c.word('cells_curv') == N - 3 and c.word('cells_wall') == 2
        assert c.word('ends') == 2 and c.word('saddles') == 0 and c.word('cells_bad') == 0
        assert c.sum('k1') == c.sum('ka') == c.sum('k2') == 0.0 and c.mean_curvature == 0.0
        assert c.pixel_ratio == N / (N - 1) and c.orientation().anisotropy == (1.0 if want[0] else -1.0)
        assert m.hist[0].sum() == N - 3 and m.hist[0][m.bins // 2] == N - 3


def paraboloid(N=129, c=64.25):
    i, j = np.indices((N, N))
    return (j - c) ** 2 + (i - c) ** 2


def test_a_paraboloid():
    N, c0, R = 129, 64.25, 40
    m = ct.contour_model(paraboloid(N, c0), float(R * R))
    c = check_identities(m, N, 'paraboloid')
    cl = m.cells
    ii, jj = np.nonzero(cl.curv)
    rho = np.hypot(ii + 0.5 - c0, jj + 0.5 - c0)
    assert len(ii) == c.word('cells_one') + c.word('cells_two') > 200
    assert np.max(np.abs(cl.kappa[cl.curv] * rho - 1.0)) <= 4 * 2.0 ** -52
    rel = c.length / (2 * math.pi * R) - 1.0
    assert -(1 / 8 + 1 / 12) / R ** 2 <= rel <= 0.0, rel
    assert abs(c.sum('k1') / (2 * math.pi) - 1.0) <= 1e-3
    assert c.word('saddles') == c.word('ends') == c.word('cells_wall') == c.word('cells_bad') == 0
    assert abs(c.mean_curvature - 1 / R) <= 1e-3 / R and abs(c.orientation().anisotropy) <= 1e-3
    assert 1.2 < c.pixel_ratio < 1.35                      # (4 / pi = 1.273)
    inv = ct.contour_model(-paraboloid(N, c0), -float(R * R))       # the below phase outside: the interface is concave
    assert np.array_equal(inv.cells.kappa[cl.curv], -cl.kappa[cl.curv])


def test_a_checkerboard_and_a_constant_field():
    N = 9
    i, j = np.indices((N, N))
    m = ct.contour_model(mh.field_of((i + j) % 2 == 0), T)
    c = check_identities(m, N, 'checkerboard')
    assert c.word('saddles') == (N - 1) ** 2 and c.word('cells_curv') == c.word('cells_one') == c.word('cells_two') == 0
    assert c.word('segments') == 2 * (N - 1) ** 2 and c.mean_curvature is None
    for v, below in ((FG, N * N), (BG, 0), (T, 0)):
        m = ct.contour_model(np.full((N, N), v), T)
        want = np.zeros(ct.CHS_CT_WORDS, dtype=np.int64)
        want[ct.CHS_CT_N_BELOW] = below
        assert np.array_equal(m.words, want) and not m.sums.any() and not m.hist.any()
        c = check_identities(m, N, 'constant')
        assert c.length == 0 and c.pixel_ratio is None and c.orientation() is None and c.quantile(0.5) is None


@pytest.mark.parametrize("bins,kmax", [(1, 0.5), (7, 0.3), (64, 1.0), (1024, 2.0)])
def test_the_histogram_is_numpys(bins, kmax):
    cl = ct.cells(smooth_field(33, 5), T)
    m = ct.model_of(cl, bins, kmax)
    kap, ell = cl.kappa[cl.curv], cl.ell[cl.curv]
    edges = np.linspace(-kmax, kmax, bins + 1)
    assert not np.isin(kap, edges).any()                   # (no kappa on a bin edge: numpy's bins are the definition's)
    assert np.array_equal(m.hist[0], np.histogram(kap, bins=edges)[0])
    assert m.words[ct.CHS_CT_HIST_UNDER] == np.count_nonzero(kap < -kmax)
    assert m.words[ct.CHS_CT_HIST_OVER] == np.count_nonzero(kap > kmax)
    assert m.hist[0].sum() > 50 and (kmax > 1 or m.words[ct.CHS_CT_HIST_UNDER] > 0 < m.words[ct.CHS_CT_HIST_OVER])
    fx = ct.fix(ell)
    for b in range(bins):
        sel = (kap >= edges[b]) & ((kap < edges[b + 1]) if b < bins - 1 else (kap <= edges[b + 1]))
        assert m.hist[1][b] == fx[sel].sum()
    c = check_identities(m, 33, f"bins {bins}")
    assert np.array_equal(c.bin_edges, edges) or np.allclose(c.bin_edges, edges, rtol=0, atol=1e-15)
    q = [c.quantile(p, w) for w in ('cells', 'length') for p in (0.1, 0.5, 0.9)]
    assert all(-kmax <= v <= kmax for v in q) and q[0] <= q[1] <= q[2] and q[3] <= q[4] <= q[5]


def test_the_result_class_rejects_what_does_not_add_up():
    m = ct.contour_model(smooth_field(16, 3), T)
    good = lambda **kw: ct.Contour(kw.get('words', m.words), m.sums, 16, T, m.bins, m.kmax, hist=kw.get('hist', m.hist))
    good()
    for k in (ct.CHS_CT_SEGMENTS, ct.CHS_CT_ENDS, ct.CHS_CT_CELLS_WALL, ct.CHS_CT_HIST_UNDER):
        w = m.words.copy()
        w[k] += 1
        with pytest.raises(ValueError):
            good(words=w)
    h = m.hist.copy()
    h[1, 0] += 1 << 50
    with pytest.raises(ValueError):
        good(hist=h)
    with pytest.raises(ValueError):
        good(hist=m.hist[:, :-1])
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match='bins'):
            ct.check_bins(bad)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='kmax'):
            ct.check_kmax(bad)
    with pytest.raises(ValueError):
        ct.cells(np.zeros((1, 1)), T)
    with pytest.raises(ValueError):
        ct.cells(np.zeros((4, 4)), float('nan'))
    d = ct.Contour(m.words, m.sums, 16, T, m.bins, m.kmax, delx=0.5)
    assert d.length_phys == d.length * 0.5 and d.mean_curvature_phys == d.mean_curvature / 0.5 and d.hist is None
    assert d.S_V == d.length / 15 ** 2 and d.S_V_phys == d.S_V / 0.5


# ---------------------------------------------------------------------------
# the library without a device
# ---------------------------------------------------------------------------
def tile_from_source():
    src = open(os.path.join(_build.CSRC, 'chs_contour.hip')).read()
    d = lambda name: int(re.search(r'#define\s+%s\s+(\d+)\b' % name, src).group(1))
    return d('CT_TW'), d('CT_TH'), d('CT_THREADS'), d('CT_FIN_THREADS')


def test_header_constants():
    hdr = open(os.path.join(_build.INCLUDE, 'chs_hip.h')).read()
    val = lambda name: int(re.search(r'#define\s+%s\s+(\d+)\b' % name, hdr).group(1))
    assert val('CHS_CT_WORDS') == ct.CHS_CT_WORDS == _lib.CHS_CT_WORDS == 16
    assert val('CHS_CT_SUMS') == ct.CHS_CT_SUMS == _lib.CHS_CT_SUMS == 6
    assert val('CHS_CT_MAX_BINS') == ct.CHS_CT_MAX_BINS == _lib.CHS_CT_MAX_BINS == 1024
    assert val('CHS_CT_FIX_BITS') == ct.CHS_CT_FIX_BITS == 30
    for k, name in enumerate(ct.WORDS):
        assert val('CHS_CT_' + name.upper()) == k == getattr(ct, 'CHS_CT_' + name.upper())
    for k, name in enumerate(ct.SUMS):
        assert val('CHS_CT_' + name.upper()) == k == getattr(ct, 'CHS_CT_' + name.upper())


def test_entry_points_that_need_no_device(hip_lib):
    tile = tile_from_source()
    assert _lib.contour_tile() == tile == (64, 16, 256, 1024) == _lib.Engine.contour_tile()
    w = ctypes.c_int32(0)
    assert hip_lib.chs_contour_tile(None, None, None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_contour_tile(ctypes.byref(w), ctypes.byref(w), ctypes.byref(w), None) == _lib.CHS_EINVAL
    # E: two terms per cell of a thread, then a finishing thread's slots; D: the two trees
    assert _lib.contour_sum_terms(8) == (8, 18) == _lib.contour_sum_terms(65)
    assert _lib.contour_sum_terms(4097) == (8 + 16 - 1, 18)          # 65 x 257 tiles: 17 slots a finishing thread
    assert _lib.contour_sum_terms(8192, tile) == (8 + 64 - 1, 18)
    words, sums = np.zeros(16, dtype=np.int64), np.zeros(6)
    o, f = _lib._i64ptr(words), _lib._dptr(sums)
    assert hip_lib.chs_contour(None, 0.5, 64, 1.0, 0, o, f) == _lib.CHS_EINVAL
    assert b'null handle' in hip_lib.chs_last_error()
    assert hip_lib.chs_contour_hist(None, 64, o) == _lib.CHS_EINVAL
    assert hip_lib.chs_contour_map(None, 2, f) == _lib.CHS_EINVAL
    assert hip_lib.chs_contour_last_ms(None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_contour(None, 0, 0.5, 64, 1.0, 0, o, f) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_contour_hist(None, 64, o) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_contour_map(None, 2, f) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_contour_last_ms(None, None) == _lib.CHS_EINVAL
    for name in ('chs_contour', 'chs_contour_hist', 'chs_contour_map', 'chs_contour_last_ms', 'chs_contour_tile',
                 'chs_batch_contour', 'chs_batch_contour_hist', 'chs_batch_contour_map', 'chs_batch_contour_last_ms'):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)


def test_the_solver_settles_its_arguments_before_the_engine():
    import chsimpy_amd
    p = chsimpy_amd.Parameters()
    p.N = 16
    s = chsimpy_amd.Solver(p)
    for kw in (dict(bins=0), dict(bins=1025), dict(kmax=0.0), dict(kmax=float('nan'))):
        with pytest.raises(ValueError):
            s.contour(**kw)
    assert s._engine is None
    assert 'contour' in chsimpy_amd.batch._Member._LOOKS and 'contour_look' in chsimpy_amd.batch._Member._LOOKS
