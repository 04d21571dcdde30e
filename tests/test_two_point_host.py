"""CPU tests of the two-point correlation's host side (chsimpy_amd/two_point.py) and of the entry points of the library
that need no device.

The definition (include/chs_hip.h: chs_two_point): phase 0 is ``(double)U < t`` (a NaN pixel and a pixel equal to t are
not phase 0), phase 1 its complement inside the grid; ``c[p][dy][dx + rmax]`` counts the positions (i, j) for which (i, j)
and (i + dy, j + dx) are both inside the grid and both of phase p, for ``0 <= dy <= rmax, |dx| <= rmax``, without
wrap-around; ``pairs(dy, dx) = (N - dy)(N - |dx|)``.  Everything is an integer: every comparison is for equality.

``pair_counts`` (the FFT model the GPU tests compare with) is held against ``pair_counts_slices`` (the definition written
out), and both against closed forms."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from chsimpy_amd import _build, _lib, two_point as tp
import test_morphology_host as mh

FG, BG, T = mh.FG, mh.BG, mh.T
SIZES = [(8, 1), (8, 7), (63, 62), (65, 64), (130, 65)]


def random_field(N, fraction, seed):
    """A two-level field with the given fraction of phase 0, a few NaN pixels and a few pixels equal to t among them."""
    rng = np.random.default_rng(seed)
    U = mh.field_of(rng.random((N, N)) < fraction)
    k = max(2, N // 8)
    U[rng.integers(0, N, k), rng.integers(0, N, k)] = T
    U[rng.integers(0, N, k), rng.integers(0, N, k)] = np.nan
    return U


def closed_forms(N, rmax):
    """(name, U, c) with c the pair counts in closed form: what the CPU and the GPU tests share."""
    out = []
    pairs = tp.pairs_table(N, rmax)
    dy = np.arange(rmax + 1)[:, None]
    dx = np.arange(-rmax, rmax + 1)[None, :]
    zero = np.zeros_like(pairs)
    out.append(('all-phase-0', np.full((N, N), FG), np.stack((pairs, zero))))
    out.append(('all-phase-1', np.full((N, N), BG), np.stack((zero, pairs))))
    # a single pixel of phase 0 at (a, b): c0 is 1 at (0, 0); c1 loses the windows' positions that are the pixel or have it
    # as their partner
    for a, b in ((0, 0), (N // 2, N - 1), (N - 1, 1)):
        U = np.full((N, N), BG)
        U[a, b] = FG
        c0 = ((dy == 0) & (dx == 0)).astype(np.int64)
        first = (a + dy <= N - 1) & (b + dx >= 0) & (b + dx <= N - 1)           # (a, b) is a position of the window
        second = (a - dy >= 0) & (b - dx >= 0) & (b - dx <= N - 1)              # (a, b) is a partner
        both = (dy == 0) & (dx == 0)
        c1 = pairs - first.astype(np.int64) - second.astype(np.int64) + both.astype(np.int64)
        out.append((f'single-pixel-{a}-{b}', U, np.stack((c0, c1))))
    # a checkerboard: the two pixels of a pair are of one phase iff dy + dx is even; phase 0 at even i + j
    i, j = np.indices((N, N))
    U = mh.field_of((i + j) % 2 == 0)
    even = ((dy + dx) % 2 == 0)
    # (the window of (dy, dx) is a rectangle of (N - dy) x (N - |dx|) positions whose corner (0, max(0, -dx)) has the parity
    # of max(0, -dx): the phase at the corner has the larger half)
    corner_is_0 = np.broadcast_to(np.maximum(0, -dx) % 2 == 0, pairs.shape)
    big, small = (pairs + 1) // 2, pairs // 2
    c0 = np.where(even, np.where(corner_is_0, big, small), 0)
    c1 = np.where(even, np.where(corner_is_0, small, big), 0)
    out.append(('checkerboard', U, np.stack((c0, c1))))
    # vertical stripes of period p: columns with j % p < p // 2 are phase 0
    for p in (2, 6):
        if N < p:
            continue
        col0 = (np.arange(N) % p) < p // 2
        U = mh.field_of(np.broadcast_to(col0, (N, N)))
        c = np.zeros((2, rmax + 1, 2 * rmax + 1), dtype=np.int64)
        for k, d in enumerate(range(-rmax, rmax + 1)):
            lo, hi = max(0, -d), N - max(0, d)                                   # the columns j with j + d inside
            n0 = int(np.count_nonzero(col0[lo:hi] & col0[lo + d:hi + d]))
            n1 = int(np.count_nonzero(~col0[lo:hi] & ~col0[lo + d:hi + d]))
            c[0, :, k] = n0 * (N - np.arange(rmax + 1))
            c[1, :, k] = n1 * (N - np.arange(rmax + 1))
        out.append((f'stripes-{p}', U, c))
    return out


# ---------------------------------------------------------------------------
# the two models
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,rmax", SIZES)
@pytest.mark.parametrize("fraction", [0.1, 0.5])
def test_the_fft_model_equals_the_slices(N, rmax, fraction):
    U = random_field(N, fraction, 31 * N + rmax)
    assert np.isnan(U).any() and (U == T).any()
    a, b = tp.pair_counts(U, T, rmax), tp.pair_counts_slices(U, T, rmax)
    assert a.dtype == b.dtype == np.int64 and a.shape == b.shape == (2, rmax + 1, 2 * rmax + 1)
    assert np.array_equal(a, b)
    X = np.nan_to_num(U, nan=np.inf) < T
    assert a[0, 0, rmax] == int(X.sum()) and a[1, 0, rmax] == N * N - int(X.sum())
    assert np.array_equal(a[:, 0, :], a[:, 0, ::-1])
    assert np.all(a[0] + a[1] <= tp.pairs_table(N, rmax)) and np.all(a >= 0)


def test_the_slices_against_a_double_loop_over_pixels():
    N, rmax = 9, 8
    U = random_field(N, 0.4, 3)
    X = np.nan_to_num(U, nan=np.inf) < T
    want = np.zeros((2, rmax + 1, 2 * rmax + 1), dtype=np.int64)
    for dy in range(rmax + 1):
        for dx in range(-rmax, rmax + 1):
            for i in range(N):
                for j in range(N):
                    if i + dy < N and 0 <= j + dx < N and X[i, j] == X[i + dy, j + dx]:
                        want[0 if X[i, j] else 1, dy, dx + rmax] += 1
    assert np.array_equal(tp.pair_counts_slices(U, T, rmax), want)


@pytest.mark.parametrize("N,rmax", [(8, 7), (33, 32), (65, 40)])
def test_closed_forms(N, rmax):
    names = []
    for name, U, want in closed_forms(N, rmax):
        for model in (tp.pair_counts, tp.pair_counts_slices):
            got = model(U, T, rmax)
            assert np.array_equal(got, want), (name, model.__name__, np.argwhere(got != want)[:5])
        names.append(name)
    assert {'all-phase-0', 'all-phase-1', 'checkerboard', 'stripes-2', 'stripes-6'} <= set(names)
    cb = dict((n, c) for n, _, c in closed_forms(N, rmax))['checkerboard']
    dy, dx = np.indices(cb.shape[1:])
    odd = (dy + dx - rmax) % 2 == 1
    assert not cb[:, odd].any() and np.array_equal((cb[0] + cb[1])[~odd], tp.pairs_table(N, rmax)[~odd])   # zero at odd dy + dx


def test_the_threshold_and_nan_pixels_are_phase_1():
    N = 8
    U = np.full((N, N), FG)
    U[2, 3], U[5, 5], U[0, 7] = T, np.nan, np.nextafter(T, 0.0)
    c = tp.pair_counts_slices(U, T, 1)
    assert c[0, 0, 1] == N * N - 2 and c[1, 0, 1] == 2
    with pytest.raises(ValueError):
        tp.pair_counts(U, float('nan'), 1)
    for bad in (0, N, -1, 1.5, True):
        with pytest.raises(ValueError):
            tp.pair_counts(U, T, bad)
    with pytest.raises(ValueError):
        tp.pair_counts(np.zeros((4, 5)), T, 1)


def test_summary_of():
    U = random_field(20, 0.5, 1)
    c = tp.pair_counts_slices(U, T, 3)
    w = tp.summary_of(c)
    X = np.nan_to_num(U, nan=np.inf) < T
    assert w.dtype == np.int64 and w.shape == (tp.CHS_TP_WORDS,) == (8,)
    assert w[tp.CHS_TP_N_BELOW] == X.sum() and w[tp.CHS_TP_N_ABOVE] == (~X).sum()
    assert w[tp.CHS_TP_ADJ_ROWS_BELOW] == (X[:, :-1] & X[:, 1:]).sum()
    assert w[tp.CHS_TP_ADJ_COLS_BELOW] == (X[:-1, :] & X[1:, :]).sum()
    assert w[tp.CHS_TP_ADJ_ROWS_ABOVE] == (~X[:, :-1] & ~X[:, 1:]).sum()
    assert w[tp.CHS_TP_ADJ_COLS_ABOVE] == (~X[:-1, :] & ~X[1:, :]).sum()
    assert w[tp.CHS_TP_SUM_BELOW] == c[0].sum() and w[tp.CHS_TP_SUM_ABOVE] == c[1].sum()
    assert tp.WORDS.index('adj_cols_above') == tp.CHS_TP_ADJ_COLS_ABOVE == 5
    for bad in (np.zeros((2, 1, 1)), np.zeros((2, 3, 6)), np.zeros((1, 3, 5)), np.zeros((3, 5))):
        with pytest.raises(ValueError):
            tp.summary_of(bad)


# ---------------------------------------------------------------------------
# the result class
# ---------------------------------------------------------------------------
def test_two_point_rejects_what_does_not_fit():
    N, rmax = 12, 4
    c = tp.pair_counts_slices(random_field(N, 0.5, 2), T, rmax)
    w = tp.summary_of(c)
    ok = tp.TwoPoint(w, N, T, rmax, counts=c)
    assert ok.counts is not c and np.array_equal(ok.counts, c) and ok.rmax == rmax and ok.delx is None
    assert tp.TwoPoint(w, N, T, rmax).counts is None

    def bad_words(k, d):
        v = w.copy()
        v[k] += d
        return v
    for k in range(tp.CHS_TP_WORDS):                                         # words and table disagree
        with pytest.raises(ValueError):
            tp.TwoPoint(bad_words(k, 1), N, T, rmax, counts=c)
    with pytest.raises(ValueError):                                          # the phases do not add to N^2
        tp.TwoPoint(bad_words(0, 1), N, T, rmax)
    with pytest.raises(ValueError):
        tp.TwoPoint(w[:7], N, T, rmax)
    asym = c.copy()                                                          # an asymmetric row dy = 0
    asym[0, 0, rmax + 2] += 1
    asym[0, 0, rmax - 1] -= 1                                                # (the sum stays: only the symmetry is broken)
    assert np.array_equal(tp.summary_of(asym), w)
    with pytest.raises(ValueError, match='symmetric'):
        tp.TwoPoint(w, N, T, rmax, counts=asym)
    over = c.copy()                                                          # c0 + c1 > pairs
    over[0, 2, 1] = tp.pairs_table(N, rmax)[2, 1] - over[1, 2, 1] + 1
    with pytest.raises(ValueError, match='pairs'):
        tp.TwoPoint(tp.summary_of(over), N, T, rmax, counts=over)
    neg = c.copy()
    neg[1, 3, 0] = -1
    with pytest.raises(ValueError):
        tp.TwoPoint(tp.summary_of(neg), N, T, rmax, counts=neg)
    with pytest.raises(ValueError):
        tp.TwoPoint(w, N, T, rmax, counts=c[:, :-1])
    for r in (0, N, 300):
        with pytest.raises(ValueError):
            tp.TwoPoint(w, N, T, r)


def hand_made_table():
    """N = 4, rmax = 2, phase 0 the left half: X[i][j] = j < 2."""
    N, rmax = 4, 2
    U = mh.field_of(np.broadcast_to(np.arange(N) < 2, (N, N)))
    c = tp.pair_counts_slices(U, T, rmax)
    return N, rmax, c


def test_s2_cross_radial_first_zero_on_a_hand_made_table():
    N, rmax, c = hand_made_table()
    # columns 0, 1 are phase 0: within a row the pairs at dx = +-1 of phase 0 are 1 of 3, at dx = +-2 none of 2
    assert c[0].tolist() == [[0, 4, 8, 4, 0], [0, 3, 6, 3, 0], [0, 2, 4, 2, 0]]
    assert np.array_equal(c[1], c[0])
    two = tp.TwoPoint(tp.summary_of(c), N, T, rmax, counts=c, delx=0.5)
    assert two.n('below') == two.n(0) == 8 == two.n('above') and two.word('adj_rows_below') == 4 and two.word('adj_cols_above') == 6
    assert two.pairs(0, 0) == 16 and two.pairs(1, -2) == 6 == two.pairs(-1, 2)
    assert two.S2('below', 0, 0) == 0.5 and two.S2('below', 0, 1) == 4 / 12 and two.S2('below', 2, -1) == 2 / 6
    assert two.S2('below', -2, 1) == two.S2('below', 2, -1) and two.S2(1, -1, 0) == 6 / 12       # the mirror image
    assert two.S2('below').shape == (3, 5) and two.S2('below')[1, 3] == 3 / 9
    assert two.cross(0, 0) == 0.0 and two.cross(0, 2) == 1.0 and two.cross(1, 1) == 3 / 9
    with pytest.raises(ValueError):
        two.S2('below', 3, 0)
    with pytest.raises(ValueError):
        two.S2('below', 1)
    with pytest.raises(ValueError):
        two.n('left')
    # shells: 0: (0,0); 1: (0,1), (1,-1), (1,0), (1,1); 2: (0,2), (1,-2), (1,2), (2,-2..2) with isqrt(8) = 2
    rad = two.radial('below')
    assert rad[0] == 8 / 16 and rad[1] == (4 + 3 + 6 + 3) / (12 + 9 + 12 + 9)
    assert rad[2] == (0 + 0 + 0 + 0 + 2 + 4 + 2 + 0) / (8 + 6 + 6 + 4 + 6 + 8 + 6 + 4)
    cov = two.autocovariance('below')
    assert cov.tolist() == [rad[0] - 0.25, rad[1] - 0.25, rad[2] - 0.25] and cov[0] > 0 > cov[2] and cov[1] > 0
    z = 1 + cov[1] / (cov[1] - cov[2])
    assert two.first_zero('below') == z * 0.5                                # physical units with delx
    assert tp.TwoPoint(two.words, N, T, rmax, counts=c).first_zero('below') == z
    assert two.along('below', 'rows').tolist() == [8 / 16, 4 / 12, 0.0] and two.along('below', 'cols').tolist() == [0.5, 0.5, 0.5]
    assert two.anisotropy('below', 1) == (4 / 12) / 0.5 and two.anisotropy('below', 2) == 0.0
    with pytest.raises(ValueError):
        two.along('below', 'diagonal')
    bare = tp.TwoPoint(two.words, N, T, rmax)
    assert bare.S2('below') is None and bare.radial(0) is None and bare.first_zero(0) is None and bare.cross(0, 1) is None
    assert bare.along(0, 'rows') is None and bare.anisotropy(0, 1) is None and bare.n('below') == 8
    assert 'TwoPoint(N=4' in repr(two)
    # no sign change: one phase alone
    full = tp.pair_counts_slices(np.full((6, 6), FG), T, 3)
    assert tp.TwoPoint(tp.summary_of(full), 6, T, 3, counts=full).first_zero('below') is None


@pytest.mark.parametrize("N,rmax", [(20, 19), (37, 12)])
def test_radial_against_a_double_loop_over_displacements(N, rmax):
    c = tp.pair_counts(random_field(N, 0.5, N), T, rmax)
    two = tp.TwoPoint(tp.summary_of(c), N, T, rmax, counts=c)
    for phase in (0, 1):
        num, den = [0] * (rmax + 1), [0] * (rmax + 1)
        for dy in range(rmax + 1):
            for dx in range(-rmax, rmax + 1):
                s = math.isqrt(dy * dy + dx * dx)
                if s > rmax or (dy == 0 and dx < 0):
                    continue
                num[s] += int(c[phase, dy, dx + rmax])
                den[s] += (N - dy) * (N - abs(dx))
        assert two.radial(phase).tolist() == [a / b for a, b in zip(num, den)]


# ---------------------------------------------------------------------------
# the library without a device
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(_build.INCLUDE, 'chs_hip.h')).read()
    val = lambda name: int(re.search(r'#define\s+%s\s+(\d+)\b' % name, hdr).group(1))
    assert val('CHS_TP_WORDS') == tp.CHS_TP_WORDS == _lib.CHS_TP_WORDS == 8
    assert val('CHS_TP_MAX_R') == tp.CHS_TP_MAX_R == _lib.CHS_TP_MAX_R == 256
    assert val('CHS_TP_CHUNK') == _lib.CHS_TP_CHUNK
    for k, name in enumerate(tp.WORDS):
        assert val('CHS_TP_' + name.upper()) == k == getattr(tp, 'CHS_TP_' + name.upper())
    src = open(os.path.join(_build.CSRC, 'chs_two_point.hip')).read()
    d = lambda name: int(re.search(r'#define\s+%s\s+(\d+)\b' % name, src).group(1))
    assert _lib.two_point_tile() == (d('TP_WORD'), d('TP_H'), d('TP_THREADS')) == (32, 64, 256)
    assert d('TP_THREADS') // d('TP_H') * d('TP_K') * d('TP_WORD') == _lib.CHS_TP_CHUNK


def test_entry_points_that_need_no_device(hip_lib):
    w = ctypes.c_int32(0)
    assert hip_lib.chs_two_point_tile(None, None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_two_point_tile(ctypes.byref(w), ctypes.byref(w), None) == _lib.CHS_EINVAL
    for N, want in ((1, 0), (2, 1), (8, 7), (257, 256), (300, 256), (0, 0), (-5, 0)):
        assert hip_lib.chs_two_point_max_r(N) == _lib.two_point_max_r(N) == tp.max_r(N) == want
        assert _lib.Engine.two_point_max_r(N) == want
    for N in (1, 2, 8, 257, 300):
        for rmax in (-1, 0, 1, 7, 8, 255, 256, 257, 299):
            want = 2 * (rmax + 1) * (2 * rmax + 1) if 1 <= rmax <= min(N - 1, 256) else 0
            assert hip_lib.chs_two_point_size(N, rmax) == _lib.two_point_size(N, rmax) == tp.table_size(N, rmax) == want
    assert hip_lib.chs_two_point_size(300, 256) == 2 * 257 * 513
    out = np.zeros(16, dtype=np.int64)
    o = _lib._i64ptr(out)
    assert hip_lib.chs_two_point(None, 0.5, 1, o) == _lib.CHS_EINVAL
    assert b'null handle' in hip_lib.chs_last_error()
    assert hip_lib.chs_two_point_counts(None, 30, o) == _lib.CHS_EINVAL
    assert hip_lib.chs_two_point_last_ms(None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_two_point(None, 0, 0.5, 1, o) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_two_point_counts(None, 30, o) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_two_point_last_ms(None, None) == _lib.CHS_EINVAL


def test_the_solver_clips_the_default_rmax_only():
    """`Solver.two_point` without a device: rmax is settled before the engine is asked for."""
    import chsimpy_amd
    assert tp.DEFAULT_RMAX == 64 and type(tp.DEFAULT_RMAX) is not int
    p = chsimpy_amd.Parameters()
    p.N = 16
    s = chsimpy_amd.Solver(p)
    for bad in (0, 16, 64, 300, 2.5):
        with pytest.raises(ValueError, match='rmax'):
            s.two_point(rmax=bad)
    assert 'two_point' in chsimpy_amd.batch._Member._LOOKS and 'two_point_look' in chsimpy_amd.batch._Member._LOOKS
