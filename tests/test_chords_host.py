"""Host side of the chord lengths of the thresholded field (chsimpy_amd/chords.py): the numpy model against a brute-force
pure-Python run-length walk, hand-made patterns whose chords are known in closed form, the identities with the morphology,
the lineal-path function against a count of the fitting segments, the consistency checks of `Chords`, the header's
constants and prototypes, and the experiment's --chords on a dry run, alone and under gloo at world 2.  No device.

`patterns` and `check_look` are shared with tests/test_gpu_chords.py, which puts the same fields on the device.
Everything is integer: every comparison is for equality."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from chsimpy_amd import _lib, chords, morphology
import test_morphology_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG, BG, T = mh.FG, mh.BG, mh.T
PHASES, DIRECTIONS = chords.PHASES, chords.DIRECTIONS
ROWS, COLS, INNER, CUT = chords.CHS_CH_ROWS, chords.CHS_CH_COLS, chords.CHS_CH_INNER, chords.CHS_CH_CUT


def tile_from_source():
    """(word_bits, lines_per_group, local_bins) of chs_chords.hip without loading the library."""
    from chsimpy_amd import _build
    src = open(os.path.join(_build.CSRC, 'chs_chords.hip')).read()
    return tuple(int(re.search(r'#define\s+%s\s+(\d+)\b' % k, src).group(1)) for k in ('CHS_CH_WORD', 'CH_GROUP', 'CH_LBINS'))


def tile_sizes(tile):
    """The N at which each phase can still go wrong: less than a word; one below / at / one above a word (the tail bits
    of the last word); two words and a bit at an odd and an even N; a last workgroup of a single line; a chord that
    bypasses the workgroup's histogram."""
    w, g, l = tile
    assert l <= 2048
    sizes = sorted({8, w - 1, w, w + 1, 2 * w + 1, 2 * w + 2, g + 1, l + 1})
    assert any(n % 2 for n in sizes) and any(n % 4 == 0 for n in sizes) and any(n % 4 == 2 for n in sizes)
    return sizes


def brute_force(X):
    """hist [2][2][2][N + 1] of the boolean phase-0 image X by the definition itself: a pure-Python walk along every line."""
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    hist = np.zeros((2, 2, 2, N + 1), dtype=np.int64)
    for d in (ROWS, COLS):
        for l in range(N):
            line = [bool(v) for v in (X[l, :] if d == ROWS else X[:, l])]
            start = 0
            for k in range(1, N + 1):
                if k == N or line[k] != line[start]:
                    cut = start == 0 or k == N
                    hist[0 if line[start] else 1, d, CUT if cut else INNER, k - start] += 1
                    start = k
    return hist


def model_look(U, t):
    hist = chords.chord_histograms(U, t)
    return chords.Chords(chords.summary_of(hist), np.asarray(U).shape[0], t, hist=hist)


def check_look(look, X, what=''):
    """A `Chords` (with its histograms where fetched) against the model of the boolean phase-0 image X."""
    X = np.asarray(X, dtype=bool)
    hist = chords.chord_histograms(mh.field_of(X), T)
    words = chords.summary_of(hist)
    assert look.N == X.shape[0]
    assert look.words.dtype == np.int64 and np.array_equal(look.words, words), (what, look.words, words)
    if look.hist is not None:
        assert look.hist.dtype == np.int64 and look.hist.shape == hist.shape
        assert np.array_equal(look.hist, hist), (what, np.argwhere(look.hist != hist)[:5])
    assert look.n('below') == int(X.sum()) and look.n('above') == int((~X).sum())
    return words


def expected_of(N, lines):
    """[phase][cls][N + 1] of one direction from its lines in closed form: `lines` is a list of (how many such lines,
    [(phase, length), ...] the line's runs from index 0 on)."""
    h = np.zeros((2, 2, N + 1), dtype=np.int64)
    total = 0
    for mult, runs in lines:
        assert sum(c for _, c in runs) == N and all(c >= 1 for _, c in runs)
        assert all(a[0] != b[0] for a, b in zip(runs, runs[1:]))
        for k, (phase, c) in enumerate(runs):
            h[phase, CUT if k in (0, len(runs) - 1) else INNER, c] += mult
        total += mult
    assert total == N
    return h


def _runs_of_segments(N, p):
    """The runs of a line of stripes of width p, phase 0 first."""
    nseg = -(-N // p)
    return [(k % 2, p if k < nseg - 1 else N - (nseg - 1) * p) for k in range(nseg)]


def _runs_with(N, spans):
    """The runs of a line of phase 1 with phase 0 on the [a, b] of `spans` (ascending, apart, inside [0, N-1])."""
    runs, at = [], 0
    for a, b in spans:
        assert at <= a <= b < N and (a > at or at == 0)
        if a > at:
            runs.append((1, a - at))
        runs.append((0, b - a + 1))
        at = b + 1
    if at < N:
        runs.append((1, N - at))
    return runs


def _mask_of_runs(runs):
    return np.concatenate([np.full(c, phase == 0) for phase, c in runs])


def patterns(N, tile):
    """Hand-made fields whose chords are known in closed form: a list of (name, U, {direction: lines for expected_of});
    phase 0 is where the mask is True.  The seam patterns put the same line once along the rows and once along the
    columns, so that a transposed plane cannot pass."""
    assert N >= 8
    w = tile[0]
    out = []

    def add(name, X, want):
        out.append((name, mh.field_of(X), want))

    none = np.zeros((N, N), dtype=bool)
    ii, jj = np.indices((N, N))
    add('all-phase-0', ~none, {ROWS: [(N, [(0, N)])], COLS: [(N, [(0, N)])]})
    add('all-phase-1', none, {ROWS: [(N, [(1, N)])], COLS: [(N, [(1, N)])]})
    for p in (1, 2, 3):
        runs = _runs_of_segments(N, p)
        n0 = sum(c for phase, c in runs if phase == 0)
        uniform = [(n0, [(0, N)]), (N - n0, [(1, N)])]
        add(f'vertical-stripes-{p}', (jj // p) % 2 == 0, {ROWS: [(N, runs)], COLS: uniform})
        add(f'horizontal-stripes-{p}', (ii // p) % 2 == 0, {ROWS: uniform, COLS: [(N, runs)]})
    even, odd = [(k % 2, 1) for k in range(N)], [((k + 1) % 2, 1) for k in range(N)]
    board = [((N + 1) // 2, even), (N // 2, odd)]
    add('checkerboard', (ii + jj) % 2 == 0, {ROWS: board, COLS: board})
    m = N // 2
    for name, (i, j) in (('corner', (0, 0)), ('far-corner', (N - 1, N - 1)), ('edge', (0, m)), ('middle', (m, m)), ('last-column', (m, N - 1))):
        X = none.copy()
        X[i, j] = True
        add(f'one-pixel-{name}', X, {ROWS: [(1, _runs_with(N, [(j, j)])), (N - 1, [(1, N)])],
                                     COLS: [(1, _runs_with(N, [(i, i)])), (N - 1, [(1, N)])]})
    # chords of N - 1, N - 2 and N pixels: at N = local_bins + 1 the first bins beyond the workgroup's histogram and its last
    line_a = [(0, N - 1), (1, 1)]                    # one pixel of the other phase at the line's end
    line_b = [(0, 1), (1, 1), (0, N - 2)]
    X = ~none
    X[2, N - 1] = False
    X[5, 1] = False
    rows = [(1, line_a), (1, line_b), (N - 2, [(0, N)])]
    other = [(1, [(0, 5), (1, 1), (0, N - 6)]), (1, [(0, 2), (1, 1), (0, N - 3)]), (N - 2, [(0, N)])]
    add('long-chords-along-rows', X, {ROWS: rows, COLS: other})
    add('long-chords-along-cols', X.T, {ROWS: other, COLS: rows})
    # runs at the seams of the words, along the rows and along the columns; the lines themselves lie at a seam of the
    # other plane (rows w - 1 and w) where the grid has one
    seams = []
    if N >= w + 1:
        seams.append(('change-at-the-seam', [(max(w - 3, 0), w - 1)]))               # ends at bit w - 1; the next starts at bit w
    if N >= w + 3:
        seams.append(('runs-either-side', [(w - 2, w - 1), (w + 1, w + 1)]))
    if N >= w + 7:
        seams.append(('across-the-seam', [(w - 4, w + 5)]))
    if N >= 30 + 3 * w + 1:
        seams.append(('three-words-from-bit-30', [(30, 30 + 3 * w - 1)]))
    if N >= 2 * w + 1:
        seams.append(('a-whole-word', [(w, 2 * w - 1)]))
    if N >= 6 * w + 40:                                  # a search backwards over more words than one load batch
        seams.append(('six-words-from-bit-10', [(10, 6 * w + 29)]))
    r0 = w - 1 if N >= w + 2 else m
    for name, spans in seams:
        runs = _runs_with(N, spans)
        X = none.copy()
        X[r0, :] = X[r0 + 1, :] = _mask_of_runs(runs)
        n0 = int(X[r0].sum())
        cross = [(n0, _runs_with(N, [(r0, r0 + 1)])), (N - n0, [(1, N)])]
        add(f'{name}-along-rows', X, {ROWS: [(2, runs), (N - 2, [(1, N)])], COLS: cross})
        add(f'{name}-along-cols', X.T, {ROWS: cross, COLS: [(2, runs), (N - 2, [(1, N)])]})
    return out


def check_pattern(look_of, name, U, want, N):
    """`look_of(U, t)` -> Chords with its histograms: the closed forms, then the model."""
    look = look_of(U, T)
    for d, lines in want.items():
        exp = expected_of(N, lines)
        got = look.hist[:, d]
        assert np.array_equal(got, exp), (name, N, DIRECTIONS[d], np.argwhere(got != exp)[:5])
    check_look(look, U < T, f"{name} N={N}")
    return look


# ---------------------------------------------------------------------------
# the numpy model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("N", [1, 2, 7, 64, 65])
def test_model_against_brute_force(N, density):
    rng = np.random.default_rng(1000 * N + int(100 * density))
    for _ in range(3):
        X = rng.random((N, N)) < density
        hist = chords.chord_histograms(mh.field_of(X), T)
        assert hist.dtype == np.int64 and hist.shape == (2, 2, 2, chords.bin_count(N))
        assert np.array_equal(hist, brute_force(X)), (N, density)
        assert not hist[..., 0].any()
        look = model_look(mh.field_of(X), T)
        check_look(look, X)
        c = np.arange(N + 1)
        for d in (ROWS, COLS):
            assert int((hist[:, d] * c).sum()) == N * N and N <= int(hist[:, d, CUT].sum()) <= 2 * N


@pytest.mark.parametrize("N", tile_sizes(tile_from_source()))
def test_patterns_with_known_answers(N):
    names = set()
    for name, U, want in patterns(N, tile_from_source()):
        check_pattern(model_look, name, U, want, N)
        names.add(name)
    w = tile_from_source()[0]
    assert ('across-the-seam-along-cols' in names) == (N >= w + 7)
    if N == tile_from_source()[2] + 1:
        assert 'three-words-from-bit-30-along-rows' in names and 'six-words-from-bit-10-along-cols' in names


def test_the_uniform_field_and_the_pixels_in_words():
    N = 9
    look = model_look(np.full((N, N), FG), T)
    for d in DIRECTIONS:
        assert look.count('below', d) == 0 and look.cut('below', d) == N and look.word('sum_cut', 'below', d) == N * N
        assert look.count('above', d) == 0 and look.cut('above', d) == 0
        assert look.mean('below', d) is None and look.mean_all('below', d) == N and look.max('below', d) is None
        assert look.max_all('below', d) == N and look.max_all('above', d) is None and look.mean_all('above', d) is None
    look = model_look(mh.field_of(np.indices((N, N)).sum(axis=0) % 2 == 0), T)       # the checkerboard
    assert look.count('below', 'rows') == (N * N + 1) // 2 - (N + 1) and look.mean('below', 'rows') == 1.0
    assert look.anisotropy('below') == 1.0 and look.mean_weighted('above', 'cols') == 1.0 and look.max('above', 'cols') == 1


@pytest.mark.parametrize("N", [8, 33])
def test_threshold_nan_and_one_ulp_fields(N):
    """The fields of test_morphology_host.hand_made: a pixel at the threshold and a NaN pixel are not phase 0; one ulp
    decides."""
    for name, U, t, want in mh.hand_made(N):
        X = np.nan_to_num(U, nan=np.inf) < t
        hist = chords.chord_histograms(U, t)
        assert np.array_equal(hist, brute_force(X)), name
        look = chords.Chords(chords.summary_of(hist), N, t, hist=hist)
        assert np.array_equal(chords.phase0(U, t), X)
        if 'n_A' in want:
            assert look.n('below') == want['n_A'], name
        if 'perimeter' in want:
            assert look.perimeter('below') == want['perimeter'], name
        if name == 'nan-pixel':
            assert look.n('above') == 1 and look.count('above', 'rows') == 1 and look.count('above', 'cols') == 1
        if name == 'one-ulp':
            assert look.n('below') == 1 and look.cut('below', 'cols') == 1 and look.count('below', 'rows') == 1
    U32 = np.full((8, 8), BG, dtype=np.float32)                     # the comparison is done in double on the stored element
    U32[1, 1] = np.float32(0.1)
    assert model_look(U32, 0.1).n('below') == 0 and model_look(U32, 0.1000001).n('below') == 1


@pytest.mark.parametrize("density", [0.2, 0.5, 0.7])
@pytest.mark.parametrize("N", [8, 33, 100])
def test_perimeter_and_area_are_the_morphologys(N, density):
    rng = np.random.default_rng(77 * N + int(100 * density))
    X = rng.random((N, N)) < density
    look = model_look(mh.field_of(X), T)
    mo = morphology.Morphology(morphology.quad_counts(mh.field_of(X), T), N, T)
    assert look.perimeter('below') == mo.perimeter and look.n('below') == mo.n_A
    mo = morphology.Morphology(morphology.quad_counts(mh.field_of(~X), T), N, T)
    assert look.perimeter('above') == mo.perimeter and look.n('above') == mo.n_A


@pytest.mark.parametrize("density", [0.3, 0.8])
def test_lineal_path_against_a_count_of_the_fitting_segments(density):
    N = 16
    X = np.random.default_rng(int(100 * density)).random((N, N)) < density
    X[3, :] = True                                                   # (a chord of N pixels: L(N) is not 0)
    look = model_look(mh.field_of(X), T)
    for phase, M in zip(PHASES, (X, ~X)):
        for d in DIRECTIONS:
            lines = M if d == 'rows' else M.T
            L = look.lineal_path(phase, d)
            assert L.dtype == np.float64 and L.shape == (N,)
            for r in range(1, N + 1):
                fit = sum(bool(lines[l, s:s + r].all()) for l in range(N) for s in range(N - r + 1))
                assert L[r - 1] == fit / (N * (N - r + 1)), (phase, d, r)
            assert L[0] == look.n(phase) / (N * N) and np.all(np.diff(L[:-1]) <= 0)
    assert look.lineal_path('below', 'rows')[-1] >= 1 / N
    assert chords.Chords(look.words, N, T).lineal_path('below', 'rows') is None


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_inscribed_disc_bounds_the_longest_chord(seed):
    """The widest point of a phase (chsimpy_amd/distance.py) has every pixel nearer than r_max in the phase: the
    offsets up to h = isqrt(d2max - 1) = ceil(r_max) - 1 along its row and its column, as far as the grid goes -- the
    walls are no background there, so the centre line of a disc at a wall is cut short by the wall.  Inside the grid
    that is 2 ceil(r_max) - 1 >= 2 r_max - 1 pixels of one chord."""
    from chsimpy_amd import distance
    N = 48
    rng = np.random.default_rng(seed)
    ii, jj = np.indices((N, N))
    X = np.zeros((N, N), dtype=bool)
    for _ in range(6):                                   # a few discs, some of them over a wall
        ci, cj, r = rng.integers(0, N), rng.integers(0, N), rng.integers(2, 9)
        X |= (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r
    U = mh.field_of(X)
    look = model_look(U, T)
    clipped = 0
    for phase in PHASES:
        D2 = distance.squared_distance(U, T, phase)
        di = distance.Distance(distance.summary_of(D2), N, T, phase)
        i, j = di.argmax
        h = math.isqrt(di.d2max - 1)
        assert h + 1 == math.ceil(di.r_max)
        for d, at in (('rows', j), ('cols', i)):
            assert min(at, h) + min(N - 1 - at, h) + 1 <= look.max_all(phase, d)
            if h <= at <= N - 1 - h:
                assert 2 * di.r_max - 1 <= 2 * h + 1 <= look.max_all(phase, d)
            else:
                clipped += 1
    U = np.full((N, N), FG)                              # the disc at the wall: r_max = N - 1, no chord longer than N
    U[:, N - 1] = BG
    di = distance.Distance(distance.summary_of(distance.squared_distance(U, T)), N, T)
    assert di.argmax == (0, 0) and 2 * di.r_max - 1 > N - 1 == model_look(U, T).max_all('below', 'rows')


def test_chords_object():
    N = 33
    X = np.random.default_rng(5).random((N, N)) < 0.6
    hist = chords.chord_histograms(mh.field_of(X), T)
    words = chords.summary_of(hist)
    co = chords.Chords(words, N, T, hist=hist, delx=0.25)
    bf = brute_force(X)
    for p, phase in enumerate(PHASES):
        for d, direction in enumerate(DIRECTIONS):
            inner = np.repeat(np.arange(N + 1), bf[p, d, INNER])
            both = np.repeat(np.arange(N + 1), bf[p, d, INNER] + bf[p, d, CUT])
            assert co.count(phase, direction) == inner.size == co.count(p, d) and co.cut(phase, direction) == both.size - inner.size
            assert co.mean(phase, direction) == int(inner.sum()) / inner.size
            assert co.mean_all(phase, direction) == int(both.sum()) / both.size
            assert co.mean_weighted(phase, direction) == int((inner * inner).sum()) / int(inner.sum())
            assert co.max(phase, direction) == inner.max() and co.max_all(phase, direction) == both.max()
            assert co.mean_phys(phase, direction) == co.mean(phase, direction) * 0.25
            for q in (0.0, 0.1, 0.5, 0.9, 1.0):
                assert co.quantile(q, phase, direction) == inner[max(1, math.ceil(q * inner.size)) - 1], q
            with pytest.raises(ValueError):
                co.quantile(1.5, phase, direction)
        assert co.anisotropy(phase) == co.mean(phase, 'rows') / co.mean(phase, 'cols')
        assert co.n(phase) == int((X if p == 0 else ~X).sum())
    bare = chords.Chords(words, N, T)
    assert bare.hist is None and bare.quantile(0.5, 'below', 'rows') is None and bare.max_all('below', 'rows') is None
    assert bare.mean_phys('below', 'rows') is None and bare.mean('below', 'rows') == co.mean('below', 'rows')
    assert 'Chords(N=33' in repr(co)
    # None where a denominator is zero
    one = model_look(np.full((8, 8), BG), T)
    assert one.n('below') == 0 and one.perimeter('below') == 0 and one.perimeter('above') == 32
    for d in DIRECTIONS:
        assert one.mean('below', d) is None and one.mean_all('below', d) is None and one.mean_weighted('below', d) is None
        assert one.max('below', d) is None and one.quantile(0.5, 'below', d) is None and one.mean_phys('below', d) is None
        assert one.mean('above', d) is None and one.mean_all('above', d) == 8.0
    assert one.anisotropy('below') is None and one.anisotropy('above') is None
    # the consistency checks
    ix = lambda name, phase, d: (phase * 2 + d) * 6 + chords.WORDS.index(name)
    w = words.copy()
    w[ix('sum_cut', 0, ROWS)] += 1
    with pytest.raises(ValueError, match='along the rows'):
        chords.Chords(w, N, T)
    w[ix('sum_cut', 0, COLS)] += 1
    with pytest.raises(ValueError, match='add to'):
        chords.Chords(w, N, T)
    w = words.copy()
    w[ix('n_cut', 1, COLS)] = 2 * N + 1
    with pytest.raises(ValueError, match='cut chords along the cols'):
        chords.Chords(w, N, T)
    w = chords.summary_of(chords.chord_histograms(np.full((N, N), FG), T))
    w[ix('n_cut', 0, ROWS)] = N - 1
    with pytest.raises(ValueError, match='cut chords along the rows'):
        chords.Chords(w, N, T)
    w = words.copy()
    w[ix('max_inner', 0, ROWS)] = 0
    with pytest.raises(ValueError, match='not the words'):
        chords.Chords(w, N, T)
    w = words.copy()
    w[ix('n_inner', 1, ROWS)] = -1
    with pytest.raises(ValueError):
        chords.Chords(w, N, T)
    bad = hist.copy()
    bad[0, 0, 0, 1] += 1
    with pytest.raises(ValueError, match='add up'):
        chords.Chords(words, N, T, hist=bad)
    bad = hist.copy()                                   # the same count and sum, another sum of squares
    k = int(np.flatnonzero(hist[0, 1, 0, :-2] * hist[0, 1, 0, 2:])[0])
    bad[0, 1, 0, k] -= 1
    bad[0, 1, 0, k + 2] -= 1
    bad[0, 1, 0, k + 1] += 2
    with pytest.raises(ValueError, match='add up'):
        chords.Chords(words, N, T, hist=bad)
    bad = hist.copy()
    bad[1, 0, 1, 0] = 1
    with pytest.raises(ValueError, match='length 0'):
        chords.Chords(words, N, T, hist=bad)
    with pytest.raises(ValueError, match='shape'):
        chords.Chords(words, N, T, hist=hist[..., :-1])
    with pytest.raises(ValueError, match='words are needed'):
        chords.Chords(words[:23], N, T)
    for bad in ('left', 2, True):
        with pytest.raises(ValueError):
            co.count(bad, 'rows')
        with pytest.raises(ValueError):
            co.count('below', bad)


def test_bad_arguments():
    U = np.zeros((8, 8))
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            chords.chord_histograms(U, bad)
    with pytest.raises(ValueError):
        chords.chord_histograms(np.zeros((8, 9)), 0.5)
    with pytest.raises(ValueError):
        chords.summary_of(np.zeros((2, 2, 9)))
    assert chords.bin_count(8) == 9 and chords.bin_count(1) == 2 and chords.bin_count(0) == 0 and chords.bin_count(-2) == 0


# ---------------------------------------------------------------------------
# header, binding, experiment
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_CH_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_CH_WORDS'] == chords.CHS_CH_WORDS == _lib.CHS_CH_WORDS == 4 * len(chords.WORDS) == 24
    for i, w in enumerate(chords.WORDS):
        assert defs['CHS_CH_' + w.upper()] == getattr(chords, 'CHS_CH_' + w.upper()) == i
    assert (defs['CHS_CH_ROWS'], defs['CHS_CH_COLS']) == (chords.CHS_CH_ROWS, chords.CHS_CH_COLS) == (0, 1)
    assert (defs['CHS_CH_INNER'], defs['CHS_CH_CUT']) == (chords.CHS_CH_INNER, chords.CHS_CH_CUT) == (0, 1)
    assert 16384 ** 3 < 2 ** 63                                      # N of chs_create is at most 16384
    w, g, l = tile_from_source()
    assert w == 64 and g % 64 == 0 and 3 <= l <= 2048


_CTYPES = dict(mh._CTYPES)
_CTYPES['int32_t*'] = ctypes.POINTER(ctypes.c_int32)
CH_SYMBOLS = ['chs_chords_bins', 'chs_chords', 'chs_chords_hist', 'chs_chords_last_ms', 'chs_chords_tile',
              'chs_batch_chords', 'chs_batch_chords_hist']


@pytest.mark.parametrize("name", CH_SYMBOLS)
def test_the_prototypes_match_the_header(hip_lib, name):
    """The argument and return types the binding declares are those of the prototype in include/chs_hip.h."""
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'^\s*(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr, flags=re.M)
    assert m, f"{name}: no prototype in the header"
    ret, args = m.group(1), [a.strip() for a in m.group(2).split(',')]
    want = []
    for a in args:
        a = re.sub(r'\[\w*\]$', '*', a)
        t = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)\s*\w*\s*(\*?)$', a)
        assert t, a
        want.append(_CTYPES[t.group(1) + ('*' if (t.group(2) or t.group(3)) else '')])
    fn = getattr(hip_lib, name)
    assert name in _lib.SYMBOLS
    assert list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert ctypes.sizeof(fn.restype) == ctypes.sizeof(_CTYPES[ret])


def test_entry_points_that_need_no_device(hip_lib):
    assert _lib.chords_tile() == tile_from_source()
    w = ctypes.c_int32(0)
    assert hip_lib.chs_chords_tile(None, None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_chords_tile(ctypes.byref(w), ctypes.byref(w), None) == _lib.CHS_EINVAL
    for N in (1, 2, 8, 33, 100, 513, 4096, 16384):
        assert hip_lib.chs_chords_bins(N) == _lib.chords_bins(N) == chords.bin_count(N) == N + 1
    assert hip_lib.chs_chords_bins(0) == 0 and hip_lib.chs_chords_bins(-3) == 0
    out = np.zeros(24, dtype=np.int64)
    assert hip_lib.chs_chords(None, 0.5, _lib._i64ptr(out)) == _lib.CHS_EINVAL
    assert hip_lib.chs_chords_hist(None, 9, _lib._i64ptr(out)) == _lib.CHS_EINVAL
    assert hip_lib.chs_chords_last_ms(None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_chords(None, 0, 0.5, _lib._i64ptr(out)) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_chords_hist(None, 9, _lib._i64ptr(out)) == _lib.CHS_EINVAL


def _chords_checks(text, rows):
    from chsimpy_amd import experiment
    lines = text.splitlines()
    assert lines[0] == 'id,threshold,' + ','.join(f"{k}_{p}_{d}" for p in PHASES for d in DIRECTIONS
                                                  for k in ('count', 'mean', 'mean_weighted', 'max', 'cut'))
    assert lines[0] == ','.join(experiment.CHORDS_COLS) and len(lines) == 1 + rows
    assert [ln.split(',')[0] for ln in lines[1:]] == [str(i) for i in range(rows)]
    for ln in lines[1:]:
        f = ln.split(',')
        i = int(f[0])
        assert len(f) == 22 and int(f[2]) == i + 1 and float(f[3]) == 3.0 and float(f[4]) == 10.0 / 3.0 and int(f[5]) == 4
        assert int(f[7]) == i + 2 and float(f[18]) == 0.1 * (i + 1) and float(f[19]) == 1.0 / (i + 3) and int(f[21]) == 17
        for k in range(4):
            g = f[2 + 5 * k:7 + 5 * k]
            assert '.' not in g[0] and '.' in g[1] and '.' in g[2] and '.' not in g[3] and '.' not in g[4]


def test_experiment_writes_the_chords_file_on_a_dry_run(tmp_path):
    """--chords adds <id>-chords.csv and leaves the result files byte for byte what they are without it, member by
    member and in batches (members without device work: launcher, gather and writer alone)."""
    from chsimpy_amd import experiment
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'plain', '--widths'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'chord', '--widths', '--chords'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'batch', '--batch', '2', '--chords'])
    finally:
        os.chdir(cwd)
    assert not (tmp_path / 'plain-chords.csv').exists() and not (tmp_path / 'batch-widths.csv').exists()
    text = (tmp_path / 'chord-chords.csv').read_text()
    _chords_checks(text, 3)
    assert (tmp_path / 'batch-chords.csv').read_text() == text
    for kind in ('results.csv', 'results-agg.csv', 'widths.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'chord-{kind}').read_bytes()
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'batch-{kind}').read_bytes()
    nan = float('nan')
    row = (0, 0.5, 0, nan, nan, 0, 8) + (3, 2.0, 2.5, 3, 1) * 2 + (1, 0.1, 1.0 / 3.0, 7, 0)
    assert experiment.write_chords(str(tmp_path / 'w'), [row]).endswith('w-chords.csv')
    assert (tmp_path / 'w-chords.csv').read_text().splitlines()[1] == (
        '0,0.5,0,nan,nan,0,8,3,2.0,2.5,3,1,3,2.0,2.5,3,1,1,0.1,0.3333333333333333,7,0')

    class _Solver:                                       # what _chords_of reads off a solver
        def __init__(self, U):
            self.U = U

        def chords(self, hist=True):
            assert hist is False
            return chords.Chords(chords.summary_of(chords.chord_histograms(self.U, T)), self.U.shape[0], T)
    U = mh.field_of(np.random.default_rng(2).random((16, 16)) < 0.5)
    co = model_look(U, T)
    got = experiment._chords_of(_Solver(U))
    assert len(got) == 21 and got[0] == T
    assert got[1:6] == (co.count('below', 'rows'), co.mean('below', 'rows'), co.mean_weighted('below', 'rows'),
                        co.max('below', 'rows'), co.cut('below', 'rows'))
    assert got[16:21] == (co.count('above', 'cols'), co.mean('above', 'cols'), co.mean_weighted('above', 'cols'),
                          co.max('above', 'cols'), co.cut('above', 'cols'))
    empty = experiment._chords_of(_Solver(np.full((8, 8), BG)))
    assert empty[1] == 0 and math.isnan(empty[2]) and math.isnan(empty[3]) and empty[4:6] == (0, 0) and empty[15] == 8


def test_experiment_chords_under_gloo_at_world_2(tmp_path):
    """`--gpus 2 --backend gloo --dry-run --chords`: two ranks gather their members' rows; rank 0 writes the file a
    single rank writes."""
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    base = ['-N', '16', '-K', '3e-4', '-R', '7', '--dry-run', '--backend', 'gloo', '--chords']
    r2 = subprocess.run([sys.executable, '-m', 'chsimpy_amd.experiment', '--gpus', '2', '--file-id', str(tmp_path / 'c2')] + base,
                        env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-3000:]
    r1 = subprocess.run([sys.executable, '-m', 'chsimpy_amd.experiment', '--file-id', str(tmp_path / 'c1')] + base,
                        env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r1.returncode == 0, r1.stderr[-3000:]
    text = (tmp_path / 'c2-chords.csv').read_text()
    _chords_checks(text, 7)
    assert text == (tmp_path / 'c1-chords.csv').read_text()
    assert 'ranks, 2' in (tmp_path / 'c2-metadata.csv').read_text() and 'c2-chords.csv' in r2.stdout
