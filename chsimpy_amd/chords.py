"""Chord lengths (linear intercepts) of both phases of the thresholded field, along rows and along columns, and the
lineal-path function that follows from them: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_chords).

For the N x N field U and a finite threshold t:

Phases.  Phase 0 (``'below'``) is the foreground of `components` with ``side='below'``: ``X[i][j] = ((double)U[i][j] <
t)``; a NaN pixel and a pixel equal to t are not phase 0.  Phase 1 (``'above'``) is the complement inside the grid.
There is no side argument: one look gives both.

Directions.  ``CHS_CH_ROWS = 0`` (``'rows'``): the lines are the rows, a chord runs along j.  ``CHS_CH_COLS = 1``
(``'cols'``): the lines are the columns, a chord runs along i.

Chord.  A maximal run of consecutive pixels of one phase within one line; its length c is in [1, N].  No wrap-around.

Classes.  ``CHS_CH_INNER = 0``: both ends are bounded by the other phase.  ``CHS_CH_CUT = 1``: the chord touches a wall:
it begins at index 0, or ends at N-1, or both; a run of length N is one cut chord.

Histogram.  ``hist[phase][dir][cls][c]``, int64, 2*2*2*(N+1) entries in that order: the chords of length c.  Bin 0 is
always 0.  ``bin_count(N) = N + 1``, and 0 for N < 1.

Summary.  ``CHS_CH_WORDS = 24`` int64 words, six per (phase, dir) in the order phase, dir (`WORDS`): ``n_inner,
sum_inner, sum2_inner, max_inner, n_cut, sum_cut`` -- the count, the sum of c, the sum of c*c and the largest c of the
class (0 without one).  The largest value is N**3, inside int64 for every N a handle takes.
"""
import math

import numpy as np

WORDS = ('n_inner', 'sum_inner', 'sum2_inner', 'max_inner', 'n_cut', 'sum_cut')
CHS_CH_N_INNER, CHS_CH_SUM_INNER, CHS_CH_SUM2_INNER, CHS_CH_MAX_INNER, CHS_CH_N_CUT, CHS_CH_SUM_CUT = range(len(WORDS))
CHS_CH_WORDS = 4 * len(WORDS)
CHS_CH_ROWS, CHS_CH_COLS = 0, 1
CHS_CH_INNER, CHS_CH_CUT = 0, 1
PHASES = ('below', 'above')
DIRECTIONS = ('rows', 'cols')


def phase_code(phase):
    """0 for ``'below'`` (or 0), 1 for ``'above'`` (or 1)."""
    if phase in PHASES:
        return PHASES.index(phase)
    if phase in (0, 1) and not isinstance(phase, bool):
        return int(phase)
    raise ValueError(f"the phase is 'below' (0) or 'above' (1), got {phase!r}")


def direction_code(direction):
    """CHS_CH_ROWS for ``'rows'`` (or 0), CHS_CH_COLS for ``'cols'`` (or 1)."""
    if direction in DIRECTIONS:
        return DIRECTIONS.index(direction)
    if direction in (0, 1) and not isinstance(direction, bool):
        return int(direction)
    raise ValueError(f"the direction is 'rows' (0) or 'cols' (1), got {direction!r}")


def bin_count(N):
    """The bins of one of the eight histograms: N + 1 (chs_chords_bins)."""
    N = int(N)
    return N + 1 if N >= 1 else 0


def phase0(U, threshold):
    """The boolean image of phase 0: the element widened to double, then ``< threshold``."""
    if not math.isfinite(float(threshold)):
        raise ValueError("the threshold must be finite")
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1] or U.shape[0] < 1:
        raise ValueError(f"a square field is needed, got shape {U.shape}")
    with np.errstate(invalid='ignore'):
        return U.astype(np.float64) < float(threshold)


def _line_histograms(M):
    """[cls][c] int64 of the runs of True along axis 1 of the boolean array M (N lines of N pixels)."""
    N = M.shape[0]
    d = np.diff(np.pad(M.astype(np.int8), ((0, 0), (1, 1))), axis=1)   # [N][N + 1]: +1 where a run starts, -1 behind its end
    start = np.nonzero(d == 1)[1]                  # (row-major: the k-th start and the k-th end are one run's)
    end = np.nonzero(d == -1)[1]
    cut = (start == 0) | (end == N)
    return np.bincount((end - start) + cut * (N + 1), minlength=2 * (N + 1)).astype(np.int64).reshape(2, N + 1)


def chord_histograms(U, threshold):
    """hist int64 [phase][dir][cls][N + 1] of the field U: the numpy model of chs_chords."""
    X = phase0(U, threshold)
    N = X.shape[0]
    hist = np.zeros((2, 2, 2, N + 1), dtype=np.int64)
    for phase, M in enumerate((X, ~X)):
        hist[phase, CHS_CH_ROWS] = _line_histograms(M)
        hist[phase, CHS_CH_COLS] = _line_histograms(np.ascontiguousarray(M.T))
    return hist


def summary_of(hist):
    """The 24 summary words of the eight histograms, an int64 array."""
    hist = np.asarray(hist, dtype=np.int64)
    if hist.ndim != 4 or hist.shape[:3] != (2, 2, 2):
        raise ValueError(f"histograms of shape (2, 2, 2, N + 1) are needed, got {hist.shape}")
    c = np.arange(hist.shape[3], dtype=np.int64)
    w = np.zeros((2, 2, len(WORDS)), dtype=np.int64)
    for phase in range(2):
        for d in range(2):
            inner, cut = hist[phase, d, CHS_CH_INNER], hist[phase, d, CHS_CH_CUT]
            w[phase, d] = (inner.sum(), (inner * c).sum(), (inner * c * c).sum(),
                           c[inner > 0].max() if (inner > 0).any() else 0, cut.sum(), (cut * c).sum())
    return w.reshape(CHS_CH_WORDS)


class Chords:
    """One look at the chord lengths of a field: ``words`` (int64 [24]; ``word(name, phase, direction)`` picks one),
    ``hist`` (int64 [2][2][2][N + 1], None unless fetched), and per ``phase in ('below', 'above')`` and ``direction in
    ('rows', 'cols')``: ``count`` (the inner chords), ``cut`` (the chords at a wall), ``mean`` (inner chords only, the
    stereological convention), ``mean_all`` (both classes), ``mean_weighted`` (the sum of c*c over the sum of c, inner),
    ``max`` (the longest inner chord), ``max_all`` (of both classes; needs the histogram), ``mean_phys`` (``mean`` times
    ``delx``), ``quantile(q, ...)`` (inner, from the histogram) and ``lineal_path(...)``; per phase ``n`` (its pixels),
    ``perimeter`` and ``anisotropy`` -- None where a denominator is zero or the input is missing -- beside ``N``,
    ``threshold``, ``delx``."""

    def __init__(self, words, N, threshold, hist=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_CH_WORDS,):
            raise ValueError(f"{CHS_CH_WORDS} words are needed, got shape {self.words.shape}")
        N, n2 = self.N, self.N * self.N
        w = self.words.reshape(2, 2, len(WORDS))
        pixels = w[:, :, CHS_CH_SUM_INNER] + w[:, :, CHS_CH_SUM_CUT]          # [phase][dir]
        for phase in range(2):
            if pixels[phase, 0] != pixels[phase, 1]:
                raise ValueError(f"phase {PHASES[phase]} has {pixels[phase, 0]} pixels along the rows and "
                                 f"{pixels[phase, 1]} along the columns")
        if int(pixels[0, 0] + pixels[1, 0]) != n2:
            raise ValueError(f"the two phases add to {int(pixels[0, 0] + pixels[1, 0])} pixels, not to N*N = {n2}")
        for d in range(2):
            cut = int(w[0, d, CHS_CH_N_CUT] + w[1, d, CHS_CH_N_CUT])
            if not N <= cut <= 2 * N:
                raise ValueError(f"{cut} cut chords along the {DIRECTIONS[d]}: not in [N, 2 N]")
        for phase in range(2):
            for d in range(2):
                ni, si, s2, mx, nc, sc = (int(v) for v in w[phase, d])
                if not (min(ni, si, s2, mx, nc, sc) >= 0 and ni <= si <= ni * mx and si <= s2 <= si * mx and mx <= N
                        and (ni == 0) == (mx == 0) and nc <= sc <= nc * N):
                    raise ValueError(f"not the words of a chord count ({PHASES[phase]}, {DIRECTIONS[d]}): {w[phase, d]}")
        self.hist = None
        if hist is not None:
            self.hist = np.array(hist, dtype=np.int64)
            if self.hist.shape != (2, 2, 2, bin_count(N)):
                raise ValueError(f"histograms of shape {(2, 2, 2, bin_count(N))} are needed, got {self.hist.shape}")
            if np.any(self.hist < 0) or np.any(self.hist[..., 0] != 0):
                raise ValueError("a histogram has a negative bin or a chord of length 0")
            if not np.array_equal(summary_of(self.hist), self.words):
                raise ValueError(f"the histograms add up to {summary_of(self.hist)}, the words are {self.words}")

    def word(self, name, phase, direction):
        """One summary word as a Python integer: ``name`` is one of `WORDS`."""
        return int(self.words[(phase_code(phase) * 2 + direction_code(direction)) * len(WORDS) + WORDS.index(name)])

    def count(self, phase, direction):
        return self.word('n_inner', phase, direction)

    def cut(self, phase, direction):
        return self.word('n_cut', phase, direction)

    def n(self, phase):
        """The pixels of the phase: every one of them is in exactly one chord of a direction."""
        return self.word('sum_inner', phase, 0) + self.word('sum_cut', phase, 0)

    def mean(self, phase, direction):
        k = self.count(phase, direction)
        return self.word('sum_inner', phase, direction) / k if k else None

    def mean_all(self, phase, direction):
        k = self.count(phase, direction) + self.cut(phase, direction)
        return self.n(phase) / k if k else None

    def mean_weighted(self, phase, direction):
        s = self.word('sum_inner', phase, direction)
        return self.word('sum2_inner', phase, direction) / s if s else None

    def max(self, phase, direction):
        return self.word('max_inner', phase, direction) if self.count(phase, direction) else None

    def max_all(self, phase, direction):
        if self.hist is None:
            return None
        both = self.hist[phase_code(phase), direction_code(direction)].sum(axis=0)
        return int(np.flatnonzero(both)[-1]) if both.any() else None

    def mean_phys(self, phase, direction):
        m = self.mean(phase, direction)
        return None if (m is None or self.delx is None) else m * self.delx

    def anisotropy(self, phase):
        """The mean inner chord along the rows over the one along the columns."""
        r, c = self.mean(phase, 'rows'), self.mean(phase, 'cols')
        return None if (r is None or c is None) else r / c

    def perimeter(self, phase):
        """Every chord has two ends, and each end is a unit edge to the other phase or to the ring around the grid:
        2 (chords along the rows + chords along the columns), both classes.  `Morphology.perimeter` for 'below'."""
        return 2 * sum(self.count(phase, d) + self.cut(phase, d) for d in DIRECTIONS)

    def quantile(self, q, phase, direction):
        """The smallest length c with at least the fraction q of the inner chords at lengths <= c."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q is in [0, 1], got {q!r}")
        k = self.count(phase, direction)
        if self.hist is None or not k:
            return None
        need = max(1, math.ceil(q * k))
        inner = self.hist[phase_code(phase), direction_code(direction), CHS_CH_INNER]
        return int(np.searchsorted(np.cumsum(inner), need, side='left'))

    def lineal_path(self, phase, direction):
        """L(r) for r = 1 ... N, a float64 array: the probability that a segment of r pixels, placed on a line of the
        direction wholly inside the grid, lies wholly in the phase: ``sum_c max(c - r + 1, 0) n(c) / (N (N - r + 1))``
        over inner and cut chords together, the numerator in exact integers.  L(1) is the area fraction."""
        if self.hist is None:
            return None
        N = self.N
        n = self.hist[phase_code(phase), direction_code(direction)].sum(axis=0)[1:]      # n(c), c = 1 ... N
        c = np.arange(1, N + 1, dtype=np.int64)
        chords_from = np.cumsum(n[::-1])[::-1]                                            # sum over c >= r of n(c)
        pixels_from = np.cumsum((n * c)[::-1])[::-1]                                      # ... of c n(c)
        num = pixels_from - (c - 1) * chords_from
        return num.astype(np.float64) / (N * (N - c + 1)).astype(np.float64)

    def __repr__(self):
        return (f"Chords(N={self.N}, threshold={self.threshold!r}, n_below={self.n('below')}, "
                + ', '.join(f"mean_{p}_{d}={self.mean(p, d)}" for p in PHASES for d in DIRECTIONS) + ')')
