"""Exact Euclidean distance transform of the thresholded field -- domain half-widths, the widest point, the histogram of
local radii ("pore size distribution"): the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_distance).

Foreground.  Exactly that of `components`: for an N x N field U and a finite threshold t, ``side='below'`` is
``X[i][j] = ((double)U[i][j] < t)`` (a NaN pixel and a pixel equal to t are background); ``side='above'`` is the
complement inside the grid.

Squared distance.  ``D2[i][j]``, an int32, is 0 for a background pixel and, for a foreground pixel, the minimum over all
background pixels (k, l) of the grid of ``(i-k)**2 + (j-l)**2``.  No wrap-around, and the box walls are not background
(the convention of ``scipy.ndimage.distance_transform_edt``).  A grid without any background pixel has
``D2 = CHS_DT_INF = 1 << 30`` everywhere: above ``2*(N-1)**2`` for every N a handle takes, and small enough that
``d*d + CHS_DT_INF`` stays inside int32.

Radius bin.  ``k = isqrt(D2)``, ``k*k <= D2 < (k+1)*(k+1)``, in integers.

Histogram.  ``hist[k]``, int64: the foreground pixels in bin k; its length is ``bin_count(N) = isqrt(2*(N-1)**2) + 1``;
CHS_DT_INF pixels are in no bin.

Summary.  Five int64 words (`WORDS`): ``fg``, the foreground pixels; ``d2max``, the largest D2 over the foreground
pixels with D2 < CHS_DT_INF (0 without one); ``d2max_first``, the smallest linear index ``i*N + j`` attaining it (-1
without one); ``sumd2``, the sum of D2 over those same pixels; ``ninf``, the pixels with D2 == CHS_DT_INF: 0 or N*N.
"""
import math

import numpy as np

from . import components

WORDS = ('fg', 'd2max', 'd2max_first', 'sumd2', 'ninf')
CHS_DT_WORDS = len(WORDS)
CHS_DT_FG, CHS_DT_D2MAX, CHS_DT_D2MAX_FIRST, CHS_DT_SUMD2, CHS_DT_NINF = range(CHS_DT_WORDS)
CHS_DT_INF = 1 << 30

side_code = components.side_code
foreground = components.foreground


def bin_count(N):
    """The length of the histogram: isqrt(2 (N-1)^2) + 1 (chs_distance_bins)."""
    N = int(N)
    return math.isqrt(2 * (N - 1) * (N - 1)) + 1 if N >= 1 else 0


def radius_bins(D2):
    """k = isqrt(D2) element by element, in integers: k*k <= D2 < (k+1)*(k+1).  An int64 array."""
    d = np.asarray(D2, dtype=np.int64)
    if np.any(d < 0):
        raise ValueError("a squared distance is not negative")
    k = np.sqrt(d.astype(np.float64)).astype(np.int64)
    k -= k * k > d                                   # (the float root is off by one at most)
    k += (k + 1) * (k + 1) <= d
    return k


def squared_distance(U, threshold, side='below'):
    """D2 int32 [N][N] of the field U: the numpy model of chs_distance, the two passes of the kernels.

    Vertical: ``G[i][j] = min(i - up, down - i)`` with the nearest background rows of column j at or above and at or
    below row i -- a running maximum down the column and a running minimum up it -- CHS_DT_INF without one.
    Horizontal, with ``h = G**2`` (INF stays INF): ``best = h[j]``; for d = 1, 2, ...: a pixel is settled once
    ``d*d >= best`` -- `best` never rises and every candidate at distance d is at least d*d -- else
    ``best = min(best, d*d + h[j-d], d*d + h[j+d])`` over the sides inside the row."""
    if not math.isfinite(float(threshold)):
        raise ValueError("the threshold must be finite")
    X = foreground(U, threshold, side)
    if X.ndim != 2 or X.shape[0] != X.shape[1]:
        raise ValueError(f"a square field is needed, got shape {X.shape}")
    N = X.shape[0]
    INF = CHS_DT_INF
    rows = np.arange(N, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(~X, rows, -INF), axis=0)
    down = np.minimum.accumulate(np.where(~X, rows, 2 * INF)[::-1], axis=0)[::-1]
    G = np.minimum(np.minimum(rows - up, down - rows), INF)
    best = np.where(G >= INF, INF, np.minimum(G, 1 << 15) ** 2)
    h = best.copy()
    for d in range(1, N):
        live = d * d < best
        if not live.any():
            break
        cand = np.full_like(h, 2 * INF)
        cand[:, d:] = h[:, :-d]                      # h[j - d]
        cand[:, :-d] = np.minimum(cand[:, :-d], h[:, d:])   # h[j + d]
        best = np.where(live, np.minimum(best, d * d + cand), best)
    return best.astype(np.int32)


def histogram_of(D2):
    """hist int64 [bin_count(N)] of a squared-distance map: the foreground pixels (D2 > 0) below CHS_DT_INF by bin."""
    D2 = np.asarray(D2)
    d = D2[(D2 > 0) & (D2 < CHS_DT_INF)]
    return np.bincount(radius_bins(d), minlength=bin_count(D2.shape[0])).astype(np.int64)


def summary_of(D2):
    """The five summary words of a squared-distance map, an int64 array."""
    D2 = np.asarray(D2, dtype=np.int64)
    flat = D2.ravel()
    fin = (flat > 0) & (flat < CHS_DT_INF)
    w = np.zeros(CHS_DT_WORDS, dtype=np.int64)
    w[CHS_DT_FG] = np.count_nonzero(flat > 0)
    w[CHS_DT_NINF] = np.count_nonzero(flat >= CHS_DT_INF)
    w[CHS_DT_D2MAX_FIRST] = -1
    if fin.any():
        w[CHS_DT_D2MAX] = flat[fin].max()
        w[CHS_DT_D2MAX_FIRST] = np.flatnonzero(fin & (flat == w[CHS_DT_D2MAX]))[0]
        w[CHS_DT_SUMD2] = flat[fin].sum()
    return w


class Distance:
    """One look at the distance transform of a field: ``fg, d2max, d2max_first, sumd2, ninf`` (Python integers),
    ``hist`` (None unless fetched), ``d2`` (the map, None unless fetched), and derived from them ``r_max`` (the radius
    of the largest disc that fits into the phase, in pixels), ``r_max_phys`` (times ``delx``), ``r2_mean``,
    ``r_floor_mean``, ``argmax`` (row, column of the widest point) and ``quantile(q)`` of the radius bins -- None where a
    denominator is zero or the input is missing -- beside ``N``, ``threshold``, ``side``."""

    def __init__(self, words, N, threshold, side='below', hist=None, d2=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.side = 'above' if side_code(side) == components.CHS_CC_ABOVE else 'below'
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_DT_WORDS,):
            raise ValueError(f"{CHS_DT_WORDS} words are needed, got shape {self.words.shape}")
        self.fg, self.d2max, self.d2max_first, self.sumd2, self.ninf = (int(w) for w in self.words)
        n2 = self.N * self.N
        if self.ninf not in (0, n2):
            raise ValueError(f"ninf is 0 or N*N, got {self.ninf}")
        finite = self.fg - self.ninf
        if not (0 <= self.fg <= n2 and finite >= 0 and 0 <= self.d2max <= 2 * (self.N - 1) ** 2
                and (finite == 0) == (self.d2max_first == -1) == (self.d2max == 0) and -1 <= self.d2max_first < n2
                and finite <= self.sumd2 <= finite * self.d2max):   # (every finite foreground pixel has D2 >= 1)
            raise ValueError(f"not the summary of a distance transform: {self.words}")
        self.hist = None
        if hist is not None:
            self.hist = np.array(hist, dtype=np.int64)
            if self.hist.shape != (bin_count(self.N),):
                raise ValueError(f"a histogram of {bin_count(self.N)} bins is needed, got shape {self.hist.shape}")
            if np.any(self.hist < 0) or int(self.hist.sum()) != finite:
                raise ValueError(f"the histogram adds up to {int(self.hist.sum())}, not to fg - ninf = {finite}")
            top = math.isqrt(self.d2max)
            if np.any(self.hist[top + 1:] != 0) or (finite and self.hist[top] == 0) or self.hist[0] != 0:
                raise ValueError(f"the histogram's last occupied bin is not isqrt(d2max) = {top}")
        self.d2 = None
        if d2 is not None:
            self.d2 = np.asarray(d2, dtype=np.int32)
            if self.d2.shape != (self.N, self.N):
                raise ValueError(f"a map of shape {(self.N, self.N)} is needed, got {self.d2.shape}")
            if not np.array_equal(summary_of(self.d2), self.words):
                raise ValueError(f"the map's summary is {summary_of(self.d2)}, the words are {self.words}")
            if self.hist is not None and not np.array_equal(histogram_of(self.d2), self.hist):
                raise ValueError("the map's histogram is not the one given")

    @property
    def finite(self):
        """The foreground pixels with a finite distance: what the means and the histogram are over."""
        return self.fg - self.ninf

    @property
    def r_max(self):
        return math.sqrt(self.d2max) if self.finite else None

    @property
    def r_max_phys(self):
        return None if (self.r_max is None or self.delx is None) else self.r_max * self.delx

    @property
    def r2_mean(self):
        return self.sumd2 / self.finite if self.finite else None

    @property
    def r_floor_mean(self):
        if self.hist is None or not self.finite:
            return None
        return int(np.dot(np.arange(len(self.hist), dtype=np.int64), self.hist)) / self.finite

    @property
    def argmax(self):
        return divmod(self.d2max_first, self.N) if self.d2max_first >= 0 else None

    def quantile(self, q):
        """The smallest radius bin k with at least the fraction q of the finite foreground pixels in bins <= k."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q is in [0, 1], got {q!r}")
        if self.hist is None or not self.finite:
            return None
        need = max(1, math.ceil(q * self.finite))
        return int(np.searchsorted(np.cumsum(self.hist), need, side='left'))

    def __repr__(self):
        return (f"Distance(N={self.N}, threshold={self.threshold!r}, side={self.side!r}, fg={self.fg}, d2max={self.d2max}, "
                f"argmax={self.argmax}, ninf={self.ninf})")
