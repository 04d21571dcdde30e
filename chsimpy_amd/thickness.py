"""Local thickness of a phase of the thresholded field -- for every pixel the radius of the largest disc that fits inside
the phase and covers it (Hildebrand and Rueegsegger), its area-weighted histogram (the pore-size or strut-size
distribution) and the mean domain width: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_thickness).

Foreground and squared distance.  Exactly those of `distance`: ``side``, the NaN and threshold conventions, walls that are
no background, ``CHS_DT_INF`` on a grid without background.

Local thickness.  ``T2[p]``, an int32, is 0 on the background and, for a foreground pixel p,
``max { D2[c] : c foreground, D2[c] < CHS_DT_INF, |p - c|**2 < D2[c] }``: the open disc of squared radius ``D2[c]`` about
c holds no background pixel.  Discs are clipped at the walls; a disc may poke out of the grid.  A grid without background
has ``T2 = CHS_DT_INF`` everywhere, with ``kept = work = 0``.

Radius bin and histogram.  ``k = isqrt(T2)``; ``hist[k]``, int64, with ``distance.bin_count(N)`` bins; INF pixels are in
no bin.

The centres that are painted.  ``E(R, a, b)`` (`reach`) is the maximum of ``|q - (a, b)|**2`` over the lattice points q
with ``|q|**2 < R``: one function for the four axis neighbours, one for the four diagonal ones.  A centre c with
``R = D2[c]`` is dropped iff one of its 8 neighbours ``c' = c + (a, b)`` inside the grid is foreground, has a finite D2
and ``D2[c'] > E(R, a, b)``; the disc of c then lies inside that of c'.  ``E >= R``, so D2 rises strictly along a chain of
drops and every chain ends at a kept centre: the map does not depend on the rule, ``kept`` and ``work`` do.  With
``rho(R) = isqrt(R - 1)``, ``work`` is the sum over the kept centres of ``(2 rho + 1)**2``.

Summary.  Seven int64 words (`WORDS`): ``fg``; ``t2max``, the largest finite T2 (0 without one); ``nmax``, the pixels
attaining it; ``sumt2`` over the finite foreground; ``ninf``, 0 or N*N; ``kept``; ``work``.
"""
import math

import numpy as np

from . import components, distance

WORDS = ('fg', 't2max', 'nmax', 'sumt2', 'ninf', 'kept', 'work')
CHS_TH_WORDS = len(WORDS)
CHS_TH_FG, CHS_TH_T2MAX, CHS_TH_NMAX, CHS_TH_SUMT2, CHS_TH_NINF, CHS_TH_KEPT, CHS_TH_WORK = range(CHS_TH_WORDS)
CHS_DT_INF = distance.CHS_DT_INF
CHS_ELIMIT = -6

side_code = components.side_code
bin_count = distance.bin_count
radius_bins = distance.radius_bins


def rho_of(R):
    """The largest integer rho with rho**2 < R, element by element (R >= 1): isqrt(R - 1)."""
    return radius_bins(np.asarray(R, dtype=np.int64) - 1)


def reach(R, diagonal=False):
    """E(R, axis) or E(R, diagonal): the maximum of ``|q - (a, b)|**2`` over the lattice points q with ``|q|**2 < R`` for
    (a, b) = (1, 0) or (1, 1); 0 for R < 1.  Every column x of the open disc, -rho <= x <= rho, ends at
    ``y(x) = isqrt(R - 1 - x*x)``, and the farthest points from (a, b) are column ends on the far side."""
    R = int(R)
    if R < 1:
        return 0
    rho = math.isqrt(R - 1)
    x = np.arange(rho + 1, dtype=np.int64)
    y = radius_bins(R - 1 - x * x)
    if diagonal:
        return int((x * x + y * y + 2 * (x + y) + 2).max())       # q = (-x, -y)
    return int((x * x + y * y + 2 * x + 1).max())                 # q = (-x, +-y)


def _shift_max(D, offsets):
    """Element by element the maximum of D over the neighbours at the given offsets, those outside the grid left out."""
    N = D.shape[0]
    pad = np.zeros((N + 2, N + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = D
    out = np.zeros_like(D)
    for a, b in offsets:
        np.maximum(out, pad[1 + a:N + 1 + a, 1 + b:N + 1 + b], out=out)
    return out


def kept_centres(D2):
    """The boolean map of the centres the pruning rule keeps, from a squared-distance map."""
    D = np.asarray(D2, dtype=np.int64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"a square map is needed, got shape {D.shape}")
    centre = (D > 0) & (D < CHS_DT_INF)
    if not centre.any():
        return centre
    ma = _shift_max(D, ((-1, 0), (1, 0), (0, -1), (0, 1)))
    md = _shift_max(D, ((-1, -1), (-1, 1), (1, -1), (1, 1)))
    values = np.unique(D[centre])
    ea = np.array([reach(R, False) for R in values], dtype=np.int64)
    ed = np.array([reach(R, True) for R in values], dtype=np.int64)
    at = np.searchsorted(values, np.where(centre, D, values[0]))
    return centre & ~(ma > ea[at]) & ~(md > ed[at])


PAINT_SMALL_RHO = 8     # paint: discs up to this rho go offset by offset, all centres at once; larger ones disc by disc


def paint(D2, centres):
    """T2 int32 [N][N]: the discs of the given centres (a boolean map) painted by maximum over a zero map.  The small
    discs offset by offset: every centre whose disc holds the offset raises the pixel there; the centres are sorted by R,
    so where several of one offset meet in a pixel the last one written is the largest.  The large discs one by one, over
    their bounding box clipped to the grid."""
    D = np.asarray(D2, dtype=np.int64)
    N = D.shape[0]
    T2 = np.zeros(N * N, dtype=np.int64)
    ci, cj = np.nonzero(centres)
    if ci.size == 0:
        return T2.reshape(N, N).astype(np.int32)
    R = D[ci, cj]
    order = np.argsort(R, kind='stable')
    ci, cj, R = ci[order], cj[order], R[order]
    small = int(np.searchsorted(R, (PAINT_SMALL_RHO + 1) ** 2, side='right'))    # rho <= PAINT_SMALL_RHO: R <= (rho + 1)^2
    big = T2.reshape(N, N)
    ii, jj = np.mgrid[0:N, 0:N]
    for i, j, r in zip(ci[small:], cj[small:], R[small:]):
        rho = math.isqrt(int(r) - 1)
        i0, i1, j0, j1 = max(0, i - rho), min(N, i + rho + 1), max(0, j - rho), min(N, j + rho + 1)
        win = big[i0:i1, j0:j1]
        win[((ii[i0:i1, j0:j1] - i) ** 2 + (jj[i0:i1, j0:j1] - j) ** 2 < r) & (win < r)] = r
    ci, cj, R = ci[:small], cj[:small], R[:small]
    if R.size == 0:
        return big.astype(np.int32)
    rho = math.isqrt(int(R[-1]) - 1)
    for dy in range(-rho, rho + 1):
        for dx in range(-rho, rho + 1):
            k = int(np.searchsorted(R, dy * dy + dx * dx, side='right'))       # the centres with R > dy^2 + dx^2
            if k == R.size:
                continue
            y, x = ci[k:] + dy, cj[k:] + dx
            ok = (y >= 0) & (y < N) & (x >= 0) & (x < N)
            p = y[ok] * N + x[ok]
            T2[p] = np.maximum(T2[p], R[k:][ok])
    return T2.reshape(N, N).astype(np.int32)


def local_thickness(D2, prune=True):
    """(T2, kept, work) of a squared-distance map: the numpy model of chs_thickness.  ``prune=False`` paints every centre
    (the same map, slowly); kept and work are those of the rule either way."""
    D = np.asarray(D2, dtype=np.int64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"a square map is needed, got shape {D.shape}")
    if np.any(D >= CHS_DT_INF):
        return np.where(D >= CHS_DT_INF, CHS_DT_INF, 0).astype(np.int32), 0, 0
    kept = kept_centres(D)
    r = rho_of(D[kept])
    work = int(((2 * r + 1) ** 2).sum())
    T2 = paint(D, kept if prune else (D > 0))
    return T2, int(np.count_nonzero(kept)), work


def histogram_of(T2):
    """hist int64 [bin_count(N)] of a thickness map: the foreground pixels (T2 > 0) below CHS_DT_INF by bin."""
    return distance.histogram_of(T2)


def summary_of(T2, kept, work):
    """The seven summary words of a thickness map and the rule's two counts, an int64 array."""
    flat = np.asarray(T2, dtype=np.int64).ravel()
    fin = (flat > 0) & (flat < CHS_DT_INF)
    w = np.zeros(CHS_TH_WORDS, dtype=np.int64)
    w[CHS_TH_FG] = np.count_nonzero(flat > 0)
    w[CHS_TH_NINF] = np.count_nonzero(flat >= CHS_DT_INF)
    if fin.any():
        w[CHS_TH_T2MAX] = flat[fin].max()
        w[CHS_TH_NMAX] = np.count_nonzero(flat[fin] == w[CHS_TH_T2MAX])
        w[CHS_TH_SUMT2] = flat[fin].sum()
    w[CHS_TH_KEPT], w[CHS_TH_WORK] = int(kept), int(work)
    return w


def model_look(U, threshold, side='below', delx=None):
    """The `Thickness` of a field by the numpy model, map and histogram included."""
    D2 = distance.squared_distance(U, threshold, side)
    T2, kept, work = local_thickness(D2)
    di = distance.Distance(distance.summary_of(D2), D2.shape[0], threshold, side, hist=distance.histogram_of(D2), d2=D2, delx=delx)
    return Thickness(summary_of(T2, kept, work), D2.shape[0], threshold, side, hist=histogram_of(T2), t2=T2, distance=di, delx=delx)


class Thickness:
    """One look at the local thickness of a field: ``fg, t2max, nmax, sumt2, ninf, kept, work`` (Python integers),
    ``hist`` (None unless fetched), ``t2`` (the map of squared local radii, None unless fetched), ``distance`` (the
    `distance.Distance` of the same look, None unless given), and derived from them ``r_max`` (the radius of the largest
    disc that fits into the phase, in pixels), ``r2_mean``, ``r_floor_mean`` (the mean radius bin),  ``mean_thickness``
    (twice that: the mean domain width) and their ``_phys`` versions (times ``delx``), ``quantile(q)`` of the radius bins,
    ``psd()`` (the fraction of the phase with radius bin >= k: the cumulative pore-size distribution) and
    ``work_per_pixel`` -- None where a denominator is zero or the input is missing -- beside ``N``, ``threshold``,
    ``side``."""

    def __init__(self, words, N, threshold, side='below', hist=None, t2=None, distance=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.side = 'above' if side_code(side) == components.CHS_CC_ABOVE else 'below'
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_TH_WORDS,):
            raise ValueError(f"{CHS_TH_WORDS} words are needed, got shape {self.words.shape}")
        self.fg, self.t2max, self.nmax, self.sumt2, self.ninf, self.kept, self.work = (int(w) for w in self.words)
        n2 = self.N * self.N
        if self.ninf not in (0, n2):
            raise ValueError(f"ninf is 0 or N*N, got {self.ninf}")
        finite = self.fg - self.ninf
        if not (0 <= self.fg <= n2 and finite >= 0 and 0 <= self.t2max <= 2 * (self.N - 1) ** 2
                and (finite == 0) == (self.t2max == 0) == (self.nmax == 0) == (self.kept == 0) == (self.work == 0)
                and 0 <= self.nmax <= finite and 0 <= self.kept <= finite and self.kept <= self.work
                and finite + self.nmax * (self.t2max - 1) <= self.sumt2 <= finite * self.t2max):
            raise ValueError(f"not the summary of a local thickness: {self.words}")
        self.hist = None
        if hist is not None:
            self.hist = np.array(hist, dtype=np.int64)
            if self.hist.shape != (bin_count(self.N),):
                raise ValueError(f"a histogram of {bin_count(self.N)} bins is needed, got shape {self.hist.shape}")
            if np.any(self.hist < 0) or int(self.hist.sum()) != finite:
                raise ValueError(f"the histogram adds up to {int(self.hist.sum())}, not to fg - ninf = {finite}")
            top = math.isqrt(self.t2max)
            if np.any(self.hist[top + 1:] != 0) or (finite and self.hist[top] < self.nmax) or self.hist[0] != 0:
                raise ValueError(f"the histogram's last occupied bin is not isqrt(t2max) = {top}")
        self.t2 = None
        if t2 is not None:
            self.t2 = np.asarray(t2, dtype=np.int32)
            if self.t2.shape != (self.N, self.N):
                raise ValueError(f"a map of shape {(self.N, self.N)} is needed, got {self.t2.shape}")
            if not np.array_equal(summary_of(self.t2, self.kept, self.work), self.words):
                raise ValueError(f"the map's summary is {summary_of(self.t2, self.kept, self.work)}, the words are {self.words}")
            if self.hist is not None and not np.array_equal(histogram_of(self.t2), self.hist):
                raise ValueError("the map's histogram is not the one given")
        self.distance = distance
        if distance is not None:
            if (distance.N, distance.fg, distance.d2max, distance.ninf) != (self.N, self.fg, self.t2max, self.ninf):
                raise ValueError("the distance look is not that of this thickness: N, fg, d2max = t2max or ninf differ")
            if self.t2 is not None and distance.d2 is not None and (np.any(self.t2 < distance.d2)
                                                                    or np.any((self.t2 > 0) != (distance.d2 > 0))):
                raise ValueError("T2 >= D2 everywhere and T2 > 0 exactly on the foreground")

    @property
    def finite(self):
        """The foreground pixels with a finite thickness: what the means and the histogram are over."""
        return self.fg - self.ninf

    def _phys(self, v):
        return None if (v is None or self.delx is None) else v * self.delx

    @property
    def r_max(self):
        return math.sqrt(self.t2max) if self.finite else None

    @property
    def r_max_phys(self):
        return self._phys(self.r_max)

    @property
    def r2_mean(self):
        return self.sumt2 / self.finite if self.finite else None

    @property
    def r2_mean_phys(self):
        return None if (self.r2_mean is None or self.delx is None) else self.r2_mean * self.delx * self.delx

    @property
    def r_floor_mean(self):
        if self.hist is None or not self.finite:
            return None
        return int(np.dot(np.arange(len(self.hist), dtype=np.int64), self.hist)) / self.finite

    @property
    def r_floor_mean_phys(self):
        return self._phys(self.r_floor_mean)

    @property
    def mean_thickness(self):
        """Twice the mean radius bin: the mean domain width in pixels."""
        r = self.r_floor_mean
        return None if r is None else 2.0 * r

    @property
    def mean_thickness_phys(self):
        return self._phys(self.mean_thickness)

    @property
    def work_per_pixel(self):
        return self.work / (self.N * self.N)

    def quantile(self, q):
        """The smallest radius bin k with at least the fraction q of the finite foreground pixels in bins <= k."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q is in [0, 1], got {q!r}")
        if self.hist is None or not self.finite:
            return None
        need = max(1, math.ceil(q * self.finite))
        return int(np.searchsorted(np.cumsum(self.hist), need, side='left'))

    def psd(self):
        """float64 [bins]: the fraction of the phase whose local radius bin is at least k -- the cumulative pore-size
        distribution; 1 at k = 0 and k = 1, 0 beyond isqrt(t2max)."""
        if self.hist is None or not self.finite:
            return None
        return np.cumsum(self.hist[::-1])[::-1] / self.finite

    def __repr__(self):
        return (f"Thickness(N={self.N}, threshold={self.threshold!r}, side={self.side!r}, fg={self.fg}, t2max={self.t2max}, "
                f"nmax={self.nmax}, kept={self.kept}, work={self.work}, ninf={self.ninf})")
