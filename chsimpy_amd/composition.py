"""The composition of the field -- the values of U themselves: range, sums, histogram, central moments and exact order
statistics: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_composition).

Every value is the element widened to float64 first, for float32 fields too.  A pixel is NaN, infinite or finite.

Integer words (`IWORDS`).  ``n_total = N*N``; ``n_nan``; ``n_inf``, the pixels that are +inf or -inf; ``n_below``, the
pixels with ``x < threshold`` (the foreground of `components` with ``side='below'``: a NaN and ``x == threshold`` are not
below, -inf is); ``n_under``, the pixels with ``x < lo``, -inf among them; ``n_over``, those with ``x > hi``, +inf among
them; ``nbins``.

Float words (`FWORDS`).  ``min`` and ``max`` over the finite pixels; ``sum`` and ``sum_below``, the sums of x over the
finite pixels and over the finite pixels below the threshold; ``center = sum / (n_total - n_nan - n_inf)``, brought into
[min, max] where rounding left it an ulp outside; ``m2, m3,
m4``, the sums of ``(x - center)**p`` over the finite pixels, not divided; ``lo, hi`` -- the caller's, or ``min`` and
``max`` -- and ``scale = nbins / (hi - lo)`` in float64, 0 unless ``hi > lo``: the numbers the bins were formed with.

Histogram.  int64 ``[nbins]``: a finite x with ``lo <= x <= hi`` is in bin ``min(nbins - 1, int((x - lo) * scale))``, a
subtraction and a multiplication in float64 (a product that is not below nbins is bin ``nbins - 1``).  A NaN pixel goes
nowhere: ``hist.sum() + n_under + n_over + n_nan == N*N``.  With ``bins=15`` and the field's own range this is the
reference's ``Uhist`` (``numpy.histogram(U, bins=15)``, chsimpy/plotview.py:159-167).

A field without a finite pixel: ``min = max = center = lo = hi = NaN``, ``scale = 0``, an empty histogram.

Order statistics.  The r-th smallest pixel (0-based) in the order of ``numpy.sort``: by the order-preserving integer key
of the value (`key_of`), where a NaN of either sign has the largest key; -0.0 and +0.0 are neighbours.  The quantile q
is the order statistic of rank ``floor(q * (n - n_nan - 1))``: ``numpy.quantile(..., method='lower')`` over the pixels
that are not NaN.
"""
import math

import numpy as np

IWORDS = ('n_total', 'n_nan', 'n_inf', 'n_below', 'n_under', 'n_over', 'nbins')
FWORDS = ('min', 'max', 'sum', 'sum_below', 'center', 'm2', 'm3', 'm4', 'lo', 'hi', 'scale')
(CHS_CMP_N_TOTAL, CHS_CMP_N_NAN, CHS_CMP_N_INF, CHS_CMP_N_BELOW, CHS_CMP_N_UNDER, CHS_CMP_N_OVER,
 CHS_CMP_NBINS) = range(len(IWORDS))
(CHS_CMP_MIN, CHS_CMP_MAX, CHS_CMP_SUM, CHS_CMP_SUM_BELOW, CHS_CMP_CENTER, CHS_CMP_M2, CHS_CMP_M3, CHS_CMP_M4, CHS_CMP_LO,
 CHS_CMP_HI, CHS_CMP_SCALE) = range(len(FWORDS))
CHS_CMP_IWORDS, CHS_CMP_FWORDS = len(IWORDS), len(FWORDS)
CHS_CMP_MAX_BINS = 4096
CHS_CMP_MAX_RANKS = 8


def key_of(x):
    """The order-preserving integer key of every element of a float64 (uint64 keys) or float32 (uint32 keys) array: the
    bits of a non-negative number with the sign bit set, those of a negative one inverted, all ones for a NaN of either
    sign.  ``key_of(a) < key_of(b)`` where ``a < b``; -0.0 comes right before +0.0."""
    x = np.asarray(x)
    if x.dtype == np.float64:
        ut, bits = np.uint64, 64
    elif x.dtype == np.float32:
        ut, bits = np.uint32, 32
    else:
        raise ValueError(f"float64 or float32 is needed, got {x.dtype}")
    b = np.ascontiguousarray(x).view(ut)
    top = ut(1) << ut(bits - 1)
    key = np.where(b & top, ~b, b | top)
    return np.where(np.isnan(x), ~ut(0), key).astype(ut)


def _square(U):
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1] or U.shape[0] < 1:
        raise ValueError(f"a square field is needed, got shape {U.shape}")
    return U


def check_bins(nbins):
    if isinstance(nbins, bool) or int(nbins) != nbins or not 1 <= int(nbins) <= CHS_CMP_MAX_BINS:
        raise ValueError(f"bins is an integer in [1, {CHS_CMP_MAX_BINS}], got {nbins!r}")
    return int(nbins)


def check_range(range):
    """(lo, hi) of a given range -- both finite, lo <= hi -- or (NaN, NaN) for None: the field's own."""
    if range is None:
        return float('nan'), float('nan')
    lo, hi = (float(v) for v in range)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"the range is two finite numbers lo <= hi, got {range!r}")
    return lo, hi


def range_model(U, nbins, range=None):
    """(lo, hi, scale) as the device forms them from the field (or from the given range)."""
    x = _square(U).astype(np.float64)
    lo, hi = check_range(range)
    if range is None:
        f = x[np.isfinite(x)]
        lo, hi = (float(f.min()), float(f.max())) if f.size else (float('nan'), float('nan'))
    return lo, hi, (float(np.float64(nbins) / (np.float64(hi) - np.float64(lo))) if hi > lo else 0.0)


def histogram_model(U, nbins, lo, hi, scale):
    """hist int64 [nbins] of the field U with the bins formed by lo, hi, scale: the numpy model of the device's."""
    x = _square(U).astype(np.float64).ravel()
    nbins = check_bins(nbins)
    with np.errstate(invalid='ignore'):
        x = x[np.isfinite(x) & (x >= lo) & (x <= hi)]
        p = (x - np.float64(lo)) * np.float64(scale)
        inside = (p >= 0.0) & (p < nbins)
        b = np.where(inside, np.where(inside, p, 0.0).astype(np.int64), nbins - 1)
    return np.bincount(b, minlength=nbins).astype(np.int64)


def select_model(U, ranks):
    """The ranks[k]-th smallest pixels of U (0-based) in the order of the keys, widened to float64."""
    U = _square(U)
    if U.dtype not in (np.float64, np.float32):
        U = U.astype(np.float64)
    flat = U.ravel()
    order = np.argsort(key_of(flat), kind='stable')
    return flat[order[np.asarray(ranks, dtype=np.int64)]].astype(np.float64)


def words_model(U, threshold, center=None, lo=None, hi=None):
    """A dict of the words that need no bins: the integer ones exactly (``n_under, n_over`` with lo and hi), ``min, max``
    exactly, and ``sum, sum_below, m2, m3, m4`` -- the central ones about `center` (None: the model's own mean) -- and the
    sums of the absolute values ``abs1, abs1_below, abs2, abs3, abs4`` that their error bounds refer to, all added up in
    ``numpy.longdouble``."""
    x = _square(U).astype(np.float64).ravel()
    ld = np.longdouble
    with np.errstate(invalid='ignore'):
        nan, fin = np.isnan(x), np.isfinite(x)
        below = x < float(threshold)
        w = dict(n_total=x.size, n_nan=int(nan.sum()), n_inf=int((~nan & ~fin).sum()), n_below=int(below.sum()))
        if lo is not None:
            w['n_under'] = int(((x < lo) | (x == -np.inf)).sum())
            w['n_over'] = int(((x > hi) | (x == np.inf)).sum())
    f = x[fin]
    fb = x[fin & below]
    w['min'], w['max'] = (float(f.min()), float(f.max())) if f.size else (float('nan'), float('nan'))

    def chunks(a):   # (longdouble copies of a large field, a piece at a time)
        return (a[k:k + (1 << 22)].astype(ld) for k in range(0, a.size, 1 << 22))
    w['sum'], w['abs1'] = sum((c.sum() for c in chunks(f)), ld(0)), sum((np.abs(c).sum() for c in chunks(f)), ld(0))
    w['sum_below'] = sum((c.sum() for c in chunks(fb)), ld(0))
    w['abs1_below'] = sum((np.abs(c).sum() for c in chunks(fb)), ld(0))
    if center is None:
        center = float(w['sum'] / f.size) if f.size else float('nan')
    w['center'] = float(center)
    for p in (2, 3, 4):
        w[f'm{p}'] = w[f'abs{p}'] = ld(0)
    for c in chunks(f):
        d = c - ld(center)
        d2 = d * d
        for p, dp in ((2, d2), (3, d2 * d), (4, d2 * d2)):
            w[f'm{p}'] += dp.sum()
            w[f'abs{p}'] += np.abs(dp).sum()
    return w


def quantile_rank(q, n_sortable):
    """The rank of the quantile q among n_sortable pixels: floor(q (n_sortable - 1))."""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q is in [0, 1], got {q!r}")
    return int(math.floor(q * (n_sortable - 1)))


class Composition:
    """One look at the values of a field: ``iw`` (int64 [7], `IWORDS`), ``fw`` (float64 [11], `FWORDS`), ``hist`` (int64
    [nbins], None unless fetched), ``quantiles`` (a dict q -> value, the exact order statistics asked for), and from them
    ``n``, ``n_nan``, ``n_inf``, ``n_finite``, ``min``, ``max``, ``mean``, ``var``, ``skewness``, ``kurtosis`` (central
    moments over the finite pixels, divided by their number), ``n_below`` and ``SA = n_below / N*N`` (the record's SA
    column), ``mean_below`` and ``mean_above`` (the compositions of the two phases; of a field without infinite pixels),
    ``edges`` (float64 [nbins + 1]), ``under``, ``over``, ``peaks()`` -- None where a denominator is zero or the input
    is missing -- beside ``N``, ``threshold``, ``delx``."""

    def __init__(self, iw, fw, N, threshold, hist=None, quantiles=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.delx = None if delx is None else float(delx)
        self.iw = np.array(iw, dtype=np.int64)
        self.fw = np.array(fw, dtype=np.float64)
        if self.iw.shape != (CHS_CMP_IWORDS,) or self.fw.shape != (CHS_CMP_FWORDS,):
            raise ValueError(f"{CHS_CMP_IWORDS} integer and {CHS_CMP_FWORDS} float words are needed, got shapes "
                             f"{self.iw.shape} and {self.fw.shape}")
        n2 = self.N * self.N
        i = {k: int(v) for k, v in zip(IWORDS, self.iw)}
        if i['n_total'] != n2 or min(i.values()) < 0 or not 1 <= i['nbins'] <= CHS_CMP_MAX_BINS:
            raise ValueError(f"not the words of a composition at N = {self.N}: {i}")
        if i['n_nan'] + i['n_inf'] > n2 or i['n_below'] > n2 or i['n_under'] + i['n_over'] + i['n_nan'] > n2:
            raise ValueError(f"the counts exceed N*N = {n2}: {i}")
        self.n, self.n_nan, self.n_inf, self.n_below = i['n_total'], i['n_nan'], i['n_inf'], i['n_below']
        self.under, self.over, self.nbins = i['n_under'], i['n_over'], i['nbins']
        self.n_finite = n2 - self.n_nan - self.n_inf
        f = {k: float(v) for k, v in zip(FWORDS, self.fw)}
        self.min, self.max, self.sum, self.sum_below = f['min'], f['max'], f['sum'], f['sum_below']
        self.lo, self.hi, self.scale = f['lo'], f['hi'], f['scale']
        if self.n_finite and math.isfinite(self.sum) and not self.min <= f['center'] <= self.max:
            raise ValueError(f"the mean {f['center']!r} is not in [min, max] = [{self.min!r}, {self.max!r}]")
        self._m = (f['m2'], f['m3'], f['m4'])
        self.mean = f['center'] if self.n_finite else None
        self.hist = None
        if hist is not None:
            self.hist = np.array(hist, dtype=np.int64)
            if self.hist.shape != (self.nbins,) or np.any(self.hist < 0):
                raise ValueError(f"a histogram of {self.nbins} counts is needed, got shape {self.hist.shape}")
            if int(self.hist.sum()) + self.under + self.over + self.n_nan != n2:
                raise ValueError(f"the histogram ({int(self.hist.sum())}), under ({self.under}), over ({self.over}) and "
                                 f"NaN ({self.n_nan}) do not add up to N*N = {n2}")
        self.quantiles = dict(quantiles or {})

    @property
    def SA(self):
        return self.n_below / self.n

    @property
    def var(self):
        return self._m[0] / self.n_finite if self.n_finite else None

    @property
    def skewness(self):
        v = self.var
        return (self._m[1] / self.n_finite) / v ** 1.5 if v else None

    @property
    def kurtosis(self):
        v = self.var
        return (self._m[2] / self.n_finite) / (v * v) if v else None

    @property
    def mean_below(self):
        return self.sum_below / self.n_below if self.n_below else None

    @property
    def mean_above(self):
        k = self.n_finite - self.n_below
        return (self.sum - self.sum_below) / k if k > 0 else None

    @property
    def edges(self):
        """float64 [nbins + 1]: bin b is [edges[b], edges[b + 1]), the last one closed; None without a range."""
        if not (math.isfinite(self.lo) and math.isfinite(self.hi)):
            return None
        return self.lo + (self.hi - self.lo) * (np.arange(self.nbins + 1, dtype=np.float64) / self.nbins)

    def peaks(self):
        """(below, above): the centre of the fullest bin among the bins whose centre lies below the threshold, and among
        the others -- the two phase compositions as the histogram shows them; None where a side has no pixel (or the
        histogram is missing)."""
        e = self.edges
        if self.hist is None or e is None:
            return None, None
        centres = 0.5 * (e[:-1] + e[1:])
        out = []
        for side in (centres < self.threshold, centres >= self.threshold):
            h = np.where(side, self.hist, 0)
            out.append(float(centres[int(np.argmax(h))]) if h.any() else None)
        return tuple(out)

    def __repr__(self):
        return (f"Composition(N={self.N}, threshold={self.threshold!r}, n_nan={self.n_nan}, min={self.min!r}, "
                f"max={self.max!r}, mean={self.mean!r}, SA={self.SA!r}, mean_below={self.mean_below!r}, "
                f"mean_above={self.mean_above!r}, quantiles={self.quantiles!r})")
