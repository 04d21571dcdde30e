"""Two-point correlation of both phases of the thresholded field: the pair counts of every displacement up to rmax, and
the two-point probability function S2, its radial average, the autocovariance and the real-space domain size that follow
from them: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_two_point).

For the N x N field U, a finite threshold t and an integer ``rmax`` with ``1 <= rmax <= max_r(N)``, where ``max_r(N) =
min(N - 1, 256)`` and is 0 for N < 2:

Phases.  These are the phases of `chords`.  Phase 0 (``'below'``) is ``X[i][j] = ((double)U[i][j] < t)``; a NaN pixel and
a pixel equal to t are not phase 0.  Phase 1 (``'above'``) is the complement inside the grid.

Displacements.  ``(dy, dx)`` with ``0 <= dy <= rmax`` and ``-rmax <= dx <= rmax``.  The other half-plane is the mirror
image (``c(-dy, -dx) = c(dy, dx)``) and is not stored.

Pair count.  ``c[p][dy][dx + rmax]`` is int64, laid out as ``[2][rmax + 1][2 rmax + 1]``: the number of positions (i, j)
for which (i, j) and (i + dy, j + dx) are both inside the grid and both of phase p.  There is no wrap-around.  The window
holds ``pairs(dy, dx) = (N - dy)(N - |dx|)`` positions.  ``table_size(N, rmax) = 2 (rmax + 1)(2 rmax + 1)``, and 0 for
arguments out of range.

Summary.  ``CHS_TP_WORDS = 8`` int64 words (`WORDS`): ``n_below, n_above``: ``c[p][0][rmax]``, the pixels of the phase;
``adj_rows_below, adj_cols_below, adj_rows_above, adj_cols_above``: ``c[p]`` at (dy, dx) = (0, 1), the neighbours within
a row, and at (1, 0), the neighbours within a column; ``sum_below, sum_above``: the sum of all entries of ``c[p]``.

Everything is an integer and every sum is order-free.
"""
import numpy as np

from .chords import PHASES, phase0, phase_code

WORDS = ('n_below', 'n_above', 'adj_rows_below', 'adj_cols_below', 'adj_rows_above', 'adj_cols_above', 'sum_below',
         'sum_above')
(CHS_TP_N_BELOW, CHS_TP_N_ABOVE, CHS_TP_ADJ_ROWS_BELOW, CHS_TP_ADJ_COLS_BELOW, CHS_TP_ADJ_ROWS_ABOVE,
 CHS_TP_ADJ_COLS_ABOVE, CHS_TP_SUM_BELOW, CHS_TP_SUM_ABOVE) = range(len(WORDS))
CHS_TP_WORDS = len(WORDS)
CHS_TP_MAX_R = 256
DIRECTIONS = ('rows', 'cols')


class _DefaultRmax(int):
    """The default rmax of `Solver.two_point`: 64, told apart from a 64 the caller wrote by identity."""


DEFAULT_RMAX = _DefaultRmax(64)


def max_r(N):
    """The largest rmax at grid size N: min(N - 1, 256), 0 for N < 2 (chs_two_point_max_r)."""
    N = int(N)
    return min(N - 1, CHS_TP_MAX_R) if N >= 2 else 0


def table_size(N, rmax):
    """The entries of the count table: 2 (rmax + 1)(2 rmax + 1), 0 for arguments out of range (chs_two_point_size)."""
    rmax = int(rmax)
    return 2 * (rmax + 1) * (2 * rmax + 1) if 1 <= rmax <= max_r(N) else 0


def check_rmax(N, rmax):
    if isinstance(rmax, bool) or int(rmax) != rmax or not 1 <= int(rmax) <= max_r(N):
        raise ValueError(f"rmax is an integer in [1, {max_r(N)}] at N = {int(N)}, got {rmax!r}")
    return int(rmax)


def pairs_table(N, rmax):
    """pairs(dy, dx) = (N - dy)(N - |dx|) as an int64 array [rmax + 1][2 rmax + 1]."""
    dy = np.arange(rmax + 1, dtype=np.int64)[:, None]
    dx = np.abs(np.arange(-rmax, rmax + 1, dtype=np.int64))[None, :]
    return (N - dy) * (N - dx)


def pair_counts(U, threshold, rmax):
    """c int64 [2][rmax + 1][2 rmax + 1] of the field U: the numpy model of chs_two_point, the zero-padded
    autocorrelation of each phase's indicator by a real FFT, rounded.  Raises unless every value is within 0.25 of an
    integer."""
    X = phase0(U, threshold)
    N = X.shape[0]
    rmax = check_rmax(N, rmax)
    P = N + rmax                                                     # no displacement up to rmax wraps around
    out = np.empty((2, rmax + 1, 2 * rmax + 1), dtype=np.int64)
    for phase, M in enumerate((X, ~X)):
        F = np.fft.rfft2(M.astype(np.float64), s=(P, P))
        A = np.fft.irfft2(F * np.conj(F), s=(P, P))                  # A[dy][dx mod P] = sum_ij M[i][j] M[i + dy][j + dx]
        c = np.concatenate((A[:rmax + 1, P - rmax:], A[:rmax + 1, :rmax + 1]), axis=1)
        r = np.rint(c)
        off = float(np.abs(c - r).max())
        if not off <= 0.25:
            raise ValueError(f"the FFT autocorrelation is {off} off an integer: too large a field for float64")
        out[phase] = r.astype(np.int64)
    return out


def pair_counts_slices(U, threshold, rmax):
    """The definition written out with array slices: one AND of two windows of the indicator per displacement."""
    X = phase0(U, threshold)
    N = X.shape[0]
    rmax = check_rmax(N, rmax)
    out = np.empty((2, rmax + 1, 2 * rmax + 1), dtype=np.int64)
    for phase, M in enumerate((X, ~X)):
        for dy in range(rmax + 1):
            for dx in range(-rmax, rmax + 1):
                a = M[:N - dy, max(0, -dx):N - max(0, dx)]           # the positions (i, j) ...
                b = M[dy:, max(0, dx):N - max(0, -dx)]               # ... and their partners (i + dy, j + dx)
                out[phase, dy, dx + rmax] = np.count_nonzero(a & b)
    return out


def summary_of(counts):
    """The 8 summary words of a count table, an int64 array."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 3 or c.shape[0] != 2 or c.shape[1] < 2 or c.shape[2] != 2 * c.shape[1] - 1:
        raise ValueError(f"a count table of shape (2, rmax + 1, 2 rmax + 1) with rmax >= 1 is needed, got {c.shape}")
    r = c.shape[1] - 1
    return np.array([c[0, 0, r], c[1, 0, r], c[0, 0, r + 1], c[0, 1, r], c[1, 0, r + 1], c[1, 1, r], c[0].sum(), c[1].sum()],
                    dtype=np.int64)


class TwoPoint:
    """One look at the two-point correlation of a field: ``N``, ``threshold``, ``rmax``, ``delx``, ``words`` (int64 [8];
    ``word(name)`` picks one) and ``counts`` (int64 [2][rmax + 1][2 rmax + 1], None unless fetched); per ``phase in
    ('below', 'above')``: ``n`` (its pixels), ``S2`` (the probability that two pixels a displacement apart are both of
    the phase, as a map or at one displacement), ``radial`` (its average over shells of integer radius), ``autocovariance``,
    ``first_zero`` (the real-space domain size), ``along`` (the cuts along the axes) and ``anisotropy``; ``pairs(dy, dx)``
    and ``cross(dy, dx)`` (the two pixels in different phases).  What needs the table is None without it."""

    def __init__(self, words, N, threshold, rmax, counts=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.rmax = check_rmax(self.N, rmax)
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_TP_WORDS,):
            raise ValueError(f"{CHS_TP_WORDS} words are needed, got shape {self.words.shape}")
        N, n2, w = self.N, self.N * self.N, [int(v) for v in self.words]
        if min(w) < 0:
            raise ValueError(f"a negative word: {self.words}")
        if w[CHS_TP_N_BELOW] + w[CHS_TP_N_ABOVE] != n2:
            raise ValueError(f"the two phases add to {w[CHS_TP_N_BELOW] + w[CHS_TP_N_ABOVE]} pixels, not to N*N = {n2}")
        for p in range(2):
            n, adj = w[CHS_TP_N_BELOW + p], w[CHS_TP_ADJ_ROWS_BELOW + 2 * p:CHS_TP_ADJ_ROWS_BELOW + 2 * p + 2]
            # (k pixels of a phase have at most k - 1 neighbours along a direction, and no entry of its table exceeds k)
            if max(adj) > max(n - 1, 0) or not n <= w[CHS_TP_SUM_BELOW + p] <= n * (self.rmax + 1) * (2 * self.rmax + 1):
                raise ValueError(f"not the words of a pair count ({PHASES[p]}): {self.words}")
        self.counts = None
        if counts is not None:
            self.counts = np.array(counts, dtype=np.int64)
            shape = (2, self.rmax + 1, 2 * self.rmax + 1)
            if self.counts.shape != shape:
                raise ValueError(f"a count table of shape {shape} is needed, got {self.counts.shape}")
            if np.any(self.counts < 0):
                raise ValueError("a negative pair count")
            if not np.array_equal(self.counts[:, 0, :], self.counts[:, 0, ::-1]):
                raise ValueError("the row dy = 0 of a count table is not symmetric in dx")
            if np.any(self.counts[0] + self.counts[1] > pairs_table(N, self.rmax)):
                raise ValueError("c0 + c1 exceeds pairs(dy, dx) at some displacement")
            if not np.array_equal(summary_of(self.counts), self.words):
                raise ValueError(f"the count table adds up to {summary_of(self.counts)}, the words are {self.words}")

    def word(self, name):
        """One summary word as a Python integer: ``name`` is one of `WORDS`."""
        return int(self.words[WORDS.index(name)])

    def n(self, phase):
        """The pixels of the phase."""
        return int(self.words[CHS_TP_N_BELOW + phase_code(phase)])

    def _check_d(self, dy, dx):
        dy, dx = int(dy), int(dx)
        if abs(dy) > self.rmax or abs(dx) > self.rmax:
            raise ValueError(f"the displacement ({dy}, {dx}) is beyond rmax = {self.rmax}")
        return (-dy, -dx) if dy < 0 else (dy, dx)     # the mirror image

    def pairs(self, dy, dx):
        """The positions of the window of the displacement: (N - |dy|)(N - |dx|)."""
        return (self.N - abs(int(dy))) * (self.N - abs(int(dx)))

    def count(self, phase, dy, dx):
        """c[phase] at (dy, dx) as a Python integer; negative dy is served through the mirror."""
        if self.counts is None:
            return None
        dy, dx = self._check_d(dy, dx)
        return int(self.counts[phase_code(phase), dy, dx + self.rmax])

    def S2(self, phase, dy=None, dx=None):
        """The two-point probability of the phase: the map ``c / pairs`` (float64 [rmax + 1][2 rmax + 1]) without a
        displacement, one value at (dy, dx); S2 at (0, 0) is the area fraction."""
        if self.counts is None:
            return None
        if dy is None and dx is None:
            return self.counts[phase_code(phase)] / pairs_table(self.N, self.rmax)
        if dy is None or dx is None:
            raise ValueError("a displacement needs both dy and dx")
        return self.count(phase, dy, dx) / self.pairs(dy, dx)

    def cross(self, dy, dx):
        """The probability that two pixels the displacement apart are of different phases: (pairs - c0 - c1) / pairs."""
        if self.counts is None:
            return None
        p = self.pairs(dy, dx)
        return (p - self.count(0, dy, dx) - self.count(1, dy, dx)) / p

    def radial(self, phase):
        """S2 averaged over shells, float64 [rmax + 1]: shell ``s = isqrt(dy^2 + dx^2)`` for ``s <= rmax`` over the stored
        half-plane without its duplicate half-line ``dy = 0, dx < 0``; the value is ``sum c / sum pairs`` over the shell,
        one division of exact integers."""
        if self.counts is None:
            return None
        r = self.rmax
        dy = np.arange(r + 1, dtype=np.int64)[:, None]
        dx = np.arange(-r, r + 1, dtype=np.int64)[None, :]
        d2 = dy * dy + dx * dx
        shell = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
        shell += (shell + 1) * (shell + 1) <= d2                    # (isqrt, whatever the rounding of the square root)
        shell -= shell * shell > d2
        keep = (shell <= r) & ~((dy == 0) & (dx < 0))
        num = np.zeros(r + 1, dtype=np.int64)
        den = np.zeros(r + 1, dtype=np.int64)
        np.add.at(num, shell[keep], self.counts[phase_code(phase)][keep])
        np.add.at(den, shell[keep], pairs_table(self.N, r)[keep])
        return num / den

    def autocovariance(self, phase):
        """``radial(phase) - (n / N^2)^2``: what is left of S2 when the two pixels are independent."""
        rad = self.radial(phase)
        return None if rad is None else rad - (self.n(phase) / (self.N * self.N)) ** 2

    def first_zero(self, phase):
        """The first sign change of the autocovariance, linearly interpolated between the two shells: the real-space
        domain size, in pixels, or in physical units where ``delx`` is known.  None without a sign change up to rmax."""
        cov = self.autocovariance(phase)
        if cov is None:
            return None
        for s in range(len(cov) - 1):
            a, b = float(cov[s]), float(cov[s + 1])
            if a > 0.0 >= b:                                        # (shell 0 holds f (1 - f) >= 0: the first change is downwards)
                z = s + a / (a - b)
                return z if self.delx is None else z * self.delx
        return None

    def along(self, phase, direction):
        """The cut of S2 along an axis, float64 [rmax + 1]: ``'rows'`` is the displacement (0, r) within a row,
        ``'cols'`` the displacement (r, 0) within a column."""
        if self.counts is None:
            return None
        if direction not in DIRECTIONS:
            raise ValueError(f"the direction is 'rows' or 'cols', got {direction!r}")
        c = self.counts[phase_code(phase)]
        r = np.arange(self.rmax + 1, dtype=np.int64)
        line = c[0, self.rmax:] if direction == 'rows' else c[:, self.rmax]
        return line / (self.N * (self.N - r))

    def anisotropy(self, phase, r):
        """S2 along the rows over S2 along the columns at distance r; None where the latter is zero."""
        if self.counts is None:
            return None
        a, b = self.S2(phase, 0, r), self.S2(phase, r, 0)
        return a / b if b else None

    def __repr__(self):
        return (f"TwoPoint(N={self.N}, threshold={self.threshold!r}, rmax={self.rmax}, n_below={self.n('below')}, "
                f"first_zero_below={self.first_zero('below')})")
