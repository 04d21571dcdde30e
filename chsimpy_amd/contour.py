"""The interface of the field below the pixel: the length of the contour line ``U = t``, its orientation tensor and the
curvature of the level set at every cell the contour crosses: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_contour).

Setting.  The N x N field ``U[i][j]``, i the row (y) and j the column (x), N >= 2; every value widened to double; a finite
threshold t.  A pixel is *below* when ``(double)U < t`` -- phase 0 of `chords`: a NaN and a pixel equal to t are not
below.  Cell (i, j), ``0 <= i, j <= N - 2``, has the corners ``a = U[i][j], b = U[i][j+1], c = U[i+1][j], d =
U[i+1][j+1]`` and the code ``below(a) + 2 below(b) + 4 below(c) + 8 below(d)``.

Vertices.  One on every grid edge whose two pixels p and q (p the one with the lower index) are unlike: ``lo`` the below
value, ``hi`` the other, ``s = (t - lo) / (hi - lo)``, ``s = 0.5`` if either value is not finite; the vertex lies at the
fraction s from p if p is below and at 1 - s otherwise.  In cell coordinates a cell's vertices are ``T = (x_T, 0), B =
(x_B, 1), L = (0, y_L), R = (1, y_R)``.

Segments (`SEGMENTS`), from the first vertex to the second: codes 1, 14: L-T; 2, 13: T-R; 4, 11: L-B; 8, 7: B-R; 3, 12:
L-R; 5, 10: T-B; 6 (a saddle): T-R and L-B; 9 (a saddle): L-T and B-R -- every below corner of a saddle is cut off on its
own, the below phase being 4-connected as for ``euler4``.  For a segment from P to Q, every operation rounded on its
own: ``dx = Q.x - P.x, dy = Q.y - P.y, l = sqrt(dx dx + dy dy)``; ``txx = dx dx / l, txy = dx dy / l, tyy = dy dy / l``,
each 0 where ``l == 0``.  A cell's ``ell`` is the sum of its l, at most two terms in the order above.

Curvature, for a crossed cell that is no saddle and has ``1 <= i, j <= N - 3``, with ``A(di, dj) = U[i+di][j+dj]``::

    ux  = ((A(0,1) + A(1,1)) - (A(0,0) + A(1,0))) 0.5
    uy  = ((A(1,0) + A(1,1)) - (A(0,0) + A(0,1))) 0.5
    uxy = (A(1,1) - A(1,0)) - (A(0,1) - A(0,0))
    uxx = (((A(0,2) - A(0,1)) - (A(0,0) - A(0,-1))) + ((A(1,2) - A(1,1)) - (A(1,0) - A(1,-1)))) 0.25
    uyy = (((A(2,0) - A(1,0)) - (A(0,0) - A(-1,0))) + ((A(2,1) - A(1,1)) - (A(0,1) - A(-1,1)))) 0.25
    g2  = ux ux + uy uy
    kappa = ((uxx (uy uy) - (2 (ux uy)) uxy) + uyy (ux ux)) / (g2 sqrt(g2))

the divergence of grad U / |grad U|: positive where the below phase is convex (a droplet of below), in 1 / pixel.  A
crossed cell that is no saddle and lacks the full stencil is a *wall cell*; one whose 16 stencil values are not all
finite or whose kappa is not finite is a *bad cell*.  Wall cells, bad cells and saddles take no part in the curvature
results; they are counted.

Fixed point.  ``fix(x) = (int64)(x 2^30)``, truncated; lengths are summed as ``fix(ell)``: order-free integers.

Words (`WORDS`, 16 int64), sums (`SUMS`, 6 float64: ``txx, txy, tyy`` over all segments, ``k1 = sum ell kappa, ka = sum
ell |kappa|, k2 = sum ell (kappa kappa)`` over the curvature cells), the histogram (``bins`` in [1, 1024], a finite ``kmax
> 0``, ``SCALE = bins / (2 kmax)``: a curvature cell with kappa in [-kmax, kmax] is in bin ``min(bins - 1, (int64)((kappa +
kmax) SCALE))``; below -kmax: ``hist_under``, above kmax: ``hist_over``; int64 [2][bins]: the cells per bin, then their
fix(ell)) and the map (float64 [2][N-1][N-1]: ell per cell, 0 where the cell is not crossed; kappa per cell, NaN where
it is not a curvature cell).
"""
import math
import types

import numpy as np

from .chords import phase0

WORDS = ('cells_one', 'cells_two', 'saddles', 'vertices_rows', 'vertices_cols', 'ends', 'segments', 'cells_curv',
         'cells_wall', 'cells_bad', 'l_fix', 'l_curv_fix', 'hist_under', 'hist_over', 'n_below', 'n_nonfinite')
(CHS_CT_CELLS_ONE, CHS_CT_CELLS_TWO, CHS_CT_SADDLES, CHS_CT_VERTICES_ROWS, CHS_CT_VERTICES_COLS, CHS_CT_ENDS,
 CHS_CT_SEGMENTS, CHS_CT_CELLS_CURV, CHS_CT_CELLS_WALL, CHS_CT_CELLS_BAD, CHS_CT_L_FIX, CHS_CT_L_CURV_FIX,
 CHS_CT_HIST_UNDER, CHS_CT_HIST_OVER, CHS_CT_N_BELOW, CHS_CT_N_NONFINITE) = range(len(WORDS))
CHS_CT_WORDS = len(WORDS)
SUMS = ('txx', 'txy', 'tyy', 'k1', 'ka', 'k2')
CHS_CT_TXX, CHS_CT_TXY, CHS_CT_TYY, CHS_CT_K1, CHS_CT_KA, CHS_CT_K2 = range(len(SUMS))
CHS_CT_SUMS = len(SUMS)
CHS_CT_MAX_BINS = 1024
CHS_CT_FIX_BITS = 30
FIX = float(1 << CHS_CT_FIX_BITS)
DEFAULT_BINS, DEFAULT_KMAX = 64, 1.0

# the segments of a code, from the first vertex to the second
SEGMENTS = {1: ('LT',), 14: ('LT',), 2: ('TR',), 13: ('TR',), 4: ('LB',), 11: ('LB',), 8: ('BR',), 7: ('BR',),
            3: ('LR',), 12: ('LR',), 5: ('TB',), 10: ('TB',), 6: ('TR', 'LB'), 9: ('LT', 'BR'), 0: (), 15: ()}
SADDLES = (6, 9)


def check_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= CHS_CT_MAX_BINS:
        raise ValueError(f"bins is an integer in [1, {CHS_CT_MAX_BINS}], got {bins!r}")
    return int(bins)


def check_kmax(kmax):
    k = float(kmax)
    if not (math.isfinite(k) and k > 0.0):
        raise ValueError(f"kmax is a finite number above 0, got {kmax!r}")
    return k


def _field(U, threshold):
    below = phase0(U, threshold)                       # (checks the shape and the threshold)
    if below.shape[0] < 2:
        raise ValueError(f"N >= 2 is needed, got {below.shape[0]}")
    return np.asarray(U).astype(np.float64), below, float(threshold)


def fix(x):
    """``(int64)(x 2^30)``, truncated, of an array of lengths."""
    return (np.asarray(x, dtype=np.float64) * FIX).astype(np.int64)


# ---------------------------------------------------------------------------
# the cells: vectorised
# ---------------------------------------------------------------------------
def _frac(p, q, t):
    pb = p < t
    lo, hi = np.where(pb, p, q), np.where(pb, q, p)
    s = (t - lo) / (hi - lo)
    s = np.where(np.isfinite(p) & np.isfinite(q), s, 0.5)
    return np.where(pb, s, 1.0 - s)


def cells(U, threshold):
    """What the definition gives cell by cell, as arrays of (N-1) x (N-1): ``code``; ``l, txx, txy, tyy`` of shape
    (2, N-1, N-1), the cell's first and second segment, 0 where it has none; ``ell``; ``kappa`` (NaN where the cell is
    not a curvature cell); the masks ``crossed, saddle, curv, wall, bad``."""
    x, below, t = _field(U, threshold)
    M = x.shape[0] - 1
    a, b, c, d = x[:-1, :-1], x[:-1, 1:], x[1:, :-1], x[1:, 1:]
    ba, bb, bc, bd = below[:-1, :-1], below[:-1, 1:], below[1:, :-1], below[1:, 1:]
    code = ba.astype(np.int64) + 2 * bb + 4 * bc + 8 * bd
    zero, one = np.zeros((M, M)), np.ones((M, M))
    with np.errstate(all='ignore'):
        vert = {'T': (_frac(a, b, t), zero), 'B': (_frac(c, d, t), one), 'L': (zero, _frac(a, c, t)), 'R': (one, _frac(b, d, t))}
        l, txx, txy, tyy = (np.zeros((2, M, M)) for _ in range(4))
        names = ('LT', 'TR', 'LB', 'BR', 'LR', 'TB')
        for k in range(2):
            lut = np.zeros(16, dtype=np.int8)               # 1 + the index of the code's k-th segment, 0 without one
            for cd, segs in SEGMENTS.items():
                if len(segs) > k:
                    lut[cd] = 1 + names.index(segs[k])
            which = lut[code]
            for n, name in enumerate(names):
                m = np.nonzero(which == n + 1)
                if not len(m[0]):
                    continue
                (px, py), (qx, qy) = vert[name[0]], vert[name[1]]
                dx, dy = qx[m] - px[m], qy[m] - py[m]
                xx, yy, xy = dx * dx, dy * dy, dx * dy
                ll = np.sqrt(xx + yy)
                z = ll == 0.0
                l[k][m] = ll
                txx[k][m] = np.where(z, 0.0, xx / ll)
                txy[k][m] = np.where(z, 0.0, xy / ll)
                tyy[k][m] = np.where(z, 0.0, yy / ll)
        saddle = np.isin(code, SADDLES)
        crossed = (code != 0) & (code != 15)
        ell = np.where(saddle, l[0] + l[1], l[0])
        # the curvature of the inner cells
        kappa = np.full((M, M), np.nan)
        inner = np.zeros((M, M), dtype=bool)
        fin = np.zeros((M, M), dtype=bool)
        if M >= 3:
            inner[1:M - 1, 1:M - 1] = True
            n = M - 2                                   # cells i, j = 1 .. N - 3
            A = lambda di, dj: x[1 + di:1 + di + n, 1 + dj:1 + dj + n]
            ux = ((A(0, 1) + A(1, 1)) - (A(0, 0) + A(1, 0))) * 0.5
            uy = ((A(1, 0) + A(1, 1)) - (A(0, 0) + A(0, 1))) * 0.5
            uxy = (A(1, 1) - A(1, 0)) - (A(0, 1) - A(0, 0))
            uxx = (((A(0, 2) - A(0, 1)) - (A(0, 0) - A(0, -1))) + ((A(1, 2) - A(1, 1)) - (A(1, 0) - A(1, -1)))) * 0.25
            uyy = (((A(2, 0) - A(1, 0)) - (A(0, 0) - A(-1, 0))) + ((A(2, 1) - A(1, 1)) - (A(0, 1) - A(-1, 1)))) * 0.25
            g2 = ux * ux + uy * uy
            kap = ((uxx * (uy * uy) - (2.0 * (ux * uy)) * uxy) + uyy * (ux * ux)) / (g2 * np.sqrt(g2))
            f = np.ones((n, n), dtype=bool)
            for di in range(-1, 3):
                for dj in range(-1, 3):
                    f &= np.isfinite(A(di, dj))
            fin[1:M - 1, 1:M - 1] = f & np.isfinite(kap)
            kappa[1:M - 1, 1:M - 1] = kap
    plain = crossed & ~saddle
    curv = plain & inner & fin
    kappa = np.where(curv, kappa, np.nan)
    return types.SimpleNamespace(N=M + 1, threshold=t, x=x, below=below, code=code, l=l, txx=txx, txy=txy, tyy=tyy, ell=ell,
                                 kappa=kappa, crossed=crossed, saddle=saddle, curv=curv, wall=plain & ~inner,
                                 bad=plain & inner & ~fin)


# ---------------------------------------------------------------------------
# the cells: a plain loop
# ---------------------------------------------------------------------------
def _frac1(p, q, t):
    pb = p < t
    lo, hi = (p, q) if pb else (q, p)
    s = (t - lo) / (hi - lo) if math.isfinite(p) and math.isfinite(q) else 0.5
    return s if pb else 1.0 - s


def cells_loop(U, threshold):
    """`cells` written as a loop over the cells, in Python floats: the definition as one would read it out."""
    x, below, t = _field(U, threshold)
    N = x.shape[0]
    M = N - 1
    code = np.zeros((M, M), dtype=np.int64)
    l, txx, txy, tyy = (np.zeros((2, M, M)) for _ in range(4))
    ell = np.zeros((M, M))
    kappa = np.full((M, M), np.nan)
    crossed, saddle, curv, wall, bad = (np.zeros((M, M), dtype=bool) for _ in range(5))
    for i in range(M):
        for j in range(M):
            a, b, c, d = float(x[i, j]), float(x[i, j + 1]), float(x[i + 1, j]), float(x[i + 1, j + 1])
            cd = (a < t) + 2 * (b < t) + 4 * (c < t) + 8 * (d < t)
            code[i, j] = cd
            segs = SEGMENTS[cd]
            if not segs:
                continue
            crossed[i, j] = True
            edge = {'T': (a, b), 'B': (c, d), 'L': (a, c), 'R': (b, d)}

            def vertex(e):
                f = _frac1(*edge[e], t)
                return {'T': (f, 0.0), 'B': (f, 1.0), 'L': (0.0, f), 'R': (1.0, f)}[e]
            total = None
            for k, name in enumerate(segs):
                (px, py), (qx, qy) = vertex(name[0]), vertex(name[1])
                dx, dy = qx - px, qy - py
                xx, yy, xy = dx * dx, dy * dy, dx * dy
                ll = math.sqrt(xx + yy)
                l[k, i, j] = ll
                if ll != 0.0:
                    txx[k, i, j], txy[k, i, j], tyy[k, i, j] = xx / ll, xy / ll, yy / ll
                total = ll if total is None else total + ll
            ell[i, j] = total
            if cd in SADDLES:
                saddle[i, j] = True
                continue
            if not (1 <= i <= N - 3 and 1 <= j <= N - 3):
                wall[i, j] = True
                continue
            A = lambda di, dj: float(x[i + di, j + dj])
            if not all(math.isfinite(A(di, dj)) for di in range(-1, 3) for dj in range(-1, 3)):
                bad[i, j] = True
                continue
            ux = ((A(0, 1) + A(1, 1)) - (A(0, 0) + A(1, 0))) * 0.5
            uy = ((A(1, 0) + A(1, 1)) - (A(0, 0) + A(0, 1))) * 0.5
            uxy = (A(1, 1) - A(1, 0)) - (A(0, 1) - A(0, 0))
            uxx = (((A(0, 2) - A(0, 1)) - (A(0, 0) - A(0, -1))) + ((A(1, 2) - A(1, 1)) - (A(1, 0) - A(1, -1)))) * 0.25
            uyy = (((A(2, 0) - A(1, 0)) - (A(0, 0) - A(-1, 0))) + ((A(2, 1) - A(1, 1)) - (A(0, 1) - A(-1, 1)))) * 0.25
            g2 = ux * ux + uy * uy
            num = (uxx * (uy * uy) - (2.0 * (ux * uy)) * uxy) + uyy * (ux * ux)
            den = g2 * math.sqrt(g2) if g2 >= 0.0 else float('nan')
            with np.errstate(all='ignore'):
                kap = float(np.float64(num) / np.float64(den))      # (0 / 0 and x / 0 as IEEE has them)
            if math.isfinite(kap):
                curv[i, j] = True
                kappa[i, j] = kap
            else:
                bad[i, j] = True
    return types.SimpleNamespace(N=N, threshold=t, x=x, below=below, code=code, l=l, txx=txx, txy=txy, tyy=tyy, ell=ell,
                                 kappa=kappa, crossed=crossed, saddle=saddle, curv=curv, wall=wall, bad=bad)


# ---------------------------------------------------------------------------
# the look's results from the cells
# ---------------------------------------------------------------------------
def bin_of(kappa, bins, kmax):
    """The bin of every kappa in [-kmax, kmax], an int64 array (the rule of the composition's histogram)."""
    kappa = np.asarray(kappa, dtype=np.float64)
    scale = np.float64(bins) / (np.float64(2.0) * np.float64(kmax))
    with np.errstate(all='ignore'):
        p = (kappa + np.float64(kmax)) * scale
        inside = (p >= 0.0) & (p < bins)
        return np.where(inside, np.where(inside, p, 0.0).astype(np.int64), bins - 1)


def model_of(cl, bins=DEFAULT_BINS, kmax=DEFAULT_KMAX):
    """words, hist, the terms of the six sums and the sums (each the ``numpy.longdouble`` sum of its terms) of the cells
    `cl` (of `cells` or `cells_loop`): the numpy model of chs_contour."""
    bins, kmax = check_bins(bins), check_kmax(kmax)
    below, code, N = cl.below, cl.code, cl.N
    w = np.zeros(CHS_CT_WORDS, dtype=np.int64)
    nb = (code & 1) + ((code >> 1) & 1) + ((code >> 2) & 1) + ((code >> 3) & 1)
    w[CHS_CT_CELLS_ONE] = np.count_nonzero((nb == 1) | (nb == 3))
    w[CHS_CT_SADDLES] = np.count_nonzero(cl.saddle)
    w[CHS_CT_CELLS_TWO] = np.count_nonzero(nb == 2) - w[CHS_CT_SADDLES]
    rows, cols = below[:, :-1] != below[:, 1:], below[:-1, :] != below[1:, :]
    w[CHS_CT_VERTICES_ROWS], w[CHS_CT_VERTICES_COLS] = np.count_nonzero(rows), np.count_nonzero(cols)
    w[CHS_CT_ENDS] = (np.count_nonzero(rows[0]) + np.count_nonzero(rows[-1]) + np.count_nonzero(cols[:, 0])
                      + np.count_nonzero(cols[:, -1]))
    w[CHS_CT_SEGMENTS] = np.count_nonzero(cl.crossed) + w[CHS_CT_SADDLES]
    w[CHS_CT_CELLS_CURV], w[CHS_CT_CELLS_WALL], w[CHS_CT_CELLS_BAD] = (np.count_nonzero(m) for m in (cl.curv, cl.wall, cl.bad))
    fx = fix(cl.ell)
    w[CHS_CT_L_FIX], w[CHS_CT_L_CURV_FIX] = fx.sum(), fx[cl.curv].sum()
    kap, ell = cl.kappa[cl.curv], cl.ell[cl.curv]
    under, over = kap < -kmax, kap > kmax
    w[CHS_CT_HIST_UNDER], w[CHS_CT_HIST_OVER] = np.count_nonzero(under), np.count_nonzero(over)
    w[CHS_CT_N_BELOW] = np.count_nonzero(below)
    w[CHS_CT_N_NONFINITE] = np.count_nonzero(~np.isfinite(cl.x))
    inside = ~under & ~over
    b = bin_of(kap[inside], bins, kmax)
    hist = np.zeros((2, bins), dtype=np.int64)
    hist[0] = np.bincount(b, minlength=bins)
    np.add.at(hist[1], b, fx[cl.curv][inside])
    terms = {'txx': cl.txx.ravel(), 'txy': cl.txy.ravel(), 'tyy': cl.tyy.ravel(),
             'k1': ell * kap, 'ka': ell * np.abs(kap), 'k2': ell * (kap * kap)}
    sums = np.array([float(terms[name].sum(dtype=np.longdouble)) for name in SUMS])
    return types.SimpleNamespace(words=w, sums=sums, hist=hist, terms=terms, ell=cl.ell, kappa=cl.kappa, cells=cl,
                                 bins=bins, kmax=kmax)


def contour_model(U, threshold, bins=DEFAULT_BINS, kmax=DEFAULT_KMAX):
    """`model_of` the vectorised `cells` of the field U."""
    return model_of(cells(U, threshold), bins, kmax)


# ---------------------------------------------------------------------------
# the result class
# ---------------------------------------------------------------------------
class Contour:
    """One look at the contour ``U = threshold`` of a field: ``N``, ``threshold``, ``bins``, ``kmax``, ``delx``,
    ``words`` (int64 [16]; ``word(name)`` picks one), ``sums`` (float64 [6]; ``sum(name)``), ``hist`` and ``hist_length``
    (int64 [bins], None unless fetched: the curvature cells per bin and their length in pixels x 2^30), ``ell_map`` and
    ``kappa_map`` (None unless fetched).  ``length`` (pixels), ``length_phys``, ``S_V`` (length per area of the cells),
    ``pixel_ratio`` (the pixel perimeter over the length: 4 / pi for an isotropic interface), ``mean_curvature``,
    ``mean_abs_curvature``, ``rms_curvature`` (per pixel; ``*_phys`` per physical length), ``orientation()``,
    ``bin_edges``, ``quantile``."""

    def __init__(self, words, sums, N, threshold, bins=DEFAULT_BINS, kmax=DEFAULT_KMAX, hist=None, map=None, delx=None):
        self.N = int(N)
        if self.N < 2:
            raise ValueError(f"N >= 2 is needed, got {N}")
        self.threshold = float(threshold)
        self.bins, self.kmax = check_bins(bins), check_kmax(kmax)
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        self.sums = np.array(sums, dtype=np.float64)
        if self.words.shape != (CHS_CT_WORDS,) or self.sums.shape != (CHS_CT_SUMS,):
            raise ValueError(f"{CHS_CT_WORDS} words and {CHS_CT_SUMS} sums are needed, got {self.words.shape}, {self.sums.shape}")
        w = {name: int(v) for name, v in zip(WORDS, self.words)}
        if min(w.values()) < 0:
            raise ValueError(f"a negative word: {self.words}")
        cells_ = (self.N - 1) ** 2
        if w['segments'] != w['cells_one'] + w['cells_two'] + 2 * w['saddles'] or w['segments'] - w['saddles'] > cells_:
            raise ValueError(f"the segments are not those of the crossed cells: {self.words}")
        if 2 * w['segments'] != 2 * (w['vertices_rows'] + w['vertices_cols']) - w['ends']:
            raise ValueError(f"the segments' ends are not the vertices: {self.words}")
        if w['cells_curv'] + w['cells_wall'] + w['cells_bad'] != w['cells_one'] + w['cells_two']:
            raise ValueError(f"curvature, wall and bad cells do not add up to the crossed cells: {self.words}")
        if w['hist_under'] + w['hist_over'] > w['cells_curv'] or w['l_curv_fix'] > w['l_fix'] or w['n_below'] > self.N ** 2 \
                or w['n_nonfinite'] > self.N ** 2:
            raise ValueError(f"not the words of a contour: {self.words}")
        self.hist = self.hist_length = None
        if hist is not None:
            h = np.array(hist, dtype=np.int64)
            if h.shape != (2, self.bins):
                raise ValueError(f"histograms of shape (2, {self.bins}) are needed, got {h.shape}")
            if np.any(h < 0) or int(h[0].sum()) + w['hist_under'] + w['hist_over'] != w['cells_curv']:
                raise ValueError("the histogram and the cells under and over it do not add up to the curvature cells")
            hl = int(h[1].sum())
            if hl > w['l_curv_fix'] or (w['hist_under'] + w['hist_over'] == 0 and hl != w['l_curv_fix']):
                raise ValueError("the histogram's lengths do not add up to the length of the curvature cells")
            self.hist, self.hist_length = h[0], h[1]
        self.ell_map = self.kappa_map = None
        if map is not None:
            m = np.asarray(map, dtype=np.float64)
            if m.shape != (2, self.N - 1, self.N - 1):
                raise ValueError(f"a map of shape (2, {self.N - 1}, {self.N - 1}) is needed, got {m.shape}")
            self.ell_map, self.kappa_map = m[0], m[1]
        self.length = w['l_fix'] / FIX
        self.length_curv = w['l_curv_fix'] / FIX
        self.length_phys = None if self.delx is None else self.length * self.delx
        self.S_V = self.length / cells_
        self.S_V_phys = None if self.delx is None else self.S_V / self.delx
        pixel = w['vertices_rows'] + w['vertices_cols']
        self.pixel_ratio = pixel / self.length if self.length > 0 else None
        txx, txy, tyy, k1, ka, k2 = (float(v) for v in self.sums)
        lc = self.length_curv
        self.mean_curvature = k1 / lc if lc > 0 else None
        self.mean_abs_curvature = ka / lc if lc > 0 else None
        self.rms_curvature = math.sqrt(k2 / lc) if lc > 0 and k2 >= 0 else None
        per = lambda v: None if v is None or self.delx is None else v / self.delx
        self.mean_curvature_phys, self.mean_abs_curvature_phys, self.rms_curvature_phys = (
            per(self.mean_curvature), per(self.mean_abs_curvature), per(self.rms_curvature))
        self.bending = k2                                # the integral of kappa^2 along the contour, in 1 / pixel

    def word(self, name):
        """One word as a Python integer: ``name`` is one of `WORDS`."""
        return int(self.words[WORDS.index(name)])

    def sum(self, name):
        """One of the six sums: ``name`` is one of `SUMS`."""
        return float(self.sums[SUMS.index(name)])

    def orientation(self):
        """``anisotropy = (TXX - TYY) / (TXX + TYY)`` (+1: every segment along x, the rows), ``offdiag = 2 TXY / (TXX +
        TYY)`` and ``angle``, the principal direction of the tangents in radians from the x axis, in (-pi/2, pi/2]; None
        without a contour."""
        txx, txy, tyy = self.sum('txx'), self.sum('txy'), self.sum('tyy')
        tr = txx + tyy
        if not tr > 0:
            return None
        return types.SimpleNamespace(anisotropy=(txx - tyy) / tr, offdiag=2.0 * txy / tr,
                                     angle=0.5 * math.atan2(2.0 * txy, txx - tyy))

    @property
    def bin_edges(self):
        """float64 [bins + 1]: from -kmax to kmax."""
        return -self.kmax + np.arange(self.bins + 1) * (2.0 * self.kmax / self.bins)

    def quantile(self, q, weight='length'):
        """The curvature below which the fraction q of the histogram lies, by cells or by length (``weight='cells'`` or
        ``'length'``), linear within its bin; None without the histogram or with an empty one."""
        if self.hist is None:
            return None
        if weight not in ('cells', 'length'):
            raise ValueError(f"the weight is 'cells' or 'length', got {weight!r}")
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q in [0, 1] is needed, got {q!r}")
        h = (self.hist if weight == 'cells' else self.hist_length).astype(np.float64)
        total = h.sum()
        if not total > 0:
            return None
        cum = np.cumsum(h)
        k = int(np.searchsorted(cum, q * total, side='left'))
        k = min(k, self.bins - 1)
        before = cum[k] - h[k]
        f = (q * total - before) / h[k] if h[k] > 0 else 0.0
        e = self.bin_edges
        return float(e[k] + f * (e[k + 1] - e[k]))

    def __repr__(self):
        return (f"Contour(N={self.N}, threshold={self.threshold!r}, length={self.length:.6g}, pixel_ratio={self.pixel_ratio}, "
                f"mean_curvature={self.mean_curvature}, cells_curv={self.word('cells_curv')})")
