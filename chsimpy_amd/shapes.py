"""The shape of every droplet -- moments, perimeter, holes, composition per connected component: the host side (numpy
only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_shapes).

The foreground X, the connectivity (4 or 8), the side, the components and their numbering by ascending ``first`` are
exactly those of `components`.  Pixel (i, j) has p = i N + j and x = (double)U[i][j].

Table.  One int64 row per component k (`COLS`):

    first      that of the component table
    area       pixels of k
    pairs_h    pixels (i, j) of k whose right neighbour (i, j+1) is foreground
    pairs_v    pixels (i, j) of k whose lower neighbour (i+1, j) is foreground
    pairs_d    connectivity 8 only, otherwise 0: the diagonal foreground pairs {(i,j), (i+1,j+1)} and {(i,j+1), (i+1,j)},
               each counted for the component of its upper pixel
    triples    connectivity 8 only, otherwise 0: the 2 x 2 cells with exactly three foreground pixels, counted for the
               component of the cell's first foreground pixel in the order a, b, c, d of `contour`
               (a = (i,j), b = (i,j+1), c = (i+1,j), d = (i+1,j+1))
    quads      the 2 x 2 cells with four foreground pixels, counted for the component of the cell's upper left pixel
    wall       unit pixel edges of k that lie on the grid's boundary (a corner pixel has two)
    si, sj, sii, sjj, sij    the sums of i, j, i^2, j^2, i j over the pixels of k
    su_fix     the sum of fix(x) over the pixels of k with fabs(x) <= 4.0
    suu_fix    the sum of fix(x x) over the same pixels, the product rounded once in double
    n_outside  pixels of k with not (fabs(x) <= 4.0): NaN, infinite, or far outside the physical range

``fix(y) = (int64)(y 2^30)``, truncated: the fixed point of `contour` (``CHS_CT_FIX_BITS``).  All pixels of a pair or a
cell that is counted belong to one component under the connectivity it is counted for, so the "counted for" rules only
make the owner unique.  With N <= 16384 no sum reaches 2^63.  Every cell is an integer and every accumulation an integer
add, so the device's table is this model's bit for bit, for both element types.

Summary.  17 int64 words (`WORDS`): the seven of `components`; the column sums of ``area, pairs_h, pairs_v, pairs_d,
triples, quads, wall, n_outside``; ``holes``, the sum of ``1 - euler`` over the components; ``inner_round``, the
components with ``wall == 0``.

Euler number of a component taken alone: ``area - pairs_h - pairs_v + quads`` at connectivity 4 (pixels, edges and unit
squares of the cubical complex) and ``area - pairs_h - pairs_v - pairs_d + triples + 3 quads`` at connectivity 8
(vertices, edges, triangles -- one per cell of three, four per cell of four -- minus the cell of four's one tetrahedron).
``holes = 1 - euler``: an island inside a hole does not fill it.
"""
import numpy as np

from . import components

COLS = ('first', 'area', 'pairs_h', 'pairs_v', 'pairs_d', 'triples', 'quads', 'wall', 'si', 'sj', 'sii', 'sjj', 'sij',
        'su_fix', 'suu_fix', 'n_outside')
SUMMED = ('area', 'pairs_h', 'pairs_v', 'pairs_d', 'triples', 'quads', 'wall', 'n_outside')
WORDS = components.WORDS + tuple('sum_' + c for c in SUMMED) + ('holes', 'inner_round')
CHS_SH_COLS, CHS_SH_WORDS = len(COLS), len(WORDS)
(CHS_SH_FIRST, CHS_SH_AREA, CHS_SH_PAIRS_H, CHS_SH_PAIRS_V, CHS_SH_PAIRS_D, CHS_SH_TRIPLES, CHS_SH_QUADS, CHS_SH_WALL,
 CHS_SH_SI, CHS_SH_SJ, CHS_SH_SII, CHS_SH_SJJ, CHS_SH_SIJ, CHS_SH_SU_FIX, CHS_SH_SUU_FIX, CHS_SH_N_OUTSIDE) = range(CHS_SH_COLS)
(CHS_SH_SUM_AREA, CHS_SH_SUM_PAIRS_H, CHS_SH_SUM_PAIRS_V, CHS_SH_SUM_PAIRS_D, CHS_SH_SUM_TRIPLES, CHS_SH_SUM_QUADS,
 CHS_SH_SUM_WALL, CHS_SH_SUM_N_OUTSIDE, CHS_SH_HOLES, CHS_SH_INNER_ROUND) = range(components.CHS_CC_WORDS, CHS_SH_WORDS)
FIX_BITS = 30
FIX = float(1 << FIX_BITS)
U_RANGE = 4.0          # fabs(x) <= U_RANGE enters su_fix and suu_fix


def fix(y):
    """(int64)(y 2^30), truncated."""
    return (np.asarray(y, dtype=np.float64) * FIX).astype(np.int64)


_SPLIT = 20


def _sums_by(k, C, *values):
    """For every int64 array v of `values` (|v| < 2^34) the exact int64 sums of v over the entries of every number of k
    (in [0, C)).  A float bincount of v itself would round from 2^53 on; v = hi 2^20 + lo with 0 <= lo < 2^20 and
    |hi| <= 2^14 gives two bincounts whose partial sums are integers below 2^20 2^28 = 2^48 -- exact in double."""
    out = []
    for v in values:
        v = np.asarray(v, dtype=np.int64)
        lo = np.bincount(k, weights=(v & ((1 << _SPLIT) - 1)).astype(np.float64), minlength=C)
        hi = np.bincount(k, weights=(v >> _SPLIT).astype(np.float64), minlength=C)
        out.append((hi.astype(np.int64) << _SPLIT) + lo.astype(np.int64))
    return out


def shape_table(U, threshold, connectivity=4, side='below', labels=None):
    """int64 [C][16] of the field U: the numpy model of chs_shapes, vectorised (bincounts over the label image, the
    wide sums in two exact halves).  ``labels``: the label image of the same look (int32 [N][N], the numbering of
    `components`) where the caller has it -- `components.label`, which finds it otherwise, is for small N."""
    connectivity = components.check_connectivity(connectivity)
    X = components.foreground(U, threshold, side)
    N = X.shape[0]
    if labels is None:
        labels = components.label(U, threshold, connectivity, side)[0]
    lab = np.asarray(labels).astype(np.int64)
    if lab.shape != (N, N) or not np.array_equal(lab >= 0, X):
        raise ValueError("the labels are not those of this foreground")
    C = int(lab.max()) + 1 if X.any() else 0
    table = np.zeros((C, CHS_SH_COLS), dtype=np.int64)
    if C == 0:
        return table

    def count(mask, owner):
        return np.bincount(owner[mask], minlength=C)

    ii, jj = np.nonzero(X)
    k = lab[ii, jj]
    first = np.full(C, N * N, dtype=np.int64)
    first[k[::-1]] = (ii * N + jj)[::-1]                  # (descending index: the smallest is written last)
    table[:, CHS_SH_FIRST] = first
    table[:, CHS_SH_AREA] = np.bincount(k, minlength=C)
    table[:, CHS_SH_PAIRS_H] = count(X[:, :-1] & X[:, 1:], lab[:, :-1])
    table[:, CHS_SH_PAIRS_V] = count(X[:-1, :] & X[1:, :], lab[:-1, :])
    a, b, c, d = X[:-1, :-1], X[:-1, 1:], X[1:, :-1], X[1:, 1:]
    la, lb = lab[:-1, :-1], lab[:-1, 1:]
    if connectivity == 8:
        table[:, CHS_SH_PAIRS_D] = count(a & d, la) + count(b & c, lb)
        three = (a.astype(np.int8) + b + c + d) == 3
        table[:, CHS_SH_TRIPLES] = count(three & a, la) + count(three & ~a, lb)
    table[:, CHS_SH_QUADS] = count(a & b & c & d, la)
    edges = (ii == 0).astype(np.int64) + (ii == N - 1) + (jj == 0) + (jj == N - 1)
    table[:, CHS_SH_WALL] = np.bincount(k, weights=edges, minlength=C)
    x = np.asarray(U).astype(np.float64)[ii, jj]
    with np.errstate(invalid='ignore'):
        inside = np.abs(x) <= U_RANGE                     # (False for a NaN)
    xin = np.where(inside, x, 0.0)
    (table[:, CHS_SH_SI], table[:, CHS_SH_SJ], table[:, CHS_SH_SII], table[:, CHS_SH_SJJ], table[:, CHS_SH_SIJ],
     table[:, CHS_SH_SU_FIX], table[:, CHS_SH_SUU_FIX]) = _sums_by(k, C, ii, jj, ii * ii, jj * jj, ii * jj, fix(xin), fix(xin * xin))
    table[:, CHS_SH_N_OUTSIDE] = np.bincount(k[~inside], minlength=C)
    return table


def euler_of(table, connectivity):
    """The Euler number of every row, int64."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, CHS_SH_COLS)
    e = t[:, CHS_SH_AREA] - t[:, CHS_SH_PAIRS_H] - t[:, CHS_SH_PAIRS_V]
    if components.check_connectivity(connectivity) == 8:
        return e - t[:, CHS_SH_PAIRS_D] + t[:, CHS_SH_TRIPLES] + 3 * t[:, CHS_SH_QUADS]
    return e + t[:, CHS_SH_QUADS]


def summary_of(table, cc_words, connectivity):
    """The 17 summary words of a shape table behind the seven words of the components look, an int64 array."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, CHS_SH_COLS)
    w = np.zeros(CHS_SH_WORDS, dtype=np.int64)
    w[:components.CHS_CC_WORDS] = cc_words
    for n, c in enumerate(SUMMED):
        w[components.CHS_CC_WORDS + n] = t[:, COLS.index(c)].sum()
    w[CHS_SH_HOLES] = (1 - euler_of(t, connectivity)).sum()
    w[CHS_SH_INNER_ROUND] = np.count_nonzero(t[:, CHS_SH_WALL] == 0)
    return w


def look(U, threshold, connectivity=4, side='below', delx=None, labels=None):
    """The `Shapes` of the field U from the numpy model alone (no device)."""
    N = np.asarray(U).shape[0]
    if labels is None:
        labels, cc_table = components.label(U, threshold, connectivity, side)
    else:
        cc_table = _cc_table_of(labels)
    co = components.Components(components.summary_of(cc_table, N), N, threshold, connectivity, side, table=cc_table,
                               labels=labels, delx=delx)
    table = shape_table(U, threshold, connectivity, side, labels=labels)
    return Shapes(summary_of(table, co.words, connectivity), table, co)


def _cc_table_of(labels):
    """The component table of a label image numbered by ascending `first`."""
    lab = np.asarray(labels)
    N = lab.shape[0]
    ii, jj = np.nonzero(lab >= 0)
    k = lab[ii, jj].astype(np.int64)
    C = int(k.max()) + 1 if k.size else 0
    table = np.zeros((C, components.CHS_CC_COLS), dtype=np.int32)
    if C:
        table[:, 1] = np.bincount(k, minlength=C)
        for col, v, fn, start in ((0, ii * N + jj, np.minimum, N * N), (2, ii, np.minimum, N), (3, ii, np.maximum, -1),
                                  (4, jj, np.minimum, N), (5, jj, np.maximum, -1)):
            acc = np.full(C, start, dtype=np.int64)
            fn.at(acc, k, v)
            table[:, col] = acc
    return table


class Shapes:
    """One look at the shapes of the droplets of a field, from the exact integers of the device's table.

    ``Shapes(words, table, components)``: the 17 summary words, the int64 [C][16] table and the `components.Components`
    (with its table) of the same look, from which ``N, threshold, connectivity, side, delx`` are taken.  The constructor
    checks what holds of any true table and raises ValueError otherwise: rows, ``first`` and ``area`` are the component
    table's; ``imin area <= si <= imax area`` and the same for ``sj``; ``pairs_h, pairs_v < area``; ``quads <=
    min(pairs_h, pairs_v)``; ``euler <= 1``; ``n_outside <= area``; the summary words are the column sums.

    Per component, numpy arrays of length ``count`` (everything that is a difference of large products is formed from
    Python integers first: ``area sii - si^2`` does not fit 64 bits):

    ``first, area, pairs_h, ... n_outside``  the columns; ``euler``; ``holes`` = 1 - euler;
    ``perimeter`` = 4 area - 2 (pairs_h + pairs_v), in unit edges, walls included; ``perimeter_inner`` = perimeter - wall;
    ``circularity_pixel`` = 4 pi area / perimeter^2; ``circularity``, the same with the perimeter scaled by pi / 4 (the
    isotropic correction of a pixel staircase, the 4 / pi of `contour.Contour.pixel_ratio`);
    ``centroid`` [C][2]: (si / area, sj / area);
    ``mu_ii, mu_jj, mu_ij``: the central second moments, the pixel's own 1 / 12 added to the two diagonal ones;
    ``major, minor`` = 4 sqrt(lambda+), 4 sqrt(lambda-): the axes of the ellipse of equal moments, the convention of
    scikit-image's regionprops; ``aspect`` = major / minor; ``eccentricity`` = sqrt(1 - lambda- / lambda+);
    ``orientation`` in (-pi/2, pi/2]: the angle of the major axis from the x axis (the direction of increasing j)
    towards the direction of increasing i; 0 for a round component;
    ``radius_eq``: as in `Components` (scaled by ``delx`` when there is one);
    ``mean_u, var_u``: mean and variance of the composition over the ``area - n_outside`` pixels inside the range, NaN
    where there is none (`mean_u_of(k)`, `var_u_of(k)` return None there).  Truncation: every fix() falls short by less
    than 2^-30 in magnitude, so |mean_u - the exact mean| < 2^-30; the mean of x x is off by less than 2^-30 + 16 2^-53
    (truncation, and the one rounding of the product), and mean_u^2 by less than 2 * 4 * 2^-30 (|x| <= 4), so
    |var_u - the exact variance| < 9 2^-30 + 2^-49 (`MEAN_U_BOUND`, `VAR_U_BOUND`);
    ``touches_wall``: wall > 0.

    `nearest_neighbour()`: centre-to-centre distance of every component to the closest other centroid (scipy's cKDTree
    on the host; inf with fewer than two components).  `population()`: summaries over the inner components (wall == 0),
    number- and area-weighted, and the (radius_eq, mean_u) pairs of a Gibbs-Thomson plot.  With ``delx``:
    ``centroid_phys, major_phys, minor_phys, perimeter_phys, perimeter_inner_phys`` (else None).
    """

    MEAN_U_BOUND = 2.0 ** -30
    VAR_U_BOUND = 9 * 2.0 ** -30 + 2.0 ** -49

    def __init__(self, words, table, components_look):
        co = components_look
        if not isinstance(co, components.Components) or co.table is None:
            raise ValueError("the Components of the same look, with its table, are needed")
        self.components = co
        self.N, self.threshold, self.connectivity, self.side, self.delx = co.N, co.threshold, co.connectivity, co.side, co.delx
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_SH_WORDS,):
            raise ValueError(f"{CHS_SH_WORDS} words are needed, got shape {self.words.shape}")
        self.table = np.array(table, dtype=np.int64).reshape(-1, CHS_SH_COLS)
        t = self.table
        for n, c in enumerate(COLS):
            setattr(self, c, t[:, n])
        self.count = t.shape[0]
        if not np.array_equal(self.words[:components.CHS_CC_WORDS], co.words):
            raise ValueError("the first seven words are not those of the components look")
        if self.count != co.count:
            raise ValueError(f"{self.count} table rows for {co.count} components")
        if not np.array_equal(self.first, co.first) or not np.array_equal(self.area, co.areas):
            raise ValueError("`first` and `area` are not those of the component table")
        bb = co.bbox.astype(np.int64)
        if np.any(bb[:, 0] * self.area > self.si) or np.any(self.si > bb[:, 1] * self.area):
            raise ValueError("si outside [imin area, imax area]")
        if np.any(bb[:, 2] * self.area > self.sj) or np.any(self.sj > bb[:, 3] * self.area):
            raise ValueError("sj outside [jmin area, jmax area]")
        if np.any(t[:, 1:CHS_SH_SIJ + 1] < 0) or np.any(self.n_outside < 0) or np.any(self.suu_fix < 0):
            raise ValueError("a negative count")
        if np.any(self.pairs_h >= self.area) or np.any(self.pairs_v >= self.area):
            raise ValueError("pairs_h and pairs_v are below the area")
        if np.any(self.quads > np.minimum(self.pairs_h, self.pairs_v)):
            raise ValueError("quads above min(pairs_h, pairs_v)")
        self.euler = euler_of(t, self.connectivity)
        if np.any(self.euler > 1):
            raise ValueError("an Euler number above 1")
        if np.any(self.n_outside > self.area):
            raise ValueError("n_outside above the area")
        want = summary_of(t, co.words, self.connectivity)
        if not np.array_equal(self.words, want):
            raise ValueError(f"the summary words are not the column sums: {self.words} against {want}")
        self.holes = 1 - self.euler
        self.total_holes, self.inner_round = int(self.words[CHS_SH_HOLES]), int(self.words[CHS_SH_INNER_ROUND])
        self.perimeter = 4 * self.area - 2 * (self.pairs_h + self.pairs_v)
        self.perimeter_inner = self.perimeter - self.wall
        self.touches_wall = self.wall > 0
        area = self.area.astype(np.float64)
        per = self.perimeter.astype(np.float64)
        self.circularity_pixel = 4.0 * np.pi * area / (per * per)
        self.circularity = self.circularity_pixel * (4.0 / np.pi) ** 2
        self.centroid = np.stack([self.si / area, self.sj / area], axis=1) if self.count else np.zeros((0, 2))
        self._moments()
        self._composition()
        s = self.delx
        self.centroid_phys = None if s is None else self.centroid * s
        self.major_phys = None if s is None else self.major * s
        self.minor_phys = None if s is None else self.minor * s
        self.perimeter_phys = None if s is None else self.perimeter * s
        self.perimeter_inner_phys = None if s is None else self.perimeter_inner * s

    def _moments(self):
        C = self.count
        mu = np.zeros((3, C))
        cols = [[int(v) for v in self.table[:, c]] for c in (CHS_SH_AREA, CHS_SH_SI, CHS_SH_SJ, CHS_SH_SII, CHS_SH_SJJ, CHS_SH_SIJ)]
        for k, (a, si, sj, sii, sjj, sij) in enumerate(zip(*cols)):   # exact integers, one division each
            a2 = a * a
            mu[0, k] = (a * sii - si * si) / a2
            mu[1, k] = (a * sjj - sj * sj) / a2
            mu[2, k] = (a * sij - si * sj) / a2
        self.mu_ii, self.mu_jj, self.mu_ij = mu[0] + 1.0 / 12.0, mu[1] + 1.0 / 12.0, mu[2]
        half = 0.5 * (self.mu_ii + self.mu_jj)
        diff = 0.5 * (self.mu_jj - self.mu_ii)
        root = np.hypot(diff, self.mu_ij)
        lp, lm = half + root, np.maximum(half - root, 0.0)
        self.major, self.minor = 4.0 * np.sqrt(lp), 4.0 * np.sqrt(lm)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.aspect = self.major / self.minor
            self.eccentricity = np.sqrt(np.maximum(1.0 - lm / lp, 0.0))
        self.orientation = 0.5 * np.arctan2(2.0 * self.mu_ij, self.mu_jj - self.mu_ii)

    def _composition(self):
        C = self.count
        self.n_inside = self.area - self.n_outside
        self.mean_u, self.var_u = np.full(C, np.nan), np.full(C, np.nan)
        for k in np.flatnonzero(self.n_inside > 0):
            n, su, suu = int(self.n_inside[k]), int(self.su_fix[k]), int(self.suu_fix[k])
            self.mean_u[k] = su / (n << FIX_BITS)
            self.var_u[k] = ((n * suu << FIX_BITS) - su * su) / (n * n << (2 * FIX_BITS))

    def mean_u_of(self, k):
        """The mean composition of component k, None where no pixel of it lies inside the range."""
        return float(self.mean_u[k]) if self.n_inside[k] > 0 else None

    def var_u_of(self, k):
        return float(self.var_u[k]) if self.n_inside[k] > 0 else None

    @property
    def radius_eq(self):
        """The radius of the disc of every component's area, in the solver's unit (in pixels without ``delx``)."""
        return self.components.radius_eq

    def nearest_neighbour(self):
        """The distance from every centroid to the closest other one, in the solver's unit (pixels without ``delx``);
        inf with fewer than two components."""
        if self.count < 2:
            return np.full(self.count, np.inf)
        from scipy.spatial import cKDTree
        d, _ = cKDTree(self.centroid).query(self.centroid, k=2)
        return d[:, 1] * (1.0 if self.delx is None else self.delx)

    def population(self):
        """Over the inner components (wall == 0): ``count``; ``mean_circularity``, ``mean_aspect``, ``mean_radius_eq``
        and their area-weighted twins ``*_by_area`` (None without an inner component); ``radius_eq`` and ``mean_u``,
        the pairs of a Gibbs-Thomson plot (the inner components with a composition)."""
        inner = ~self.touches_wall
        n = int(inner.sum())
        out = {'count': n}
        w = self.area[inner].astype(np.float64)
        for name, v in (('mean_circularity', self.circularity), ('mean_aspect', self.aspect), ('mean_radius_eq', self.radius_eq)):
            out[name] = float(np.mean(v[inner])) if n else None
            out[name + '_by_area'] = float(np.sum(v[inner] * w) / np.sum(w)) if n else None
        has = inner & (self.n_inside > 0)
        out['radius_eq'], out['mean_u'] = self.radius_eq[has], self.mean_u[has]
        return out

    def __repr__(self):
        return (f"Shapes(N={self.N}, threshold={self.threshold!r}, connectivity={self.connectivity}, side={self.side!r}, "
                f"count={self.count}, holes={self.total_holes}, inner_round={self.inner_round})")
