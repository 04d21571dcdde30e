"""Connected components of the thresholded field -- droplet count, sizes, bounding boxes, spanning: the host side (numpy
only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_components).

Foreground.  For an N x N field U and a finite threshold t: ``side='below'`` is ``X[i][j] = ((double)U[i][j] < t)``,
exactly the foreground of `morphology` (a NaN pixel and a pixel equal to t are background); ``side='above'`` is the
complement inside the grid, ``!((double)U[i][j] < t)`` (a NaN pixel and a pixel equal to t are foreground).

Connectivity.  4 joins edge neighbours, 8 joins edge and corner neighbours.  No wrap-around; nothing outside the grid is
foreground.

Components.  A component is a maximal connected set of foreground pixels; its ``first`` is the smallest linear index
``i*N + j`` of its pixels; components are numbered 0 .. C-1 by ascending ``first``, which makes the result unique.

Table.  One int32 row per component (`COLS`): ``first, area, imin, imax, jmin, jmax``.

Summary.  Seven int64 words (`WORDS`): ``count``; ``area``, the foreground pixels; ``largest``, the largest area (0
without a component); ``sumsq``, the sum of area^2; ``inner``, the components whose bounding box touches none of rows 0
and N-1 and columns 0 and N-1; ``spanning``, those with imin == 0 and imax == N-1, or jmin == 0 and jmax == N-1;
``largest_first``, the ``first`` of the largest component (the smallest on a tie, -1 without one).

Labels.  int32 [N][N]: the component number of the pixel, -1 for background.

With `morphology.Morphology` at the same threshold: ``euler8 == count(below, 8) - inner(above, 4)`` and
``euler4 == count(below, 4) - inner(above, 8)``.
"""
import numpy as np

from . import morphology

WORDS = ('count', 'area', 'largest', 'sumsq', 'inner', 'spanning', 'largest_first')
COLS = ('first', 'area', 'imin', 'imax', 'jmin', 'jmax')
CHS_CC_WORDS, CHS_CC_COLS = len(WORDS), len(COLS)
(CHS_CC_COUNT, CHS_CC_AREA, CHS_CC_LARGEST, CHS_CC_SUMSQ, CHS_CC_INNER, CHS_CC_SPANNING,
 CHS_CC_LARGEST_FIRST) = range(CHS_CC_WORDS)
CHS_CC_BELOW, CHS_CC_ABOVE = 0, 1
SIDES = {'below': CHS_CC_BELOW, 'above': CHS_CC_ABOVE}


def side_code(side):
    """CHS_CC_BELOW / CHS_CC_ABOVE of 'below' / 'above' (or of the code itself)."""
    if side in SIDES:
        return SIDES[side]
    if side in (CHS_CC_BELOW, CHS_CC_ABOVE) and not isinstance(side, bool):
        return int(side)
    raise ValueError(f"side is 'below' or 'above', got {side!r}")


def check_connectivity(connectivity):
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity is 4 or 8, got {connectivity!r}")
    return int(connectivity)


def foreground(U, threshold, side='below'):
    """X of the definition, a boolean N x N array."""
    X = morphology.foreground(U, threshold)
    return ~X if side_code(side) == CHS_CC_ABOVE else X


def label(U, threshold, connectivity=4, side='below'):
    """(labels int32 [N][N], table int32 [C][6]) of the field U: the numpy model of chs_components.  Every foreground
    pixel starts with its own linear index and takes the minimum over its neighbourhood, with pointer jumping between
    the sweeps, until nothing changes: the label is then the component's ``first``.  For small N."""
    connectivity = check_connectivity(connectivity)
    X = foreground(U, threshold, side)
    N = X.shape[0]
    big = N * N
    lab = np.where(X, np.arange(big, dtype=np.int64).reshape(N, N), big)
    shifts = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    while True:
        P = np.full((N + 2, N + 2), big, dtype=np.int64)
        P[1:-1, 1:-1] = lab
        new = lab.copy()
        for di, dj in shifts:
            for sg in (1, -1):
                new = np.minimum(new, P[1 + sg * di:N + 1 + sg * di, 1 + sg * dj:N + 1 + sg * dj])
        new = np.where(X, new, big)
        flat = np.append(new.ravel(), big)          # (entry `big`: background points at itself)
        for _ in range(2):                          # pointer jumping: a pixel takes its label's label
            flat = flat[flat]
        new = np.where(X, flat[:big].reshape(N, N), big)
        if np.array_equal(new, lab):
            break
        lab = new
    firsts = np.unique(lab[X])
    labels = np.full((N, N), -1, dtype=np.int32)
    labels[X] = np.searchsorted(firsts, lab[X]).astype(np.int32)
    C = firsts.size
    table = np.zeros((C, CHS_CC_COLS), dtype=np.int32)
    if C:
        ii, jj = np.nonzero(X)
        k = labels[ii, jj]
        table[:, 0] = firsts
        table[:, 1] = np.bincount(k, minlength=C)
        for col, v, fn in ((2, ii, np.minimum), (3, ii, np.maximum), (4, jj, np.minimum), (5, jj, np.maximum)):
            acc = np.full(C, N if fn is np.minimum else -1, dtype=np.int64)
            fn.at(acc, k, v)
            table[:, col] = acc
    return labels, table


def summary_of(table, N):
    """The seven summary words of a table, an int64 array."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, CHS_CC_COLS)
    first, area, imin, imax, jmin, jmax = table.T
    w = np.zeros(CHS_CC_WORDS, dtype=np.int64)
    w[CHS_CC_COUNT] = table.shape[0]
    w[CHS_CC_AREA] = area.sum()
    w[CHS_CC_SUMSQ] = int(np.sum(area * area))
    w[CHS_CC_INNER] = np.count_nonzero((imin > 0) & (imax < N - 1) & (jmin > 0) & (jmax < N - 1))
    w[CHS_CC_SPANNING] = np.count_nonzero(((imin == 0) & (imax == N - 1)) | ((jmin == 0) & (jmax == N - 1)))
    w[CHS_CC_LARGEST_FIRST] = -1
    if table.shape[0]:
        w[CHS_CC_LARGEST] = area.max()
        w[CHS_CC_LARGEST_FIRST] = first[area == area.max()].min()
    return w


class Components:
    """One look at the components of a field: ``count, area, largest, sumsq, inner, spanning, largest_first`` (Python
    integers), ``areas, first, bbox`` (None without the table; bbox is [C][4]: imin, imax, jmin, jmax), ``labels`` (None
    unless fetched), ``mean_area``, ``weighted_mean_area``, ``radius_eq``, ``size_histogram(bins)``, and ``N``,
    ``threshold``, ``connectivity``, ``side``."""

    def __init__(self, words, N, threshold, connectivity=4, side='below', table=None, labels=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.connectivity = check_connectivity(connectivity)
        self.side = 'above' if side_code(side) == CHS_CC_ABOVE else 'below'
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_CC_WORDS,):
            raise ValueError(f"{CHS_CC_WORDS} words are needed, got shape {self.words.shape}")
        (self.count, self.area, self.largest, self.sumsq, self.inner, self.spanning,
         self.largest_first) = (int(w) for w in self.words)
        if not (0 <= self.count <= self.area <= self.N * self.N and self.largest <= self.area
                and self.inner + self.spanning <= self.count and (self.count == 0) == (self.largest_first == -1)):
            raise ValueError(f"not the summary of a labelling: {self.words}")
        self.table = self.areas = self.first = self.bbox = None
        if table is not None:
            self.table = np.array(table, dtype=np.int32).reshape(-1, CHS_CC_COLS)
            self.first, self.areas, self.bbox = self.table[:, 0], self.table[:, 1], self.table[:, 2:]
            if len(self.areas) != self.count:
                raise ValueError(f"{len(self.areas)} table rows for {self.count} components")
            if int(self.areas.sum(dtype=np.int64)) != self.area:
                raise ValueError(f"the areas add up to {int(self.areas.sum(dtype=np.int64))}, not to {self.area}")
            if np.any(np.diff(self.first.astype(np.int64)) <= 0):
                raise ValueError("`first` is not strictly increasing")
        self.labels = None
        if labels is not None:
            self.labels = np.asarray(labels, dtype=np.int32)
            if self.labels.shape != (self.N, self.N):
                raise ValueError(f"labels of shape {(self.N, self.N)} are needed, got {self.labels.shape}")

    @property
    def mean_area(self):
        return self.area / self.count if self.count else 0.0

    @property
    def weighted_mean_area(self):
        return self.sumsq / self.area if self.area else 0.0

    @property
    def radius_eq(self):
        """The radius of the disc of every component's area, in the solver's unit (in pixels without ``delx``)."""
        if self.areas is None:
            return None
        return np.sqrt(self.areas / np.pi) * (1.0 if self.delx is None else self.delx)

    def size_histogram(self, bins=10):
        """``numpy.histogram`` of the areas: (counts, bin edges)."""
        if self.areas is None:
            raise ValueError("the size histogram needs the table")
        return np.histogram(self.areas, bins=bins)

    def __repr__(self):
        return (f"Components(N={self.N}, threshold={self.threshold!r}, connectivity={self.connectivity}, side={self.side!r}, "
                f"count={self.count}, area={self.area}, largest={self.largest}, spanning={self.spanning})")
