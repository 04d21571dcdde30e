"""Geodesic look at a phase of the thresholded field -- distance from a wall through the phase alone, geodesic tortuosity,
accessible fraction: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_geodesic).

Foreground.  Foreground, ``side`` ('below' / 'above') and ``connectivity`` (4 or 8) are those of `components`, with no
wrap-around.

Source and target.  ``source`` is one of four walls: 0 'top' is row 0, 1 'bottom' is row N-1, 2 'left' is column 0, 3
'right' is column N-1.  The target is the opposite wall.  The depth k of a pixel is its distance in pixels from the source
wall along that axis, 0 to N-1.

Steps.  A path moves from a foreground pixel to a foreground neighbour.  At connectivity 4 an axial step costs 1 and there
is no diagonal step: ``UNIT`` = 1.  At connectivity 8 an axial step costs 3 and a diagonal step 4 (the 3-4 chamfer
metric): ``UNIT`` = 3.  A diagonal step needs only its two end pixels to be foreground -- the rule that makes them one
component at connectivity 8.  In free space G / UNIT lies within [0.9428, 1.0541] of the Euclidean length.

The map.  ``G[p]`` is an int32: -1 for background, 0 for a foreground pixel on the source wall, otherwise the smallest
cost of a path from any such pixel to p; `CHS_GEO_INF` (INT32_MAX) marks a foreground pixel that no path reaches.

Result words (`WORDS`, int64): ``fg``; ``sources``, the foreground pixels on the source wall; ``reached``, sources
included; ``target_fg`` and ``target_reached`` on the target wall; ``gmin_target``, the smallest G on the target wall, and
``gmin_target_pos``, the smallest position along the wall that has it (-1 when none is reached); ``gsum_target``;
``gmax``, the largest G of a reached pixel, and ``gmax_first``, the smallest linear index that has it (-1 when none);
``gsum``; ``unit``; ``cc_count``, the components of the components look, and ``cc_reached``, those that hold a source
pixel; ``rounds``, the relaxation rounds used, and ``limit``, the round limit that applied.  Every word but ``rounds`` is
unique for a given field and arguments; ``rounds`` is only ever compared with bounds (the model reports the least a look
can use: 1, or 0 without a source pixel).

Histogram.  ``bins(N)`` = 4N bins of int64: bin d counts the reached pixels with ``G // UNIT == d``; the last bin takes
everything at or beyond 4N - 1.  Its running sum is the accessible amount of phase within depth d of the face.

Profile.  [N][3] int64: for every depth k the foreground pixels, the reached pixels and the sum of G over the reached
pixels of that line.  Line N-1 repeats ``target_fg``, ``target_reached`` and ``gsum_target``.

The model exists twice -- `relax`, vectorised sweeps to the fixed point, and `dijkstra`, a plain heap Dijkstra -- and
tests/test_geodesic_host.py holds one against the other.
"""
import heapq

import numpy as np

from . import components

WORDS = ('fg', 'sources', 'reached', 'target_fg', 'target_reached', 'gmin_target', 'gmin_target_pos', 'gsum_target', 'gmax',
         'gmax_first', 'gsum', 'unit', 'cc_count', 'cc_reached', 'rounds', 'limit')
CHS_GEO_WORDS = len(WORDS)
(CHS_GEO_FG, CHS_GEO_SOURCES, CHS_GEO_REACHED, CHS_GEO_TARGET_FG, CHS_GEO_TARGET_REACHED, CHS_GEO_GMIN_TARGET,
 CHS_GEO_GMIN_TARGET_POS, CHS_GEO_GSUM_TARGET, CHS_GEO_GMAX, CHS_GEO_GMAX_FIRST, CHS_GEO_GSUM, CHS_GEO_UNIT, CHS_GEO_CC_COUNT,
 CHS_GEO_CC_REACHED, CHS_GEO_ROUNDS, CHS_GEO_LIMIT) = range(CHS_GEO_WORDS)
UNIQUE = [k for k in range(CHS_GEO_WORDS) if k != CHS_GEO_ROUNDS]     # the words two looks must agree on
CHS_GEO_INF = 2 ** 31 - 1
TILE = 64
SOURCES = {'top': 0, 'bottom': 1, 'left': 2, 'right': 3}
SOURCE_NAMES = ('top', 'bottom', 'left', 'right')
CHAMFER_BOUNDS = (0.9428, 1.0541)     # G / UNIT over the Euclidean length in free space at connectivity 8

_BIG = 1 << 40                        # the model's "unreached" while it works: above every cost
_RUN = 1 << 43                        # what separates the runs of a line in a scan: above _BIG + every cost


def source_code(source):
    """0 .. 3 of 'top' / 'bottom' / 'left' / 'right' (or of the code itself)."""
    if source in SOURCES:
        return SOURCES[source]
    if source in (0, 1, 2, 3) and not isinstance(source, bool):
        return int(source)
    raise ValueError(f"source is 'top', 'bottom', 'left' or 'right', got {source!r}")


def unit_of(connectivity):
    return 3 if components.check_connectivity(connectivity) == 8 else 1


def bins(N):
    """The length of the histogram at grid size N (chs_geodesic_bins)."""
    return 4 * int(N)


def rounds_default(N):
    """The default round limit at grid size N (chs_geodesic_rounds_default): 32 nt^2 + 64, nt = ceil(N / 64)."""
    nt = -(-int(N) // TILE)
    return 32 * nt * nt + 64


def depth_of(N, source):
    """int [N][N]: the depth of every pixel from the source wall."""
    code = source_code(source)
    k = np.arange(N)
    line = k if code in (0, 2) else N - 1 - k
    return np.broadcast_to(line[:, None] if code < 2 else line[None, :], (N, N))


def _to_top(A, code):
    """The array seen with the source wall as row 0 (a view); `_from_top` undoes it.  The step costs are symmetric."""
    return (A, A[::-1], A.T, A[:, ::-1].T)[code]


def _from_top(A, code):
    return (A, A[::-1], A.T, A.T[:, ::-1])[code]


# ---------------------------------------------------------------------------
# the model, twice
# ---------------------------------------------------------------------------
def _scan(G, X, a):
    """Every row of G relaxed along itself, left to right: G[j] <- min over k <= j of the same run of foreground of
    G[k] + a (j - k).  A running minimum of G - a j; the runs are kept apart by an offset that falls from run to run."""
    j = np.arange(G.shape[-1], dtype=np.int64)
    off = a * j + _RUN * np.cumsum(~X, axis=-1)
    return np.where(X, np.minimum(G, np.minimum.accumulate(G - off, axis=-1) + off), _BIG)


def _row_step(G, X, i, k, a, d, frozen=None):
    """Row i relaxed against row k (the one above or below) and along itself; True if it fell anywhere.  A pixel of
    `frozen` gives its value on and takes none."""
    prev = G[k]
    cand = prev + a
    if d:
        cand[1:] = np.minimum(cand[1:], prev[:-1] + d)
        cand[:-1] = np.minimum(cand[:-1], prev[1:] + d)
    hold = (lambda row: row) if frozen is None else (lambda row: np.where(frozen[i], G[i], row))
    row = hold(np.where(X[i], np.minimum(G[i], cand), _BIG))
    row = hold(_scan(row, X[i], a))
    row = hold(_scan(row[::-1], X[i][::-1], a)[::-1])
    fell = bool(np.any(row < G[i]))
    G[i] = row
    return fell


def relax(X, connectivity=8, source='top'):
    """G (int32 [N][N]) of the boolean foreground X by vectorised relaxation: rows downwards, each against the row above
    and along itself, then upwards against the row below, until a whole pass lowers nothing.  Every edge is then relaxed:
    the fixed point, which -- the values being costs of real paths -- is the map of the definition."""
    code = source_code(source)
    a = unit_of(connectivity)
    d = 4 if a == 3 else 0
    X = np.ascontiguousarray(_to_top(np.asarray(X, dtype=bool), code))
    N = X.shape[0]
    G = np.full((N, N), _BIG, dtype=np.int64)
    G[0, X[0]] = 0
    fell = True
    while fell:
        fell = False
        for i in range(1, N):
            fell |= _row_step(G, X, i, i - 1, a, d)
        for i in range(N - 2, -1, -1):
            fell |= _row_step(G, X, i, i + 1, a, d)
    out = np.where(X, np.where(G >= _BIG, CHS_GEO_INF, G), -1).astype(np.int32)
    return np.ascontiguousarray(_from_top(out, code))


def _steps(connectivity):
    a = unit_of(connectivity)
    s = [(-1, 0, a), (1, 0, a), (0, -1, a), (0, 1, a)]
    if a == 3:
        s += [(-1, -1, 4), (-1, 1, 4), (1, -1, 4), (1, 1, 4)]
    return s


def dijkstra(X, connectivity=8, source='top'):
    """G of the boolean foreground X by a plain heap Dijkstra from all the source pixels at once.  For small N."""
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    depth = depth_of(N, source)
    steps = _steps(connectivity)
    G = np.where(X, CHS_GEO_INF, -1).astype(np.int64)
    heap = []
    for i, j in zip(*np.nonzero(X & (depth == 0))):
        G[i, j] = 0
        heap.append((0, int(i), int(j)))
    heapq.heapify(heap)
    while heap:
        g, i, j = heapq.heappop(heap)
        if g > G[i, j]:
            continue
        for di, dj, w in steps:
            y, x = i + di, j + dj
            if 0 <= y < N and 0 <= x < N and X[y, x] and g + w < G[y, x]:
                G[y, x] = g + w
                heapq.heappush(heap, (g + w, y, x))
    return G.astype(np.int32)


def certificate(G, connectivity=8, source='top'):
    """The violations of (a) to (d) of the definition by the map G, counted per pixel and neighbour as the device counts
    them: 0 exactly when G holds the shortest-path costs of its own foreground (G >= 0)."""
    G = np.asarray(G, dtype=np.int64)
    N = G.shape[0]
    fgm = G >= 0
    reached = fgm & (G != CHS_GEO_INF)
    P = np.full((N + 2, N + 2), -1, dtype=np.int64)
    P[1:-1, 1:-1] = G
    bad = 0
    pred = np.zeros((N, N), dtype=bool)
    for di, dj, w in _steps(connectivity):
        Q = P[1 + di:N + 1 + di, 1 + dj:N + 1 + dj]
        qfg = Q >= 0
        bad += int(np.count_nonzero(fgm & ~reached & qfg & (Q != CHS_GEO_INF)))                  # (d)
        bad += int(np.count_nonzero(reached & qfg & ((Q == CHS_GEO_INF) | (Q > G + w))))        # (a)
        pred |= reached & qfg & (Q != CHS_GEO_INF) & (Q + w == G)
    bad += int(np.count_nonzero(fgm & ((G == 0) != (depth_of(N, source) == 0))))                # (c)
    bad += int(np.count_nonzero(reached & (G > 0) & ~pred))                                     # (b)
    bad += int(np.count_nonzero(G < -1))
    return bad


def stats_of(G, connectivity=8, source='top', cc_count=0, cc_reached=0, rounds=None, limit=None):
    """(words int64 [16], hist int64 [4N], profile int64 [N][3]) of a map G."""
    G = np.asarray(G, dtype=np.int64)
    N = G.shape[0]
    code = source_code(source)
    unit = unit_of(connectivity)
    depth = depth_of(N, code)
    fgm = G >= 0
    reached = fgm & (G != CHS_GEO_INF)
    Gr = np.where(reached, G, 0)
    w = np.zeros(CHS_GEO_WORDS, dtype=np.int64)
    w[CHS_GEO_FG] = fgm.sum()
    w[CHS_GEO_SOURCES] = (fgm & (depth == 0)).sum()
    w[CHS_GEO_REACHED] = reached.sum()
    target = depth == N - 1
    w[CHS_GEO_TARGET_FG] = (fgm & target).sum()
    tr = reached & target
    w[CHS_GEO_TARGET_REACHED] = tr.sum()
    w[CHS_GEO_GMIN_TARGET] = w[CHS_GEO_GMIN_TARGET_POS] = -1
    if tr.any():
        gmin = G[tr].min()
        ii, jj = np.nonzero(tr & (G == gmin))
        w[CHS_GEO_GMIN_TARGET] = gmin
        w[CHS_GEO_GMIN_TARGET_POS] = (jj if code < 2 else ii).min()
    w[CHS_GEO_GSUM_TARGET] = Gr[target].sum()
    w[CHS_GEO_GMAX] = w[CHS_GEO_GMAX_FIRST] = -1
    if reached.any():
        gmax = G[reached].max()
        w[CHS_GEO_GMAX] = gmax
        w[CHS_GEO_GMAX_FIRST] = np.flatnonzero((reached & (G == gmax)).ravel())[0]
    w[CHS_GEO_GSUM] = Gr.sum()
    w[CHS_GEO_UNIT] = unit
    w[CHS_GEO_CC_COUNT], w[CHS_GEO_CC_REACHED] = cc_count, cc_reached
    w[CHS_GEO_ROUNDS] = (1 if w[CHS_GEO_SOURCES] else 0) if rounds is None else rounds
    w[CHS_GEO_LIMIT] = rounds_default(N) if limit is None else limit
    nb = bins(N)
    hist = np.bincount(np.minimum(G[reached] // unit, nb - 1), minlength=nb).astype(np.int64)
    profile = np.zeros((N, 3), dtype=np.int64)
    k = depth.ravel()
    profile[:, 0] = np.bincount(k, weights=fgm.ravel(), minlength=N)
    profile[:, 1] = np.bincount(k, weights=reached.ravel(), minlength=N)
    np.add.at(profile[:, 2], k, Gr.ravel())
    return w, hist, profile


def model_look(U, t, connectivity=8, side='below', source='top', method='relax', limit=None):
    """The `Geodesic` of the field U thresholded at t: the numpy model of chs_geodesic, by `relax` or by `dijkstra`."""
    X = components.foreground(U, t, side)
    N = X.shape[0]
    G = {'relax': relax, 'dijkstra': dijkstra}[method](X, connectivity, source)
    labels, table = components.label(U, t, connectivity, side)
    holds = np.unique(labels[X & (depth_of(N, source) == 0)])
    words, hist, profile = stats_of(G, connectivity, source, cc_count=table.shape[0], cc_reached=holds.size, limit=limit)
    return Geodesic(words, N, t, connectivity, side, source, hist=hist, profile=profile, g=G)


# ---------------------------------------------------------------------------
# the synchronous tile model: a bound for the rounds of a device look
# ---------------------------------------------------------------------------
def _tile_fixed_point(W, XW, a, d, woke):
    """The window W (a tile and its one-pixel halo, int64, _BIG where there is no cost) with the tile's own pixels
    relaxed to the fixed point and the halo held fixed.  `woke` marks the pixels of the window that fell since the tile
    was at its fixed point: only the rows beside them, and then the rows beside a row that fell, are visited."""
    halo = np.ones(W.shape, dtype=bool)
    halo[1:-1, 1:-1] = False
    n = W.shape[0]
    rows = np.flatnonzero(woke.any(axis=1))
    dirty = np.zeros(n + 2, dtype=bool)
    for k in (0, 1, 2):
        dirty[rows + k] = True            # (dirty[i + 1]: row i)
    dirty = dirty[1:-1]
    dirty[[0, n - 1]] = False
    while dirty.any():
        for order in (range(1, n - 1), range(n - 2, 0, -1)):
            for i in order:
                if not dirty[i]:
                    continue
                dirty[i] = False
                if _row_step(W, XW, i, i - 1, a, d, halo) | _row_step(W, XW, i, i + 1, a, d, halo):
                    dirty[i - 1] = i > 1
                    dirty[i + 1] = i < n - 2
    return W


def rounds_bound(mask, connectivity=8, source='top'):
    """The synchronous tile model of the device's rounds on the boolean foreground `mask`: 64 x 64 tiles, every active
    tile (those whose tile or halo holds a pixel that fell in the round before; the source pixels count as fallen in round 0)
    relaxed to its fixed point against the previous round's halo.  Returns the last round in which any value changed, plus
    1 (1 where nothing ever changes, 0 without a source pixel).  A device look never needs more rounds than that: its
    halo words are never older than the previous round's, relaxation is monotone in its inputs, so after every round the
    device's map is at or below this model's -- and never below the final one."""
    code = source_code(source)
    a = unit_of(connectivity)
    d = 4 if a == 3 else 0
    X = np.ascontiguousarray(_to_top(np.asarray(mask, dtype=bool), code))
    N = X.shape[0]
    if not X[0].any():
        return 0
    # (the tiles of the device lie on the original grid: seen from the source wall they start at the far end for the
    # sources 1 and 3 -- the offset of the first tile)
    first = (N % TILE or TILE) if code in (1, 3) else TILE
    edges = [0] + list(range(first, N, TILE)) + [N]
    cuts = list(range(0, N, TILE)) + [N]
    rows, cols = edges, cuts
    XP = np.zeros((N + 2, N + 2), dtype=bool)
    XP[1:-1, 1:-1] = X
    G = np.full((N + 2, N + 2), _BIG, dtype=np.int64)
    G[1, 1:-1][X[0]] = 0
    changed = np.zeros((N + 2, N + 2), dtype=bool)
    changed[1, 1:-1] = X[0]
    last, r = 0, 0
    while changed.any():
        r += 1
        prev = G.copy()
        now = np.zeros_like(changed)
        for r0, r1 in zip(rows[:-1], rows[1:]):
            for c0, c1 in zip(cols[:-1], cols[1:]):
                if not changed[r0:r1 + 2, c0:c1 + 2].any():
                    continue
                W = _tile_fixed_point(prev[r0:r1 + 2, c0:c1 + 2].copy(), XP[r0:r1 + 2, c0:c1 + 2], a, d,
                                      changed[r0:r1 + 2, c0:c1 + 2])
                inner = W[1:-1, 1:-1]
                now[r0 + 1:r1 + 1, c0 + 1:c1 + 1] = inner < G[r0 + 1:r1 + 1, c0 + 1:c1 + 1]
                G[r0 + 1:r1 + 1, c0 + 1:c1 + 1] = inner
        if now.any():
            last = r
        changed = now
    return last + 1


# ---------------------------------------------------------------------------
# the result
# ---------------------------------------------------------------------------
class Geodesic:
    """One geodesic look: the sixteen words as Python integers (`WORDS`), ``hist`` ([4N], None unless fetched),
    ``profile`` ([N][3], None unless fetched), ``G`` (the int32 map, None unless fetched), and ``N``, ``threshold``,
    ``connectivity``, ``side``, ``source``, ``delx``.  Lengths are in pixels; the ``_phys`` values are scaled with
    ``delx``.  Refuses words that no map has."""

    def __init__(self, words, N, threshold, connectivity=8, side='below', source='top', hist=None, profile=None, g=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.connectivity = components.check_connectivity(connectivity)
        self.side = 'above' if components.side_code(side) == components.CHS_CC_ABOVE else 'below'
        self.source = SOURCE_NAMES[source_code(source)]
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_GEO_WORDS,):
            raise ValueError(f"{CHS_GEO_WORDS} words are needed, got shape {self.words.shape}")
        for name, v in zip(WORDS, self.words):
            setattr(self, name, int(v))
        N = self.N
        ok = (0 <= self.sources <= self.reached <= self.fg <= N * N and self.sources <= N
              and 0 <= self.target_reached <= self.target_fg <= N and self.target_reached <= self.reached
              and self.unit == unit_of(self.connectivity)
              and (self.sources == 0) == (self.reached == 0) == (self.rounds == 0)
              and (self.target_reached == 0) == (self.gmin_target == -1) == (self.gmin_target_pos == -1)
              and (self.reached == 0) == (self.gmax == -1) == (self.gmax_first == -1)
              and -1 <= self.gmin_target_pos < N and -1 <= self.gmax_first < N * N
              and (self.target_reached == 0 or self.unit * (N - 1) <= self.gmin_target <= self.gmax)
              and self.gmin_target * self.target_reached <= self.gsum_target <= self.gsum <= max(self.gmax, 0) * self.reached
              and 0 <= self.cc_reached <= min(self.cc_count, self.sources) and (self.cc_reached == 0) == (self.sources == 0)
              and 0 <= self.rounds <= self.limit)
        if not ok:
            raise ValueError(f"not the words of a geodesic map: {dict(zip(WORDS, self.words.tolist()))}")
        self.hist = None
        if hist is not None:
            self.hist = np.array(hist, dtype=np.int64)
            if self.hist.shape != (bins(N),) or int(self.hist.sum()) != self.reached or (self.hist < 0).any():
                raise ValueError(f"the histogram has {bins(N)} bins that add up to REACHED = {self.reached}")
            if self.reached and (int(self.hist[0]) < self.sources or np.flatnonzero(self.hist)[-1] != min(self.gmax // self.unit, bins(N) - 1)):
                raise ValueError("the histogram does not fit SOURCES and GMAX")
        self.profile = None
        if profile is not None:
            self.profile = np.array(profile, dtype=np.int64)
            if self.profile.shape != (N, 3):
                raise ValueError(f"a profile of shape {(N, 3)} is needed, got {self.profile.shape}")
            last = [self.target_fg, self.target_reached, self.gsum_target]
            if (self.profile.sum(axis=0).tolist() != [self.fg, self.reached, self.gsum] or self.profile[N - 1].tolist() != last
                    or (N > 1 and self.profile[0].tolist() != [self.sources, self.sources, 0])
                    or (self.profile[:, 1] > self.profile[:, 0]).any() or (self.profile < 0).any()):
                raise ValueError("the profile does not fit the words")
        self.G = None
        if g is not None:
            self.G = np.asarray(g, dtype=np.int32)
            if self.G.shape != (N, N):
                raise ValueError(f"a map of shape {(N, N)} is needed, got {self.G.shape}")

    def _scale(self, v):
        if self.delx is None:
            raise ValueError("physical lengths need delx")
        return v * self.delx

    @property
    def percolates(self):
        """Whether the target wall is reached."""
        return self.target_reached > 0

    @property
    def shortest_path(self):
        """The length of the shortest way across, in pixels (inf when not percolating)."""
        return self.gmin_target / self.unit if self.percolates else float('inf')

    @property
    def tortuosity(self):
        """GMIN_TARGET / (UNIT (N-1)): the shortest way across over the straight one; inf when not percolating."""
        return self.shortest_path / (self.N - 1) if self.N > 1 else (1.0 if self.percolates else float('inf'))

    @property
    def mean_tortuosity(self):
        """The same ratio averaged over the reached target pixels."""
        if not self.percolates:
            return float('inf')
        if self.N == 1:
            return 1.0
        return self.gsum_target / (self.target_reached * self.unit * (self.N - 1))

    def tortuosity_profile(self):
        """float [N]: mean G / (UNIT k) over the reached pixels of depth k; nan where no pixel is reached and at k = 0."""
        if self.profile is None:
            raise ValueError("the tortuosity profile needs the profile")
        k = np.arange(self.N, dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            out = self.profile[:, 2] / (self.profile[:, 1] * self.unit * k)
        out[(self.profile[:, 1] == 0) | (k == 0)] = np.nan
        return out

    @property
    def accessible_fraction(self):
        """REACHED / FG (0 without foreground)."""
        return self.reached / self.fg if self.fg else 0.0

    def depth_cdf(self):
        """float [4N]: the fraction of the phase that is accessible within the path length d of the face."""
        if self.hist is None:
            raise ValueError("the depth distribution needs the histogram")
        return np.cumsum(self.hist) / self.fg if self.fg else np.zeros(bins(self.N))

    @property
    def isolated(self):
        """FG - REACHED: the foreground pixels that no path reaches."""
        return self.fg - self.reached

    @property
    def max_reach(self):
        """GMAX / UNIT: the longest shortest path, in pixels (0 without a reached pixel)."""
        return max(self.gmax, 0) / self.unit

    @property
    def mean_path(self):
        """GSUM / (UNIT REACHED): the mean path length to a reached pixel, in pixels."""
        return self.gsum / (self.unit * self.reached) if self.reached else 0.0

    @property
    def g(self):
        """The map as float in pixels: nan for background, inf for unreached."""
        if self.G is None:
            return None
        out = self.G / float(self.unit)
        out[self.G < 0] = np.nan
        out[self.G == CHS_GEO_INF] = np.inf
        return out

    @property
    def shortest_path_phys(self):
        return self._scale(self.shortest_path)

    @property
    def max_reach_phys(self):
        return self._scale(self.max_reach)

    @property
    def mean_path_phys(self):
        return self._scale(self.mean_path)

    @property
    def g_phys(self):
        return None if self.G is None else self._scale(self.g)

    def depth_phys(self):
        """float [4N]: the path lengths of the histogram's bins (their lower ends) in the solver's unit."""
        return self._scale(np.arange(bins(self.N), dtype=np.float64))

    def __repr__(self):
        return (f"Geodesic(N={self.N}, threshold={self.threshold!r}, connectivity={self.connectivity}, side={self.side!r}, "
                f"source={self.source!r}, fg={self.fg}, reached={self.reached}, percolates={self.percolates}, "
                f"tortuosity={self.tortuosity:.4f}, rounds={self.rounds})")
