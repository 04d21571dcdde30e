"""Droplet tracking from look to look -- overlaps, merges, births, deaths: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_track).

A *frame* is the component-number image of a track look: int32 [N][N], -1 for background, numbered as `components`
numbers (by ascending ``first``), together with its count and its ``(threshold, connectivity, side)``.  A handle keeps
at most one frame, on the device.  Pixel p has ``a = frame[p]`` and ``b`` = its number in the current look; its key is
``(a, b)``.

Pair table.  int64 [P][3]: one row ``(a, b, n)`` for every key other than (-1, -1) that at least one pixel has; ``n`` is
the number of such pixels; the rows are sorted by ``(a, b)``.  Rows with ``b = -1`` are the pixels droplet ``a`` lost to
the background, rows with ``a = -1`` the ground droplet ``b`` gained from it.  Every cell is an integer and every
accumulation an integer add, so the device's table is this model's bit for bit, for both element types.

Words.  25 int64 (`WORDS`): the 17 of `shapes`; ``have_prev``; ``prev_count``, the frame's count; ``pairs`` = P;
``overlap``, the pixels with a >= 0 and b >= 0; ``lost``, a >= 0 and b = -1; ``gained``, a = -1 and b >= 0; ``heads``, the
pixels with a key other than (-1, -1) that differs from the key of the left and of the upper neighbour (a wall counts as
different) -- the raster-first pixel of every key is one, so ``pairs <= heads``; ``slots``, the slots of the device's
hash table, the power of two >= 2 heads and at least 1024.  Without a frame ``have_prev = 0`` and the words behind it
are 0.

Overlap tracking assumes that the two looks are close enough in time for a droplet to overlap itself: `Track` links
droplets that share pixels and nothing else.  It does not try to follow a droplet that moved further than its own size
between the looks (advection, a large gap in time) -- such a droplet reads as one that vanished and one that was born.
"""
from collections import namedtuple

import numpy as np

from . import shapes

OVERLAP_WORDS = ('have_prev', 'prev_count', 'pairs', 'overlap', 'lost', 'gained', 'heads', 'slots')
WORDS = shapes.WORDS + OVERLAP_WORDS
CHS_TR_WORDS = len(WORDS)
(CHS_TR_HAVE_PREV, CHS_TR_PREV_COUNT, CHS_TR_PAIRS, CHS_TR_OVERLAP, CHS_TR_LOST, CHS_TR_GAINED, CHS_TR_HEADS,
 CHS_TR_SLOTS) = range(shapes.CHS_SH_WORDS, CHS_TR_WORDS)
MIN_SLOTS = 1024
KINDS = ('vanished', 'born', 'continued', 'merged', 'split', 'mixed')

Family = namedtuple('Family', 'kind prev now')


def _images(frame, labels_now):
    a, b = np.asarray(frame), np.asarray(labels_now)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape != b.shape:
        raise ValueError(f"two square number images of one size are needed, got {a.shape} and {b.shape}")
    a, b = a.astype(np.int64), b.astype(np.int64)
    if a.min(initial=0) < -1 or b.min(initial=0) < -1:
        raise ValueError("a number image holds -1 or a component number")
    return a, b


def pair_table(frame, labels_now):
    """int64 [P][3]: the rows (a, b, n) of the two number images, sorted by (a, b) -- np.unique over the keys."""
    a, b = _images(frame, labels_now)
    counted = (a >= 0) | (b >= 0)
    key, n = np.unique(((a[counted] + 1) << 32) | (b[counted] + 1), return_counts=True)
    return np.stack([(key >> 32) - 1, (key & 0xffffffff) - 1, n.astype(np.int64)], axis=1).reshape(-1, 3)


def heads(frame, labels_now):
    """The pixels with a key other than (-1, -1) that differs from the left and from the upper neighbour's."""
    a, b = _images(frame, labels_now)
    like_left, like_up = np.zeros(a.shape, dtype=bool), np.zeros(a.shape, dtype=bool)
    like_left[:, 1:] = (a[:, 1:] == a[:, :-1]) & (b[:, 1:] == b[:, :-1])
    like_up[1:, :] = (a[1:, :] == a[:-1, :]) & (b[1:, :] == b[:-1, :])
    return int(np.count_nonzero(((a >= 0) | (b >= 0)) & ~like_left & ~like_up))


def slots_of(nheads):
    """The slots of the device's hash table: the power of two >= 2 heads, at least `MIN_SLOTS`."""
    s = MIN_SLOTS
    while s < 2 * int(nheads):
        s *= 2
    return s


def words_of(shape_words, frame, labels_now):
    """The 25 words of a track look: the 17 of the shapes look of now, then those of the overlap with ``frame`` (None:
    no frame)."""
    w = np.zeros(CHS_TR_WORDS, dtype=np.int64)
    w[:shapes.CHS_SH_WORDS] = shape_words
    if frame is None:
        return w
    a, b = _images(frame, labels_now)
    t = pair_table(a, b)
    h = heads(a, b)
    w[CHS_TR_HAVE_PREV] = 1
    w[CHS_TR_PREV_COUNT] = int(a.max(initial=-1)) + 1
    w[CHS_TR_PAIRS] = t.shape[0]
    w[CHS_TR_OVERLAP] = t[(t[:, 0] >= 0) & (t[:, 1] >= 0), 2].sum()
    w[CHS_TR_LOST] = t[t[:, 1] < 0, 2].sum()
    w[CHS_TR_GAINED] = t[t[:, 0] < 0, 2].sum()
    w[CHS_TR_HEADS] = h
    w[CHS_TR_SLOTS] = slots_of(h)
    return w


def _roots(n, u, v):
    """The smallest node of the connected component of every node of the graph on n nodes with the edges (u[k], v[k])."""
    root = np.arange(n, dtype=np.int64)
    while True:
        before = root.copy()
        m = np.minimum(root[u], root[v])
        np.minimum.at(root, u, m)
        np.minimum.at(root, v, m)
        while True:                                        # pointer jumping
            nxt = root[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        if np.array_equal(root, before):
            return root


class Track:
    """One track look: the droplets of now (`now`, a `shapes.Shapes`) against those of the frame (`prev`, the `Shapes`
    of the look that kept it), linked by the exact pixel counts of the device's pair table.

    ``Track(words, pairs, prev, now, steps=(s0, s1), times=(t0, t1))``: the 25 words, the int64 [P][3] pair table, the
    two `Shapes` (``prev`` is None where the look found no frame) and the solver's step count and ``time_passed`` at
    both looks.  The constructor checks what holds of any true table and raises ValueError otherwise: the rows are
    sorted strictly by (a, b), every n is positive, a < prev.count and b < now.count, the rows of every droplet add up
    to its area in its own look, and the words are the table's sums.

    Without a frame (``have_prev`` False) there is nothing to link: `pairs` is empty and the derived methods raise
    ValueError.

    Overlap tracking assumes looks close enough in time that a droplet overlaps itself; this class does not try to
    follow droplets that moved further.  Everything below is derived from integers:

    `links(min_overlap=1)`: the rows with a, b >= 0 and n >= min_overlap.  `predecessors(b)`, `successors(a)`: the
    rows (a, n) of droplet b of now, the rows (b, n) of droplet a of the frame.
    `families(min_overlap=1)`: the connected components of the bipartite link graph as `Family(kind, prev, now)`, the
    numbers ascending, by (droplets of the frame, droplets of now): (1, 0) ``vanished``, (0, 1) ``born``, (1, 1)
    ``continued``, (>= 2, 1) ``merged``, (1, >= 2) ``split``, (>= 2, >= 2) ``mixed``.  `counts()`: how many of each.
    `growth()`: for the continued droplets ``a, b``, ``area, radius_eq, mean_u`` at both looks (``*_prev, *_now``),
    their differences ``d_*``, the centroid displacement ``shift`` [k][2] and its length ``distance`` (scaled by
    ``delx`` where there is one, like ``radius_eq``), ``dt`` and the rates ``*_rate`` per unit of ``time_passed`` (NaN
    without times or with dt = 0) -- ``radius_rate`` against ``radius_eq_prev`` is the LSW plot.
    `area_budget()`: the area the vanished droplets lost, the born ones gained and the other kinds exchanged; the
    entries add up exactly to ``total`` = now's area - prev's area.
    """

    def __init__(self, words, pairs, prev, now, steps=(None, None), times=(None, None)):
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_TR_WORDS,):
            raise ValueError(f"{CHS_TR_WORDS} words are needed, got shape {self.words.shape}")
        if not isinstance(now, shapes.Shapes) or not (prev is None or isinstance(prev, shapes.Shapes)):
            raise ValueError("`now` is a shapes.Shapes, `prev` one or None")
        if not np.array_equal(self.words[:shapes.CHS_SH_WORDS], now.words):
            raise ValueError("the first 17 words are not those of the shapes look of now")
        self.prev, self.now = prev, now
        self.pairs = np.array(pairs, dtype=np.int64).reshape(-1, 3)
        for name, v in zip(OVERLAP_WORDS, self.words[shapes.CHS_SH_WORDS:]):
            setattr(self, 'n_' + name if name in ('pairs', 'heads', 'slots') else name, int(v))
        if self.have_prev not in (0, 1):
            raise ValueError(f"have_prev = {self.have_prev}")
        self.have_prev = bool(self.have_prev)
        self.steps_prev, self.steps_now = steps
        self.time_prev, self.time_now = times
        t = self.pairs
        if not self.have_prev:
            if prev is not None or t.size or np.any(self.words[shapes.CHS_SH_WORDS:]):
                raise ValueError("without a frame there is no previous look, no pair and no overlap word")
            return
        if prev is None:
            raise ValueError("the look found a frame: the Shapes of the look that kept it are needed")
        if prev.N != now.N:
            raise ValueError(f"the looks have N = {prev.N} and {now.N}")
        a, b, n = t[:, 0], t[:, 1], t[:, 2]
        if self.prev_count != prev.count or self.n_pairs != t.shape[0]:
            raise ValueError(f"{self.prev_count} droplets in the frame and {self.n_pairs} pairs by the words, "
                             f"{prev.count} and {t.shape[0]} by the tables")
        key = ((a + 1) << 32) | (b + 1)
        if np.any(a < -1) or np.any(b < -1) or np.any(a >= prev.count) or np.any(b >= now.count) or np.any(key == 0):
            raise ValueError("a row outside the numbers of the two looks")
        if np.any(np.diff(key) <= 0):
            raise ValueError("the rows are not sorted strictly by (a, b)")
        if np.any(n <= 0):
            raise ValueError("a row without pixels")
        if not np.array_equal(_sum_by(a, n, prev.count), prev.area) or not np.array_equal(_sum_by(b, n, now.count), now.area):
            raise ValueError("the rows of a droplet do not add up to its area")
        both = (a >= 0) & (b >= 0)
        want = (int(n[both].sum()), int(n[b < 0].sum()), int(n[a < 0].sum()))
        if (self.overlap, self.lost, self.gained) != want:
            raise ValueError(f"overlap, lost, gained = {(self.overlap, self.lost, self.gained)} by the words, {want} by the table")
        if self.n_pairs > self.n_heads or self.n_slots != slots_of(self.n_heads):
            raise ValueError(f"{self.n_pairs} pairs, {self.n_heads} heads, {self.n_slots} slots")

    def _need_prev(self):
        if not self.have_prev:
            raise ValueError("the look found no frame: nothing to link")

    def links(self, min_overlap=1):
        """int64 [k][3]: the rows (a, b, n) with a, b >= 0 and n >= min_overlap."""
        self._need_prev()
        t = self.pairs
        return t[(t[:, 0] >= 0) & (t[:, 1] >= 0) & (t[:, 2] >= int(min_overlap))]

    def predecessors(self, b, min_overlap=1):
        """int64 [k][2]: (a, n) of the droplets of the frame that droplet b of now overlaps."""
        t = self.links(min_overlap)
        return t[t[:, 1] == int(b)][:, [0, 2]]

    def successors(self, a, min_overlap=1):
        """int64 [k][2]: (b, n) of the droplets of now that droplet a of the frame overlaps."""
        t = self.links(min_overlap)
        return t[t[:, 0] == int(a)][:, [1, 2]]

    def families(self, min_overlap=1):
        """The connected components of the bipartite link graph, a list of `Family(kind, prev, now)` ordered by their
        smallest droplet (those of the frame before those of now)."""
        t = self.links(min_overlap)
        ca, cb = self.prev.count, self.now.count
        root = _roots(ca + cb, t[:, 0], ca + t[:, 1])
        order = np.argsort(root, kind='stable')
        cuts = np.flatnonzero(np.diff(root[order])) + 1
        out = []
        for nodes in np.split(order, cuts) if ca + cb else []:
            p = tuple(int(x) for x in nodes[nodes < ca])
            q = tuple(int(x) - ca for x in nodes[nodes >= ca])
            out.append(Family(_kind(len(p), len(q)), p, q))
        return out

    def counts(self, min_overlap=1):
        """{kind: number of families} for every kind of `KINDS`."""
        out = dict.fromkeys(KINDS, 0)
        for f in self.families(min_overlap):
            out[f.kind] += 1
        return out

    def growth(self, min_overlap=1):
        """The continued droplets at both looks: a dict of arrays of one length (see the class)."""
        fam = [f for f in self.families(min_overlap) if f.kind == 'continued']
        a = np.array([f.prev[0] for f in fam], dtype=np.int64)
        b = np.array([f.now[0] for f in fam], dtype=np.int64)
        out = {'a': a, 'b': b}
        for name in ('area', 'radius_eq', 'mean_u'):
            vp, vn = getattr(self.prev, name)[a], getattr(self.now, name)[b]
            out[name + '_prev'], out[name + '_now'], out['d_' + name] = vp, vn, vn - vp
        scale = 1.0 if self.now.delx is None else self.now.delx
        out['shift'] = (self.now.centroid[b] - self.prev.centroid[a]) * scale
        out['distance'] = np.hypot(out['shift'][:, 0], out['shift'][:, 1])
        dt = None if self.time_prev is None or self.time_now is None else float(self.time_now) - float(self.time_prev)
        out['dt'] = dt
        for name in ('area', 'radius_eq', 'mean_u'):
            d = out['d_' + name].astype(np.float64)
            out[name.replace('_eq', '') + '_rate'] = d / dt if dt else np.full(d.shape, np.nan)
        return out

    def area_budget(self, min_overlap=1):
        """{kind: the area its families have now minus the area they had}, ``exchanged`` = the sum over continued,
        merged, split and mixed, ``total`` = now's area - prev's area = vanished + born + exchanged, all Python
        integers."""
        out = dict.fromkeys(KINDS, 0)
        for f in self.families(min_overlap):
            out[f.kind] += sum(int(self.now.area[k]) for k in f.now) - sum(int(self.prev.area[k]) for k in f.prev)
        out['exchanged'] = sum(out[k] for k in ('continued', 'merged', 'split', 'mixed'))
        out['total'] = int(self.now.area.sum()) - int(self.prev.area.sum())
        return out

    def __repr__(self):
        if not self.have_prev:
            return f"Track(N={self.now.N}, no frame, now={self.now.count})"
        return (f"Track(N={self.now.N}, prev={self.prev.count}, now={self.now.count}, pairs={self.n_pairs}, "
                f"overlap={self.overlap}, lost={self.lost}, gained={self.gained})")


def _sum_by(k, n, count):
    """int64 [count]: the sums of n over the rows of every number k >= 0 (n stays below 2^28: exact in double)."""
    has = k >= 0
    return np.bincount(k[has], weights=n[has].astype(np.float64), minlength=count).astype(np.int64)


def _kind(nprev, nnow):
    if nnow == 0:
        return 'vanished'
    if nprev == 0:
        return 'born'
    if nprev == 1:
        return 'continued' if nnow == 1 else 'split'
    return 'merged' if nnow == 1 else 'mixed'


def look(U_prev, U_now, threshold, connectivity=4, side='below', delx=None, steps=(None, None), times=(None, None)):
    """The `Track` of two fields from the numpy model alone (no device): both looks at one (threshold, connectivity,
    side).  ``U_prev`` None: a first look, without a frame."""
    now = shapes.look(U_now, threshold, connectivity, side, delx=delx)
    if U_prev is None:
        return Track(words_of(now.words, None, None), np.zeros((0, 3), dtype=np.int64), None, now, steps, times)
    prev = shapes.look(U_prev, threshold, connectivity, side, delx=delx)
    frame, labels = prev.components.labels, now.components.labels
    return Track(words_of(now.words, frame, labels), pair_table(frame, labels), prev, now, steps, times)
