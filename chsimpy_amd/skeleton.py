"""Skeleton of a phase of the thresholded field -- its medial network by a topology-preserving parallel thinning: junctions,
dead ends and links, the length of network per area, its coordination and the width of its narrowest necks: the host side
(numpy only, no device).  The model works on packed uint64 words, 64 pixels a word, as the device does.

The definition the device, this model and every test share (include/chs_hip.h: chs_skeleton).

Foreground.  ``side``, the NaN and threshold conventions and ``D2`` are exactly those of `distance`; the mask that is
thinned is ``D2 > 0``.  For the thinning everything outside the box is background; the foreground is 8-connected and the
background 4-connected.

Neighbourhood.  The neighbours of a pixel are ``x0 .. x7`` clockwise from north: N, NE, E, SE, S, SW, W, NW (north is row
i - 1, east column j + 1).  ``B = sum x_k``; the Yokoi 8-connectivity number is
``Y = sum over k in {0, 2, 4, 6} of (not x_k) and (x_{k+1} or x_{k+2})``, indices mod 8.

Sub-iteration.  One of direction d deletes, synchronously, every foreground pixel whose neighbour in direction d is
background, with ``Y == 1`` and ``B >= 2``.  Sub-iteration ``i = 1, 2, ...`` has direction ``(N, S, E, W)[(i - 1) % 4]``.

Skeleton.  The plane after the first four consecutive sub-iterations that delete nothing; ``subiters`` is the index of the
last sub-iteration that deleted a pixel, 0 if none did.

The plane.  ``N x ceil(N / 64)`` uint64; bit j of word w of a row is column ``64 w + j``; the bits at or beyond N are zero.

Words (`WORDS`, B and Y taken in the skeleton): ``fg``; ``pixels``; ``isolated`` (B = 0); ``ends`` (B = 1); ``y1 .. y4``,
the skeleton pixels by Yokoi number (edge, link, branch, crossing); ``axial`` and ``diagonal``, the pairs of skeleton pixels
that are 4-adjacent and diagonally adjacent; ``sumd2`` and ``d2max`` over the skeleton pixels with a finite D2;
``d2min_link``, the smallest D2 over the ``Y == 2`` pixels (0 without one); ``ninf``; ``euler8``, the Euler number of the
skeleton at 8-connectivity, ``pixels - axial - diagonal + (2 x 2 windows of exactly three pixels) + 3 (full windows)``;
``subiters``; ``limit``.

Histogram.  ``hist[k]``, int64, ``distance.bin_count(N)`` bins: the skeleton pixels with ``isqrt(D2) == k``; INF pixels are
in no bin.
"""
import math

import numpy as np

from . import components, distance

WORDS = ('fg', 'pixels', 'isolated', 'ends', 'y1', 'y2', 'y3', 'y4', 'axial', 'diagonal', 'sumd2', 'd2max', 'd2min_link',
         'ninf', 'euler8', 'subiters', 'limit')
CHS_SK_WORDS = len(WORDS)
(CHS_SK_FG, CHS_SK_PIXELS, CHS_SK_ISOLATED, CHS_SK_ENDS, CHS_SK_Y1, CHS_SK_Y2, CHS_SK_Y3, CHS_SK_Y4, CHS_SK_AXIAL,
 CHS_SK_DIAGONAL, CHS_SK_SUMD2, CHS_SK_D2MAX, CHS_SK_D2MIN_LINK, CHS_SK_NINF, CHS_SK_EULER8, CHS_SK_SUBITERS,
 CHS_SK_LIMIT) = range(CHS_SK_WORDS)
CHS_DT_INF = distance.CHS_DT_INF
CHS_ELIMIT = -6
DIRECTIONS = ('N', 'S', 'E', 'W')           # of sub-iterations 1, 2, 3, 4 and again
MAX_FACTOR = 16                             # max_subiters is at most that many defaults

side_code = components.side_code
bin_count = distance.bin_count
radius_bins = distance.radius_bins

_ONE, _TOP = np.uint64(1), np.uint64(63)


class LimitReached(RuntimeError):
    """The model's CHS_ELIMIT: the limit was used up while a pixel was deleted in its last four sub-iterations."""

    def __init__(self, subiters, limit):
        super().__init__(f"a pixel was deleted in sub-iteration {subiters}, max_subiters = {limit}")
        self.subiters, self.limit = int(subiters), int(limit)


def subiters_default(N):
    """The default limit of the sub-iterations: 4 N + 64 (chs_skeleton_subiters_default); 0 for N < 1."""
    N = int(N)
    return 4 * N + 64 if N >= 1 else 0


def check_limit(N, max_subiters):
    """The limit a look at grid size N runs under: None or 0 is the default; outside [0, 16 defaults] is a ValueError."""
    d = subiters_default(N)
    m = 0 if max_subiters is None else int(max_subiters)
    if m < 0 or m > MAX_FACTOR * d:
        raise ValueError(f"max_subiters = {m} is outside [0, {MAX_FACTOR * d}]")
    return m or d


def words_of_row(N):
    return (int(N) + 63) // 64


def pack(mask):
    """The packed plane, uint64 [N][ceil(N / 64)], of a boolean N x N image."""
    X = np.asarray(mask, dtype=bool)
    if X.ndim != 2 or X.shape[0] != X.shape[1]:
        raise ValueError(f"a square image is needed, got shape {X.shape}")
    N = X.shape[0]
    W = words_of_row(N)
    pad = np.zeros((N, 64 * W), dtype=np.uint8)
    pad[:, :N] = X
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder='little')).view('<u8').astype(np.uint64).reshape(N, W)


def unpack(plane, N):
    """The boolean N x N image of a packed plane."""
    P = np.ascontiguousarray(np.asarray(plane, dtype=np.uint64).astype('<u8'))
    N = int(N)
    if P.shape != (N, words_of_row(N)):
        raise ValueError(f"a plane of shape {(N, words_of_row(N))} is needed, got {P.shape}")
    bits = np.unpackbits(P.view(np.uint8).reshape(N, -1), axis=1, bitorder='little')
    if bits[:, N:].any():
        raise ValueError("a bit at or beyond N is set")
    return bits[:, :N].astype(bool)


def popcount(P):
    """The set bits of an array of words, a Python integer."""
    return int(np.unpackbits(np.ascontiguousarray(P).view(np.uint8)).sum(dtype=np.int64))


def _rows(P, di):
    """out[i] = P[i + di], zero outside."""
    out = np.zeros_like(P)
    if di < 0:
        out[-di:] = P[:di]
    elif di > 0:
        out[:-di] = P[di:]
    else:
        out[:] = P
    return out


def _west(P):
    """bit j <- column 64 w + j - 1: the word shifted up, the top bit of the word to the left coming in at the bottom."""
    out = P << _ONE
    out[:, 1:] |= P[:, :-1] >> _TOP
    return out


def _east(P):
    """bit j <- column 64 w + j + 1."""
    out = P >> _ONE
    out[:, :-1] |= P[:, 1:] << _TOP
    return out


def neighbour_planes(P):
    """The eight neighbour planes x0 .. x7 of a packed plane."""
    up, dn = _rows(P, -1), _rows(P, 1)
    return [up, _east(up), _east(P), _east(dn), dn, _west(dn), _west(P), _west(up)]


def _terms(x):
    return [~x[k] & (x[k + 1] | x[(k + 2) % 8]) for k in (0, 2, 4, 6)]


def _some_two(x):
    some, two = np.zeros_like(x[0]), np.zeros_like(x[0])
    for v in x:
        two |= some & v
        some |= v
    return some, two


def deletes(P, direction):
    """The plane of the pixels that a sub-iteration of `direction` (0 .. 3: N, S, E, W) deletes from the plane P."""
    x = neighbour_planes(P)
    t = _terms(x)
    two_terms = (t[0] & t[1]) | (t[2] & t[3]) | ((t[0] | t[1]) & (t[2] | t[3]))
    y1 = (t[0] | t[1] | t[2] | t[3]) & ~two_terms
    _, two = _some_two(x)
    return P & ~x[(0, 4, 2, 6)[direction]] & y1 & two


def thin(plane, max_subiters=None):
    """(skeleton plane, subiters) of a packed plane: the numpy model of the thinning.  `LimitReached` as the device's
    CHS_ELIMIT."""
    P = np.array(plane, dtype=np.uint64)
    limit = check_limit(P.shape[0], max_subiters)
    last = 0
    for i in range(1, limit + 1):
        d = deletes(P, (i - 1) % 4)
        if d.any():
            P &= ~d
            last = i
        elif i >= last + 4:
            return P, last
    raise LimitReached(last, limit)


def kinds(P):
    """The masks of a plane's pixels by what they are in it: a dict of packed planes -- ``isolated, ends, b2``,
    ``y0 .. y4``, ``axial_e, axial_s, diag_se, diag_sw`` (a pair at its northern or western pixel), ``tri`` and ``full`` (a
    2 x 2 window of exactly three and of four pixels, at the window's top-left corner)."""
    x = neighbour_planes(P)
    some, two = _some_two(x)
    t = _terms(x)
    s01, c01, s23, c23 = t[0] ^ t[1], t[0] & t[1], t[2] ^ t[3], t[2] & t[3]
    b0, carry = s01 ^ s23, s01 & s23
    b1, b2 = c01 ^ c23 ^ carry, c01 & c23
    a, b, d, e = P, x[2], x[4], x[3]
    return {'isolated': P & ~some, 'ends': P & some & ~two, 'b2': P & two,
            'y0': P & ~b0 & ~b1 & ~b2, 'y1': P & b0 & ~b1, 'y2': P & ~b0 & b1, 'y3': P & b0 & b1, 'y4': P & b2,
            'axial_e': P & x[2], 'axial_s': P & x[4], 'diag_se': P & x[3], 'diag_sw': P & x[5],
            'tri': (a & b & (d ^ e)) | (d & e & (a ^ b)), 'full': a & b & d & e}


def euler8_of_plane(P):
    """The Euler number of a packed plane at 8-connectivity."""
    k = kinds(P)
    return (popcount(P) - popcount(k['axial_e']) - popcount(k['axial_s']) - popcount(k['diag_se']) - popcount(k['diag_sw'])
            + popcount(k['tri']) + 3 * popcount(k['full']))


def summary_of(plane, D2, fg, subiters, limit):
    """The seventeen words of a skeleton plane on the squared-distance map D2, an int64 array."""
    P = np.asarray(plane, dtype=np.uint64)
    D = np.asarray(D2, dtype=np.int64)
    N = D.shape[0]
    k = kinds(P)
    w = np.zeros(CHS_SK_WORDS, dtype=np.int64)
    w[CHS_SK_FG] = int(fg)
    w[CHS_SK_PIXELS] = popcount(P)
    w[CHS_SK_ISOLATED], w[CHS_SK_ENDS] = popcount(k['isolated']), popcount(k['ends'])
    for y in range(1, 5):
        w[CHS_SK_Y1 + y - 1] = popcount(k[f'y{y}'])
    w[CHS_SK_AXIAL] = popcount(k['axial_e']) + popcount(k['axial_s'])
    w[CHS_SK_DIAGONAL] = popcount(k['diag_se']) + popcount(k['diag_sw'])
    d = D[unpack(P, N)]
    fin = d[d < CHS_DT_INF]
    w[CHS_SK_SUMD2] = fin.sum()
    w[CHS_SK_D2MAX] = fin.max() if fin.size else 0
    links = D[unpack(k['y2'], N)]
    w[CHS_SK_D2MIN_LINK] = links.min() if links.size else 0
    w[CHS_SK_NINF] = d.size - fin.size
    w[CHS_SK_EULER8] = w[CHS_SK_PIXELS] - w[CHS_SK_AXIAL] - w[CHS_SK_DIAGONAL] + popcount(k['tri']) + 3 * popcount(k['full'])
    w[CHS_SK_SUBITERS], w[CHS_SK_LIMIT] = int(subiters), int(limit)
    return w


def histogram_of(plane, D2):
    """hist int64 [bin_count(N)]: the skeleton pixels with a finite D2 by ``isqrt(D2)``."""
    D = np.asarray(D2, dtype=np.int64)
    N = D.shape[0]
    d = D[unpack(plane, N)]
    return np.bincount(radius_bins(d[d < CHS_DT_INF]), minlength=bin_count(N)).astype(np.int64)


def skeleton_of(D2, max_subiters=None):
    """(words, hist, plane) of a squared-distance map: the numpy model of chs_skeleton behind its distance look."""
    D = np.asarray(D2, dtype=np.int64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"a square map is needed, got shape {D.shape}")
    limit = check_limit(D.shape[0], max_subiters)
    phase = pack(D > 0)
    plane, last = thin(phase, limit)
    return summary_of(plane, D, popcount(phase), last, limit), histogram_of(plane, D), plane


def model_look(U, threshold, side='below', delx=None, max_subiters=None):
    """The `Skeleton` of a field by the numpy model, histogram and plane included."""
    D2 = distance.squared_distance(U, threshold, side)
    words, hist, plane = skeleton_of(D2, max_subiters)
    return Skeleton(words, D2.shape[0], threshold, side, hist=hist, plane=plane, delx=delx)


class Skeleton:
    """One look at the skeleton of a phase: the seventeen words by name (`WORDS`, Python integers), ``hist`` (alias
    ``width_hist``; None unless fetched) and ``plane`` (the packed words; None unless fetched), and derived from them
    ``junctions = y3 + y4``; ``branches_estimate = (ends + 3 y3 + 4 y4) / 2``, the links of the network if every branch
    pixel joined three of them, every crossing four and every link ended at two of these; ``coordination``, the mean
    number of links at a junction, ``(3 y3 + 4 y4) / junctions``; ``length = axial + sqrt(2) diagonal``, the length of the
    network in pixel units -- the three pixels of a junction triangle are joined pairwise, so such a triangle is counted
    twice (two sides where the network passes once) --; ``length_per_area``; ``r2_mean``, the mean squared half-width along
    the network; ``r_max``; ``neck_radius``, the half-width at the narrowest link; their ``_phys`` versions (with
    ``delx``); ``quantile(q)`` of the width bins; ``mask()``, the unpacked boolean image -- None where a denominator is zero
    or the input is missing -- beside ``N``, ``threshold``, ``side``."""

    def __init__(self, words, N, threshold, side='below', hist=None, plane=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.side = 'above' if side_code(side) == components.CHS_CC_ABOVE else 'below'
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_SK_WORDS,):
            raise ValueError(f"{CHS_SK_WORDS} words are needed, got shape {self.words.shape}")
        for name, v in zip(WORDS, self.words):
            setattr(self, name, int(v))
        n2 = self.N * self.N
        finite = self.pixels - self.ninf
        if not (0 <= self.pixels <= self.fg <= n2 and (self.pixels == 0) == (self.fg == 0)
                and min(self.isolated, self.ends, self.y1, self.y2, self.y3, self.y4, self.axial, self.diagonal) >= 0
                and self.isolated + self.ends <= self.pixels and self.y1 + self.y2 + self.y3 + self.y4 <= self.pixels
                and 0 <= self.ninf <= self.pixels and 0 <= self.d2max < CHS_DT_INF and (finite == 0) == (self.d2max == 0)
                and finite <= self.sumd2 <= finite * self.d2max and (self.d2min_link == 0 or self.y2 > 0)
                and 0 <= self.subiters and self.subiters + 4 <= self.limit):
            raise ValueError(f"not the summary of a skeleton: {self.words}")
        self.hist = None
        if hist is not None:
            self.hist = np.array(hist, dtype=np.int64)
            if self.hist.shape != (bin_count(self.N),):
                raise ValueError(f"a histogram of {bin_count(self.N)} bins is needed, got shape {self.hist.shape}")
            if np.any(self.hist < 0) or int(self.hist.sum()) != finite:
                raise ValueError(f"the histogram adds up to {int(self.hist.sum())}, not to pixels - ninf = {finite}")
            top = math.isqrt(self.d2max)
            if np.any(self.hist[top + 1:] != 0) or (finite and self.hist[top] < 1) or self.hist[0] != 0:
                raise ValueError(f"the histogram's last occupied bin is not isqrt(d2max) = {top}")
        self.plane = None
        if plane is not None:
            self.plane = np.array(plane, dtype=np.uint64)
            image = unpack(self.plane, self.N)                 # (checks the shape and the bits beyond N)
            if int(np.count_nonzero(image)) != self.pixels:
                raise ValueError(f"the plane holds {int(np.count_nonzero(image))} pixels, the words say {self.pixels}")
            if euler8_of_plane(self.plane) != self.euler8:
                raise ValueError("the plane's Euler number is not the one given")

    width_hist = property(lambda self: self.hist)

    @property
    def finite(self):
        """The skeleton pixels with a finite D2: what the means and the histogram are over."""
        return self.pixels - self.ninf

    def _phys(self, v):
        return None if (v is None or self.delx is None) else v * self.delx

    @property
    def junctions(self):
        return self.y3 + self.y4

    @property
    def branches_estimate(self):
        return (self.ends + 3 * self.y3 + 4 * self.y4) / 2

    @property
    def coordination(self):
        return (3 * self.y3 + 4 * self.y4) / self.junctions if self.junctions else None

    @property
    def length(self):
        return self.axial + math.sqrt(2.0) * self.diagonal

    @property
    def length_phys(self):
        return self._phys(self.length)

    @property
    def length_per_area(self):
        return self.length / (self.N * self.N)

    @property
    def length_per_area_phys(self):
        return None if self.delx is None else self.length_per_area / self.delx

    @property
    def r2_mean(self):
        return self.sumd2 / self.finite if self.finite else None

    @property
    def r2_mean_phys(self):
        return None if (self.r2_mean is None or self.delx is None) else self.r2_mean * self.delx * self.delx

    @property
    def r_max(self):
        return math.sqrt(self.d2max) if self.finite else None

    @property
    def r_max_phys(self):
        return self._phys(self.r_max)

    @property
    def neck_radius(self):
        return math.sqrt(self.d2min_link) if (self.y2 and self.d2min_link < CHS_DT_INF) else None

    @property
    def neck_radius_phys(self):
        return self._phys(self.neck_radius)

    def quantile(self, q):
        """The smallest width bin k with at least the fraction q of the finite skeleton pixels in bins <= k."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q is in [0, 1], got {q!r}")
        if self.hist is None or not self.finite:
            return None
        need = max(1, math.ceil(q * self.finite))
        return int(np.searchsorted(np.cumsum(self.hist), need, side='left'))

    def mask(self):
        """The skeleton as a boolean N x N image; None unless the plane was fetched."""
        return None if self.plane is None else unpack(self.plane, self.N)

    def __repr__(self):
        return (f"Skeleton(N={self.N}, threshold={self.threshold!r}, side={self.side!r}, fg={self.fg}, pixels={self.pixels}, "
                f"ends={self.ends}, junctions={self.junctions}, euler8={self.euler8}, subiters={self.subiters})")
