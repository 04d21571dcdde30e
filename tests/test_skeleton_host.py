"""Host tests (no GPU) of the skeleton look: the packed numpy model of chsimpy_amd/skeleton.py against a plain per-pixel
implementation of the definition written here with a 256-entry table, the topology it keeps against scipy's labelling,
closed cases, the words against their definitions, the limit arithmetic, the result class, the header and the binding,
and the host model of the per-word functions (tests/skel_model.cpp, built with the address and undefined-behaviour
sanitizers).  No device.

The definition (include/chs_hip.h: chs_skeleton).  The neighbours of a pixel are x0 .. x7 clockwise from north; B is
their sum; Y = sum over k in {0, 2, 4, 6} of (not x_k) and (x_{k+1} or x_{k+2}); sub-iteration i = 1, 2, ... of direction
(N, S, E, W)[(i - 1) % 4] deletes, synchronously, every foreground pixel whose neighbour in that direction is background,
with Y == 1 and B >= 2; the skeleton is the plane after the first four consecutive sub-iterations that delete nothing.
Everything is integer: every comparison is for equality.

`patterns`, `random_masks` and `reference` are shared with tests/test_gpu_skeleton.py, which puts the same masks on the
device."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from chsimpy_amd import _lib, batch, distance, morphology, skeleton
import test_distance_host as dh
import test_morphology_host as mh

ROOT = dh.ROOT
INF = dh.INF
T = dh.T
SIDES = dh.SIDES

# ---------------------------------------------------------------------------
# the reference, written out: a table over the 256 neighbourhoods, bit k of the code is x_k
# ---------------------------------------------------------------------------
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # x0 .. x7: N, NE, E, SE, S, SW, W, NW
TOWARD = (0, 4, 2, 6)                                                                # the x_k of directions N, S, E, W


def _tables():
    B, Y = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    for code in range(256):
        x = [(code >> k) & 1 for k in range(8)]
        B[code] = sum(x)
        Y[code] = sum(1 for k in (0, 2, 4, 6) if not x[k] and (x[k + 1] or x[(k + 2) % 8]))
    return B, Y


B_OF, Y_OF = _tables()


def codes_of(X):
    """The neighbourhood code of every pixel of a boolean image, everything outside being background."""
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    P = np.pad(X, 1)
    code = np.zeros((N, N), dtype=np.int64)
    for k, (di, dj) in enumerate(OFFSETS):
        code |= P[1 + di:N + 1 + di, 1 + dj:N + 1 + dj].astype(np.int64) << k
    return code


def pixel_thin(X, limit=None):
    """(skeleton image, subiters) by the definition, pixel by pixel through the table; None for the image at the limit."""
    X = np.array(X, dtype=bool)
    last, i = 0, 0
    while True:
        i += 1
        if limit is not None and i > limit:
            return None, last
        code = codes_of(X)
        gone = X & (((code >> TOWARD[(i - 1) % 4]) & 1) == 0) & (Y_OF[code] == 1) & (B_OF[code] >= 2)
        if gone.any():
            X &= ~gone
            last = i
        elif i >= last + 4:
            return X, last


def pixel_words(S, D2, fg, subiters, limit):
    """The seventeen words of a skeleton image by their definitions."""
    S = np.asarray(S, dtype=bool)
    D = np.asarray(D2, dtype=np.int64)
    code = codes_of(S)
    B, Y = B_OF[code], Y_OF[code]
    w = np.zeros(skeleton.CHS_SK_WORDS, dtype=np.int64)
    w[skeleton.CHS_SK_FG], w[skeleton.CHS_SK_PIXELS] = fg, S.sum()
    w[skeleton.CHS_SK_ISOLATED], w[skeleton.CHS_SK_ENDS] = (S & (B == 0)).sum(), (S & (B == 1)).sum()
    for y in range(1, 5):
        w[skeleton.CHS_SK_Y1 + y - 1] = (S & (Y == y)).sum()
    w[skeleton.CHS_SK_AXIAL] = (S[:, :-1] & S[:, 1:]).sum() + (S[:-1] & S[1:]).sum()
    w[skeleton.CHS_SK_DIAGONAL] = (S[:-1, :-1] & S[1:, 1:]).sum() + (S[:-1, 1:] & S[1:, :-1]).sum()
    d = D[S]
    fin = d[d < INF]
    w[skeleton.CHS_SK_SUMD2], w[skeleton.CHS_SK_D2MAX] = fin.sum(), (fin.max() if fin.size else 0)
    links = D[S & (Y == 2)]
    w[skeleton.CHS_SK_D2MIN_LINK] = links.min() if links.size else 0
    w[skeleton.CHS_SK_NINF] = d.size - fin.size
    w[skeleton.CHS_SK_EULER8] = mh.euler_by_labelling(S)[0]
    w[skeleton.CHS_SK_SUBITERS], w[skeleton.CHS_SK_LIMIT] = subiters, limit
    return w


def d2_of(X):
    """The squared distances of a mask by scipy (CHS_DT_INF by the definition where the grid has no background)."""
    X = np.asarray(X, dtype=bool)
    if X.all():
        return np.full(X.shape, INF, dtype=np.int64)
    return np.rint(ndimage.distance_transform_edt(X) ** 2).astype(np.int64)


# ---------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------
def ring(N):
    ii, jj = np.indices((N, N))
    r2 = (2 * ii - (N - 1)) ** 2 + (2 * jj - (N - 1)) ** 2
    return (r2 <= (N - 2) ** 2) & (r2 >= (N // 2) ** 2)


def plus(N):
    X = np.zeros((N, N), dtype=bool)
    X[N // 2, 1:N - 1] = True
    X[1:N - 1, N // 2] = True
    return X


def patterns(N):
    """Masks with the carries across word and row boundaries among them: [(name, X)]."""
    assert N >= 8
    ii, jj = np.indices((N, N))
    out = [('full', np.ones((N, N), dtype=bool)), ('empty', np.zeros((N, N), dtype=bool)), ('ring', ring(N)), ('plus', plus(N)),
           ('diagonal', np.eye(N, dtype=bool)), ('antidiagonal', np.eye(N, dtype=bool)[::-1].copy()),
           ('thick diagonal', np.abs(ii - jj) <= 2), ('bands', (ii // 5) % 2 == 0), ('columns', (jj // 3) % 2 == 0),
           ('checker', (ii + jj) % 2 == 0), ('blocks', ((ii // 7) + (jj // 7)) % 2 == 0), ('frame', (ii % (N - 1) == 0) | (jj % (N - 1) == 0))]
    pair = np.zeros((N, N), dtype=bool)
    pair[:, N // 2 - 1:N // 2 + 1] = True                     # at N = 128: the columns 63 | 64
    out.append(('column pair', pair))
    if N > 64:
        d = np.zeros((N, N), dtype=bool)
        for k in range(60, min(N, 70)):
            d[k, k] = True                                    # a diagonal line through (63, 63) - (64, 64)
        out.append(('diagonal through 63-64', d))
        c = np.zeros((N, N), dtype=bool)
        c[2:N - 2, 63:65] = True                              # a column pair at 63 | 64
        out.append(('columns 63-64', c))
        b = np.zeros((N, N), dtype=bool)
        b[N // 2 - 1:N // 2 + 2, 1:N - 1] = True              # a 3-wide bar across the word border
        out.append(('bar', b))
    return out


def random_masks(N, densities=(0.3, 0.6, 0.8, 0.95)):
    rng = np.random.default_rng(100 * N + 7)
    return [(f"p={p}", rng.random((N, N)) < p) for p in densities]


@functools.lru_cache(maxsize=None)
def _reference(key):
    X = _MASKS[key]
    S, last = pixel_thin(X)
    return S, last


_MASKS = {}


def reference(name, X):
    """(skeleton image, subiters) of a mask by the per-pixel implementation, computed once."""
    key = (name, X.shape[0], X.tobytes())
    _MASKS[key] = X
    return _reference(key)


def check_against_pixels(X, what):
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    S, last = reference(what, X)
    D2 = d2_of(X)
    words, hist, plane = skeleton.skeleton_of(D2)
    limit = skeleton.subiters_default(N)
    assert np.array_equal(skeleton.unpack(plane, N), S), what
    assert np.array_equal(words, pixel_words(S, D2, int(X.sum()), last, limit)), (what, words)
    d = D2[S]
    assert np.array_equal(hist, np.bincount(distance.radius_bins(d[d < INF]), minlength=distance.bin_count(N))), what
    return words, S


# ---------------------------------------------------------------------------
# 1. the packed model against the per-pixel implementation
# ---------------------------------------------------------------------------
def test_pack_and_unpack():
    rng = np.random.default_rng(3)
    for N in (1, 2, 63, 64, 65, 129):
        X = rng.random((N, N)) < 0.5
        P = skeleton.pack(X)
        assert P.shape == (N, (N + 63) // 64) and P.dtype == np.uint64
        assert np.array_equal(skeleton.unpack(P, N), X) and skeleton.popcount(P) == int(X.sum())
        for i, j in ((0, 0), (N - 1, N - 1), (N // 2, N - 1)):
            assert bool((int(P[i, j // 64]) >> (j % 64)) & 1) == bool(X[i, j])
    bad = skeleton.pack(np.ones((65, 65), dtype=bool))
    bad[3, 1] |= np.uint64(2)
    with pytest.raises(ValueError):
        skeleton.unpack(bad, 65)


@pytest.mark.parametrize("N", [1, 2, 8, 63, 64, 65, 129])
def test_packed_model_against_the_per_pixel_rule_on_random_masks(N):
    for name, X in random_masks(N):
        check_against_pixels(X, f"random N={N} {name}")


@pytest.mark.parametrize("N", [8, 65, 129])
def test_packed_model_against_the_per_pixel_rule_on_patterns(N):
    for name, X in patterns(N):
        words, S = check_against_pixels(X, f"{name} N={N}")
        assert words[skeleton.CHS_SK_EULER8] == mh.euler_by_labelling(X)[0], name


def test_one_sub_iteration_of_every_direction():
    rng = np.random.default_rng(5)
    for N in (5, 64, 70):
        X = rng.random((N, N)) < 0.7
        code = codes_of(X)
        for d in range(4):
            want = X & (((code >> TOWARD[d]) & 1) == 0) & (Y_OF[code] == 1) & (B_OF[code] >= 2)
            assert np.array_equal(skeleton.unpack(skeleton.deletes(skeleton.pack(X), d), N), want), (N, d)


# ---------------------------------------------------------------------------
# 2. the topology: all 4 x 4 masks
# ---------------------------------------------------------------------------
def _per_tile_components(X, structure, pitch, tiles):
    """The components of X that lie in each pitch x pitch tile, the tiles starting at (1, 1): no component but that of the
    gaps is in two tiles."""
    L, n = ndimage.label(X, structure)
    ii, jj = np.nonzero(L)
    tile = np.maximum(ii - 1, 0) // pitch * tiles + np.maximum(jj - 1, 0) // pitch
    pairs = np.unique(np.stack([tile, L[ii, jj]]), axis=1)
    return np.bincount(pairs[0], minlength=tiles * tiles)


def test_all_4x4_masks_keep_their_topology():
    """All 65,536 masks in one image, each in a 5 x 5 tile of its own behind a one-pixel margin: a pixel's neighbourhood ends at
    the one-pixel gap, so the tiles are thinned independently (a sample of them is thinned alone as well).  Per mask: the skeleton
    is a subset, a fixed point, and has the 8-components of the mask and the 4-components of its padded background."""
    tiles, pitch = 256, 5
    N = tiles * pitch + 1
    m = np.arange(1 << 16).reshape(tiles, tiles)
    X = np.zeros((N, N), dtype=bool)
    for b in range(16):
        X[1 + b // 4::pitch, 1 + b % 4::pitch] = (m >> b) & 1
    P, last = skeleton.thin(skeleton.pack(X))
    S = skeleton.unpack(P, N)
    assert not (S & ~X).any() and 0 < last + 4 <= 2 * 4 + 1 + 4
    for d in range(4):
        assert not skeleton.deletes(P, d).any(), d
    assert np.array_equal(_per_tile_components(S, mh.EIGHT, pitch, tiles), _per_tile_components(X, mh.EIGHT, pitch, tiles))
    # the background: the gaps are one component for every tile; what else lies in a tile are its holes
    assert np.array_equal(_per_tile_components(~S, mh.FOUR, pitch, tiles), _per_tile_components(~X, mh.FOUR, pitch, tiles))
    for k in range(0, 1 << 16, 97):
        i, j = divmod(k, tiles)
        i0, j0 = 1 + i * pitch, 1 + j * pitch
        own = X[i0:i0 + 4, j0:j0 + 4]
        alone, _ = skeleton.thin(skeleton.pack(own))
        assert np.array_equal(skeleton.unpack(alone, 4), S[i0:i0 + 4, j0:j0 + 4]), k
        assert ndimage.label(~np.pad(own, 1), mh.FOUR)[1] == ndimage.label(~np.pad(skeleton.unpack(alone, 4), 1), mh.FOUR)[1]


def test_random_masks_keep_their_topology():
    rng = np.random.default_rng(9)
    for N in (6, 17, 33, 65):
        for p in (0.4, 0.6, 0.8):
            X = rng.random((N, N)) < p
            S, _ = reference(f"topology {N} {p}", X)
            assert not (S & ~X).any()
            assert ndimage.label(S, mh.EIGHT)[1] == ndimage.label(X, mh.EIGHT)[1]
            assert ndimage.label(~np.pad(S, 1), mh.FOUR)[1] == ndimage.label(~np.pad(X, 1), mh.FOUR)[1]


# ---------------------------------------------------------------------------
# 3. closed cases
# ---------------------------------------------------------------------------
def look_of(X, **kw):
    return skeleton.model_look(mh.field_of(X), T, **kw)


def test_closed_cases():
    N = 16
    empty = look_of(np.zeros((N, N), dtype=bool), delx=0.5)
    assert not empty.words[:15].any() and empty.subiters == 0 and empty.limit == 4 * N + 64
    assert empty.r2_mean is None and empty.neck_radius is None and empty.coordination is None and empty.quantile(0.5) is None
    one = np.zeros((N, N), dtype=bool)
    one[5, 9] = True
    sk = look_of(one)
    assert (sk.fg, sk.pixels, sk.isolated, sk.ends, sk.euler8, sk.subiters) == (1, 1, 1, 0, 1, 0)
    assert (sk.sumd2, sk.d2max, sk.d2min_link, sk.axial, sk.diagonal) == (1, 1, 0, 0, 0)
    line = np.zeros((N, N), dtype=bool)
    line[7, 2:13] = True
    sk = look_of(line)
    assert np.array_equal(sk.mask(), line) and (sk.ends, sk.y2, sk.y1, sk.subiters) == (2, 9, 2, 0)
    assert (sk.axial, sk.diagonal, sk.length, sk.d2min_link, sk.neck_radius) == (10, 0, 10.0, 1, 1.0)
    bar = np.zeros((N, N), dtype=bool)
    bar[6:9, 1:15] = True
    sk = look_of(bar)
    S, last = reference('bar 16', bar)                                             # its centre line, by the per-pixel rule
    want = np.zeros((N, N), dtype=bool)
    want[7, 1:15] = True                                                           # (the end pixels stay: B >= 2 fails there)
    assert np.array_equal(S, want) and np.array_equal(sk.mask(), want) and sk.subiters == last
    assert sk.ends == 2 and sk.euler8 == 1 and sk.pixels == sk.y2 + 2 and sk.d2max == 4
    S, last = reference('plus 16', plus(N))                                        # (pinned to the per-pixel rule)
    sk = look_of(plus(N))
    assert np.array_equal(sk.mask(), S) and sk.subiters == last == 0 and sk.ends == 4
    code = codes_of(S)
    assert (sk.y3, sk.y4) == (int((S & (Y_OF[code] == 3)).sum()), int((S & (Y_OF[code] == 4)).sum())) == (0, 0)
    # (the centre of an axis-parallel plus has its four axial neighbours set: Y = 0 there and Y = 2 on the arms beside it)
    assert sk.junctions == 0 and sk.coordination is None and sk.branches_estimate == 2.0 and sk.pixels - sk.y1 - sk.y2 == 1
    x = np.zeros((N, N), dtype=bool)
    x[np.arange(2, 13), np.arange(2, 13)] = x[np.arange(2, 13), 14 - np.arange(2, 13)] = True
    sk = look_of(x)                                                                # a diagonal cross: a crossing
    assert np.array_equal(sk.mask(), x) and (sk.ends, sk.y3, sk.y4, sk.junctions, sk.coordination) == (4, 0, 1, 1, 4.0)
    r = look_of(ring(33))
    assert r.euler8 == 0 == mh.euler_by_labelling(ring(33))[0] and r.ends == 0 and r.isolated == 0 and r.pixels == r.y2
    for n, count in ((8, 17), (64, 129), (65, 130), (200, 401)):
        full = look_of(np.ones((n, n), dtype=bool))
        assert full.subiters + 4 == count and full.ninf == full.pixels > 0 and full.euler8 == 1 and full.fg == n * n
        assert full.sumd2 == 0 and full.d2max == 0 and not full.hist.any()


def test_euler8_is_that_of_morphology():
    rng = np.random.default_rng(21)
    for N in (8, 64, 65, 100):
        for p in (0.3, 0.6, 0.9):
            X = rng.random((N, N)) < p
            e = morphology.Morphology(morphology.quad_counts(mh.field_of(X), T), N, T).euler8
            assert skeleton.euler8_of_plane(skeleton.pack(X)) == e == mh.euler_by_labelling(X)[0]
            sk = look_of(X)
            assert sk.euler8 == e and sk.fg == int(X.sum())
            above = look_of(X, side='above')
            assert above.fg == N * N - sk.fg and above.euler8 == mh.euler_by_labelling(~X)[0]


# ---------------------------------------------------------------------------
# 4. the limit
# ---------------------------------------------------------------------------
def test_the_limit_arithmetic(hip_lib):
    last = 0
    for N in (1, 2, 8, 100, 512, 4096, 16384):
        d = hip_lib.chs_skeleton_subiters_default(N)
        assert d == _lib.skeleton_subiters_default(N) == skeleton.subiters_default(N) == 4 * N + 64 and d > last
        last = d
    assert hip_lib.chs_skeleton_subiters_default(0) == 0 and hip_lib.chs_skeleton_subiters_default(-4) == 0
    assert skeleton.subiters_default(0) == 0
    assert skeleton.check_limit(8, None) == skeleton.check_limit(8, 0) == 96 and skeleton.check_limit(8, 16 * 96) == 16 * 96
    for bad in (-1, 16 * 96 + 1):
        with pytest.raises(ValueError):
            skeleton.check_limit(8, bad)
    full = skeleton.pack(np.ones((65, 65), dtype=bool))
    _, need = skeleton.thin(full)
    assert need == 126
    with pytest.raises(skeleton.LimitReached) as e:
        skeleton.thin(full, 16)
    assert (e.value.subiters, e.value.limit) == (16, 16)
    with pytest.raises(skeleton.LimitReached) as e:
        skeleton.thin(full, need + 3)                   # the last four were not all quiet
    assert (e.value.subiters, e.value.limit) == (need, need + 3)
    assert skeleton.thin(full, need + 4)[1] == need
    with pytest.raises(skeleton.LimitReached) as e:
        skeleton.thin(skeleton.pack(np.zeros((8, 8), dtype=bool)), 3)
    assert (e.value.subiters, e.value.limit) == (0, 3)
    assert pixel_thin(np.ones((65, 65), dtype=bool), 16) == (None, 16)


# ---------------------------------------------------------------------------
# 5. the result class
# ---------------------------------------------------------------------------
def test_skeleton_object():
    X = random_masks(65)[2][1]
    sk = skeleton.model_look(mh.field_of(X), T, delx=0.25)
    assert sk.N == 65 and sk.side == 'below' and sk.threshold == T and sk.width_hist is sk.hist
    assert sk.junctions == sk.y3 + sk.y4 and sk.branches_estimate == (sk.ends + 3 * sk.y3 + 4 * sk.y4) / 2
    assert sk.coordination == (3 * sk.y3 + 4 * sk.y4) / sk.junctions
    assert sk.length == sk.axial + np.sqrt(2.0) * sk.diagonal and sk.length_phys == sk.length * 0.25
    assert sk.length_per_area == sk.length / 65 ** 2 and sk.length_per_area_phys == sk.length_per_area / 0.25
    assert sk.r2_mean == sk.sumd2 / sk.finite and sk.r2_mean_phys == sk.r2_mean * 0.0625
    assert sk.neck_radius == np.sqrt(sk.d2min_link) and sk.neck_radius_phys == sk.neck_radius * 0.25
    assert 1 <= sk.quantile(0.0) <= sk.quantile(0.5) <= sk.quantile(1.0) == int(np.sqrt(sk.d2max))
    assert sk.mask().sum() == sk.pixels and 'Skeleton(' in repr(sk)
    bare = skeleton.Skeleton(sk.words, 65, T)
    assert bare.hist is None and bare.mask() is None and bare.quantile(0.5) is None and bare.length_phys is None
    with pytest.raises(ValueError):
        sk.quantile(1.5)
    with pytest.raises(ValueError):
        skeleton.Skeleton(sk.words[:-1], 65, T)
    for index, value in ((skeleton.CHS_SK_PIXELS, sk.fg + 1), (skeleton.CHS_SK_SUBITERS, sk.limit - 3), (skeleton.CHS_SK_ENDS, -1)):
        w = sk.words.copy()
        w[index] = value
        with pytest.raises(ValueError):
            skeleton.Skeleton(w, 65, T)
    with pytest.raises(ValueError):
        skeleton.Skeleton(sk.words, 65, T, hist=sk.hist[:-1])
    h = sk.hist.copy()
    h[1] += 1
    with pytest.raises(ValueError):
        skeleton.Skeleton(sk.words, 65, T, hist=h)
    p = sk.plane.copy()
    p[0, 0] ^= np.uint64(1)
    with pytest.raises(ValueError):
        skeleton.Skeleton(sk.words, 65, T, plane=p)
    with pytest.raises(ValueError):
        skeleton.model_look(mh.field_of(X), T, side='left')


# ---------------------------------------------------------------------------
# 6. header, binding
# ---------------------------------------------------------------------------
SK_SYMBOLS = ['chs_skeleton_subiters_default', 'chs_skeleton', 'chs_skeleton_hist', 'chs_skeleton_plane', 'chs_skeleton_last_ms',
              'chs_skeleton_thin_ms', 'chs_batch_skeleton', 'chs_batch_skeleton_hist', 'chs_batch_skeleton_plane',
              'chs_batch_skeleton_last_ms', 'chs_batch_skeleton_thin_ms']
_CTYPES = dict(dh._CTYPES)
_CTYPES['int64_t'] = ctypes.c_int64
_CTYPES['uint64_t*'] = ctypes.POINTER(ctypes.c_uint64)


def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_SK_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_SK_WORDS'] == skeleton.CHS_SK_WORDS == _lib.CHS_SK_WORDS == len(skeleton.WORDS) == 17
    for i, w in enumerate(skeleton.WORDS):
        assert defs['CHS_SK_' + w.upper()] == getattr(skeleton, 'CHS_SK_' + w.upper()) == i
    assert (_lib.CHS_SK_SUBITERS, _lib.CHS_SK_LIMIT) == (skeleton.CHS_SK_SUBITERS, skeleton.CHS_SK_LIMIT)
    assert _lib.CHS_ELIMIT == skeleton.CHS_ELIMIT == -6 and skeleton.CHS_DT_INF == INF
    assert issubclass(_lib.SkeletonLimitError, _lib.EngineError)
    e = _lib.SkeletonLimitError('x', 7, 5)
    assert (e.subiters, e.limit) == (7, 5)
    host = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_skel_host.h')).read()
    dirs = {k: int(v) for k, v in re.findall(r'#define\s+CHS_SK_DIR_([NSEW])\s+(\d+)\b', host)}
    assert tuple(sorted(dirs, key=dirs.get)) == skeleton.DIRECTIONS and sorted(dirs.values()) == [0, 1, 2, 3]
    src = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_skeleton.hip')).read()
    assert int(re.search(r'#define\s+SK_MAX_FACTOR\s+(\d+)ll', src).group(1)) == skeleton.MAX_FACTOR


@pytest.mark.parametrize("name", SK_SYMBOLS)
def test_the_prototypes_match_the_header(hip_lib, name):
    """The argument and return types the binding declares are those of the prototype in include/chs_hip.h."""
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'^\s*(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr, flags=re.M)
    assert m, f"{name}: no prototype in the header"
    ret, args = m.group(1), [a.strip() for a in m.group(2).split(',')]
    want = []
    for a in args:
        a = re.sub(r'\[\w*\]$', '*', a)
        t = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)\s*\w*\s*(\*?)$', a)
        assert t, a
        want.append(_CTYPES[t.group(1) + ('*' if (t.group(2) or t.group(3)) else '')])
    fn = getattr(hip_lib, name)
    assert name in _lib.SYMBOLS
    assert list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert ctypes.sizeof(fn.restype) == ctypes.sizeof(_CTYPES[ret])


def test_the_members_forward_the_look():
    assert {'skeleton', 'skeleton_look'} <= set(batch._Member._LOOKS)
    for cls in (_lib.Engine, _lib.Batch):
        for name in ('skeleton', 'skeleton_look', 'skeleton_hist', 'skeleton_plane', 'skeleton_ms', 'skeleton_thin_ms'):
            assert callable(getattr(cls, name))


# ---------------------------------------------------------------------------
# 7. the host model of the per-word functions
# ---------------------------------------------------------------------------
def test_host_model_of_the_word_functions(tmp_path):
    """tests/skel_model.cpp: chs_sk::deletes and chs_sk::kinds_of through the header the kernels compile
    (chs_skel_host.h) against per-pixel loops, and whole thinnings with two planes -- its own executable, under the
    address and undefined-behaviour sanitizers."""
    from chsimpy_amd import _build
    exe = str(tmp_path / 'skel_model')
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I' + _build.CSRC,
                    os.path.join(ROOT, 'tests', 'skel_model.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and '\n0 failures' in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert int(re.search(r'(\d+) checks', r.stdout).group(1)) >= 200
    hdr = open(os.path.join(_build.CSRC, 'chs_skel_host.h')).read()
    assert not re.search(r'#include\s*[<"](hip/|chs_common|chs_look|chs_fast|chs_cx)', hdr)
    prog = open(os.path.join(ROOT, 'tests', 'skel_model.cpp')).read()
    assert re.findall(r'#include\s*"([^"]+)"', prog) == ['chs_skel_host.h']
    dev = open(os.path.join(_build.CSRC, 'chs_skeleton.hip')).read()
    assert '#include "chs_skel_host.h"' in dev
    for fn in ('chs_sk::deletes(', 'chs_sk::kinds_of(', 'chs_sk::euler8_of(', 'chs_sk::dir_of('):
        assert fn in dev, fn


def test_the_kernels_use_no_scratch():
    """Every kernel of chs_skeleton.hip compiles for gfx950 with ScratchSize 0 (tools/scratch_check.py's reader)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('scratch_check', os.path.join(ROOT, 'tools', 'scratch_check.py'))
    sc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sc)
    rows = sc.kernels(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_skeleton.hip'))
    names = {r[0] for r in rows}
    assert {'k_sk_mask', 'k_sk_euler', 'k_sk_stats'} <= names and sum('k_sk_thin<' in n for n in names) == 4, names
    assert all(r[1] == 0 for r in rows), rows
