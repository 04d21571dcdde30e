"""Host side of the distance transform of the thresholded field (chsimpy_amd/distance.py): the numpy model of the two
passes against ``scipy.ndimage.distance_transform_edt`` and against an O(N^4) brute force, hand-made patterns with known
answers, the radius bins, the consistency checks of `Distance`, the header's constants and prototypes, and the
experiment's --widths on a dry run, alone and under gloo at world 2.  No device.

`reference`, `patterns` and `check_look` are shared with tests/test_gpu_distance.py, which puts the same fields on the
device.  Everything is integer: every comparison is for equality.  scipy is never handed a grid without background --
its result there is not defined -- the all-foreground sentinel is checked against the definition alone."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

from chsimpy_amd import _lib, components, distance
import test_morphology_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG, BG, T = mh.FG, mh.BG, mh.T
INF = 1 << 30
SIDES = ('below', 'above')


def tile_from_source():
    """(band_rows, row_chunk) of chs_distance.hip without loading the library."""
    from chsimpy_amd import _build
    src = open(os.path.join(_build.CSRC, 'chs_distance.hip')).read()
    common = open(os.path.join(_build.CSRC, 'chs_common.h')).read()
    band = int(re.search(r'#define\s+CHS_DT_BAND\s+(\d+)\b', src).group(1))
    chunk = re.search(r'#define\s+CHS_DT_CHUNK\s+(\w+)\b', src).group(1)
    if not chunk.isdigit():
        chunk = re.search(r'#define\s+%s\s+(\d+)\b' % chunk, common).group(1)
    return band, int(chunk)


def tile_sizes(tile):
    """The N at which each phase can still go wrong: one band, one below / at / one above a band, more than two bands,
    and one either side of a row chunk where that differs; at least one is no multiple of four (the element loads)."""
    b, c = tile
    sizes = [8, b - 1, b, b + 1, 2 * b + 1] + [n for n in (c - 1, c + 1) if n not in (b - 1, b + 1)]
    sizes = sorted({n for n in sizes if 8 <= n <= 513})
    assert any(n % 4 for n in sizes) and any(n % 4 == 0 for n in sizes)
    return sizes


def reference(X):
    """(D2 int32 [N][N], words int64 [5], hist int64 [bins]) of the boolean foreground X by the definition: scipy's exact
    transform where the grid has background (its value is exact after rint up to N = 513), CHS_DT_INF where it has
    none; the words and the histogram by plain counting with math.isqrt."""
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    assert N <= 513
    if X.all():
        D2 = np.full((N, N), INF, dtype=np.int32)
    elif not X.any():
        D2 = np.zeros((N, N), dtype=np.int32)
    else:
        D2 = np.rint(ndimage.distance_transform_edt(X) ** 2).astype(np.int32)
    flat = D2.ravel().astype(np.int64)
    fin = flat[(flat > 0) & (flat < INF)]
    words = np.array([int(X.sum()), 0, -1, 0, int((flat == INF).sum())], dtype=np.int64)
    hist = np.zeros(math.isqrt(2 * (N - 1) ** 2) + 1, dtype=np.int64)
    if fin.size:
        words[1] = fin.max()
        words[2] = int(np.flatnonzero(flat == fin.max())[0])
        words[3] = fin.sum()
        vals, counts = np.unique(fin, return_counts=True)
        for v, c in zip(vals, counts):
            hist[math.isqrt(int(v))] += c
    return D2, words, hist


def isqrt_of(v):
    """math.isqrt element by element for an int64 array of values below 2^52 (the float root is off by one at most)."""
    v = np.asarray(v, dtype=np.int64)
    k = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    k -= k * k > v
    k += (k + 1) * (k + 1) <= v
    return k


def words_and_hist(D2):
    """(words int64 [5], hist int64 [bins]) of a squared-distance map by plain counting, at any N."""
    N = D2.shape[0]
    flat = D2.ravel().astype(np.int64)
    fin = flat[(flat > 0) & (flat < INF)]
    words = np.array([int((flat > 0).sum()), 0, -1, 0, int((flat == INF).sum())], dtype=np.int64)
    bins = math.isqrt(2 * (N - 1) ** 2) + 1
    hist = np.zeros(bins, dtype=np.int64)
    if fin.size:
        words[1] = fin.max()
        words[2] = int(np.flatnonzero(flat == fin.max())[0])
        words[3] = fin.sum()
        hist = np.bincount(isqrt_of(fin), minlength=bins).astype(np.int64)
    return words, hist


def reference_exact(X):
    """`reference` at any N: (D2, words, hist) of the boolean foreground X from the INDICES of scipy's exact transform,
    D2 = (i - ii)^2 + (j - jj)^2 in integers with (ii, jj) the nearest background pixel scipy names -- no rounded float
    anywhere.  All foreground: CHS_DT_INF; all background: 0, as in `reference`."""
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    if X.all():
        D2 = np.full((N, N), INF, dtype=np.int32)
    elif not X.any():
        D2 = np.zeros((N, N), dtype=np.int32)
    else:
        idx = ndimage.distance_transform_edt(X, return_distances=False, return_indices=True)
        di = np.arange(N, dtype=np.int64)[:, None] - idx[0]
        dj = np.arange(N, dtype=np.int64)[None, :] - idx[1]
        assert not X[idx[0], idx[1]].any()               # (what scipy names is a background pixel)
        D2 = (di * di + dj * dj).astype(np.int32)
    words, hist = words_and_hist(D2)
    assert words[0] == int(X.sum())
    return D2, words, hist


def closed_form(N, background):
    """D2 int32 [N][N] of a grid that is foreground but for the pixels `background`: min_k (i-i_k)^2 + (j-j_k)^2."""
    i = np.arange(N, dtype=np.int64)
    D2 = None
    for ik, jk in background:
        d = ((i - ik) ** 2)[:, None] + ((i - jk) ** 2)[None, :]
        D2 = d if D2 is None else np.minimum(D2, d)
    return D2.astype(np.int32)


def check_look(di, X, what=''):
    """A `Distance` (with histogram and map where fetched) against the reference of the boolean foreground X."""
    D2, words, hist = reference(X)
    assert di.words.dtype == np.int64 and np.array_equal(di.words, words), (what, di.words, words)
    assert np.array_equal(D2 > 0, X)
    if di.hist is not None:
        assert di.hist.dtype == np.int64 and np.array_equal(di.hist, hist), what
    if di.d2 is not None:
        assert di.d2.dtype == np.int32 and np.array_equal(di.d2, D2), (what, np.argwhere(di.d2 != D2)[:5])
    return words


def check_against(di, ref, what=''):
    """A `Distance` (with histogram and map where fetched) against a (D2, words, hist) computed once by the caller."""
    D2, words, hist = ref
    assert di.words.dtype == np.int64 and np.array_equal(di.words, words), (what, di.words, words)
    if di.hist is not None:
        assert di.hist.dtype == np.int64 and di.hist.shape == hist.shape, what
        assert np.array_equal(di.hist, hist), (what, np.flatnonzero(di.hist != hist)[:5])
    if di.d2 is not None:
        assert di.d2.dtype == np.int32 and np.array_equal(di.d2, D2), (what, np.argwhere(di.d2 != D2)[:5])


def model_look(U, t, side):
    D2 = distance.squared_distance(U, t, side)
    return distance.Distance(distance.summary_of(D2), np.asarray(U).shape[0], t, side, hist=distance.histogram_of(D2), d2=D2)


def patterns(N, tile):
    """Hand-made fields with known answers: a list of (name, U, {attribute of Distance: value}) for the side below the
    threshold T; the foreground is where the mask is True."""
    assert N >= 8
    b = tile[0]
    B = b if N > b else N // 2                       # a band border where the grid has one
    out = []

    def add(name, X, **want):
        out.append((name, mh.field_of(X), want))

    none = np.zeros((N, N), dtype=bool)
    ii, jj = np.indices((N, N))
    add('all-background', none, fg=0, d2max=0, d2max_first=-1, sumd2=0, ninf=0)
    add('all-foreground', ~none, fg=N * N, d2max=0, d2max_first=-1, sumd2=0, ninf=N * N)
    for i, j in ((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)):   # the longest search; the last bin of the histogram
        X = ~none
        X[i, j] = False
        add(f'background-corner-{i}-{j}', X, fg=N * N - 1, d2max=2 * (N - 1) ** 2, ninf=0,
            d2max_first=(N - 1 - i) * N + (N - 1 - j), sumd2=2 * N * sum(k * k for k in range(N)))
    X = none.copy()
    X[N // 3, N - 3] = True
    add('one-foreground-pixel', X, fg=1, d2max=1, d2max_first=(N // 3) * N + N - 3, sumd2=1)
    for name, rows in (('row-B-1', (B - 1,)), ('row-B', (B,)), ('rows-B-1-and-B', (B - 1, B)), ('last-row', (N - 1,))):
        X = ~none
        X[list(rows), :] = False                     # background only there: the band carries
        far = max(rows[0], N - 1 - rows[-1])
        add(name, X, fg=N * (N - len(rows)), d2max=far * far, ninf=0,
            d2max_first=0 if rows[0] >= N - 1 - rows[-1] else (N - 1) * N)
    X = ~none
    X[:, N - 1] = False
    add('last-column', X, fg=N * (N - 1), d2max=(N - 1) ** 2, d2max_first=0, ninf=0)
    for w in (1, 2, 7):   # (the first stripe lies at the wall, which is no background: its outer pixels are w away)
        add(f'vertical-stripes-{w}', (jj // w) % 2 == 0, d2max=w * w, d2max_first=0, ninf=0)
        add(f'horizontal-stripes-{w}', (ii // w) % 2 == 0, d2max=w * w, d2max_first=0, ninf=0)
    add('checkerboard', (ii + jj) % 2 == 0, fg=(N * N + 1) // 2, d2max=1, d2max_first=0, sumd2=(N * N + 1) // 2, ninf=0)
    c, r2 = (N - 1) / 2.0, (N / 3.0) ** 2
    disc = (ii - c) ** 2 + (jj - c) ** 2 <= r2
    add('disc-of-background', ~disc, fg=N * N - int(disc.sum()), ninf=0)
    add('disc-of-foreground', disc, fg=int(disc.sum()), ninf=0)
    return out


def check_pattern(look, name, U, want, N):
    """`look(U, t, side)` -> Distance with histogram and map: the known answers, then the reference, on both sides."""
    below = look(U, T, 'below')
    for k, v in want.items():
        assert getattr(below, k) == v, (name, N, k, getattr(below, k), v)
    check_look(below, U < T, f"{name} N={N} below")
    above = look(U, T, 'above')
    check_look(above, ~(U < T), f"{name} N={N} above")
    assert below.fg + above.fg == N * N
    if name.startswith('background-corner'):
        assert below.hist[-1] >= 1 and below.r_max == math.sqrt(2 * (N - 1) ** 2)   # (the far corner is in the last bin)


def brute_force(X):
    """D2 by the definition itself, O(N^4): every foreground pixel against every background pixel."""
    N = X.shape[0]
    D2 = np.zeros((N, N), dtype=np.int64)
    bi, bj = np.nonzero(~X)
    for i, j in zip(*np.nonzero(X)):
        D2[i, j] = ((bi - i) ** 2 + (bj - j) ** 2).min() if bi.size else INF
    return D2


# ---------------------------------------------------------------------------
# the numpy model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.6, 0.95])
@pytest.mark.parametrize("N", [8, 33, 65])
def test_model_against_scipy(N, density):
    rng = np.random.default_rng(1000 * N + int(1000 * density))
    U = mh.field_of(rng.random((N, N)) < density)
    for side in SIDES:
        X = (U < T) if side == 'below' else ~(U < T)
        assert X.any() and not X.all()
        assert np.array_equal(distance.foreground(U, T, side), X)
        want = np.rint(ndimage.distance_transform_edt(X) ** 2)
        D2 = distance.squared_distance(U, T, side)
        assert D2.dtype == np.int32 and np.array_equal(D2, want), (N, density, side)
        di = model_look(U, T, side)
        check_look(di, X, f"N={N} {density} {side}")
        assert di.side == side and di.fg == int(X.sum()) and di.ninf == 0


@pytest.mark.parametrize("density", [0.3, 0.6, 0.95, 0.995])
@pytest.mark.parametrize("N", [8, 13, 16])
def test_model_against_brute_force(N, density):
    rng = np.random.default_rng(31 * N + int(1000 * density))
    X = rng.random((N, N)) < density
    for Y in (X, ~X, np.ones((N, N), dtype=bool), np.zeros((N, N), dtype=bool)):
        assert np.array_equal(distance.squared_distance(mh.field_of(Y), T), brute_force(Y))


def _assert_same_reference(a, b, what):
    for x, y, k in zip(a, b, ('D2', 'words', 'hist')):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("N", [8, 33, 65, 513])
def test_reference_exact_equals_reference_up_to_513(N):
    """The index-based reference against the rounded-float one where that is exact: the random densities of the tests
    above, both sides, the two uniform grids, and the patterns of `patterns`."""
    for density in (0.3, 0.6, 0.95, 0.995):
        X = np.random.default_rng(1000 * N + int(1000 * density)).random((N, N)) < density
        for Y in (X, ~X):
            _assert_same_reference(reference_exact(Y), reference(Y), (N, density))
    for Y in (np.ones((N, N), dtype=bool), np.zeros((N, N), dtype=bool)):
        _assert_same_reference(reference_exact(Y), reference(Y), (N, 'uniform'))
    if N <= 65:
        for name, U, _ in patterns(N, tile_from_source()):
            for Y in (U < T, ~(U < T)):
                _assert_same_reference(reference_exact(Y), reference(Y), (N, name))


def test_reference_exact_equals_the_model_above_513():
    """N = 700, beyond `reference`: the index-based reference and the numpy model of the two passes give the same map,
    words and histogram at a dense, a sparse and a nearly empty background."""
    N = 700
    for density in (0.6, 0.95, 0.999):
        U = mh.field_of(np.random.default_rng(700 + int(1000 * density)).random((N, N)) < density)
        D2 = distance.squared_distance(U, T)
        ref = reference_exact(U < T)
        assert np.array_equal(ref[0], D2), density
        assert np.array_equal(ref[1], distance.summary_of(D2)) and np.array_equal(ref[2], distance.histogram_of(D2))
        assert ref[1][1] >= 2 and ref[1][4] == 0


@pytest.mark.parametrize("background", [((0, 0),), ((0, 0), (699, 3), (350, 699))], ids=['one-pixel', 'three-pixels'])
def test_reference_exact_equals_the_closed_form(background):
    """N = 700, a background of one pixel and of three: D2 = min_k (i - i_k)^2 + (j - j_k)^2."""
    N = 700
    X = np.ones((N, N), dtype=bool)
    for i, j in background:
        X[i, j] = False
    D2 = closed_form(N, background)
    ref = reference_exact(X)
    assert np.array_equal(ref[0], D2)
    assert np.array_equal(ref[1], distance.summary_of(D2)) and np.array_equal(ref[2], distance.histogram_of(D2))
    if len(background) == 1:
        assert ref[1].tolist() == [N * N - 1, 2 * (N - 1) ** 2, N * N - 1, 2 * N * sum(k * k for k in range(N)), 0]
        assert ref[2][-1] >= 1 and len(ref[2]) == distance.bin_count(N)


def test_the_sentinel_and_ninf_by_the_definition():
    for N in (8, 33):
        D2 = distance.squared_distance(np.full((N, N), FG), T)
        assert D2.dtype == np.int32 and np.all(D2 == distance.CHS_DT_INF) and distance.CHS_DT_INF == INF
        w = distance.summary_of(D2)
        assert list(w) == [N * N, 0, -1, 0, N * N]
        assert distance.histogram_of(D2).sum() == 0 and len(distance.histogram_of(D2)) == distance.bin_count(N)
        di = distance.Distance(w, N, T, hist=distance.histogram_of(D2), d2=D2)
        assert di.r_max is None and di.r2_mean is None and di.r_floor_mean is None and di.argmax is None
        assert di.quantile(0.5) is None and di.finite == 0
        above = model_look(np.full((N, N), FG), T, 'above')
        assert above.fg == 0 and above.ninf == 0 and not above.d2.any() and above.r_max is None
    assert INF > 2 * (16384 - 1) ** 2 and (16384 - 1) ** 2 + INF < 2 ** 31


@pytest.mark.parametrize("N", tile_sizes(tile_from_source()))
def test_patterns_with_known_answers(N):
    for name, U, want in patterns(N, tile_from_source()):
        check_pattern(model_look, name, U, want, N)


@pytest.mark.parametrize("N", [8, 33])
def test_threshold_nan_and_one_ulp_fields(N):
    """The fields of test_morphology_host.hand_made: a pixel at the threshold and a NaN pixel are background below and
    foreground above; one ulp decides."""
    for name, U, t, _ in mh.hand_made(N):
        Xb = np.nan_to_num(U, nan=np.inf) < t
        check_look(model_look(U, t, 'below'), Xb, name)
        check_look(model_look(U, t, 'above'), ~Xb, name)
        if name == 'nan-pixel':
            above = model_look(U, t, 'above')             # the NaN pixel alone is foreground there
            assert model_look(U, t, 'below').d2[3, 4] == 0 and above.d2[3, 4] == 1 and above.fg == 1
        if name == 'one-ulp':
            assert model_look(U, t, 'below').fg == 1 and model_look(U, t, 'above').fg == N * N - 1


def test_radius_bins_at_perfect_squares_and_one_below():
    ks = np.array([1, 2, 3, 7, 100, 1000, 4095, 5791, 23169, 32767], dtype=np.int64)
    assert np.array_equal(distance.radius_bins(ks * ks), ks)
    assert np.array_equal(distance.radius_bins(ks * ks - 1), ks - 1)
    assert np.array_equal(distance.radius_bins(ks * ks + 2 * ks), ks)           # one below the next square
    assert np.array_equal(distance.radius_bins([0, 1, 2, 3, 4, 5, 8, 9]), [0, 1, 1, 1, 2, 2, 2, 3])
    every = np.arange(0, 70000, dtype=np.int64)
    assert np.array_equal(distance.radius_bins(every), [math.isqrt(int(v)) for v in every])
    assert distance.radius_bins(np.zeros((3, 3), dtype=np.int32)).shape == (3, 3)
    with pytest.raises(ValueError):
        distance.radius_bins([-1])
    for N in (1, 2, 8, 100, 4096, 16384):
        assert distance.bin_count(N) == math.isqrt(2 * (N - 1) ** 2) + 1
    assert distance.bin_count(8) == 10 and distance.bin_count(0) == 0


def test_distance_object():
    N = 33
    U = mh.field_of(np.random.default_rng(5).random((N, N)) < 0.8)
    D2 = distance.squared_distance(U, T)
    words, hist = distance.summary_of(D2), distance.histogram_of(D2)
    di = distance.Distance(words, N, T, 'below', hist=hist, d2=D2, delx=0.25)
    fin = D2[D2 > 0].astype(np.int64)
    assert di.fg == fin.size == di.finite and di.d2max == fin.max() and di.sumd2 == fin.sum()
    assert di.r_max == math.sqrt(di.d2max) and di.r_max_phys == di.r_max * 0.25 and di.r2_mean == fin.sum() / fin.size
    ks = np.array([math.isqrt(int(v)) for v in fin])
    assert di.r_floor_mean == ks.sum() / ks.size
    assert di.argmax == divmod(int(np.flatnonzero(D2.ravel() == fin.max())[0]), N)
    srt = np.sort(ks)
    for q in (0.0, 0.1, 0.5, 0.9, 1.0):
        assert di.quantile(q) == srt[max(1, math.ceil(q * srt.size)) - 1], q
    assert di.quantile(1.0) == math.isqrt(di.d2max)
    with pytest.raises(ValueError):
        di.quantile(1.5)
    bare = distance.Distance(words, N, T, 1)
    assert bare.side == 'above' and bare.hist is None and bare.d2 is None and bare.r_floor_mean is None
    assert bare.quantile(0.5) is None and bare.r_max == di.r_max and bare.r_max_phys is None
    # the consistency checks
    bad = hist.copy()
    bad[1] += 1
    with pytest.raises(ValueError, match='adds up'):
        distance.Distance(words, N, T, hist=bad)
    bad = hist.copy()
    bad[1] -= 1
    bad[-1] += 1
    with pytest.raises(ValueError, match='isqrt'):
        distance.Distance(words, N, T, hist=bad)
    with pytest.raises(ValueError, match='bins'):
        distance.Distance(words, N, T, hist=hist[:-1])
    for k, v in ((distance.CHS_DT_NINF, 1), (distance.CHS_DT_NINF, N * N - 1), (distance.CHS_DT_FG, N * N + 1),
                 (distance.CHS_DT_D2MAX_FIRST, -1), (distance.CHS_DT_D2MAX_FIRST, N * N), (distance.CHS_DT_SUMD2, 0)):
        w = words.copy()
        w[k] = v
        with pytest.raises(ValueError):
            distance.Distance(w, N, T)
    bad = D2.copy()
    bad[di.argmax] += 1
    with pytest.raises(ValueError, match='map'):
        distance.Distance(words, N, T, d2=bad)
    bad = hist.copy()                                 # a histogram that fits the words, but is not the map's
    assert math.isqrt(di.d2max) >= 2 and hist[1] > 1
    bad[1] -= 1
    bad[2] += 1
    assert distance.Distance(words, N, T, hist=bad).hist[2] == hist[2] + 1
    with pytest.raises(ValueError, match='histogram'):
        distance.Distance(words, N, T, hist=bad, d2=D2)
    with pytest.raises(ValueError):
        distance.Distance(words, N, T, d2=D2[:-1])
    with pytest.raises(ValueError):
        distance.Distance(words[:4], N, T)
    with pytest.raises(ValueError):
        distance.Distance(words, N, T, side='left')


def test_bad_arguments():
    U = np.zeros((8, 8))
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            distance.squared_distance(U, bad)
    with pytest.raises(ValueError):
        distance.squared_distance(np.zeros((8, 9)), 0.5)
    with pytest.raises(ValueError):
        distance.squared_distance(U, 0.5, side='left')
    assert distance.side_code is components.side_code


# ---------------------------------------------------------------------------
# header, binding, experiment
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_DT_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_DT_WORDS'] == distance.CHS_DT_WORDS == _lib.CHS_DT_WORDS == len(distance.WORDS) == 5
    for i, w in enumerate(distance.WORDS):
        assert defs['CHS_DT_' + w.upper()] == getattr(distance, 'CHS_DT_' + w.upper()) == i
    m = re.search(r'#define\s+CHS_DT_INF\s+\(1\s*<<\s*(\d+)\)', hdr)
    assert m and 1 << int(m.group(1)) == distance.CHS_DT_INF == _lib.CHS_DT_INF == INF
    assert distance.CHS_DT_INF > 2 * (16384 - 1) ** 2                    # N of chs_create is at most 16384


_CTYPES = dict(mh._CTYPES)
_CTYPES['int32_t*'] = ctypes.POINTER(ctypes.c_int32)
DT_SYMBOLS = ['chs_distance_bins', 'chs_distance', 'chs_distance_hist', 'chs_distance_map', 'chs_distance_last_ms',
              'chs_distance_tile', 'chs_batch_distance', 'chs_batch_distance_hist', 'chs_batch_distance_map']


@pytest.mark.parametrize("name", DT_SYMBOLS)
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


def test_entry_points_that_need_no_device(hip_lib):
    assert _lib.distance_tile() == tile_from_source()
    assert hip_lib.chs_distance_tile(None, None) == _lib.CHS_EINVAL
    for N in (1, 2, 8, 33, 100, 513, 4096, 8192, 16384):
        assert hip_lib.chs_distance_bins(N) == _lib.distance_bins(N) == distance.bin_count(N)
    assert hip_lib.chs_distance_bins(0) == 0 and hip_lib.chs_distance_bins(-3) == 0


def _widths_checks(text, rows):
    from chsimpy_amd import experiment
    lines = text.splitlines()
    assert lines[0] == ('id,threshold,fg_below,r_max_below,r2_mean_below,r_floor_mean_below,q50_below,q90_below,'
                        'fg_above,r_max_above,r2_mean_above,r_floor_mean_above,q50_above,q90_above')
    assert lines[0] == ','.join(experiment.WIDTHS_COLS) and len(lines) == 1 + rows
    assert [ln.split(',')[0] for ln in lines[1:]] == [str(i) for i in range(rows)]
    for ln in lines[1:]:
        f = ln.split(',')
        i = int(f[0])
        assert len(f) == 14 and int(f[2]) == i + 1 and int(f[2]) + int(f[8]) == 16 * 16
        assert float(f[9]) == i + 2 and '.' in f[9] and '.' not in f[2] and '.' not in f[12] and int(f[13]) == i + 2


def test_experiment_writes_the_widths_file_on_a_dry_run(tmp_path):
    """--widths adds <id>-widths.csv and leaves the result files byte for byte what they are without it, member by
    member and in batches (members without device work: launcher, gather and writer alone)."""
    from chsimpy_amd import experiment
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'plain', '--droplets'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'wide', '--droplets', '--widths'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'batch', '--batch', '2', '--widths'])
    finally:
        os.chdir(cwd)
    assert not (tmp_path / 'plain-widths.csv').exists() and not (tmp_path / 'batch-droplets.csv').exists()
    text = (tmp_path / 'wide-widths.csv').read_text()
    _widths_checks(text, 3)
    assert (tmp_path / 'batch-widths.csv').read_text() == text
    for kind in ('results.csv', 'results-agg.csv', 'droplets.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'wide-{kind}').read_bytes()
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'batch-{kind}').read_bytes()
    nan = float('nan')
    row = (0, 0.5, 0, nan, nan, nan, -1, -1, 256, 3.0, 2.5, 1.25, 1, 2)
    assert experiment.write_widths(str(tmp_path / 'w'), [row]).endswith('w-widths.csv')
    assert (tmp_path / 'w-widths.csv').read_text().splitlines()[1] == '0,0.5,0,nan,nan,nan,-1,-1,256,3.0,2.5,1.25,1,2'
    di = model_look(mh.field_of(np.random.default_rng(2).random((16, 16)) < 0.5), T, 'below')
    side = experiment._widths_side(di)
    assert side == (di.fg, di.r_max, di.r2_mean, di.r_floor_mean, di.quantile(0.5), di.quantile(0.9))
    assert experiment._widths_side(model_look(np.full((8, 8), BG), T, 'below'))[4:] == (-1, -1)


def test_experiment_widths_under_gloo_at_world_2(tmp_path):
    """`--gpus 2 --backend gloo --dry-run --widths`: two ranks gather their members' rows; rank 0 writes the file a
    single rank writes."""
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    base = ['-N', '16', '-K', '3e-4', '-R', '7', '--dry-run', '--backend', 'gloo', '--widths']
    r2 = subprocess.run([sys.executable, '-m', 'chsimpy_amd.experiment', '--gpus', '2', '--file-id', str(tmp_path / 'w2')] + base,
                        env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-3000:]
    r1 = subprocess.run([sys.executable, '-m', 'chsimpy_amd.experiment', '--file-id', str(tmp_path / 'w1')] + base,
                        env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r1.returncode == 0, r1.stderr[-3000:]
    text = (tmp_path / 'w2-widths.csv').read_text()
    _widths_checks(text, 7)
    assert text == (tmp_path / 'w1-widths.csv').read_text()
    assert 'ranks, 2' in (tmp_path / 'w2-metadata.csv').read_text() and 'w2-widths.csv' in r2.stdout
