"""Host side of the geodesic look (chsimpy_amd/geodesic.py): the two models against each other and against
scipy.sparse.csgraph.dijkstra on the explicit pixel graph, closed forms for all four sources, the certificate, the
synchronous tile model against the default round limit, the consistency checks of `Geodesic`, the header's constants and
prototypes, and the host model of the relaxation rounds (tests/geo_model.cpp, built with the address and
undefined-behaviour sanitizers).  No device.

The definition (include/chs_hip.h: chs_geodesic).  Foreground, ``side`` and ``connectivity`` are those of chs_components,
with no wrap-around.  ``source`` is one of four walls: 0 is row 0, 1 is row N-1, 2 is column 0, 3 is column N-1; the target
is the opposite wall; the depth k of a pixel is its distance from the source wall along that axis.  A path moves from a
foreground pixel to a foreground neighbour: at connectivity 4 an axial step costs 1 (UNIT = 1), at connectivity 8 an axial
step costs 3 and a diagonal step 4 (UNIT = 3), a diagonal step needing only its two end pixels to be foreground.  G[p] is
-1 for background, 0 for a foreground pixel on the source wall, otherwise the smallest cost of a path from any such pixel
to p, CHS_GEO_INF for a foreground pixel that no path reaches.  Bin d of the histogram (4N bins) counts the reached pixels
with G // UNIT == d, the last bin everything beyond; the profile holds, per depth, the foreground pixels, the reached
pixels and the sum of G over them.  Every comparison of map, histogram, profile and the 15 unique words is for equality;
ROUNDS is only ever compared with bounds.

`patterns`, `random_masks`, `check_look` and `model` are shared with tests/test_gpu_geodesic.py, which puts the same
fields on the device."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from chsimpy_amd import _lib, batch, components, geodesic
import test_morphology_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = mh.T
SIDES = ('below', 'above')
CONNS = (4, 8)
SOURCES = (0, 1, 2, 3)
INF = geodesic.CHS_GEO_INF


# ---------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------
def serpentine(N):
    """Even rows full, odd rows one pixel at alternating ends: a one-pixel corridor through the whole grid."""
    X = np.zeros((N, N), dtype=bool)
    X[0::2] = True
    for k, i in enumerate(range(1, N, 2)):
        X[i, N - 1 if k % 2 == 0 else 0] = True
    return X


def spiral(N):
    """A one-pixel corridor that winds inwards from the corner (0, 0), walls one pixel thick."""
    X = np.zeros((N, N), dtype=bool)
    i = j = 0
    di, dj = 0, 1
    X[0, 0] = True
    for _ in range(N * N):
        ni, nj = i + di, j + dj
        ahead = (0 <= ni < N and 0 <= nj < N and not X[ni, nj]
                 and not (0 <= ni + di < N and 0 <= nj + dj < N and X[ni + di, nj + dj]))
        if not ahead:
            di, dj = dj, -di
            ni, nj = i + di, j + dj
            if not (0 <= ni < N and 0 <= nj < N) or X[ni, nj] or (0 <= ni + di < N and 0 <= nj + dj < N and X[ni + di, nj + dj]):
                break
        i, j = ni, nj
        X[i, j] = True
    return X


def comb(N):
    """A spine along row 0 and column 0 with teeth: dead ends of every length."""
    X = np.zeros((N, N), dtype=bool)
    X[0] = True
    X[:, 0] = True
    for j in range(2, N, 2):
        X[:1 + (j * 7) % N, j] = True
    return X


def islands(N):
    """A frame that every wall touches, and blocks inside it that nothing reaches."""
    X = np.zeros((N, N), dtype=bool)
    X[0], X[N - 1], X[:, 0], X[:, N - 1] = True, True, True, True
    for i in range(2, N - 3, 5):
        for j in range(2, N - 3, 5):
            X[i:i + 2, j:j + 3] = True
    return X


def staircase(N, back=False):
    """A corridor whose only link between two tiles is a diagonal step through a tile corner: down column 63 to (63, 63),
    over the corner to (64, 64) and down column 64 -- or, `back`, down column 64 to (63, 64), over to (64, 63) and down
    column 63.  The other two pixels of the corner are background, so the tile behind is reached only if a changed corner
    pixel wakes the diagonal neighbour: what a flagging rule of sides alone gets wrong."""
    assert N >= 130
    X = np.zeros((N, N), dtype=bool)
    a, b = (64, 63) if back else (63, 64)
    X[0:64, a] = True
    X[64:N, b] = True
    return X


def patterns(N):
    out = [('full', np.ones((N, N), dtype=bool)), ('empty', np.zeros((N, N), dtype=bool))]
    inner = np.zeros((N, N), dtype=bool)
    inner[1:-1, 1:-1] = True
    out.append(('no sources', inner))                          # every source wall is background
    out += [('serpentine', serpentine(N)), ('serpentine T', serpentine(N).T.copy()), ('spiral', spiral(N)), ('comb', comb(N)),
            ('islands', islands(N)), ('diagonal', np.eye(N, dtype=bool)), ('antidiagonal', np.eye(N, dtype=bool)[::-1].copy())]
    if N >= 130:
        out += [('staircase', staircase(N)), ('staircase back', staircase(N, True))]
    return out


DENSITY = {4: 0.62, 8: 0.45}


# (N, connectivity): the first seed whose mask percolates from the top wall and the first whose mask does not, found by a
# search over the seeds on the CPU (the densities lie above the percolation thresholds, so most masks percolate)
SEEDS = {(33, 4): (0, 1), (33, 8): (0, 4), (100, 4): (0, 21), (100, 8): (0, 200), (128, 4): (0, 2), (128, 8): (0, 854),
         (129, 4): (0, 83), (129, 8): (0, 5)}


@functools.lru_cache(maxsize=None)
def random_masks(N, conn):
    """Random masks at density 0.62 (connectivity 4) or 0.45 (8): a percolating and a non-percolating one (source top),
    which is asserted here: [(seed, X, percolates)]."""
    out = []
    for seed in SEEDS[N, conn]:
        X = np.random.default_rng(1000 * N + 10 * seed + conn).random((N, N)) < DENSITY[conn]
        G = geodesic.relax(X, conn, 0)
        out.append((seed, X, bool(((G[N - 1] >= 0) & (G[N - 1] != INF)).any())))
    assert [perc for _, _, perc in out] == [True, False], (N, conn)
    return out


@functools.lru_cache(maxsize=None)
def _model_cached(key, conn, source):
    X = _MASKS[key]
    G = geodesic.relax(X, conn, source)
    return G, geodesic.stats_of(G, conn, source)


_MASKS = {}


def model(X, conn, source):
    """(G, (words, hist, profile)) of the mask X by the vectorised model, computed once per mask and arguments; the
    component words are not filled in."""
    key = (X.shape[0], X.tobytes())
    _MASKS[key] = X
    return _model_cached(key, conn, source)


def check_look(got, X, conn, source, what=''):
    """A `Geodesic` with map, histogram and profile against the model of the mask X, bit for bit; ROUNDS against its
    bounds."""
    G, (words, hist, profile) = model(X, conn, source)
    assert np.array_equal(got.G, G), what
    labels, table = components.label(mh.field_of(X), T, conn)
    words = words.copy()
    words[geodesic.CHS_GEO_CC_COUNT] = table.shape[0]
    words[geodesic.CHS_GEO_CC_REACHED] = np.unique(labels[X & (geodesic.depth_of(X.shape[0], source) == 0)]).size
    words[geodesic.CHS_GEO_LIMIT] = got.limit
    assert np.array_equal(got.words[geodesic.UNIQUE], words[geodesic.UNIQUE]), (what, got.words, words)
    assert np.array_equal(got.hist, hist) and np.array_equal(got.profile, profile), what
    assert geodesic.certificate(got.G, conn, source) == 0, what
    if got.sources == 0:
        assert got.rounds == 0, what
    else:
        assert 1 <= got.rounds <= geodesic.rounds_bound(X, conn, source), (what, got.rounds)


# ---------------------------------------------------------------------------
# 1. the two models, and scipy
# ---------------------------------------------------------------------------
def all_masks():
    out = []
    for N in (8, 65):
        out += [(f"{name} N={N}", X) for name, X in patterns(N)]
    out += [(f"{name} N=130", X) for name, X in patterns(130) if name in ('staircase', 'staircase back', 'serpentine')]
    for N in (33, 100):
        for conn in CONNS:
            out += [(f"random N={N} seed={seed} d={DENSITY[conn]}", X) for seed, X, _ in random_masks(N, conn)]
    return out


MASKS = all_masks()


@pytest.mark.parametrize("name,X", MASKS, ids=[m[0] for m in MASKS])
def test_the_two_models_agree(name, X):
    for conn in CONNS:
        for source in SOURCES:
            a, b = geodesic.relax(X, conn, source), geodesic.dijkstra(X, conn, source)
            assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (name, conn, source)
            assert np.array_equal(a >= 0, X)


def graph_of(X, conn):
    from scipy import sparse
    N = X.shape[0]
    idx = np.arange(N * N).reshape(N, N)
    rows, cols, ws = [], [], []
    for di, dj, w in geodesic._steps(conn):
        src = X[max(0, -di):N - max(0, di), max(0, -dj):N - max(0, dj)] & X[max(0, di):N - max(0, -di), max(0, dj):N - max(0, -dj)]
        a = idx[max(0, -di):N - max(0, di), max(0, -dj):N - max(0, dj)][src]
        b = idx[max(0, di):N - max(0, -di), max(0, dj):N - max(0, -dj)][src]
        rows.append(a); cols.append(b); ws.append(np.full(a.size, w))
    return sparse.csr_matrix((np.concatenate(ws), (np.concatenate(rows), np.concatenate(cols))), shape=(N * N, N * N))


@pytest.mark.parametrize("name,X", MASKS[::3], ids=[m[0] for m in MASKS[::3]])
def test_models_against_scipy_on_the_pixel_graph(name, X):
    csgraph = pytest.importorskip('scipy.sparse.csgraph')
    N = X.shape[0]
    for conn in CONNS:
        graph = graph_of(X, conn)
        for source in SOURCES:
            srcs = np.flatnonzero((X & (geodesic.depth_of(N, source) == 0)).ravel())
            want = np.where(X, INF, -1).astype(np.int64)
            if srcs.size:
                d = csgraph.dijkstra(graph, directed=True, indices=srcs, min_only=True).reshape(N, N)
                want = np.where(X, np.where(np.isfinite(d), d, INF), -1).astype(np.int64)
            for fn in (geodesic.relax, geodesic.dijkstra):
                assert np.array_equal(fn(X, conn, source), want), (name, conn, source, fn.__name__)


# ---------------------------------------------------------------------------
# 2. closed forms, for all four sources
# ---------------------------------------------------------------------------
def oriented(X, source):
    """The mask drawn for source top, turned so that it means the same for `source`."""
    return np.ascontiguousarray(geodesic._from_top(X, source))


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("N", [1, 8, 65])
def test_closed_forms(N, conn, source):
    unit = geodesic.unit_of(conn)
    depth = geodesic.depth_of(N, source)
    full = np.ones((N, N), dtype=bool)
    for fn in (geodesic.relax, geodesic.dijkstra):
        assert np.array_equal(fn(full, conn, source), unit * depth)                        # the full grid: G = UNIT k
        if N == 1:
            continue
        top = np.zeros((N, N), dtype=bool)
        top[:, N // 3] = True                                                              # a straight corridor
        X = oriented(top, source)
        assert np.array_equal(fn(X, conn, source), np.where(X, unit * depth, -1))
        X = np.eye(N, dtype=bool)                                                          # the main diagonal
        G = fn(X, conn, source)
        if conn == 8:
            assert np.array_equal(G, np.where(X, 4 * depth, -1))
        else:
            assert np.array_equal(G, np.where(X, np.where(depth == 0, 0, INF), -1))
        top = np.zeros((N, N), dtype=bool)                                                 # an L: down column 1, then along row m
        m = N // 2
        top[:m + 1, 1] = True
        top[m, 1:] = True
        want = np.full((N, N), -1, dtype=np.int64)
        want[:m + 1, 1] = unit * np.arange(m + 1)
        want[m, 1:] = unit * (m + np.arange(N - 1))
        if conn == 8:
            want[m, 2:] -= 2                                                               # the corner is cut: 4 for 3 + 3
        assert np.array_equal(fn(oriented(top, source), conn, source), oriented(want, source))
    w, hist, profile = geodesic.stats_of(unit * depth, conn, source, cc_count=1, cc_reached=1)
    g = geodesic.Geodesic(w, N, T, conn, 'below', source, hist=hist, profile=profile)
    assert g.fg == g.reached == N * N and g.sources == g.target_reached == N and g.gmin_target == g.gmax == unit * (N - 1)
    assert g.gmin_target_pos == 0 and g.gmax_first == (0 if N == 1 else [N * (N - 1), 0, N - 1, 0][source])
    assert np.array_equal(hist[:N], np.full(N, N)) and not hist[N:].any()
    assert np.array_equal(profile, np.stack([np.full(N, N), np.full(N, N), unit * N * np.arange(N)], axis=1))
    assert g.tortuosity == 1.0 and g.mean_tortuosity == 1.0 and g.accessible_fraction == 1.0 and g.isolated == 0


def test_the_chamfer_bound_in_free_space():
    """G / UNIT over the Euclidean length, from a single source pixel over a full grid: within [0.9428, 1.0541], and
    both ends are met -- the bound DESIGN.md states."""
    N = 200
    X = np.ones((N, N), dtype=bool)
    X[0, 1:] = False                                           # one source pixel, (0, 0); row 1 on is free
    G = geodesic.relax(X, 8, 0)
    ii, jj = np.mgrid[0:N, 0:N]
    far = (ii >= 1) & (ii >= jj)                               # straight lines from (0, 0) that stay inside the free part
    ratio = G[far] / 3.0 / np.hypot(ii[far], jj[far])
    lo, hi = geodesic.CHAMFER_BOUNDS
    assert lo <= ratio.min() and ratio.max() <= hi
    assert ratio.min() < lo + 2e-4 and ratio.max() > hi - 2e-4
    assert abs(lo - 4 / (3 * np.sqrt(2))) < 1e-4 and abs(hi - np.sqrt(10) / 3) < 1e-4


# ---------------------------------------------------------------------------
# 3. the certificate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
def test_the_certificate_holds_for_the_model_and_fails_one_off(conn):
    rng = np.random.default_rng(5)
    masks = [X for _, X in patterns(33)] + [X for _, X, _ in random_masks(33, conn)]
    tried = 0
    for X in masks:
        for source in SOURCES:
            G = geodesic.relax(X, conn, source)
            assert geodesic.certificate(G, conn, source) == 0
            ii, jj = np.nonzero((G >= 0) & (G != INF))
            for k in rng.permutation(ii.size)[:6]:
                for delta in (1, -1):
                    if G[ii[k], jj[k]] + delta < 0:
                        continue
                    H = G.copy()
                    H[ii[k], jj[k]] += delta
                    assert geodesic.certificate(H, conn, source) > 0, (conn, source, ii[k], jj[k], delta)
                    tried += 1
            un = np.argwhere(G == INF)
            if un.size and ii.size:                             # an unreached pixel beside a reached one: (d)
                H = G.copy()
                H[ii[0], jj[0]] = INF
                assert geodesic.certificate(H, conn, source) > 0
    assert tried > 100


# ---------------------------------------------------------------------------
# 4. the rounds of the tile model against the default limit
# ---------------------------------------------------------------------------
def test_rounds_default(hip_lib):
    for N, want in ((1, 96), (8, 96), (64, 96), (65, 192), (130, 352), (4096, 32 * 4096 + 64)):
        assert geodesic.rounds_default(N) == _lib.geodesic_rounds_default(N) == hip_lib.chs_geodesic_rounds_default(N) == want
        assert geodesic.bins(N) == _lib.geodesic_bins(N) == 4 * N
    assert hip_lib.chs_geodesic_rounds_default(0) == 0 and hip_lib.chs_geodesic_bins(0) == 0


def test_the_serpentine_stays_within_the_default_limit():
    """The one-pixel serpentine is what the default limit admits: the tile model needs 2, 35 and 132 rounds at N = 8, 65
    and 130, against limits of 96, 192 and 352 -- and more than 16 at N = 130."""
    got = {N: geodesic.rounds_bound(serpentine(N), 4, 'top') for N in (8, 65, 130)}
    assert got[8] <= 2 and got[65] == 35 and got[130] == 132, got
    for N, r in got.items():
        assert 1 <= r <= geodesic.rounds_default(N)
    assert got[130] > 16
    for conn in CONNS:
        for source in SOURCES:
            for X in (serpentine(130), serpentine(130).T):
                assert geodesic.rounds_bound(X, conn, source) <= geodesic.rounds_default(130)


def test_rounds_bound_of_simple_masks():
    N = 130
    empty = np.zeros((N, N), dtype=bool)
    assert geodesic.rounds_bound(empty, 8, 'top') == 0
    lone = np.eye(N, dtype=bool)
    assert geodesic.rounds_bound(lone, 4, 'top') == 1                  # only the source pixel: nothing ever changes
    full = np.ones((N, N), dtype=bool)
    for source in SOURCES:
        assert geodesic.rounds_bound(full, 4, source) == 4              # three tiles deep: a round each, and one more
    assert geodesic.rounds_bound(lone, 8, 'top') == 4                   # through the corners (63,63)-(64,64), (127,127)-(128,128)


# ---------------------------------------------------------------------------
# 5. the result class
# ---------------------------------------------------------------------------
def test_geodesic_object():
    N = 40
    _, X, perc = [m for m in random_masks(33, 4)][0]
    U = mh.field_of(islands(N))
    g = geodesic.model_look(U, T, 4, 'below', 'left')
    h = geodesic.model_look(U, T, 4, 'below', 'left', method='dijkstra')
    assert np.array_equal(g.words, h.words) and np.array_equal(g.hist, h.hist) and np.array_equal(g.profile, h.profile)
    assert g.percolates and g.source == 'left' and g.side == 'below' and g.connectivity == 4 and g.unit == 1
    assert g.tortuosity == 1.0 and g.shortest_path == N - 1 and g.mean_tortuosity > 1.0      # along the frame's rows
    assert g.isolated == g.fg - g.reached > 0 and g.accessible_fraction == g.reached / g.fg < 1.0
    assert g.cc_reached == 1 and g.cc_count > 1 and g.rounds == 1 and g.limit == geodesic.rounds_default(N)
    cdf = g.depth_cdf()
    assert cdf.shape == (4 * N,) and np.all(np.diff(cdf) >= 0) and cdf[-1] == g.accessible_fraction and cdf[0] == g.sources / g.fg
    tp = g.tortuosity_profile()
    assert np.isnan(tp[0]) and np.all(tp[1:] >= 1.0) and tp[N - 1] == g.mean_tortuosity
    gm = g.g
    assert np.isnan(gm[~islands(N)]).all() and np.isinf(gm[3, 3]) and gm[0, N - 1] == N - 1
    with pytest.raises(ValueError):
        g.shortest_path_phys
    p = geodesic.Geodesic(g.words, N, T, 4, 'below', 'left', hist=g.hist, profile=g.profile, g=g.G, delx=0.25)
    assert p.shortest_path_phys == 0.25 * (N - 1) and p.max_reach_phys == 0.25 * p.max_reach and p.mean_path_phys == 0.25 * p.mean_path
    assert np.array_equal(p.g_phys[islands(N) & np.isfinite(gm)], 0.25 * gm[islands(N) & np.isfinite(gm)]) and p.depth_phys()[4] == 1.0
    e = geodesic.model_look(mh.field_of(np.eye(N, dtype=bool)), T, 4)                        # not percolating
    assert not e.percolates and e.tortuosity == float('inf') and e.mean_tortuosity == float('inf') and e.reached == 1
    e8 = geodesic.model_look(mh.field_of(np.eye(N, dtype=bool)), T, 8)
    assert e8.percolates and e8.tortuosity == 4 / 3 and e8.unit == 3
    none = geodesic.model_look(mh.field_of(np.zeros((N, N), dtype=bool)), T, 8)
    assert none.fg == 0 and none.accessible_fraction == 0.0 and none.rounds == 0 and not none.depth_cdf().any()
    up = geodesic.model_look(U, T, 8, 'above', 'bottom')                                     # the complement: no wall pixel
    assert up.sources == 0 and up.reached == 0 and up.fg == N * N - g.fg and up.gmax == -1
    # words that no map has
    W = geodesic
    for k, v in ((W.CHS_GEO_REACHED, g.fg + 1), (W.CHS_GEO_SOURCES, g.reached + 1), (W.CHS_GEO_UNIT, 3), (W.CHS_GEO_GMIN_TARGET, -1),
                 (W.CHS_GEO_GMIN_TARGET, N - 2), (W.CHS_GEO_GMAX, -1), (W.CHS_GEO_TARGET_REACHED, g.target_fg + 1),
                 (W.CHS_GEO_CC_REACHED, g.cc_count + 1), (W.CHS_GEO_ROUNDS, 0), (W.CHS_GEO_ROUNDS, g.limit + 1),
                 (W.CHS_GEO_GSUM, g.gmax * g.reached + 1), (W.CHS_GEO_GMAX_FIRST, N * N)):
        bad = g.words.copy()
        bad[k] = v
        with pytest.raises(ValueError):
            geodesic.Geodesic(bad, N, T, 4, 'below', 'left')
    with pytest.raises(ValueError):
        geodesic.Geodesic(g.words[:-1], N, T, 4, 'below', 'left')
    for hist in (g.hist[:-1], g.hist + (np.arange(4 * N) == 1), np.roll(g.hist, 1)):
        with pytest.raises(ValueError):
            geodesic.Geodesic(g.words, N, T, 4, 'below', 'left', hist=hist)
    for prof in (g.profile[:-1], g.profile + 1, g.profile[::-1]):
        with pytest.raises(ValueError):
            geodesic.Geodesic(g.words, N, T, 4, 'below', 'left', profile=prof)
    with pytest.raises(ValueError):
        geodesic.Geodesic(g.words, N, T, 4, 'below', 'left', g=g.G[:-1])
    for bad in ('middle', 4, -1, True):
        with pytest.raises(ValueError):
            geodesic.source_code(bad)
    assert [geodesic.source_code(s) for s in ('top', 'bottom', 'left', 'right', 2)] == [0, 1, 2, 3, 2]
    assert 'tortuosity=1.0000' in repr(g)


def test_both_sides_and_the_hand_made_fields():
    for N in (8, 33):
        for name, U, t, _ in mh.hand_made(N):
            for side in SIDES:
                X = components.foreground(U, t, side)
                for conn in CONNS:
                    g = geodesic.model_look(U, t, conn, side, 'top')
                    assert g.fg == int(X.sum()) and np.array_equal(g.G >= 0, X), (name, side)
                    assert np.array_equal(g.G, geodesic.dijkstra(X, conn, 0))


# ---------------------------------------------------------------------------
# 6. the header, the binding
# ---------------------------------------------------------------------------
GEO_SYMBOLS = [s for s in _lib.SYMBOLS if 'geodesic' in s]
_CTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double,
           'chs_handle': ctypes.c_void_p, 'chs_batch': ctypes.c_void_p, 'int32_t*': ctypes.POINTER(ctypes.c_int32),
           'int64_t*': ctypes.POINTER(ctypes.c_int64), 'double*': ctypes.POINTER(ctypes.c_double)}


def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v, 0) for k, v in re.findall(r'#define\s+(CHS_GEO_[A-Z_0-9]+)\s+(0x[0-9a-f]+|\d+)\b', hdr)}
    assert defs['CHS_GEO_WORDS'] == geodesic.CHS_GEO_WORDS == _lib.CHS_GEO_WORDS == len(geodesic.WORDS) == 16
    assert defs['CHS_GEO_INF'] == geodesic.CHS_GEO_INF == np.iinfo(np.int32).max
    for i, w in enumerate(geodesic.WORDS):
        assert defs['CHS_GEO_' + w.upper()] == getattr(geodesic, 'CHS_GEO_' + w.upper()) == i
    assert (_lib.CHS_GEO_ROUNDS, _lib.CHS_GEO_LIMIT) == (geodesic.CHS_GEO_ROUNDS, geodesic.CHS_GEO_LIMIT)
    assert geodesic.UNIQUE == [k for k in range(16) if k != 14]
    shared = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_geo_host.h')).read()
    assert int(re.search(r'#define\s+CHS_GEO_T\s+(\d+)', shared).group(1)) == geodesic.TILE
    assert int(re.search(r'#define\s+CHS_GEO_UNREACHED\s+(0x[0-9a-f]+)', shared).group(1), 0) == geodesic.CHS_GEO_INF
    assert issubclass(_lib.GeodesicLimitError, _lib.EngineError)
    e = _lib.GeodesicLimitError('x', 16, 16)
    assert (e.rounds, e.limit) == (16, 16)
    assert len(GEO_SYMBOLS) == 13


@pytest.mark.parametrize("name", GEO_SYMBOLS)
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
    assert list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert ctypes.sizeof(fn.restype) == ctypes.sizeof(_CTYPES[ret])


def test_the_members_forward_the_look():
    assert {'geodesic', 'geodesic_look'} <= set(batch._Member._LOOKS)
    for cls in (_lib.Engine, _lib.Batch):
        for name in ('geodesic', 'geodesic_look', 'geodesic_hist', 'geodesic_profile', 'geodesic_map', 'geodesic_ms',
                     'geodesic_rounds_default'):
            assert callable(getattr(cls, name))


# ---------------------------------------------------------------------------
# 7. the host model of the rounds
# ---------------------------------------------------------------------------
def test_host_model_of_the_relaxation_rounds(tmp_path):
    """tests/geo_model.cpp: the in-tile relaxation and the flagging rule through the header the kernel compiles
    (chs_geo_host.h), tile rounds in scrambled orders with halo loads that return an earlier value, against Dijkstra --
    its own executable, under the address and undefined-behaviour sanitizers."""
    from chsimpy_amd import _build
    exe = str(tmp_path / 'geo_model')
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I' + _build.CSRC,
                    os.path.join(ROOT, 'tests', 'geo_model.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and '\n0 failures' in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert int(re.search(r'(\d+) checks', r.stdout).group(1)) > 1000
    hdr = open(os.path.join(_build.CSRC, 'chs_geo_host.h')).read()
    assert not re.search(r'#include\s*[<"](hip/|chs_common|chs_look|chs_fast|chs_cx)', hdr)
    prog = open(os.path.join(ROOT, 'tests', 'geo_model.cpp')).read()
    assert re.findall(r'#include\s*"([^"]+)"', prog) == ['chs_geo_host.h']
    dev = open(os.path.join(_build.CSRC, 'chs_geodesic.hip')).read()
    assert '#include "chs_geo_host.h"' in dev
    for fn in ('chs_geo::relax_segment(', 'chs_geo::wakes(', 'chs_geo::nb_of(', 'CHS_GEO_SWEEP_CAP'):
        assert fn in dev, fn
