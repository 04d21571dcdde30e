"""Host tests (no GPU) of the local thickness: the numpy model of chsimpy_amd/thickness.py against a brute-force painter
over ALL foreground centres, the pruning rule against its direct evaluation, the invariants of the definition, the two
entry points that need no device (chs_thickness_reach, chs_thickness_work_default), the result class and the binding.

Reference: the centres and their radii come from ``np.rint(scipy.ndimage.distance_transform_edt(X) ** 2)`` (CHS_DT_INF
by the definition where the grid has no background: tests/test_distance_host.py, reference); every centre's open disc is
painted by maximum.  Everything is integer: every comparison is for equality."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from chsimpy_amd import _lib, batch, distance, thickness
import test_distance_host as dh
import test_morphology_host as mh

ROOT = dh.ROOT
INF = dh.INF
T = dh.T
SIDES = dh.SIDES


# ---------------------------------------------------------------------------
# the reference, written out
# ---------------------------------------------------------------------------
def brute_reach(R, diagonal):
    """E(R, a, b) over every lattice point of the open disc."""
    a, b = (1, 1) if diagonal else (1, 0)
    rho = math.isqrt(R - 1)
    q = np.arange(-rho, rho + 1, dtype=np.int64)
    qx, qy = np.meshgrid(q, q, indexing='ij')
    inside = qx * qx + qy * qy < R
    return int(((qx - a) ** 2 + (qy - b) ** 2)[inside].max())


def column_reach(R, diagonal):
    """E(R, a, b) over the two ends of every column of the open disc: |q - (a, b)|^2 is convex along a column, so its
    maximum over the column is at an end (checked against brute_reach for small R below)."""
    a, b = (1, 1) if diagonal else (1, 0)
    rho = math.isqrt(R - 1)
    qx = np.arange(-rho, rho + 1, dtype=np.int64)
    y = dh.isqrt_of(R - 1 - qx * qx)
    return int(np.maximum((qx - a) ** 2 + (y - b) ** 2, (qx - a) ** 2 + (-y - b) ** 2).max())


def brute_thickness(D2):
    """T2 by the definition: the open disc of EVERY finite foreground centre, painted by maximum."""
    D2 = np.asarray(D2, dtype=np.int64)
    N = D2.shape[0]
    if (D2 >= INF).any():
        return np.where(D2 >= INF, INF, 0).astype(np.int32)
    T2 = np.zeros((N, N), dtype=np.int64)
    ii, jj = np.mgrid[0:N, 0:N]
    for i, j in zip(*np.nonzero(D2)):
        R = int(D2[i, j])
        rho = math.isqrt(R - 1)
        i0, i1, j0, j1 = max(0, i - rho), min(N, i + rho + 1), max(0, j - rho), min(N, j + rho + 1)
        disc = (ii[i0:i1, j0:j1] - i) ** 2 + (jj[i0:i1, j0:j1] - j) ** 2 < R
        win = T2[i0:i1, j0:j1]
        win[disc & (win < R)] = R
    return T2.astype(np.int32)


def brute_rule(D2):
    """(kept, work) by the rule of the definition, neighbour by neighbour, with the column-end E."""
    D2 = np.asarray(D2, dtype=np.int64)
    N = D2.shape[0]
    if (D2 >= INF).any():
        return 0, 0
    E = {}
    kept = work = 0
    for i, j in zip(*np.nonzero(D2)):
        R = int(D2[i, j])
        if R not in E:
            E[R] = (column_reach(R, False), column_reach(R, True))
        dropped = False
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                if (a or b) and 0 <= i + a < N and 0 <= j + b < N and D2[i + a, j + b] > E[R][1 if (a and b) else 0]:
                    dropped = True
        if not dropped:
            kept += 1
            work += (2 * math.isqrt(R - 1) + 1) ** 2
    return kept, work


def patterns(N):
    """(name, X) hand-made foregrounds at grid size N: one background pixel in the corner (its discs leave the grid over
    two walls) and inside, a disc, an annulus, stripes that reach the opposite walls, the full and the empty grid."""
    i, j = np.mgrid[0:N, 0:N]
    c = (N - 1) / 2.0
    r2 = (i - c) ** 2 + (j - c) ** 2
    full = np.ones((N, N), dtype=bool)
    corner, inside = full.copy(), full.copy()
    corner[0, 0] = False
    inside[N // 3, N // 2 + 1] = False
    w = max(2, N // 9)
    return [('corner pixel', corner), ('inside pixel', inside), ('disc', r2 < (0.4 * N) ** 2),
            ('annulus', (r2 < (0.45 * N) ** 2) & (r2 >= (0.2 * N) ** 2)), ('stripes', (j // w) % 2 == 0),
            ('full', full), ('empty', ~full)]


def smooth_noise(N, seed=5, sigma=4.0):
    g = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((N, N)), sigma)
    return g < np.median(g)


def cases():
    """(name, X): the cases of the definition's own check."""
    out = []
    for N in (8, 100, 129):
        rng = np.random.default_rng(7 * N)
        for density in (0.3, 0.6, 0.95):
            out.append((f"random {density} N={N}", rng.random((N, N)) < density))
    for N in (32, 65):
        out += [(f"{name} N={N}", X) for name, X in patterns(N) if 'pixel' in name]
    out += [(f"{name} N=65", X) for name, X in patterns(65) if 'pixel' not in name]
    out.append(("smooth noise N=128", smooth_noise(128)))
    return out


CASES = cases()
_REFERENCE = {}


def reference(name, X):
    """(D2, T2, kept, work) of a case by brute force, computed once."""
    if name not in _REFERENCE:
        D2 = dh.reference(X)[0]
        D2.setflags(write=False)
        T2 = brute_thickness(D2)
        T2.setflags(write=False)
        _REFERENCE[name] = (D2, T2) + brute_rule(D2)
    return _REFERENCE[name]


def check_invariants(T2, kept, work, D2, what=''):
    D2 = np.asarray(D2, dtype=np.int64)
    T2 = np.asarray(T2, dtype=np.int64)
    N = D2.shape[0]
    assert np.all(T2 >= D2), what
    assert np.array_equal(T2 > 0, D2 > 0), what
    fg, ninf = int((D2 > 0).sum()), int((D2 >= INF).sum())
    if ninf:
        assert ninf == N * N and np.all(T2 == INF) and kept == 0 and work == 0, what
    elif fg:
        assert T2.max() == D2.max() and np.isin(T2[T2 > 0], D2).all() and 1 <= kept <= fg and work >= kept, what
    else:
        assert not T2.any() and kept == 0 and work == 0, what
    hist = thickness.histogram_of(T2)
    assert hist.shape == (distance.bin_count(N),) and int(hist.sum()) == fg - ninf and hist[0] == 0, what
    w = thickness.summary_of(T2, kept, work)
    assert list(w[[0, 4, 5, 6]]) == [fg, ninf, kept, work], what
    if fg - ninf:
        assert w[1] == D2.max() and w[2] == int((T2 == w[1]).sum()) >= 1 and w[3] == int(T2.sum()), what
    else:
        assert list(w[1:4]) == [0, 0, 0], what


def check_look(th, X, what=''):
    """A `Thickness` with map and histogram (the device's or the model's) against the model on the foreground X."""
    D2 = distance.squared_distance(mh.field_of(X), T, 'below')
    T2, kept, work = thickness.local_thickness(D2)
    assert np.array_equal(th.t2, T2), what
    assert np.array_equal(th.words, thickness.summary_of(T2, kept, work)), (what, th.words, thickness.summary_of(T2, kept, work))
    assert np.array_equal(th.hist, thickness.histogram_of(T2)), what
    if th.distance is not None:
        assert np.array_equal(th.distance.words, distance.summary_of(D2)), what
        if th.distance.d2 is not None:
            assert np.array_equal(th.distance.d2, D2), what
    check_invariants(th.t2, th.kept, th.work, D2, what)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,X", CASES, ids=[c[0] for c in CASES])
def test_model_against_the_brute_force_painter(name, X):
    D2, T2ref, kept_ref, work_ref = reference(name, X)
    assert np.array_equal(distance.squared_distance(mh.field_of(X), T), D2)       # the model's centres are scipy's
    T2, kept, work = thickness.local_thickness(D2)
    assert np.array_equal(T2, T2ref), name
    assert (kept, work) == (kept_ref, work_ref), name
    assert int(thickness.kept_centres(D2).sum()) == kept
    check_invariants(T2, kept, work, D2, name)
    check_look(thickness.model_look(mh.field_of(X), T), X, name)


@pytest.mark.parametrize("name,X", [c for c in CASES if 'N=8' in c[0] or 'N=32' in c[0]], ids=lambda v: v if isinstance(v, str) else '')
def test_the_map_does_not_depend_on_the_rule(name, X):
    D2 = reference(name, X)[0]
    pruned, unpruned = thickness.local_thickness(D2), thickness.local_thickness(D2, prune=False)
    assert np.array_equal(pruned[0], unpruned[0]) and pruned[1:] == unpruned[1:]


def test_both_sides_and_the_full_and_empty_grids():
    N = 16
    X = np.random.default_rng(3).random((N, N)) < 0.7
    U = mh.field_of(X)
    for side, fg in (('below', X), ('above', ~X)):
        th = thickness.model_look(U, T, side)
        assert th.side == side and np.array_equal(th.t2 > 0, fg) and th.fg == int(fg.sum())
        assert np.array_equal(th.t2, brute_thickness(dh.reference(fg)[0]))
    full = thickness.model_look(mh.field_of(np.ones((N, N), dtype=bool)), T)
    assert np.all(full.t2 == INF) and (full.fg, full.ninf, full.kept, full.work, full.t2max) == (N * N, N * N, 0, 0, 0)
    assert full.hist.sum() == 0 and full.r_max is None and full.psd() is None and full.quantile(0.5) is None
    empty = thickness.model_look(mh.field_of(np.zeros((N, N), dtype=bool)), T)
    assert not empty.t2.any() and not empty.words.any() and not empty.hist.any()


def test_the_pruning_pays_on_a_smooth_field():
    """The rule of the definition keeps a small part of a smooth field's foreground (8 to 16 % in the definition's own
    check; the bound here is loose on purpose)."""
    D2 = reference(*CASES[-1])[0]
    _, kept, work = thickness.local_thickness(D2)
    assert 0 < kept < 0.25 * int((D2 > 0).sum())


# ---------------------------------------------------------------------------
# E, the default limit: no device
# ---------------------------------------------------------------------------
def test_column_reach_is_brute_reach():
    for R in list(range(1, 400)) + [1000, 4097, 9999]:
        for diagonal in (False, True):
            assert column_reach(R, diagonal) == brute_reach(R, diagonal), (R, diagonal)


def test_reach_of_the_library_and_of_the_model(hip_lib):
    rng = np.random.default_rng(11)
    Rs = list(range(1, 20000)) + [int(r) for r in rng.integers(20000, 1 << 29, 300)] + [(1 << 29), (1 << 30) - 1]
    for R in Rs:
        for diagonal in (0, 1):
            want = column_reach(R, bool(diagonal))
            assert hip_lib.chs_thickness_reach(R, diagonal) == want == thickness.reach(R, bool(diagonal)), (R, diagonal)
            assert want >= R and want >= (math.isqrt(R - 1) + 1) ** 2
    assert _lib.thickness_reach(50, True) == column_reach(50, True)
    for R in (0, -5, 1 << 30, (1 << 31) - 1):
        assert hip_lib.chs_thickness_reach(R, 0) == 0 and hip_lib.chs_thickness_reach(R, 1) == 0
    assert thickness.reach(0) == 0


def test_work_default(hip_lib):
    last = 0
    for N in (1, 2, 8, 100, 512, 4096, 8192, 16384):
        d = hip_lib.chs_thickness_work_default(N)
        assert d == _lib.thickness_work_default(N) and d >= 1024 * N * N and d > last and 16 * d < 1 << 63
        last = d
    assert hip_lib.chs_thickness_work_default(0) == 0 and hip_lib.chs_thickness_work_default(-4) == 0


# ---------------------------------------------------------------------------
# the result class
# ---------------------------------------------------------------------------
def test_thickness_object():
    N = 24
    X = smooth_noise(N, seed=2, sigma=2.0)
    U = mh.field_of(X)
    th = thickness.model_look(U, T, delx=0.5)
    assert th.N == N and th.threshold == T and th.side == 'below' and th.fg == int(X.sum()) and th.finite == th.fg
    assert th.r_max == math.sqrt(th.t2max) and th.r_max_phys == 0.5 * th.r_max
    assert th.r2_mean == th.t2.sum() / th.fg and th.r2_mean_phys == 0.25 * th.r2_mean
    k = dh.isqrt_of(th.t2[th.t2 > 0])
    assert th.r_floor_mean == k.sum() / th.fg and th.mean_thickness == 2 * th.r_floor_mean
    assert th.mean_thickness_phys == 0.5 * th.mean_thickness and th.r_floor_mean_phys == 0.5 * th.r_floor_mean
    assert th.work_per_pixel == th.work / N ** 2 and th.kept == int(thickness.kept_centres(th.distance.d2).sum())
    psd = th.psd()
    assert psd[0] == psd[1] == 1.0 and np.all(np.diff(psd) <= 0) and psd[math.isqrt(th.t2max)] > 0
    assert not psd[math.isqrt(th.t2max) + 1:].any()
    for kk in range(len(psd)):
        assert psd[kk] == (k >= kk).sum() / th.fg
    assert 1 <= th.quantile(0.0) <= th.quantile(0.5) <= th.quantile(0.9) <= th.quantile(1.0) == math.isqrt(th.t2max)
    assert th.quantile(0.5) == int(np.sort(k)[math.ceil(0.5 * th.fg) - 1])
    bare = thickness.Thickness(th.words, N, T)
    assert bare.hist is None and bare.t2 is None and bare.distance is None and bare.r_floor_mean is None
    assert bare.mean_thickness is None and bare.psd() is None and bare.r_max_phys is None and 'kept=' in repr(bare)
    # inconsistent input
    w = th.words
    with pytest.raises(ValueError):
        thickness.Thickness(w[:6], N, T)
    for at, v in ((0, N * N + 1), (4, 3), (1, 0), (2, 0), (2, th.fg + 1), (5, 0), (5, th.fg + 1), (6, th.kept - 1), (3, th.fg - 1),
                  (3, th.fg * th.t2max + 1)):
        bad = w.copy()
        bad[at] = v
        with pytest.raises(ValueError):
            thickness.Thickness(bad, N, T)
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, hist=th.hist[:-1])
    h = th.hist.copy()
    h[1] += 1
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, hist=h)
    h = th.hist.copy()
    h[math.isqrt(th.t2max) + 1] += 1
    h[1] -= 1
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, hist=h)
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, t2=th.t2[:-1])
    m = th.t2.copy()
    i, j = np.argwhere(m == 0)[0]
    m[i, j] = 1
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, t2=m)
    m = th.t2.copy()
    a, b = np.argwhere((m > 0) & (m < th.t2max))[:2]
    m[tuple(a)], m[tuple(b)] = m[tuple(a)] + 1, m[tuple(b)] - 1          # the same sum, another histogram or map
    if np.array_equal(thickness.histogram_of(m), th.hist):
        assert np.array_equal(thickness.summary_of(m, th.kept, th.work), w)
    else:
        with pytest.raises(ValueError):
            thickness.Thickness(w, N, T, hist=th.hist, t2=m)
    Y = X.copy()
    Y[tuple(np.argwhere(X)[0])] = False                                  # one foreground pixel fewer
    other = thickness.model_look(mh.field_of(Y), T).distance
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, distance=other)
    with pytest.raises(ValueError):
        thickness.Thickness(w, N, T, side='left')
    with pytest.raises(ValueError):
        th.quantile(1.5)
    with pytest.raises(ValueError):
        thickness.local_thickness(np.zeros((3, 4)))


# ---------------------------------------------------------------------------
# header, binding
# ---------------------------------------------------------------------------
TH_SYMBOLS = ['chs_thickness_work_default', 'chs_thickness_reach', 'chs_thickness', 'chs_thickness_hist', 'chs_thickness_map',
              'chs_thickness_last_ms', 'chs_batch_thickness', 'chs_batch_thickness_hist', 'chs_batch_thickness_map',
              'chs_batch_thickness_last_ms']
_CTYPES = dict(dh._CTYPES)
_CTYPES['int64_t'] = ctypes.c_int64


def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_TH_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_TH_WORDS'] == thickness.CHS_TH_WORDS == _lib.CHS_TH_WORDS == len(thickness.WORDS) == 7
    for i, w in enumerate(thickness.WORDS):
        assert defs['CHS_TH_' + w.upper()] == getattr(thickness, 'CHS_TH_' + w.upper()) == i
    assert (_lib.CHS_TH_KEPT, _lib.CHS_TH_WORK) == (thickness.CHS_TH_KEPT, thickness.CHS_TH_WORK)
    codes = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_E[A-Z]+)\s+\((-\d+)\)', hdr)}
    m = re.search(r'#define\s+CHS_ELIMIT\s+\((CHS_E[A-Z]+)\s*-\s*(\d+)\)', hdr)      # (written relative to the last literal code)
    assert m and codes[m.group(1)] - int(m.group(2)) == _lib.CHS_ELIMIT == thickness.CHS_ELIMIT == -6
    assert _lib.CHS_ELIMIT not in codes.values() and len(set(codes.values())) == len(codes)
    assert issubclass(_lib.ThicknessLimitError, _lib.EngineError)
    e = _lib.ThicknessLimitError('x', 7, 5)
    assert (e.work, e.limit) == (7, 5)


@pytest.mark.parametrize("name", TH_SYMBOLS)
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
    assert {'thickness', 'thickness_look'} <= set(batch._Member._LOOKS)
    for cls in (_lib.Engine, _lib.Batch):
        for name in ('thickness', 'thickness_look', 'thickness_hist', 'thickness_map', 'thickness_ms'):
            assert callable(getattr(cls, name))
