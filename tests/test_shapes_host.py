"""Host side of the droplet shapes (chsimpy_amd/shapes.py): the vectorised numpy model against a reference written here
with scipy.ndimage and plain loops, hand-made fields with known answers, the invariants that tie the look to `morphology`
and `components`, the consistency checks of `Shapes`, the truncation bound of the composition, the header's constants and
prototypes.  No device.

`reference_table`, `special_field` and `serpentine` are shared with tests/test_gpu_shapes.py.  Everything in the table is an
integer: every comparison of it is for equality."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from chsimpy_amd import _lib, components, morphology, shapes
import test_components_host as cchost
import test_morphology_host as mh

ROOT = cchost.ROOT
FG, BG, T = mh.FG, mh.BG, mh.T
SIDES = ('below', 'above')
OTHER = {4: 8, 8: 4}


def fg_of(U, t, side):
    X = np.nan_to_num(np.asarray(U, dtype=np.float64), nan=np.inf) < t
    return X if side == 'below' else ~X


# ---------------------------------------------------------------------------
# the reference: scipy's labelling, scipy's sums, plain loops over the pixels
# ---------------------------------------------------------------------------
def enclosed(mask, connectivity):
    """The components of the boolean image `mask` under `connectivity` that do not reach a ring of `mask` around the grid."""
    lab, n = ndimage.label(np.pad(mask, 1, constant_values=True), structure=cchost.STRUCTURE[connectivity])
    return n - 1 if n else 0


def reference_table(U, t, connectivity, side):
    """(table int64 [C][16], holes int64 [C], labels, component table) of the field U, independent of the model:
    scipy.ndimage.label renumbered by ascending `first` (test_components_host.reference), ndimage.sum and center_of_mass
    for the area and the positional sums, loops over the pixels for the pairs, the cells, the wall and the fixed-point
    sums, and per component the enclosed components of ``labels != k`` under the other connectivity for the holes."""
    U = np.asarray(U, dtype=np.float64)
    X = fg_of(U, t, side)
    N = X.shape[0]
    labels, cctab = cchost.reference(X, connectivity)
    C = cctab.shape[0]
    tab = np.zeros((C, shapes.CHS_SH_COLS), dtype=np.int64)
    holes = np.zeros(C, dtype=np.int64)
    if C == 0:
        return tab, holes, labels, cctab
    idx = np.arange(C)
    ii, jj = np.indices((N, N))
    one = np.ones((N, N))
    area = ndimage.sum(one, labels, idx)
    com = np.array(ndimage.center_of_mass(one, labels, idx)).reshape(C, 2)
    tab[:, 0] = cctab[:, 0]
    tab[:, 1] = area
    tab[:, 8] = np.rint(com[:, 0] * area)
    tab[:, 9] = np.rint(com[:, 1] * area)
    for col, v in ((8, ii), (9, jj), (10, ii * ii), (11, jj * jj), (12, ii * jj)):
        s = ndimage.sum(v.astype(np.float64), labels, idx)
        assert np.array_equal(s, np.rint(s))
        if col in (8, 9):
            assert np.array_equal(tab[:, col], s)                  # center_of_mass and sum agree
        tab[:, col] = s
    fgp = lambda i, j: 0 <= i < N and 0 <= j < N and bool(X[i, j])
    for i in range(N):
        for j in range(N):
            k = labels[i, j]
            if k < 0:
                continue
            r = tab[k]
            r[2] += fgp(i, j + 1)
            r[3] += fgp(i + 1, j)
            r[7] += (i == 0) + (i == N - 1) + (j == 0) + (j == N - 1)
            x = float(U[i, j])
            if abs(x) <= 4.0:
                r[13] += int(x * 2.0 ** 30)
                r[14] += int((x * x) * 2.0 ** 30)
            else:
                r[15] += 1
    for i in range(N - 1):
        for j in range(N - 1):
            cell = [(i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)]
            f = [bool(X[q]) for q in cell]
            if connectivity == 8:
                if f[0] and f[3]:
                    tab[labels[cell[0]], 4] += 1
                if f[1] and f[2]:
                    tab[labels[cell[1]], 4] += 1
                if sum(f) == 3:
                    tab[labels[cell[f.index(True)]], 5] += 1
            if all(f):
                tab[labels[cell[0]], 6] += 1
    for k in range(C):
        holes[k] = enclosed(labels != k, OTHER[connectivity])
    return tab, holes, labels, cctab


def model_look(U, t, connectivity, side, delx=None):
    return shapes.look(U, t, connectivity, side, delx=delx)


def special_field(N, rng, t=T):
    """Values in (0, 1) with a few NaN, infinities, out-of-range, range-edge and threshold-equal pixels."""
    U = rng.random((N, N))
    n = max(1, N // 6)
    for v in (np.nan, np.inf, -np.inf, 5.0, -7.5, 4.0, -4.0, t, np.nextafter(4.0, 5.0)):
        U[rng.integers(0, N, n), rng.integers(0, N, n)] = v
    return U


def serpentine(N):
    """One pixel wide, through every row: even rows full, odd rows one pixel at alternating ends."""
    ii, jj = np.indices((N, N))
    return (ii % 2 == 0) | ((ii % 2 == 1) & (jj == np.where((ii // 2) % 2 == 0, N - 1, 0)))


# ---------------------------------------------------------------------------
# 1. the model against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_model_against_the_scipy_reference(seed):
    rng = np.random.default_rng(700 + seed)
    for N in (2 + seed, int(rng.integers(2, 41)), int(rng.integers(2, 41))):
        density = rng.choice([0.3, 0.5, 0.6, 0.75])
        U = special_field(N, rng) if seed % 2 else np.where(rng.random((N, N)) < density, 0.5 * rng.random((N, N)), 0.5 + 0.5 * rng.random((N, N)))
        if seed % 3 == 0:                                 # a morphologically closed field: larger droplets, real holes
            U = np.where(ndimage.binary_closing(U < T, structure=mh.EIGHT), U * 0.4, 0.6 + 0.4 * rng.random((N, N)))
        for conn in (4, 8):
            for side in SIDES:
                want, holes, labels, cctab = reference_table(U, T, conn, side)
                got = shapes.shape_table(U, T, conn, side)
                assert got.dtype == np.int64 and np.array_equal(got, want), (N, conn, side)
                assert np.array_equal(1 - shapes.euler_of(got, conn), holes), (N, conn, side)
                sh = model_look(U, T, conn, side)
                assert np.array_equal(sh.holes, holes) and sh.total_holes == int(holes.sum())
                assert np.array_equal(sh.components.table, cctab) and np.array_equal(sh.components.labels, labels)
                # the model with the labels handed in (the path of the large fields) is the same table
                assert np.array_equal(shapes.shape_table(U, T, conn, side, labels=labels), want)


# ---------------------------------------------------------------------------
# 2. hand-made fields with known answers
# ---------------------------------------------------------------------------
def disc(N, ci, cj, r):
    ii, jj = np.indices((N, N))
    return (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r


def test_a_disc():
    """A disc of radius r = 20 around a pixel centre.  It is convex and has r + r + 1 rows and columns, so its pixel
    perimeter is exactly 2 (rows + columns) = 8 r + 4.  Its pixels are those whose centres lie within r, so their union
    contains the disc of radius r - sqrt(2)/2 and lies in that of radius r + sqrt(2)/2: pi (r -+ 0.7072)^2 bounds the
    area, and with it circularity = 64 area / (pi perimeter^2) lies in ((r -+ 0.7072) / (r + 0.5))^2.  The quarter-turn
    symmetry makes mu_ii == mu_jj and mu_ij == 0: aspect 1."""
    r = 20
    sh = model_look(mh.field_of(disc(48, 24, 24, r)), T, 4, 'below')
    assert sh.count == 1 and sh.holes[0] == 0 and sh.euler[0] == 1 and not sh.touches_wall[0]
    assert sh.perimeter[0] == 8 * r + 4 == sh.perimeter_inner[0]
    lo, hi = ((r - 0.7072) / (r + 0.5)) ** 2, ((r + 0.7072) / (r + 0.5)) ** 2
    assert lo < sh.circularity[0] < hi and hi - lo < 0.14
    assert sh.circularity_pixel[0] == pytest.approx(sh.circularity[0] * (np.pi / 4) ** 2, rel=1e-15)
    assert abs(sh.aspect[0] - 1) < 0.01 and sh.eccentricity[0] < 0.15
    assert np.array_equal(sh.centroid[0], [24.0, 24.0])
    assert abs(sh.major[0] - 2 * r) < 1.0 and abs(sh.radius_eq[0] - r) < 0.7072


def test_rings_islands_and_nested_rings():
    N = 40
    ring = disc(N, 20, 20, 12) & ~disc(N, 20, 20, 8)
    island = disc(N, 20, 20, 3)
    inner_ring = disc(N, 20, 20, 6) & ~disc(N, 20, 20, 3)
    for conn in (4, 8):
        sh = model_look(mh.field_of(ring), T, conn, 'below')
        assert sh.count == 1 and sh.holes[0] == 1 and sh.euler[0] == 0 and sh.total_holes == 1
        sh = model_look(mh.field_of(ring | island), T, conn, 'below')       # the island does not fill the hole
        assert sh.count == 2 and list(sh.holes) == [1, 0] and sh.area[1] == int(island.sum())
        assert np.array_equal(sh.centroid[1], [20.0, 20.0]) and sh.nearest_neighbour()[0] < 1e-9
        sh = model_look(mh.field_of(ring | inner_ring), T, conn, 'below')   # two nested rings
        assert sh.count == 2 and list(sh.holes) == [1, 1] and sh.total_holes == 2 and sh.inner_round == 2
        above = model_look(mh.field_of(ring | inner_ring), T, conn, 'above')  # the matrix, the gap between them, the core
        assert above.count == 3 and sorted(above.holes) == [0, 1, 1]


def ellipse(N, c, a, b, angle):
    """Semi-axis a along the direction at `angle` from the x (j) axis towards increasing i, b across it."""
    ii, jj = np.indices((N, N))
    di, dj = ii - c, jj - c
    cs, sn = np.round(np.cos(angle), 15), np.round(np.sin(angle), 15)   # (exactly 0, or equal in magnitude, where they are)
    u = dj * cs + di * sn
    v = -dj * sn + di * cs
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


@pytest.mark.parametrize("angle,exact", [(0.0, 0.0), (np.pi / 2, np.pi / 2), (np.pi / 4, np.pi / 4), (-np.pi / 4, -np.pi / 4),
                                         (0.3, None)])
def test_ellipses_of_axis_ratio_two(angle, exact):
    """Semi-axes 24 and 12.  Where a mirror symmetry of the grid maps the ellipse onto itself the orientation is exact:
    mu_ij == 0 for the axis-aligned ones, mu_ii == mu_jj for the diagonal ones.  The aspect: the moments are sums over
    rows of chords that are each off by at most one pixel in at least 24, with both signs along the boundary, and the 1/12
    of the pixel is 0.2 % of the smaller moment (12^2 / 4 = 36): 3 % bounds the ratio of the two axes generously."""
    sh = model_look(mh.field_of(ellipse(64, 32, 24, 12, angle)), T, 8, 'below')
    assert sh.count == 1 and sh.holes[0] == 0
    assert abs(sh.aspect[0] / 2 - 1) < 0.03 and abs(sh.major[0] / 48 - 1) < 0.03 and abs(sh.minor[0] / 24 - 1) < 0.03
    assert abs(sh.eccentricity[0] - np.sqrt(0.75)) < 0.02
    if exact is not None:
        assert sh.orientation[0] == exact
    else:
        assert abs(sh.orientation[0] - angle) < 0.02
    assert -np.pi / 2 < sh.orientation[0] <= np.pi / 2


def test_a_diagonal_line():
    N = 9
    U = mh.field_of(np.eye(N, dtype=bool))
    sh = model_look(U, T, 8, 'below')
    assert sh.count == 1 and sh.euler[0] == 1 and sh.pairs_d[0] == sh.area[0] - 1 == N - 1
    assert sh.pairs_h[0] == sh.pairs_v[0] == sh.triples[0] == sh.quads[0] == 0 and sh.wall[0] == 4
    assert sh.orientation[0] == np.pi / 4 and sh.aspect[0] > 10
    sh = model_look(U, T, 4, 'below')
    assert sh.count == N and np.all(sh.area == 1) and np.all(sh.euler == 1) and np.all(sh.pairs_d == 0)
    anti = model_look(mh.field_of(np.eye(N, dtype=bool)[:, ::-1]), T, 8, 'below')
    assert anti.count == 1 and anti.pairs_d[0] == N - 1 and anti.orientation[0] == -np.pi / 4


@pytest.mark.parametrize("N", [2, 3, 8, 9])
def test_checkerboard_full_empty(N):
    ii, jj = np.indices((N, N))
    board = mh.field_of((ii + jj) % 2 == 0)
    half = (N * N + 1) // 2
    sh = model_look(board, T, 4, 'below')
    assert sh.count == half and np.all(sh.area == 1) and np.all(sh.perimeter == 4) and sh.total_holes == 0
    sh = model_look(board, T, 8, 'below')
    assert sh.count == 1 and sh.area[0] == half and sh.pairs_d[0] == (N - 1) ** 2 and sh.triples[0] == sh.quads[0] == 0
    assert sh.holes[0] == 1 - (half - (N - 1) ** 2)
    for conn in (4, 8):
        full = model_look(mh.field_of(np.ones((N, N), dtype=bool)), T, conn, 'below')
        assert full.count == 1 and full.area[0] == N * N and full.wall[0] == 4 * N == full.perimeter[0]
        assert full.perimeter_inner[0] == 0 and full.quads[0] == (N - 1) ** 2 and full.holes[0] == 0 and full.inner_round == 0
        assert full.pairs_h[0] == full.pairs_v[0] == N * (N - 1) and full.triples[0] == 0
        assert full.pairs_d[0] == (2 * (N - 1) ** 2 if conn == 8 else 0)
        assert full.sii[0] == N * sum(i * i for i in range(N)) and full.sij[0] == sum(range(N)) ** 2
        empty = model_look(mh.field_of(np.zeros((N, N), dtype=bool)), T, conn, 'below')
        assert empty.count == 0 and empty.table.shape == (0, 16) and empty.total_holes == 0 and empty.inner_round == 0
        assert empty.nearest_neighbour().shape == (0,) and empty.population()['count'] == 0
        assert np.array_equal(empty.words, np.array([0, 0, 0, 0, 0, 0, -1] + [0] * 10))


def test_a_droplet_in_a_corner():
    N = 12
    X = np.zeros((N, N), dtype=bool)
    X[:3, :2] = True               # the corner: three edges on row 0's side ... two columns, three rows
    X[6:8, 5:9] = True             # an inner one
    X[N - 1, 4:9] = True           # along the last row
    sh = model_look(mh.field_of(X), T, 4, 'below', delx=0.5)
    assert list(sh.wall) == [5, 0, 5] and list(sh.touches_wall) == [True, False, True] and sh.inner_round == 1
    assert list(sh.perimeter) == [10, 12, 12] and list(sh.perimeter_inner) == [5, 12, 7]
    assert np.array_equal(sh.centroid, [[1.0, 0.5], [6.5, 6.5], [N - 1.0, 6.0]])
    assert np.array_equal(sh.centroid_phys, sh.centroid * 0.5) and np.array_equal(sh.perimeter_phys, sh.perimeter * 0.5)
    assert np.array_equal(sh.major_phys, sh.major * 0.5) and np.array_equal(sh.radius_eq, np.sqrt(sh.area / np.pi) * 0.5)
    # a w x h rectangle: mu = (h^2 - 1) / 12 + 1 / 12 = h^2 / 12, so the axes are 4 sqrt(h^2 / 12) and 4 sqrt(w^2 / 12)
    assert sh.major[1] == pytest.approx(4 * np.sqrt(16 / 12), rel=1e-14) and sh.minor[1] == pytest.approx(4 * np.sqrt(4 / 12), rel=1e-14)
    assert sh.orientation[1] == 0.0 and sh.orientation[0] == np.pi / 2
    nn = sh.nearest_neighbour()
    assert nn[1] == pytest.approx(0.5 * np.hypot(4.5, 0.5)) and nn[2] == nn[1]
    pop = sh.population()
    assert pop['count'] == 1 and pop['mean_aspect'] == pytest.approx(2.0) and pop['mean_aspect_by_area'] == pytest.approx(2.0)
    assert len(pop['radius_eq']) == len(pop['mean_u']) == 1 and pop['mean_u'][0] == pytest.approx(FG, abs=2.0 ** -30)
    bare = model_look(mh.field_of(X), T, 4, 'below')
    assert bare.centroid_phys is None and bare.major_phys is None and bare.perimeter_phys is None


def test_values_outside_the_range_and_at_the_threshold():
    """NaN, +inf and 5.0 are not below the threshold: foreground of the side above, where they land in n_outside; 4.0 and
    -4.0 are inside the range; -inf and -7.5 are below every threshold and outside the range; a pixel equal to the
    threshold is background below and foreground above."""
    N = 6
    U = np.full((N, N), 0.25)
    U[0, 0], U[0, 1], U[0, 2], U[0, 3], U[0, 4] = np.nan, np.inf, 5.0, 4.0, T
    U[2, 0], U[2, 1], U[2, 2] = -4.0, -np.inf, -7.5
    U[1, :] = 0.75                                          # a background row below: row 0 is a component of `above`
    above = model_look(U, T, 4, 'above')
    assert above.count == 1 and above.area[0] == 5 + N and above.n_outside[0] == 3
    below = model_look(U, T, 4, 'below')                    # (0, 5) alone, and the rows from 2 on
    assert below.count == 2 and list(below.area) == [1, (N - 2) * N] and list(below.n_outside) == [0, 2]
    k = 1
    inside = [-4.0] + [0.25] * ((N - 2) * N - 3)
    assert below.su_fix[k] == sum(int(v * 2.0 ** 30) for v in inside)
    assert below.suu_fix[k] == sum(int(v * v * 2.0 ** 30) for v in inside)
    assert below.mean_u_of(k) == pytest.approx(np.mean(inside), abs=2.0 ** -30)
    vals = [4.0, T] + [0.75] * N
    assert above.su_fix[0] == sum(int(v * 2.0 ** 30) for v in vals) and above.n_inside[0] == len(vals)
    # a component wholly outside the range has no composition
    V = np.full((N, N), 0.75)
    V[3, 3] = -np.inf
    lone = model_look(V, T, 4, 'below')
    assert lone.count == 1 and lone.n_outside[0] == 1 and lone.mean_u_of(0) is None and lone.var_u_of(0) is None
    assert np.isnan(lone.mean_u[0]) and lone.su_fix[0] == 0


# ---------------------------------------------------------------------------
# 3. the invariants that tie the looks together
# ---------------------------------------------------------------------------
def check_invariants(sh, mo, inner_other, what=''):
    """Of a look at the side below: its perimeters and walls add up to the morphology's, its Euler numbers to euler4 or
    euler8, and its holes are the inner components of the other side under the other connectivity."""
    assert int(sh.perimeter.sum()) == mo.perimeter and int(sh.wall.sum()) == mo.border, what
    assert int(sh.perimeter_inner.sum()) == mo.perimeter_inner and int(sh.area.sum()) == mo.n_A, what
    assert int(sh.euler.sum()) == (mo.euler8 if sh.connectivity == 8 else mo.euler4), what
    assert sh.total_holes == inner_other, what


@pytest.mark.parametrize("density", [0.3, 0.5, 0.593, 0.8])
@pytest.mark.parametrize("N", [8, 33, 70])
def test_invariants_against_morphology_and_components(N, density):
    rng = np.random.default_rng(31 * N + int(1000 * density))
    U = mh.field_of(rng.random((N, N)) < density)
    mo = morphology.Morphology(morphology.quad_counts(U, T), N, T)
    for conn in (4, 8):
        sh = model_look(U, T, conn, 'below')
        other = cchost.model_look(U, T, OTHER[conn], 'above')
        check_invariants(sh, mo, other.inner, f"N={N} {density} {conn}")
        ab = model_look(U, T, conn, 'above')
        assert ab.total_holes == cchost.model_look(U, T, OTHER[conn], 'below').inner
        assert int(sh.area.sum()) + int(ab.area.sum()) == N * N
        # a pixel edge is foreground-background from either side: the inner perimeters of the two sides are one number
        assert int(sh.perimeter_inner.sum()) == int(ab.perimeter_inner.sum())


# ---------------------------------------------------------------------------
# 4. the constructor's checks
# ---------------------------------------------------------------------------
def test_the_constructor_rejects_a_table_with_one_cell_changed():
    N = 24
    X = disc(N, 8, 8, 5) | (disc(N, 16, 17, 6) & ~disc(N, 16, 17, 2))
    X[0, 20:23] = True
    sh = model_look(mh.field_of(X), T, 4, 'below')
    assert sh.count == 3 and list(sh.holes) == [0, 0, 1]
    co, words, table = sh.components, sh.words, sh.table
    C = shapes

    def bad(col, row, delta, match, fix_words=True):
        t = table.copy()
        t[row, col] += delta
        w = shapes.summary_of(t, co.words, 4) if fix_words else words
        with pytest.raises(ValueError, match=match):
            shapes.Shapes(w, t, co)

    bad(C.CHS_SH_AREA, 1, 1, 'component table')
    bad(C.CHS_SH_FIRST, 2, 1, 'component table')
    with pytest.raises(ValueError, match='rows'):
        shapes.Shapes(shapes.summary_of(table[:-1], co.words, 4), table[:-1], co)
    bad(C.CHS_SH_SI, 1, int(table[1, C.CHS_SH_AREA]) * N, 'si outside')
    bad(C.CHS_SH_SI, 1, -int(table[1, C.CHS_SH_SI]) - 1, 'si outside')
    bad(C.CHS_SH_SJ, 2, int(table[2, C.CHS_SH_AREA]) * N, 'sj outside')
    bad(C.CHS_SH_PAIRS_H, 0, int(table[0, C.CHS_SH_AREA]), 'below the area')
    bad(C.CHS_SH_PAIRS_V, 0, int(table[0, C.CHS_SH_AREA]), 'below the area')
    bad(C.CHS_SH_QUADS, 1, int(table[1, C.CHS_SH_PAIRS_H]), 'quads above')
    bad(C.CHS_SH_PAIRS_H, 1, -3, 'Euler number above 1')
    bad(C.CHS_SH_N_OUTSIDE, 2, int(table[2, C.CHS_SH_AREA]) + 1, 'n_outside above')
    bad(C.CHS_SH_WALL, 1, 1, 'column sums', fix_words=False)
    bad(C.CHS_SH_PAIRS_V, 2, -1, 'column sums', fix_words=False)
    for n in range(shapes.CHS_SH_WORDS):
        w = words.copy()
        w[n] += 1
        with pytest.raises(ValueError):
            shapes.Shapes(w, table, co)
    with pytest.raises(ValueError, match='17 words'):
        shapes.Shapes(words[:-1], table, co)
    with pytest.raises(ValueError, match='with its table'):
        shapes.Shapes(words, table, components.Components(co.words, N, T, 4, 'below'))
    with pytest.raises(ValueError):
        shapes.shape_table(mh.field_of(X), T, 4, 'below', labels=np.zeros((N, N), dtype=np.int32))
    for kw in (dict(connectivity=6), dict(side='left')):
        with pytest.raises(ValueError):
            shapes.shape_table(mh.field_of(X), T, **kw)
    assert 'Shapes(N=24' in repr(sh)


# ---------------------------------------------------------------------------
# 5. the truncation bound of the composition
# ---------------------------------------------------------------------------
def test_mean_and_variance_within_the_truncation_bound():
    """A smooth field; droplets of a few hundred pixels.  The float reference: numpy's mean and variance of the
    component's values, themselves good to n 2^-52 |x|^2 -- far below the bounds the docstring of Shapes derives,
    2^-30 for mean_u and 9 2^-30 + 2^-49 for var_u."""
    N = 64
    ii, jj = np.indices((N, N))
    U = 0.5 + 0.45 * np.sin(2 * np.pi * ii / 21.0) * np.cos(2 * np.pi * jj / 17.0) + 0.01 * np.sin(0.37 * ii * jj)
    for side in SIDES:
        sh = model_look(U, T, 4, side)
        assert sh.count >= 6 and sh.area.max() > 100 and np.all(sh.n_outside == 0)
        for k in range(sh.count):
            x = U[sh.components.labels == k]
            slack = len(x) * 2.0 ** -52
            assert abs(sh.mean_u[k] - x.mean()) <= shapes.Shapes.MEAN_U_BOUND + slack
            assert abs(sh.var_u[k] - x.var()) <= shapes.Shapes.VAR_U_BOUND + slack
        assert shapes.Shapes.MEAN_U_BOUND == 2.0 ** -30 and shapes.Shapes.VAR_U_BOUND < 10 * 2.0 ** -30
        big = int(np.argmax(sh.area))
        assert sh.var_u[big] > 1e-4                          # (the bound is small against what it bounds)
    neg = model_look(-U, -T, 4, 'below')                     # truncation is towards zero for negative values too
    for k in range(neg.count):
        x = -U[neg.components.labels == k]
        assert abs(neg.mean_u[k] - x.mean()) <= 2.0 ** -30 + len(x) * 2.0 ** -52


# ---------------------------------------------------------------------------
# 6. header and binding
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_SH_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_SH_COLS'] == shapes.CHS_SH_COLS == _lib.CHS_SH_COLS == len(shapes.COLS) == 16
    assert defs['CHS_SH_WORDS'] == shapes.CHS_SH_WORDS == _lib.CHS_SH_WORDS == len(shapes.WORDS) == 17
    for i, c in enumerate(shapes.COLS):
        assert defs['CHS_SH_' + c.upper()] == getattr(shapes, 'CHS_SH_' + c.upper()) == i
    for i, w in enumerate(shapes.WORDS[7:], start=7):
        assert defs['CHS_SH_' + w.upper()] == getattr(shapes, 'CHS_SH_' + w.upper()) == i
    assert shapes.WORDS[:7] == components.WORDS
    ct = int(re.search(r'#define\s+CHS_CT_FIX_BITS\s+(\d+)', hdr).group(1))
    assert ct == shapes.FIX_BITS == 30 and shapes.FIX == 2.0 ** 30


SH_SYMBOLS = ['chs_shapes', 'chs_shapes_table', 'chs_shapes_last_ms', 'chs_batch_shapes', 'chs_batch_shapes_table']


@pytest.mark.parametrize("name", SH_SYMBOLS)
def test_the_prototypes_match_the_header(hip_lib, name):
    cchost.test_the_prototypes_match_the_header(hip_lib, name)


def test_the_sweep_kernel_is_in_the_source_list():
    from chsimpy_amd import _build
    assert os.path.join(_build.CSRC, 'chs_shapes.hip') in _build.source_files()
