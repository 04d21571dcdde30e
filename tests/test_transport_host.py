"""Host side of the transport look (chsimpy_amd/transport.py): the numpy model of the device's conjugate-gradient solve
against scipy.sparse.linalg.spsolve on the same system, closed forms for all four sources, the certificate, the consistency
checks of `Transport`, the limit path and the header's constants.  No device.

The definition (include/chs_hip.h: chs_transport).  The active pixels are those of the 4-connected components of the mask
whose bounding box touches both the source wall and the opposite one.  Two 4-adjacent active pixels share a bond of
conductance 1; an active pixel on the source wall has a bond of conductance 2 to the face at c = 1, one on the target wall a
bond of conductance 2 to the face at c = 0.  F_in = sum over the source wall of 2 (1 - c), F_out = sum over the target wall
of 2 c, cut[k] the flux through the face between depth k-1 and k.  With r = b - A c: |F_out - F*|, |F_in - F*| and |cut[k] -
F_out| are at most |r|_1.  A solve is accepted only if |r|_1 <= tol min(F_in, F_out) for the true residual.

The rounding bound `rounding(active, N)`.  r_p = b_p - (d_p c_p - sum of at most four neighbours) is at most six terms, b_p
= 2, d_p <= 6, |c| <= 1 up to the residual: their magnitudes add up to at most 12, so that r_p evaluated in any order, with
or without fused multiply-adds, is within 6 u 12 = 36 eps of the exact one (u = eps / 2).  Two evaluations of |r|_1
therefore differ by at most 72 eps ACTIVE, plus the rounding of two sums of ACTIVE non-negative terms, 2 ACTIVE u |r|_1 <=
eps ACTIVE as |r|_1 < 1 for every accepted solve here.  F_in, F_out, a cut or CSUM is a sum of at most n terms of magnitude
at most 2 (n <= N for the fluxes, n <= ACTIVE for CSUM, magnitude <= 1): any order gives it within n u 2 n <= eps n^2; two
orders differ by twice that.  Hence rounding = eps (73 ACTIVE + 2 N^2) for the fluxes and residual norms; the profile's
second column uses 2 eps N^2.  CSUM is a sum of ACTIVE terms in [0, 1] (up to the residual) taken as a tree: on the device a
value passes through at most 16 adds in its thread, 6 shuffle levels and 3 adds over the wavefronts, then at most 16 adds
over the tiles of a thread (4096 tiles at N = 4096), 6 levels and 3 adds again: 50 roundings, an error of at most 50 u
CSUM <= 25 eps ACTIVE; numpy's pairwise sum has blocks of 128 and log2(ACTIVE / 128) levels above them, at most (128 +
log2 ACTIVE) u ACTIVE.  `csum_bound(ACTIVE)` = eps ACTIVE (89 + log2 ACTIVE / 2) covers both, and CSUM is also held to the sum
of the profile's second column within that bound plus the column's own.

`patterns`, `reference_of`, `rounding` and `check_solution` are shared with tests/test_gpu_transport.py, which puts the
same masks on the device."""
import functools
import os
import re

import numpy as np
import pytest

from chsimpy_amd import _lib, batch, solver, transport
import test_geodesic_host as gh
import test_morphology_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = mh.T
SOURCES = (0, 1, 2, 3)
W = transport
EPS = float(np.finfo(np.float64).eps)


def rounding(active, N):
    return EPS * (73.0 * active + 2.0 * N * N)


def csum_bound(active):
    return EPS * active * (89.0 + 0.5 * np.log2(max(active, 1)))


# ---------------------------------------------------------------------------
# masks, all for the source 'top'; `oriented` turns them to another source
# ---------------------------------------------------------------------------
def oriented(X, source):
    """The mask X, made for the source 0, as the source `source` sees it."""
    return np.ascontiguousarray((X, X[::-1], X.T, X.T[:, ::-1])[source])


def channels(N):
    """Straight channels from wall to wall of widths 1, 2 and 3 (as far as they fit): (mask, total width)."""
    X = np.zeros((N, N), dtype=bool)
    w, j = 0, 1
    for width in (1, 2, 3):
        if j + width < N:
            X[:, j:j + width] = True
            w += width
            j += width + 2
    return X, w


def serpentine(N):
    """A one-pixel corridor of L pixels that touches the top and the bottom wall with one pixel each: full rows joined at
    alternating ends, a single pixel in the first and in the last row."""
    X = np.zeros((N, N), dtype=bool)
    first = 1 if N % 2 else 2
    X[:first, 0] = True
    right = True
    for i in range(first, N - 1, 2):
        X[i] = True
        X[i + 1, N - 1 if right else 0] = True
        right = not right
    assert X[0].sum() == 1 and X[N - 1].sum() == 1
    return X


def comb(N):
    """A one-pixel channel down column 0 with teeth: dead ends to the right in every other row, of every length."""
    X = np.zeros((N, N), dtype=bool)
    X[:, 0] = True
    for i in range(1, N - 1, 2):
        X[i, :2 + (i * 7) % (N - 2)] = True
    return X


def plate(N):
    """The full grid cut by a wall in the middle row with one gap of two pixels."""
    X = np.ones((N, N), dtype=bool)
    X[N // 2] = False
    X[N // 2, N // 3:N // 3 + 2] = True
    return X


def no_span(N):
    """Foreground on both walls and none across."""
    X = np.ones((N, N), dtype=bool)
    X[N // 2] = False
    return X


def beside(N):
    """A spanning channel (columns 0 and 1) and, beside it, a component on the top wall alone, one on the bottom wall
    alone and an island that touches nothing."""
    assert N >= 8
    X = np.zeros((N, N), dtype=bool)
    X[:, :2] = True
    X[:N // 2 - 1, 3] = True
    X[N // 2 + 1:, 3] = True
    X[N // 2 - 1:N // 2 + 1, 5:7] = True
    return X


def patterns(N):
    """[(name, mask for the source 0, F* in closed form or None)]"""
    ch, w = channels(N)
    sp = serpentine(N)
    return [('full', np.ones((N, N), dtype=bool), 1.0), ('channels', ch, w / N), ('serpentine', sp, 1.0 / int(sp.sum())),
            ('comb', comb(N), 1.0 / N), ('plate', plate(N), None), ('no span', no_span(N), 0.0), ('empty', np.zeros((N, N), dtype=bool), 0.0),
            ('beside', beside(N), 2.0 / N)]


# ---------------------------------------------------------------------------
# references, once per mask
# ---------------------------------------------------------------------------
_KEEP = {}


@functools.lru_cache(maxsize=None)
def _reference(key, source):
    X = _KEEP[key]
    S = transport.System(X, source)
    cmap, F = transport.reference(X, source)
    c = np.where(S.active, cmap, 0.0)
    res1 = float(np.abs(S.residual_of(c)).sum()) if S.active.any() else 0.0
    words = transport.stats_of(S.map_of(np.zeros(X.shape)), source, system=S)[0]
    return S, cmap, F, res1, words


def reference_of(X, source):
    """(System, the map of spsolve, its F, the 1-norm of its residual, the model's integer words) of a mask."""
    key = (X.shape[0], X.tobytes())
    _KEEP[key] = X
    return _reference(key, source)


def check_solution(X, source, cmap, words, vals, profile, what, tol=W.TOL_DEFAULT, limit=None, closed=None):
    """What a look -- the model's or the device's -- is held to (the issue: 'What a device look is held to')."""
    N = X.shape[0]
    S, ref_map, F_ref, ref_res1, ref_words = reference_of(X, source)
    u = W.UNIQUE[:-1]
    assert np.array_equal(np.asarray(words)[u], ref_words[u]), (what, words, ref_words)
    assert words[W.CHS_TRN_LIMIT] == (W.iters_default(N) if limit is None else limit), what
    assert np.array_equal(cmap == W.BACKGROUND, ~X) and np.array_equal(cmap == W.EXCLUDED, X & ~S.active), what
    active = int(S.active.sum())
    if active == 0:
        assert not np.asarray(vals).any() and not profile.any() and words[W.CHS_TRN_ITERS] == 0 and words[W.CHS_TRN_CHECKS] == 0, what
        return
    rb = rounding(active, N)
    c = np.where(S.active, cmap, 0.0)
    r = S.residual_of(c)
    res1, resinf = float(np.abs(r).sum()), float(np.abs(r).max())
    fin, fout = S.fluxes(c)
    f_in, f_out, g_res1, g_resinf, cut_min, cut_max, csum, g_tol = (float(x) for x in vals)
    assert g_tol == tol, what
    assert abs(g_res1 - res1) <= rb and abs(g_resinf - resinf) <= 72 * EPS, (what, g_res1, res1, g_resinf, resinf)
    assert abs(f_in - fin) <= rb and abs(f_out - fout) <= rb, (what, f_in, fin, f_out, fout)
    assert res1 <= tol * min(fin, fout) + rb, (what, res1, fin, fout)                       # acceptance, recomputed
    assert abs(f_out - F_ref) <= g_res1 + ref_res1 + rb, (what, f_out, F_ref, g_res1, ref_res1)   # flux
    assert abs(f_in - F_ref) <= g_res1 + ref_res1 + rb, (what, f_in, F_ref)
    cuts = profile[:, 0]
    assert cuts[0] == f_in and cuts[N] == f_out and cuts.min() == cut_min and cuts.max() == cut_max, what
    assert np.all(np.abs(cuts - f_out) <= g_res1 + rb), (what, float(np.abs(cuts - f_out).max()), g_res1)   # conservation
    _, _, p_ref = transport.stats_of(cmap, source, system=S)
    assert np.array_equal(profile[:, 2], p_ref[:, 2]) and not profile[N, 1:].any(), what
    assert np.all(np.abs(cuts - p_ref[:, 0]) <= rb), what
    assert np.all(np.abs(profile[:, 1] - p_ref[:, 1]) <= 2 * EPS * N * N), what
    assert abs(csum - float(c.sum())) <= csum_bound(active), (what, csum, float(c.sum()))
    assert abs(csum - float(profile[:, 1].sum())) <= csum_bound(active) + 2 * EPS * N * N, what
    assert 1 <= words[W.CHS_TRN_CHECKS] <= words[W.CHS_TRN_ITERS] <= words[W.CHS_TRN_LIMIT], what
    if closed is not None:
        assert abs(f_out - closed) <= g_res1 + rb and abs(f_in - closed) <= g_res1 + rb, (what, f_out, f_in, closed, g_res1)


# ---------------------------------------------------------------------------
# 1. the reference itself, and the model against it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 13, 65])
def test_closed_forms_hold_for_spsolve(N):
    for name, X, closed in patterns(N):
        if closed is None:
            continue
        for source in SOURCES:
            _, _, F, res1, _ = reference_of(oriented(X, source), source)
            assert abs(F - closed) <= 1e-13, (name, N, source, F, closed)
            assert res1 <= 1e-12


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("N", [8, 13, 65])
def test_patterns(N, source):
    names = set()
    for name, X0, closed in patterns(N):
        X = oriented(X0, source)
        cmap, words, vals, profile = transport.solve(X, source)
        check_solution(X, source, cmap, words, vals, profile, f"{name} N={N} source={source}", closed=closed)
        t = transport.Transport(words, vals, N, T, 'below', source, profile=profile, c=cmap, delx=0.5)
        assert t.percolates == (closed != 0.0) and t.source == W.SOURCE_NAMES[source]
        names.add(name)
    assert names == {'full', 'channels', 'serpentine', 'comb', 'plate', 'no span', 'empty', 'beside'}


def test_the_full_grid_and_the_properties():
    N = 13
    cmap, words, vals, profile = transport.solve(np.ones((N, N), dtype=bool), 'top')
    t = transport.Transport(words, vals, N, T, profile=profile, c=cmap, delx=0.25)
    assert abs(t.deff - 1.0) <= t.deff_bound <= 1e-6 and t.porosity == 1.0 and t.active_fraction == 1.0
    assert abs(t.tortuosity_factor - 1.0) <= 2e-6 and abs(t.formation_factor - 1.0) <= 2e-6
    assert t.conservation <= 2 * t.res1 + rounding(N * N, N) and t.conservation == t.cut_max - t.cut_min
    assert np.allclose(t.mean_c_profile(), 1.0 - (np.arange(N) + 0.5) / N, atol=1e-6)      # linear between the faces
    assert np.array_equal(t.flux_profile(), profile[:, 0]) and t.flux_profile().shape == (N + 1,)
    assert np.array_equal(t.depth_phys(), (np.arange(N) + 0.5) * 0.25) and np.array_equal(t.face_phys(), np.arange(N + 1) * 0.25)
    assert t.bonds == 2 * N * (N - 1) and t.src_pixels == t.tgt_pixels == N and t.cc_count == t.cc_spanning == 1
    assert 'deff=' in repr(t)
    with pytest.raises(ValueError):
        transport.Transport(words, vals, N, T).depth_phys()
    bare = transport.Transport(words, vals, N, T)
    with pytest.raises(ValueError):
        bare.flux_profile()
    with pytest.raises(ValueError):
        bare.mean_c_profile()


def test_the_teeth_of_the_comb_carry_no_flux():
    """c is constant along a tooth to within the bound: the difference of two neighbours of a tooth is the flux through
    the bond between them, which is the sum of the residuals of the pixels beyond it, at most |r|_1 -- over a tooth of m
    pixels at most m |r|_1 (plus the rounding of the residual's evaluation)."""
    N = 65
    X = comb(N)
    cmap, words, vals, _ = transport.solve(X, 'top')
    res1 = vals[W.CHS_TRN_RES1]
    seen = 0
    for i in range(1, N - 1, 2):
        tooth = cmap[i, :2 + (i * 7) % (N - 2)]
        assert np.all(np.abs(tooth - tooth[0]) <= tooth.size * (res1 + rounding(int(X.sum()), N))), i
        seen = max(seen, tooth.size)
    assert seen > N // 2
    spine = cmap[:, 0]                                                  # the channel: linear, as without the teeth
    assert np.allclose(spine, 1.0 - (np.arange(N) + 0.5) / N, atol=N * res1 + 1e-12)


def test_excluded_pixels():
    N = 13
    X = beside(N)
    for source in (0, 1):
        cmap, words, vals, profile = transport.solve(oriented(X, source), source)
        Xo = oriented(X, source)
        assert np.all(cmap[:, :2] >= 0) and np.all(cmap[Xo & (np.arange(N)[None, :] >= 2)] == W.EXCLUDED)
        assert np.all(cmap[~Xo] == W.BACKGROUND)
        assert words[W.CHS_TRN_FG] == X.sum() and words[W.CHS_TRN_ACTIVE] == 2 * N
        assert words[W.CHS_TRN_CC_COUNT] == 4 and words[W.CHS_TRN_CC_SPANNING] == 1
    cmap, words, vals, profile = transport.solve(X, 'left')             # nothing spans from left to right
    assert words[W.CHS_TRN_ACTIVE] == 0 and words[W.CHS_TRN_ITERS] == 0 and not vals.any() and not profile.any()
    assert np.all(cmap[X] == W.EXCLUDED) and words[W.CHS_TRN_CC_COUNT] == 4 and words[W.CHS_TRN_FG] == X.sum()
    t = transport.Transport(words, vals, N, T, source='left', profile=profile, c=cmap)
    assert not t.percolates and t.deff == 0.0 and t.formation_factor == float('inf') and t.tortuosity_factor == float('inf')
    assert t.active_fraction == 0.0


# ---------------------------------------------------------------------------
# 2. random masks, all sources; columns equal the transposed problem
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 100])
def test_random_masks(N):
    masks = gh.random_masks(N, 4)
    assert {perc for _, _, perc in masks} == {True, False}
    for seed, X, perc in masks:
        for source in SOURCES:
            cmap, words, vals, profile = transport.solve(X, source)
            check_solution(X, source, cmap, words, vals, profile, f"N={N} seed={seed} source={source}")
            if source < 2:
                assert (words[W.CHS_TRN_ACTIVE] > 0) == perc


def test_columns_equal_the_transposed_problem():
    N = 33
    _, X, _ = gh.random_masks(N, 4)[0]
    for a, b in ((2, 0), (3, 1)):
        S, Sb = transport.System(X, a), transport.System(np.ascontiguousarray(X.T), b)
        assert np.array_equal(S.active, Sb.active.T) and np.array_equal(S.degree, Sb.degree.T) and np.array_equal(S.b, Sb.b.T)
        assert S.bonds == Sb.bonds and (S.cc_count, S.cc_spanning) == (Sb.cc_count, Sb.cc_spanning)
        swap = {W.UP: W.LEFT, W.LEFT: W.UP, W.DOWN: W.RIGHT, W.RIGHT: W.DOWN, W.SRC: W.SRC, W.TGT: W.TGT, W.ACT: W.ACT}
        turned = sum(((Sb.codes.T & bit) != 0) * to for bit, to in swap.items())
        assert np.array_equal(S.codes, turned)
        ma, Fa = transport.reference(X, a)
        mb, Fb = transport.reference(np.ascontiguousarray(X.T), b)
        assert abs(Fa - Fb) <= 1e-13 and np.allclose(ma, mb.T, atol=1e-12, rtol=0)
    codes, degree, bvec = transport.system_of(X, 'top')                 # unpacks as the issue names it
    assert codes.dtype == np.uint8 and degree.shape == bvec.shape == (N, N)
    assert np.array_equal(degree[codes == 0], np.zeros(int((codes == 0).sum())))


def test_the_matrix_is_the_operator():
    N = 33
    _, X, _ = gh.random_masks(N, 4)[0]
    S = transport.System(X, 'left')
    A, b = S.matrix()
    assert abs(A - A.T).max() == 0 and np.array_equal(b, S.b[S.active])
    rng = np.random.default_rng(5)
    c = np.where(S.active, rng.random((N, N)), -7.0)                    # what lies off the active set is not read
    assert np.allclose(S.apply(c)[S.active], A @ c[S.active], atol=1e-13, rtol=0)
    assert not S.apply(c)[~S.active].any()
    assert np.array_equal(S.residual_of(c), S.b - S.apply(c))
    import scipy.sparse.linalg as sla
    assert sla.eigsh(A.asfptype(), k=1, which='SA', return_eigenvectors=False)[0] > 0      # positive definite


# ---------------------------------------------------------------------------
# 3. the certificate at loose and tight tolerances
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-2, 1e-4, 1e-9])
def test_the_certificate(tol):
    N = 33
    _, X, _ = gh.random_masks(N, 4)[0]
    for source in SOURCES:
        S, _, F, ref_res1, _ = reference_of(X, source)
        cmap, words, vals, profile = transport.solve(X, source, tol)
        check_solution(X, source, cmap, words, vals, profile, f"tol={tol} source={source}", tol=tol)
        r = S.residual_of(np.where(S.active, cmap, 0.0))
        res1 = float(np.abs(r).sum())
        rb = rounding(int(S.active.sum()), N)
        for k in range(N + 1):                                          # |cut[k] - F_out| = |sum over depth >= k of r_p|
            tail = float(r[S.depth >= k].sum())
            assert abs((profile[k, 0] - vals[W.CHS_TRN_F_OUT]) - tail) <= rb, (k, source)
            assert abs(tail) <= res1
        assert abs(vals[W.CHS_TRN_F_OUT] - F) <= res1 + ref_res1 + rb and abs(vals[W.CHS_TRN_F_IN] - F) <= res1 + ref_res1 + rb
    loose = transport.solve(X, 0, 1e-2)[1][W.CHS_TRN_ITERS]
    tight = transport.solve(X, 0, 1e-9)[1][W.CHS_TRN_ITERS]
    assert loose < tight


def test_stats_of_reads_a_map():
    N = 33
    _, X, _ = gh.random_masks(N, 4)[0]
    cmap, words, vals, profile = transport.solve(X, 'right')
    w, v, p = transport.stats_of(cmap, 'right', iters=words[W.CHS_TRN_ITERS], checks=words[W.CHS_TRN_CHECKS], tol=vals[W.CHS_TRN_TOL])
    assert np.array_equal(w, words) and np.array_equal(v, vals) and np.array_equal(p, profile)
    bad = cmap.copy()
    i, j = np.argwhere(cmap >= 0)[0]
    bad[i, j] = W.EXCLUDED
    with pytest.raises(ValueError):
        transport.stats_of(bad, 'right')
    U = mh.field_of(X)
    look = transport.model_look(U, T, 'below', 'right')
    assert np.array_equal(look.words, words) and np.array_equal(look.C, cmap)
    above = transport.model_look(mh.field_of(~X), T, 'above', 'right')
    assert np.array_equal(above.words, words) and above.side == 'above'


# ---------------------------------------------------------------------------
# 4. the limit and the arguments
# ---------------------------------------------------------------------------
def test_the_limit():
    N = 65
    X = serpentine(N)
    with pytest.raises(transport.IterationLimit) as e:
        transport.solve(X, 'top', max_iters=16)
    assert (e.value.iters, e.value.limit) == (16, 16)
    cmap, words, vals, profile = transport.solve(X, 'top')              # the default is enough
    assert 16 < words[W.CHS_TRN_ITERS] <= words[W.CHS_TRN_LIMIT] == transport.iters_default(N) == 48 * N + 64
    same = transport.solve(X, 'top', max_iters=0)                       # 0: the default
    assert np.array_equal(same[1], words) and np.array_equal(same[0], cmap)
    for bad in (-1, 16 * transport.iters_default(N) + 1):
        with pytest.raises(ValueError):
            transport.solve(X, 'top', max_iters=bad)
    for bad in (0.0, 1e-13, 0.011, float('nan'), -1e-6):
        with pytest.raises(ValueError):
            transport.solve(X, 'top', tol=bad)
    for ok in (1e-12, 1e-2):
        assert transport.check_tol(ok) == ok
    with pytest.raises(ValueError):
        transport.solve(X, 'middle')
    with pytest.raises(ValueError):
        transport.System(np.ones((3, 4), dtype=bool))
    assert issubclass(_lib.TransportLimitError, _lib.EngineError)
    err = _lib.TransportLimitError('x', 16, 16)
    assert (err.iters, err.limit) == (16, 16)


def test_transport_refuses_words_no_solve_has():
    N = 33
    _, X, _ = gh.random_masks(N, 4)[0]
    cmap, words, vals, profile = transport.solve(X, 'top')
    transport.Transport(words, vals, N, T, profile=profile, c=cmap)

    def broken(wi=None, wv=None, vi=None, vv=None, prof=profile, c=cmap):
        w, v = words.copy(), vals.copy()
        if wi is not None:
            w[wi] = wv
        if vi is not None:
            v[vi] = vv
        with pytest.raises(ValueError):
            transport.Transport(w, v, N, T, profile=prof, c=c)

    broken(W.CHS_TRN_ACTIVE, words[W.CHS_TRN_FG] + 1)
    broken(W.CHS_TRN_ACTIVE, 0)
    broken(W.CHS_TRN_CC_SPANNING, words[W.CHS_TRN_CC_COUNT] + 1)
    broken(W.CHS_TRN_SRC_PIXELS, N + 1)
    broken(W.CHS_TRN_TGT_PIXELS, 0)
    broken(W.CHS_TRN_BONDS, 2 * words[W.CHS_TRN_ACTIVE] + 1)
    broken(W.CHS_TRN_ITERS, words[W.CHS_TRN_LIMIT] + 1)
    broken(W.CHS_TRN_ITERS, 0)
    broken(W.CHS_TRN_CHECKS, words[W.CHS_TRN_ITERS] + 1)
    broken(vi=W.CHS_TRN_RES1, vv=2 * vals[W.CHS_TRN_TOL] * vals[W.CHS_TRN_F_OUT])      # not accepted
    broken(vi=W.CHS_TRN_RESINF, vv=2 * vals[W.CHS_TRN_RES1])
    broken(vi=W.CHS_TRN_F_IN, vv=-1.0)
    broken(vi=W.CHS_TRN_F_OUT, vv=float('nan'))
    broken(vi=W.CHS_TRN_CUT_MIN, vv=vals[W.CHS_TRN_CUT_MAX] + 1e-3)
    broken(vi=W.CHS_TRN_CUT_MAX, vv=vals[W.CHS_TRN_CUT_MAX] + 1.0)                       # the cuts are too far apart
    broken(vi=W.CHS_TRN_TOL, vv=0.5)
    broken(vi=W.CHS_TRN_CSUM, vv=words[W.CHS_TRN_ACTIVE] + 1.0)
    p = profile.copy(); p[N, 1] = 1.0
    broken(prof=p)
    p = profile.copy(); p[3, 2] += 1.0
    broken(prof=p)
    p = profile.copy(); p[0, 0] += 1e-9
    broken(prof=p)
    broken(prof=profile[:N])
    broken(c=cmap[:N - 1])
    with pytest.raises(ValueError):
        transport.Transport(words[:9], vals, N, T)
    with pytest.raises(ValueError):
        transport.Transport(words, vals[:7], N, T)
    zero_w = np.zeros(W.CHS_TRN_WORDS, dtype=np.int64)
    zero_w[W.CHS_TRN_LIMIT] = transport.iters_default(N)
    transport.Transport(zero_w, np.zeros(W.CHS_TRN_VALS), N, T)         # the look of an empty mask
    some = np.zeros(W.CHS_TRN_VALS); some[W.CHS_TRN_TOL] = 1e-6
    with pytest.raises(ValueError):
        transport.Transport(zero_w, some, N, T)                         # ACTIVE == 0: every value is 0


# ---------------------------------------------------------------------------
# 5. header, bindings, methods
# ---------------------------------------------------------------------------
def test_header_and_bindings():
    text = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (CHS_TRN_\w+) (\d+)', text)}
    assert defs['CHS_TRN_WORDS'] == W.CHS_TRN_WORDS == _lib.CHS_TRN_WORDS == len(W.WORDS)
    assert defs['CHS_TRN_VALS'] == W.CHS_TRN_VALS == _lib.CHS_TRN_VALS == len(W.VALS)
    for k, name in enumerate(W.WORDS):
        assert defs['CHS_TRN_' + name.upper()] == k == getattr(W, 'CHS_TRN_' + name.upper())
    for k, name in enumerate(W.VALS):
        assert defs['CHS_TRN_' + name.upper()] == k == getattr(W, 'CHS_TRN_' + name.upper())
    assert (_lib.CHS_TRN_CC_COUNT, _lib.CHS_TRN_ITERS, _lib.CHS_TRN_LIMIT) == (W.CHS_TRN_CC_COUNT, W.CHS_TRN_ITERS, W.CHS_TRN_LIMIT)
    assert re.search(r'#define CHS_TR_WORDS 25\b', text)                 # (CHS_TR_ is and stays the tracking look's prefix)
    names = ['chs_transport_iters_default', 'chs_transport', 'chs_transport_profile', 'chs_transport_map', 'chs_transport_last_ms',
             'chs_transport_solve_ms', 'chs_batch_transport', 'chs_batch_transport_profile', 'chs_batch_transport_map',
             'chs_batch_transport_last_ms', 'chs_batch_transport_solve_ms']
    for name in names:
        assert name in _lib.SYMBOLS and re.search(r'\b' + name + r'\(', text), name
    hip = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_transport.hip')).read()
    assert f'#define TRN_FACTOR {W.ITERS_FACTOR}ll' in hip and f'#define TRN_SLACK {W.ITERS_SLACK}ll' in hip
    assert f'#define TRN_MAX_FACTOR {W.MAX_FACTOR}ll' in hip
    for bit, name in ((W.UP, 'UP'), (W.DOWN, 'DOWN'), (W.LEFT, 'LEFT'), (W.RIGHT, 'RIGHT'), (W.SRC, 'SRC'), (W.TGT, 'TGT'), (W.ACT, 'ACT')):
        assert f'#define TRN_{name} {bit}u' in hip
    assert 'atomicAdd(double' not in hip and 'unsafeAtomicAdd' not in hip             # no float atomics
    for cls in (solver.Solver, batch.BatchSolver, _lib.Engine, _lib.Batch):
        assert callable(getattr(cls, 'transport'))
    assert 'transport' in batch._Member._LOOKS and 'transport_look' in batch._Member._LOOKS
    import inspect
    sig = inspect.signature(solver.Solver.transport)
    assert list(sig.parameters)[1:] == ['threshold', 'side', 'source', 'tol', 'profile', 'map', 'max_iters']
    assert sig.parameters['tol'].default == 1e-6 and sig.parameters['source'].default == 'top' and sig.parameters['map'].default is False
