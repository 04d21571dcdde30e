"""GPU tests (``-m gpu``) of the composition look on the device (chs_composition / chs_composition_select and their
batch entries, chsimpy_amd/csrc/chs_composition.hip).

Reference: the numpy models of chsimpy_amd/composition.py (tests/test_composition_host.py holds them against numpy's
sort and histogram) on the field as downloaded with ``get_U`` -- the exact values the device holds, also for fp32.
Everything integer, MIN, MAX and every selected value is compared for equality; LO, HI, SCALE and CENTER are read back and
handed to the model, so that the model bins and centres with the device's own doubles; the float sums are held to

    |device - exact| <= (E + D + p + 2) 2^-53 sum |x - c|^p

(E the elements a thread adds one after the other, D the depth of the trees above it, both from
``chs_composition_tile``; p = 1 and c = 0 for SUM and SUM_BELOW), the exact sums added up in ``numpy.longdouble``.

The shapes are the smallest at which each part can go wrong: N = 8 (one partial workgroup, 16-byte loads), N = 100 on the
direct engine, N = 129 fp32 (odd: element loads), N = 513 fp64 (odd, more than one workgroup), N = 512 fp32 (16-byte loads
of four, several workgroups)."""
import os
import re

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _build, _lib, composition as cmp, morphology
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_composition_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
NAN = float('nan')
CASES = [(8, 'chirp', 'float64'), (100, 'direct', 'float64'), (129, 'chirp', 'float32'), (513, 'chirp', 'float64'),
         (512, 'fast', 'float32')]
IDS = [f"N{c[0]}-{c[1]}-{c[2]}" for c in CASES]
U53 = 2.0 ** -53


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, nbins=15, rng=None, hist=True):
    lo, hi = cmp.check_range(rng)
    iw, fw, h = eng.composition_look(t, nbins, lo, hi, hist)
    return cmp.Composition(iw, fw, eng.N, t, hist=h)


def same(a, b):
    return a == b or (a != a and b != b)


def check_look(co, Ud, t, what, rng=None, sums=True):
    """One look against the models on the field Ud the device holds."""
    N = co.N
    c, lo, hi, scale = (float(co.fw[k]) for k in (cmp.CHS_CMP_CENTER, cmp.CHS_CMP_LO, cmp.CHS_CMP_HI, cmp.CHS_CMP_SCALE))
    w = cmp.words_model(Ud, t, center=c, lo=lo, hi=hi)
    for k in ('n_total', 'n_nan', 'n_inf', 'n_below', 'n_under', 'n_over'):
        assert int(co.iw[cmp.IWORDS.index(k)]) == w[k], (what, k, int(co.iw[cmp.IWORDS.index(k)]), w[k])
    assert same(co.min, w['min']) and same(co.max, w['max']), (what, co.min, w['min'], co.max, w['max'])
    if rng is None:
        assert same(lo, co.min) and same(hi, co.max), (what, lo, hi)
    else:
        assert (lo, hi) == tuple(float(v) for v in rng), what
    assert scale == (float(np.float64(co.nbins) / (np.float64(hi) - np.float64(lo))) if hi > lo else 0.0), (what, scale)
    nfin = co.n_finite
    if nfin:
        assert c == min(max(co.sum / nfin, co.min), co.max), (what, c, co.sum, nfin)
    else:
        assert c != c and co.min != co.min and co.max != co.max and scale == 0.0, what
    if co.hist is not None:
        assert np.array_equal(co.hist, cmp.histogram_model(Ud, co.nbins, lo, hi, scale)), what
    if sums:
        E, D = _lib.composition_sum_terms(N)
        ld = np.longdouble
        for name, exact, p, total in (('sum', w['sum'], 1, w['abs1']), ('sum_below', w['sum_below'], 1, w['abs1_below']),
                                      ('m2', w['m2'], 2, w['abs2']), ('m3', w['m3'], 3, w['abs3']), ('m4', w['m4'], 4, w['abs4'])):
            got = ld(co.fw[cmp.FWORDS.index(name)])
            err, bound = abs(got - exact), ld(E + D + p + 2) * ld(U53) * total
            print(f"composition {what} {name}: |device - exact| = {float(err):.3e}, bound {float(bound):.3e} (E {E}, D {D})")
            assert err <= bound, (what, name, float(err), float(bound))
    return w


def check_select(eng, Ud, what):
    n2 = eng.N * eng.N
    eight = [0, 1, n2 // 2, n2 - 2, n2 - 1, 1, n2 // 2, 0]       # with repeats, in no order
    for ranks in ([n2 // 2], eight):
        got = eng.composition_select(ranks)
        assert np.array_equal(got, cmp.select_model(Ud, ranks), equal_nan=True), (what, ranks, got)


def hand_made_fields(N, fp32):
    """(name, U, threshold): the fields with known trouble."""
    rng = np.random.default_rng(3 * N + 1)
    ij = np.add.outer(np.arange(N), np.arange(N))
    out = [('constant', np.full((N, N), 0.3), T),
           ('checkerboard', np.where(ij % 2 == 0, 0.25, 0.9375), T)]
    out += [(name, U, t) for name, U, t, _ in mh.hand_made(N)]
    out.append(('specials', host.special_field(N, np.float32 if fp32 else np.float64).astype(np.float64), T))
    out.append(('all-distinct', rng.permutation(N * N).reshape(N, N) / float(N * N), 0.5))   # (distinct in fp32 too: N*N <= 2^24)
    return out


# ---------------------------------------------------------------------------
# 1. hand-made fields
# ---------------------------------------------------------------------------
def test_the_tile_is_the_sources(gpu):
    assert _lib.composition_tile() == host.tile_from_source()


@pytest.mark.parametrize("N,engine,dtype", CASES, ids=IDS)
def test_hand_made_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    names = []
    for name, U, t in hand_made_fields(N, dtype == 'float32'):
        eng.set_U(U)
        Ud = eng.get_U()
        what = f"{name} N={N} {engine} {dtype}"
        co = dev_look(eng, t)
        check_look(co, Ud, t, what, sums=False)
        assert co.n_below == morphology.Morphology(eng.morphology(t), N, t).n_A, what
        check_select(eng, Ud, what)
        names.append(name)
        if name == 'constant':
            c = float(Ud[0, 0])
            assert (co.min, co.max, co.lo, co.hi, co.scale) == (c, c, c, c, 0.0) and co.hist.tolist() == [N * N] + [0] * 14
            assert co.under == co.over == 0 and np.all(eng.composition_select([0, N * N - 1, 5]) == c)
        if name == 'checkerboard':
            assert sorted(co.hist[[0, 14]].tolist()) == [N * N // 2, N * N - N * N // 2] and int(co.hist[1:14].sum()) == 0
        if name == 'specials':
            assert co.n_nan == 2 and co.n_inf == 2 and (co.under, co.over) == (1, 1) and (co.min, co.max) == (-2.5, 7.0)
        if name == 'all-distinct':
            assert len(np.unique(Ud)) == N * N
            assert np.array_equal(eng.composition_select([0, 7, N * N - 1]), np.sort(Ud.ravel())[[0, 7, N * N - 1]])
    assert {'constant', 'checkerboard', 'specials', 'all-distinct'} <= set(names) and len(names) > 5
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random fields: every bin count, both kinds of range, the float sums, determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine,dtype", CASES, ids=IDS)
def test_random_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    rng = np.random.default_rng(17 * N + len(engine))
    U = rng.random((N, N)) * 1.5 - 0.25
    k = max(2, N // 16)
    U[rng.integers(0, N, k), rng.integers(0, N, k)] = T          # a few pixels at the threshold: not below
    eng.set_U(U)
    Ud = eng.get_U()
    assert np.array_equal(Ud == T, U == T)
    for nbins in (1, 15, 256, 4096):
        for given in (None, (0.125, 0.8125)):
            what = f"N={N} {engine} {dtype} nbins={nbins} range={given}"
            co = dev_look(eng, T, nbins, given)
            check_look(co, Ud, T, what, given, sums=(nbins == 15))
            assert 0 < co.n_below < N * N and co.nbins == nbins
            assert (co.under > 0 and co.over > 0) if given else (co.under == co.over == 0)
            again = dev_look(eng, T, nbins, given)               # the same look twice: the same bits
            assert again.iw.tobytes() == co.iw.tobytes() and again.fw.tobytes() == co.fw.tobytes()
            assert np.array_equal(again.hist, co.hist)
    check_select(eng, Ud, f"N={N} {engine} {dtype}")
    assert eng.composition_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. the reference's histogram
# ---------------------------------------------------------------------------
UHIST = [(8, 'chirp', 'float64'), (100, 'direct', 'float64'), (129, 'chirp', 'float32'), (513, 'chirp', 'float64')]


@pytest.mark.parametrize("N,engine,dtype", UHIST, ids=[f"N{c[0]}-{c[2]}" for c in UHIST])
def test_the_references_histogram(gpu, N, engine, dtype):
    """``bins=15, range=None`` is numpy.histogram(U, bins=15) of the field the device holds: the reference's Uhist."""
    assert [(n, np.dtype(d).name) for n, d in host.UHIST_CASES] == [(c[0], c[2]) for c in UHIST]
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype), host.start_field(N, np.float64).astype(dtype).astype(np.float64))
    s.prepare()
    assert s._engine.engine == engine
    co = s.composition(bins=15, range=None)
    Ud = s._engine.get_U()
    assert np.array_equal(co.hist, np.histogram(Ud, bins=15)[0]) and int(co.hist.sum()) == N * N
    assert np.allclose(co.edges, np.histogram(Ud, bins=15)[1], rtol=4e-16, atol=0)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    iw, fw = np.zeros(cmp.CHS_CMP_IWORDS, dtype=np.int64), np.zeros(cmp.CHS_CMP_FWORDS)
    hist = np.zeros(4097, dtype=np.int64)
    ranks, vals, ms = np.zeros(9, dtype=np.int64), np.zeros(9), np.zeros(1)
    i, f, h, r, v = _lib._i64ptr(iw), _lib._dptr(fw), _lib._i64ptr(hist), _lib._i64ptr(ranks), _lib._dptr(vals)
    assert gpu.chs_composition(eng._h, 0.5, 15, NAN, NAN, i, f) == _lib.CHS_ESTATE            # no field yet
    assert gpu.chs_composition_select(eng._h, 1, r, v) == _lib.CHS_ESTATE
    assert gpu.chs_composition_hist(eng._h, 15, h) == _lib.CHS_ESTATE                         # no look yet
    assert gpu.chs_composition_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    with pytest.raises(AssertionError):
        s.composition()
    s.prepare()
    assert gpu.chs_composition_select(eng._h, 1, r, v) == _lib.CHS_OK                         # a look of its own
    assert gpu.chs_composition_hist(eng._h, 15, h) == _lib.CHS_ESTATE                         # ... without a histogram
    assert gpu.chs_composition(eng._h, 0.875, 15, NAN, NAN, i, f) == _lib.CHS_OK
    assert gpu.chs_composition_hist(eng._h, 15, h) == _lib.CHS_OK and int(hist[:15].sum()) == N * N
    assert gpu.chs_composition_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    want, ms0 = hist[:15].copy(), float(ms[0])
    inf = float('inf')
    bad_looks = [(0.5, 0, NAN, NAN, i, f), (0.5, 4097, NAN, NAN, i, f), (0.5, -1, NAN, NAN, i, f), (0.5, 15, 0.0, NAN, i, f),
                 (0.5, 15, NAN, 1.0, i, f), (0.5, 15, 1.0, 0.0, i, f), (0.5, 15, 0.0, inf, i, f), (0.5, 15, -inf, 1.0, i, f),
                 (0.5, 15, NAN, NAN, None, f), (0.5, 15, NAN, NAN, i, None), (NAN, 15, NAN, NAN, i, f), (inf, 15, 0.0, 1.0, i, f)]
    ranks[1] = N * N
    bad_selects = [(0, r, v), (9, r, v), (-1, r, v), (2, r, v), (1, None, v), (1, r, None)]
    ranks[2] = -1

    def undisturbed():
        hist[:] = 0
        assert gpu.chs_composition_hist(eng._h, 15, h) == _lib.CHS_OK and np.array_equal(hist[:15], want)
        assert gpu.chs_composition_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and float(ms[0]) == ms0
    for args in bad_looks:
        assert gpu.chs_composition(eng._h, *args) == _lib.CHS_EINVAL, args
        assert gpu.chs_last_error().decode().startswith('chs_composition: ')
        undisturbed()
    for args in bad_selects:
        assert gpu.chs_composition_select(eng._h, *args) == _lib.CHS_EINVAL, args
        undisturbed()
    assert gpu.chs_composition_select(eng._h, 3, _lib._i64ptr(ranks[1:]), v) == _lib.CHS_EINVAL   # (N*N, -1, 0)
    assert gpu.chs_composition(None, 0.5, 15, NAN, NAN, i, f) == _lib.CHS_EINVAL
    assert gpu.chs_composition_last_ms(eng._h, None) == _lib.CHS_EINVAL
    for bins in (14, 16, 0, -1, 4096):                                                         # a wrong nbins on fetch
        assert gpu.chs_composition_hist(eng._h, bins, h) == _lib.CHS_EINVAL
        assert 'expected 15' in gpu.chs_last_error().decode()
    assert gpu.chs_composition_hist(eng._h, 15, None) == _lib.CHS_EINVAL
    undisturbed()
    # a select after the look keeps the histogram and takes the time
    ranks[0] = 5
    assert gpu.chs_composition_select(eng._h, 1, r, v) == _lib.CHS_OK
    hist[:] = 0
    assert gpu.chs_composition_hist(eng._h, 15, h) == _lib.CHS_OK and np.array_equal(hist[:15], want)
    assert vals[0] == np.sort(eng.get_U().ravel())[5]
    for call in (lambda: s.composition(bins=0), lambda: s.composition(range=(1.0, 0.0)), lambda: s.composition(quantiles=(1.5,))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.EngineError):
        s.composition(threshold=NAN)
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_composition_hist(b._h, 15, h) == _lib.CHS_ESTATE
    assert gpu.chs_batch_composition(b._h, 0, 0.5, 15, NAN, NAN, i, f) == _lib.CHS_ESTATE     # no field yet
    bs.prepare()
    for member in (-1, 2):
        assert gpu.chs_batch_composition(b._h, member, 0.5, 15, NAN, NAN, i, f) == _lib.CHS_EINVAL
        assert gpu.chs_batch_composition_select(b._h, member, 1, r, v) == _lib.CHS_EINVAL
    assert gpu.chs_batch_composition(b._h, 1, 0.875, 15, NAN, NAN, i, f) == _lib.CHS_OK
    assert gpu.chs_batch_composition_hist(b._h, 16, h) == _lib.CHS_EINVAL
    assert gpu.chs_batch_composition_hist(b._h, 15, h) == _lib.CHS_OK and int(hist[:15].sum()) == N * N
    assert gpu.chs_batch_composition_last_ms(b._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 5. the run does not notice
# ---------------------------------------------------------------------------
def _looks(s):
    co = s.composition(bins=256, quantiles=(0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 0.5))
    assert len(co.quantiles) == 7 and co.quantiles[0.0] == co.min and co.quantiles[1.0] == co.max
    s._engine.composition_select([3])
    s.composition(hist=False, quantiles=())


def test_a_look_between_calls_does_not_change_the_run(gpu):
    """N = 128 fast fp64: two calls of 20 steps with composition() and a select between them give the record rows, the
    state and the field of the two calls without them, bit for bit."""
    def run(look):
        s = tgs.solver(128, 1000, 'fast')
        s.rederive_hat = False
        s.prepare()
        s.solve_or_resume(20)
        look(s)
        s.solve_or_resume(20)
        st = s._engine.get_state()
        out = (s.solution.timedata.data().copy(), s._engine.get_U(),
               (st.delt, st.time_delta_sum, st.time_passed, st.tau0, st.t0, st.computed_steps, st.skip_check, st.stop_reason))
        s.close(fetch_U=False)
        return out
    got, ref = run(_looks), run(lambda s: None)
    assert got[0].shape == ref[0].shape == (40, 9)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]


def test_a_look_at_a_member_does_not_change_the_batch(gpu):
    def run(look):
        bs = BatchSolver(tgs._members(128, 3, 100))
        bs.prepare()
        bs.solve_or_resume(20)
        look(bs)
        bs.solve_or_resume(20)
        out = tgs._batch_snap(bs)
        bs.close(fetch_U=False)
        return out
    got, ref = run(lambda bs: _looks(bs.solvers[1])), run(lambda bs: None)
    for m in range(3):
        assert got[m][0].tobytes() == ref[m][0].tobytes() and got[m][1].tobytes() == ref[m][1].tobytes(), m
        assert got[m][2] == ref[m][2], m


# ---------------------------------------------------------------------------
# 6. batches
# ---------------------------------------------------------------------------
def _same_look(a, b):
    return (a.iw.tobytes() == b.iw.tobytes() and a.fw.tobytes() == b.fw.tobytes() and np.array_equal(a.hist, b.hist)
            and a.quantiles == b.quantiles and a.threshold == b.threshold)


@pytest.mark.parametrize("N,engine", [(100, 'chirp'), (128, 'fast')])
def test_batch_equals_the_single_solvers(gpu, N, engine):
    B = 3
    ps = tgs._members(N, B, 100)
    for m, p in enumerate(ps):
        p.engine = engine
        p.threshold = p.XXX + 1e-3 * (m - 1)
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(10)
    cos = bs.composition()
    assert len(cos) == B and [co.threshold for co in cos] == [p.threshold for p in ps]
    for m in range(B):
        Ud = bs.solvers[m]._engine.get_U()
        check_look(cos[m], Ud, ps[m].threshold, f"member {m} N={N}")
        n = N * N
        assert cos[m].quantiles == {q: float(np.sort(Ud.ravel())[cmp.quantile_rank(q, n)]) for q in (0.05, 0.5, 0.95)}
        assert _same_look(bs.composition(m), cos[m]) and _same_look(bs.solvers[m].composition(), cos[m]), m
    assert cos[0].fw.tobytes() != cos[1].fw.tobytes()
    assert bs.composition(0, hist=False).hist is None and bs.composition(2, bins=4, range=(0.0, 1.0)).nbins == 4
    assert bs._batch.composition_ms() >= 0.0
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(10)
        assert s._engine.engine == engine and _same_look(s.composition(), cos[m]), m
        s.close(fetch_U=False)


def test_experiment_composition_batch_equals_member_path(gpu, tmp_path, capsys):
    """`-N 128 -R 3 -n 40 --composition` one by one and with `--batch 2` write the same -composition.csv, every row what
    the numpy model gives on the member's exported final field, and leave -results.csv what it is without the flag."""
    from chsimpy_amd import experiment as ex
    base = ['-N', '128', '-R', '3', '-n', '40']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--concurrent', '1', '--composition', '--export-csv', 'U', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '2', '--composition', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    one = open(tmp_path / 'one-composition.csv').read()
    assert one == open(tmp_path / 'batch-composition.csv').read()
    lines = one.splitlines()
    assert lines[0] == ','.join(ex.COMPOSITION_COLS) and len(lines) == 4
    for i, ln in enumerate(lines[1:]):
        f = ln.split(',')
        U = np.loadtxt(tmp_path / f'one-run{i}.solution.U.csv', delimiter=',')
        t = float(f[1])
        assert U.shape == (128, 128) and int(f[0]) == i and t == chsimpy_amd.Parameters().threshold and int(f[2]) == 0
        srt = np.sort(U.ravel())
        assert (float(f[3]), float(f[4])) == (srt[0], srt[-1]) and float(f[7]) == np.count_nonzero(U < t) / U.size
        assert [float(v) for v in f[10:]] == [srt[cmp.quantile_rank(q, U.size)] for q in (0.05, 0.5, 0.95)]
        assert abs(float(f[5]) - U.mean()) < 1e-13 and abs(float(f[6]) - U.var()) < 1e-13
        assert float(f[8]) < t < float(f[9])
    assert not (tmp_path / 'plain-composition.csv').exists()
    plain = open(tmp_path / 'plain-results.csv', 'rb').read()
    assert plain == open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()


# ---------------------------------------------------------------------------
# 7. streamed loads
# ---------------------------------------------------------------------------
MIB = 1 << 20
ESZ = {'float64': 8, 'float32': 4}
# the smallest N that reaches each streamed instantiation: (N, element type, pixels per load)
STREAMED = [(4097, 'float64', 1), (4098, 'float64', 2), (5793, 'float32', 1), (5796, 'float32', 4)]


def cache_bound_from_source():
    """The byte count of chs_grid_exceeds_cache (chs_common.h), read from its text."""
    src = open(os.path.join(_build.CSRC, 'chs_common.h')).read()
    m = re.search(r'chs_grid_exceeds_cache\(size_t N, size_t elem_bytes\)\s*\{\s*return 2 \* N \* N \* elem_bytes > '
                  r'\(\(size_t\)(\d+) << (\d+)\);', src)
    assert m, "chs_grid_exceeds_cache is not what this module was written for"
    return int(m.group(1)) << int(m.group(2))


def test_the_sizes_lie_on_their_side_of_the_cache_bound():
    """Every streamed size is above the bound the launcher uses: these tests cannot fall back to the cached kernels."""
    bound = cache_bound_from_source()
    assert bound == 256 * MIB
    src = open(os.path.join(_build.CSRC, 'chs_composition.hip')).read()
    assert 'chs_grid_exceeds_cache((size_t)s->N, sizeof(T))' in src and 's->N % V == 0' in src
    for N, dtype, V in STREAMED:
        assert 2 * N * N * ESZ[dtype] > 256 * MIB, (N, dtype)
        n0 = N - (16 // ESZ[dtype] if V > 1 else 1)      # the size before it with this load width
        assert 2 * n0 * n0 * ESZ[dtype] <= 256 * MIB, (N, dtype)                       # (the smallest such N)
        assert (N % (16 // ESZ[dtype]) == 0) == (V > 1), (N, dtype)                    # (16-byte rows or not)
    assert 2 * 4096 * 4096 * 8 == 256 * MIB


@pytest.mark.parametrize("N,dtype,V", STREAMED, ids=[f"N{c[0]}-{c[1]}" for c in STREAMED])
def test_streamed_loads(gpu, N, dtype, V):
    s = chsimpy_amd.Solver(make(N, 2, 'auto', dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == 'direct' and 2 * N * N * ESZ[dtype] > 256 * MIB
    rng = np.random.default_rng(N)
    U = rng.random((N, N), dtype=np.float32).astype(np.float64) * 1.5 - 0.25
    U[7, N - 1] = NAN
    eng.set_U(U)
    Ud = eng.get_U()
    del U
    co = dev_look(eng, T, 256, (0.0, 1.0))
    check_look(co, Ud, T, f"streamed N={N} {dtype}", (0.0, 1.0))
    assert co.n_nan == 1 and co.under > 0 and co.over > 0 and 0 < co.n_below < N * N
    n = N * N
    ranks = [n // 20, n // 2, n - 2]                             # (rank n - 1 is the NaN)
    flat = Ud.ravel()
    assert np.array_equal(eng.composition_select(ranks), np.partition(flat, ranks)[ranks])
    assert np.isnan(eng.composition_select([n - 1])[0])
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 8. an evolved field
# ---------------------------------------------------------------------------
def test_an_evolved_field(gpu):
    """N = 512 fast fp64 after 2000 steps: SA is the record's, the phases lie on their sides of the threshold."""
    N, steps = 512, 2000
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    t = s.params.threshold
    co = s.composition()
    Ud = s._engine.get_U()
    check_look(co, Ud, t, f"evolved N={N}")
    assert co.threshold == t and co.nbins == 15 and co.n_nan == 0 and co.n_inf == 0
    assert co.SA == float(sol.timedata.data()[-1, 3]) and 0.0 < co.SA < 1.0
    assert co.mean_below < t < co.mean_above and co.min < co.mean_below and co.mean_above < co.max
    below, above = co.peaks()
    assert below is not None and above is not None and below < t <= above
    srt = np.sort(Ud.ravel())
    assert co.quantiles == {q: float(srt[cmp.quantile_rank(q, N * N)]) for q in (0.05, 0.5, 0.95)}
    assert co.quantiles[0.5] == np.quantile(Ud, 0.5, method='lower')
    assert co.var > 0 and co.kurtosis > 0 and co.SA == s.morphology().SA
    s.close(fetch_U=False)
