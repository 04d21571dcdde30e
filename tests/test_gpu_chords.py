"""GPU tests (``-m gpu``) of the chord lengths of the thresholded field on the device (chs_chords / chs_batch_chords,
chsimpy_amd/csrc/chs_chords.hip).

Reference: the numpy model ``chords.chord_histograms`` (tests/test_chords_host.py holds it against a brute-force walk) on
the phase-0 image of the field as downloaded with ``get_U`` -- the exact values the device holds, also for fp32 -- and,
for the hand-made patterns, the chords in closed form.  Everything is integer: every comparison is for equality of the 24
words and of the eight histograms.

``W, G, L`` are the pixels of a line in one word, the lines of a workgroup of the walk and the lengths below which a
chord goes to the workgroup's histogram (``_lib.chords_tile()``); the pattern sizes are the smallest at which each phase
can still go wrong."""
import math

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, chords, experiment as ex
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_chords_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
TILE = host.tile_from_source()        # (the library's own is checked against it below)
W, G, L = TILE


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, hist=True):
    words, hi = eng.chords_look(t, hist)
    return chords.Chords(words, eng.N, t, hist=hi)


def phase0_of(Ud, t):
    return np.nan_to_num(np.asarray(Ud, dtype=np.float64), nan=np.inf) < t


# ---------------------------------------------------------------------------
# 1. patterns
# ---------------------------------------------------------------------------
def test_the_tile_is_the_sources(gpu):
    assert _lib.chords_tile() == TILE
    assert host.tile_sizes(TILE) == sorted({8, W - 1, W, W + 1, 2 * W + 1, 2 * W + 2, G + 1, L + 1})


def _pattern_look(eng, check_upload=False):
    def look(U, t):
        eng.set_U(U)
        if check_upload:
            assert np.array_equal(eng.get_U() < t, U < t)
        return dev_look(eng, t)
    return look


@pytest.mark.parametrize("N", host.tile_sizes(TILE))
def test_patterns_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    look = _pattern_look(eng)
    names = []
    for name, U, want in host.patterns(N, TILE):
        host.check_pattern(look, name, U, want, N)
        names.append(name)
    assert 'checkerboard' in names and 'all-phase-0' in names and 'long-chords-along-cols' in names
    if N == L + 1:                                       # the chords that go past the workgroup's histogram
        assert 'three-words-from-bit-30-along-cols' in names and 'six-words-from-bit-10-along-rows' in names
        co = look(np.full((N, N), host.FG), T)
        assert co.hist[0, :, host.CUT, L + 1].tolist() == [N, N] and int(co.hist.sum()) == 2 * N
    for name, U, t, _ in mh.hand_made(N):               # the threshold, NaN and one-ulp fields
        host.check_look(look(U, t), phase0_of(U, t), f"{name} N={N}")
    s.close(fetch_U=False)


@pytest.mark.parametrize("N", [2 * W + 1, 2 * W + 4])
def test_patterns_on_the_device_fp32(gpu, N):
    """An odd N and a multiple of four: the mask kernel loads element by element at every N."""
    s, eng = engine_of(N, 'chirp', 'float32')
    look = _pattern_look(eng, check_upload=True)
    for name, U, want in host.patterns(N, TILE):
        host.check_pattern(look, name, U, want, N)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random fields: both parities, every engine and element type
# ---------------------------------------------------------------------------
RANDOM_CASES = [(8, 'chirp', 'float64'), (100, 'chirp', 'float32'), (129, 'chirp', 'float32'), (512, 'fast', 'float32'),
                (513, 'chirp', 'float64'), (100, 'direct', 'float64')]


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    rng = np.random.default_rng(17 * N + len(engine))
    for density in (0.3, 0.6, 0.95):
        U = mh.field_of(rng.random((N, N)) < density)
        k = max(2, N // 16)
        U[rng.integers(0, N, k), rng.integers(0, N, k)] = T     # a few pixels at the threshold: not phase 0
        eng.set_U(U)
        Ud = eng.get_U()
        assert np.array_equal(Ud == T, U == T)
        co = dev_look(eng, T)
        host.check_look(co, phase0_of(Ud, T), f"N={N} {engine} {dtype} {density}")
        assert 0 < co.n('below') < N * N
        if N >= 100:                                             # (at N = 8 every chord of a phase may lie at a wall)
            assert co.count('below', 'rows') > 0 and co.count('above', 'cols') > 0
    assert eng.chords_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field; the other looks of the same handle
# ---------------------------------------------------------------------------
def test_an_evolved_field_against_the_model_and_the_other_looks(gpu):
    """After 40 steps at N = 512 fp64 on the fast engine, thresholded at the field's median: the device equals the
    model; perimeter and area are the morphology's, the area the distance transform's foreground; the centre line of
    the largest inscribed disc is no longer than the longest chord."""
    N, steps = 512, 40
    s = tgs.solver(N, steps + 1, 'fast')
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == 'fast' and sol.computed_steps == steps + 1
    U = s._engine.get_U()
    t = float(np.median(U))
    co = s.chords(t)
    host.check_look(co, phase0_of(U, t), f"evolved N={N}")
    assert co.threshold == t and co.N == N and co.delx == sol.delx and co.hist is not None
    mo = s.morphology(t)
    assert co.perimeter('below') == mo.perimeter and co.n('below') == mo.n_A == s.distance(t).fg
    assert 0 < co.n('below') < N * N
    for phase in host.PHASES:
        di = s.distance(t, side=phase)
        assert di.fg == co.n(phase) and di.d2max >= 1
        i, j = di.argmax
        h = math.isqrt(di.d2max - 1)                     # every pixel nearer than r_max is the phase's: |offset| <= h
        for d, at in (('rows', j), ('cols', i)):
            assert min(at, h) + min(N - 1 - at, h) + 1 <= co.max_all(phase, d), (phase, d)
            if h <= at <= N - 1 - h:                     # the disc's centre line lies inside the grid
                assert 2 * di.r_max - 1 <= 2 * math.ceil(di.r_max) - 1 == 2 * h + 1 <= co.max_all(phase, d)
            assert co.mean_phys(phase, d) == co.mean(phase, d) * sol.delx
            assert 1 <= co.quantile(0.5, phase, d) <= co.quantile(0.9, phase, d) <= co.max(phase, d) <= co.max_all(phase, d)
        assert co.lineal_path(phase, 'rows')[0] == co.n(phase) / (N * N) == co.lineal_path(phase, 'cols')[0]
    bare = s.chords(t, hist=False)
    assert bare.hist is None and np.array_equal(bare.words, co.words)
    own = s.chords()                                     # params.threshold
    assert own.threshold == s.params.threshold and own.n('below') == s.morphology().n_A and own.hist is not None
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. determinism; a look changes nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_two_looks_give_the_same_bits(gpu, N, engine):
    s = tgs.solver(N, 8, engine)
    s.prepare()
    s.solve_or_resume(4)
    t = float(np.median(s._engine.get_U()))
    a, b = s.chords(t), s.chords(t)
    assert a.count('below', 'rows') > 1 and np.array_equal(a.words, b.words) and np.array_equal(a.hist, b.hist)
    s.close(fetch_U=False)


OBSERVE_CASES = [c for c in tgs.OBSERVE_CASES if c[0] <= 128 and not c[4]]     # the fast and the chirp engine


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES, ids=[f"N{c[0]}-{c[1]}" for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with chords() between them against the same calls with get_U() between them: all nine record columns, the
    state and the final field, bit for bit."""
    assert {c[1] for c in OBSERVE_CASES} == {'fast', 'chirp'}

    def look(s):
        s.chords()
        s.chords(hist=False)
    got, Ug = tgs._observed_run(N, engine, calls, look, seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert got[-1][0].shape[0] == 1 + sum(calls) - (1 if seed is None else 0)
    assert np.array_equal(Ug, Ur)


# ---------------------------------------------------------------------------
# 5. batches
# ---------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a.words, b.words) and np.array_equal(a.hist, b.hist)


@pytest.mark.parametrize("N,engine", [(256, 'fast'), (136, 'chirp')])
def test_batch_equals_the_single_solvers_and_leaves_the_members_alone(gpu, N, engine):
    B = 3
    ps = tgs._members(N, B, 100)                         # (three members with their own A0, A1 and seed)
    for m, p in enumerate(ps):
        p.threshold = p.XXX + 1e-3 * (m - 1)             # ... and their own threshold
    ts = [p.threshold for p in ps]
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    cos = bs.chords()                                    # every member at its own threshold
    assert len(cos) == B and [co.threshold for co in cos] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    for m in range(B):
        host.check_look(cos[m], phase0_of(fields[m], ts[m]), f"member {m}")
        assert _same(bs.chords(m), cos[m]), m                                   # member = m
        assert _same(bs.solvers[m].chords(), cos[m]), m                         # through the member's Solver
        assert 0 < cos[m].n('below') < N * N
    assert not np.array_equal(cos[0].words, cos[1].words)
    same = bs.chords(threshold=ts[1])                                            # one threshold for all
    for m in range(B):
        host.check_look(same[m], phase0_of(fields[m], ts[1]), f"member {m} at one threshold")
    assert _same(bs.chords(2, threshold=ts), cos[2])
    assert bs.chords(0, hist=False).hist is None
    with pytest.raises(ValueError):
        bs.chords(threshold=[0.5])
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert _same(s.chords(), cos[m]), m
        s.close(fetch_U=False)
    ref = BatchSolver(ps)                                # the members' next call without the looks
    ref.prepare()
    ref.solve_or_resume(20)
    ref.solve_or_resume(5)
    plain = tgs._batch_snap(ref)
    ref.close(fetch_U=False)
    for m in range(B):
        assert np.array_equal(looked[m][0], plain[m][0]) and np.array_equal(looked[m][1], plain[m][1]), m
        assert looked[m][2] == plain[m][2], m


# ---------------------------------------------------------------------------
# 5b. experiment
# ---------------------------------------------------------------------------
class ModelSolver:
    """What experiment._chords_of asks of a Solver, answered by the numpy model on a field."""

    def __init__(self, U, threshold):
        self.U, self.threshold = U, threshold

    def chords(self, hist=False):
        return host.model_look(self.U, self.threshold)


def test_experiment_chords_batch_equals_member_path(gpu, tmp_path, capsys):
    """`-N 136 -R 4 -n 80 --chords` one by one and with `--batch 2` write identical -chords.csv, their -results.csv is
    byte for byte that of a run without the flag, and without the flag no such file appears.  Every row is what
    experiment._chords_of gives from the numpy model on the member's exported final field (the floats are written with
    repr: the parsed values are compared exactly)."""
    base = ['-N', '136', '-R', '4', '-n', '80']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--concurrent', '1', '--chords', '--export-csv', 'U', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '2', '--chords', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    one, batch = open(tmp_path / 'one-chords.csv').read(), open(tmp_path / 'batch-chords.csv').read()
    assert one == batch
    lines = one.splitlines()
    assert lines[0] == ','.join(ex.CHORDS_COLS) and len(lines) == 5
    ints = [c in ex.MEASUREMENTS[4].int_cols for c in ex.CHORDS_COLS]
    assert ex.MEASUREMENTS[4].key == 'chords' and sum(ints) == 13
    for i, ln in enumerate(lines[1:]):
        f = ln.split(',')
        got = [int(v) if k else float(v) for v, k in zip(f, ints)]
        U = np.loadtxt(tmp_path / f'one-run{i}.solution.U.csv', delimiter=',')
        assert U.shape == (136, 136) and got[0] == i and got[1] == chsimpy_amd.Parameters().threshold
        want = (i,) + ex._chords_of(ModelSolver(U, got[1]))
        assert len(got) == len(want) == 22
        assert all(g == w or (g != g and w != w) for g, w in zip(got, want)), (i, got, want)
        assert got[2] > 0 and got[17] > 0                                        # inner chords of both phases
    assert not (tmp_path / 'plain-chords.csv').exists()
    plain = open(tmp_path / 'plain-results.csv', 'rb').read()
    assert plain == open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    N = 128
    s = tgs.solver(N, 4, 'fast')
    eng = s._get_engine()
    nb = _lib.chords_bins(N)
    assert nb == N + 1
    out = np.zeros(_lib.CHS_CH_WORDS, dtype=np.int64)
    hist = np.zeros(8 * (nb + 1) + 1, dtype=np.int64)
    ms = np.zeros(1)
    o, h = _lib._i64ptr(out), _lib._i64ptr(hist)
    assert gpu.chs_chords(eng._h, 0.5, o) == _lib.CHS_ESTATE                                 # no field yet
    for call in (lambda: gpu.chs_chords_hist(eng._h, nb, h), lambda: gpu.chs_chords_last_ms(eng._h, _lib._dptr(ms))):
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.chords()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert gpu.chs_chords(eng._h, bad, o) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_chords(eng._h, 0.5, None) == _lib.CHS_EINVAL
    assert gpu.chs_chords(None, 0.5, o) == _lib.CHS_EINVAL
    assert gpu.chs_chords_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_chords_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_chords_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE                 # none of them was a look
    assert gpu.chs_chords_hist(eng._h, nb, h) == _lib.CHS_ESTATE
    t = float(np.median(eng.get_U()))
    assert gpu.chs_chords(eng._h, t, o) == _lib.CHS_OK
    assert out[0] > 0 and gpu.chs_chords_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for bins in (nb - 1, nb + 1, 8 * nb, 0, -1):
        assert gpu.chs_chords_hist(eng._h, bins, h) == _lib.CHS_EINVAL
        assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_chords_hist(eng._h, nb, None) == _lib.CHS_EINVAL
    hist[8 * nb] = -7
    assert gpu.chs_chords_hist(eng._h, nb, h) == _lib.CHS_OK
    assert hist[8 * nb] == -7
    assert np.array_equal(chords.summary_of(hist[:8 * nb].reshape(2, 2, 2, nb)), out)
    with pytest.raises(_lib.EngineError):
        s.chords(float('nan'))
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_chords(b._h, 0, 0.5, o) == _lib.CHS_ESTATE                          # no fields yet
    assert gpu.chs_batch_chords_hist(b._h, nb, h) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, -2, 65536):
        assert gpu.chs_batch_chords(b._h, member, 0.5, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_chords(b._h, 1, float('nan'), o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_chords(b._h, 1, 0.5, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_chords(None, 1, 0.5, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_chords_hist(None, nb, h) == _lib.CHS_EINVAL
    assert gpu.chs_batch_chords_hist(b._h, nb, h) == _lib.CHS_ESTATE                         # none of them was a look
    assert gpu.chs_batch_chords(b._h, 1, 0.5, o) == _lib.CHS_OK
    assert gpu.chs_batch_chords_hist(b._h, nb + 1, h) == _lib.CHS_EINVAL
    assert f"expected {nb}" in gpu.chs_last_error().decode()
    assert gpu.chs_batch_chords_hist(b._h, nb, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_chords_hist(b._h, nb, h) == _lib.CHS_OK
    co = chords.Chords(out, 128, 0.5, hist=hist[:8 * nb].reshape(2, 2, 2, nb))
    assert co.n('below') == int((bs.solvers[1]._engine.get_U() < 0.5).sum())
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 7. the looks of one handle side by side (they share the scaffold of chs_look.h)
# ---------------------------------------------------------------------------
def _models(Ud, t):
    """What the fetches behind a look at `Ud` below `t` hold, by the numpy models."""
    from chsimpy_amd import components, distance
    D2 = distance.squared_distance(Ud, t, 'below')
    labels, table = components.label(Ud, t, 4, 'below')
    return {'chords_hist': chords.chord_histograms(Ud, t), 'distance_hist': distance.histogram_of(D2), 'distance_map': D2,
            'components_table': table, 'components_labels': labels}


def _fetches(e):
    return {k: getattr(e, k)() for k in ('chords_hist', 'distance_hist', 'distance_map', 'components_table', 'components_labels')}


def _assert_fetches(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("N,dtype", [(65, 'float64'), (68, 'float32')])
def test_the_five_looks_in_turn_do_not_disturb_each_other(gpu, N, dtype):
    """N = 65 fp64: a row is one 64-bit word and a bit, no 16-byte rows; N = 68 fp32: 16-byte loads, a partial last word.
    All five looks first, every fetch afterwards: each still holds its own look, equal to the numpy model."""
    s = tgs.solver(N, 4, 'chirp', dtype)
    s.prepare()
    eng = s._engine
    eng.set_U(mh.field_of(np.random.default_rng(N).random((N, N)) < 0.55))
    Ud = eng.get_U()
    assert eng.structure_factor().shape == (int(gpu.chs_structure_factor_bins(N)),)
    mw = eng.morphology(T)
    cw = eng.components(T, 4, _lib.CHS_CC_BELOW)
    dw = eng.distance(T, _lib.CHS_CC_BELOW)
    hw = eng.chords(T)
    want = _models(Ud, T)
    _assert_fetches(_fetches(eng), want, f"N={N} {dtype}")
    from chsimpy_amd import components, distance
    assert np.array_equal(cw, components.summary_of(want['components_table'], N))
    assert np.array_equal(dw, distance.summary_of(want['distance_map']))
    assert np.array_equal(hw, chords.summary_of(want['chords_hist']))
    assert int(mw[1:6].sum()) + int(mw[0]) == (N + 1) ** 2 and 0 < int(dw[0]) == int((Ud < T).sum()) < N * N
    for ms in (eng.morphology_ms(), eng.components_ms(), eng.distance_ms(), eng.chords_ms()):
        assert ms >= 0.0
    assert np.all(eng.structure_factor_ms() >= 0.0)
    s.close(fetch_U=False)


def test_a_rejected_look_leaves_the_last_one_in_place(gpu):
    """A call with a threshold that is not finite is refused before anything of the last look is touched: morphology,
    components, distance and chords alike go on answering for the look before it, its time included."""
    N = 65
    s = tgs.solver(N, 4, 'chirp')
    s.prepare()
    eng = s._engine
    eng.set_U(mh.field_of(np.random.default_rng(5).random((N, N)) < 0.5))
    eng.morphology(T), eng.components(T, 4, _lib.CHS_CC_BELOW), eng.distance(T, _lib.CHS_CC_BELOW), eng.chords(T)
    before = _fetches(eng)
    times = (eng.morphology_ms(), eng.components_ms(), eng.distance_ms(), eng.chords_ms())
    assert min(times) >= 0.0
    _assert_fetches(before, _models(eng.get_U(), T), 'the good looks')
    o = _lib._i64ptr(np.zeros(32, dtype=np.int64))
    for bad in (float('nan'), float('inf')):
        for rc in (gpu.chs_morphology(eng._h, bad, o), gpu.chs_components(eng._h, bad, 4, 0, o),
                   gpu.chs_distance(eng._h, bad, 0, o), gpu.chs_chords(eng._h, bad, o)):
            assert rc == _lib.CHS_EINVAL and 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_components(eng._h, float('nan'), 5, 0, o) == _lib.CHS_EINVAL      # doubly wrong: the threshold comes first
    assert 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_distance(eng._h, float('nan'), 2, o) == _lib.CHS_EINVAL
    assert 'finite' in gpu.chs_last_error().decode()
    _assert_fetches(_fetches(eng), before, 'after the rejected calls')
    assert (eng.morphology_ms(), eng.components_ms(), eng.distance_ms(), eng.chords_ms()) == times
    s.close(fetch_U=False)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_batch_buffers_hold_the_last_member_looked_at(gpu, order):
    """B = 2 at N = 128: a batch has one buffer set per kind of look; after looks at both members what is fetched is the
    second one's."""
    bs = BatchSolver(tgs._members(128, 2, 10))
    bs.prepare()
    b = bs._batch
    fields = [b.get_U(m) for m in range(2)]
    ts = [float(np.median(U)) for U in fields]
    assert not np.array_equal(fields[0] < ts[0], fields[1] < ts[1])
    for m in order:
        b.chords(m, ts[m]), b.distance(m, ts[m], _lib.CHS_CC_BELOW), b.components(m, ts[m], 4, _lib.CHS_CC_BELOW)
    last = order[-1]
    _assert_fetches(_fetches(b), _models(fields[last], ts[last]), f"member {last} after {order}")
    bs.close(fetch_U=False)
