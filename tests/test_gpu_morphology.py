"""GPU tests (``-m gpu``) of the morphology of the thresholded field computed on the device (chs_morphology /
chs_batch_morphology, chsimpy_amd/csrc/chs_morphology.hip).

Reference: ``morphology.quad_counts`` -- the numpy model that tests/test_morphology_host.py checks against a labelling
by scipy.ndimage -- of the field as downloaded with ``get_U``: the exact values the device holds, also for fp32.  The
results are integers, so every comparison is for equality of all seven words.

The kernel's tile is 128 x 512 windows of the (N+1) x (N+1) there are (MORPH_TR, MORPH_TC); the sizes below are one
below, equal to and one above both extents, in the vector and in the element-wise load path, at every engine."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, experiment as ex, morphology
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_morphology_host as host

pytestmark = pytest.mark.gpu

T = host.T


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


# ---------------------------------------------------------------------------
# 1. random two-level fields: all seven words, every load path, engine and tile edge
# ---------------------------------------------------------------------------
RANDOM_CASES = [(8, 'chirp', 'float64'), (100, 'chirp', 'float32'), (127, 'chirp', 'float64'), (128, 'fast', 'float64'),
                (129, 'chirp', 'float32'), (511, 'chirp', 'float64'), (512, 'fast', 'float32'), (513, 'chirp', 'float64'),
                (100, 'direct', 'float64'), (2049, 'chirp', 'float32'), (4096, 'fast', 'float64')]


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_two_level_fields(gpu, N, engine, dtype):
    """0.2 or 0.8 per pixel with probability 1/2, a few pixels exactly at the threshold (background)."""
    rng = np.random.default_rng(7 * N + len(engine))
    U = np.where(rng.random((N, N)) < 0.5, host.FG, host.BG)
    k = max(4, N // 16)
    U[rng.integers(0, N, k), rng.integers(0, N, k)] = T
    U[0, 0] = U[N - 1, N - 1] = U[N // 2, N - 1] = T
    s, eng = engine_of(N, engine, dtype)
    eng.set_U(U)
    got = eng.morphology(T)
    Ud = eng.get_U()
    assert np.array_equal(Ud == T, U == T)            # (0.5 survives the fp32 storage; 0.2 and 0.8 stay on their sides)
    want = morphology.quad_counts(Ud, T)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    mo = morphology.Morphology(got, N, T)
    assert mo.n_A == int((Ud < T).sum()) and 0 < mo.n_A < N * N
    # another threshold on the same handle: everything is foreground but the NaN-free field's pixels >= 0.8
    assert np.array_equal(eng.morphology(host.BG), morphology.quad_counts(Ud, host.BG))
    assert eng.morphology_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. the hand-made fields of the host test, on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 129])
def test_hand_made_fields_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    for name, U, t, want in host.hand_made(N):
        eng.set_U(U)
        got = eng.morphology(t)
        assert np.array_equal(got, morphology.quad_counts(U, t)), (name, got)
        host.check_hand_made(got, N, t, want, name)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. after a run: the area is the SA the run recorded
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_after_a_run_the_area_is_the_recorded_SA(gpu, N, engine):
    steps = 40                                         # (tests/test_gpu_spectrum.py: FIELD_CASES)
    s = tgs.solver(N, steps + 1, engine)
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == engine and sol.computed_steps == steps + 1
    mo = s.morphology()
    assert mo.threshold == s.params.threshold and mo.N == N
    n_A = round(float(sol.SA[-1]) * N * N)
    assert 0 < n_A < N * N                             # a two-phase picture at the threshold of the record
    assert mo.n_A == n_A
    assert np.array_equal(mo.words, morphology.quad_counts(sol.U, s.params.threshold))
    assert mo.interface_phys == mo.perimeter_inner * sol.delx and mo.perimeter_inner > 0
    lower = s.morphology(s.params.threshold - 1e-3)    # an explicit threshold
    assert np.array_equal(lower.words, morphology.quad_counts(sol.U, s.params.threshold - 1e-3)) and lower.n_A <= mo.n_A
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. a look changes nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp'), (4096, 'fast')])
def test_two_looks_give_the_same_words(gpu, N, engine):
    s = tgs.solver(N, 8, engine)
    s.prepare()
    a, b = s.morphology().words, s.morphology().words
    assert np.array_equal(a, b)
    s.solve_or_resume(4)
    c, d = s.morphology().words, s.morphology().words
    assert np.array_equal(c, d) and not np.array_equal(a, c)
    s.close(fetch_U=False)


@pytest.mark.parametrize("N,engine,calls,seed,kw", tgs.OBSERVE_CASES,
                         ids=[f"N{c[0]}-{c[1]}" + ('-adaptive' if c[4] else '') for c in tgs.OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with morphology() between them against the same calls with get_U() between them: all nine record columns,
    the state and the final field, bit for bit."""
    got, Ug = tgs._observed_run(N, engine, calls, lambda s: s.morphology(), seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert got[-1][0].shape[0] == 1 + sum(calls) - (1 if seed is None else 0)
    assert np.array_equal(Ug, Ur)


@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_a_look_behind_a_stopped_call(gpu, N, engine):
    """A call that the time limit ended leaves the device's halt flag set.  The look does not read it: the words are
    those of the field the call left, the state is what it was, and the resumed call gives what it gives behind a
    get_U."""
    kw = dict(time_max=30 * 3e-8 / 1.71e-8 / 60)      # (tests/test_gpu_spectrum.py: test_a_look_behind_a_stopped_call)

    def run(look):
        s = tgs.solver(N, 500, engine, **kw)
        s.prepare()
        s.solve_or_resume()
        assert s.solution.stop_reason == 'time-limit' and s.solution.computed_steps < 40
        seen = look(s)
        st = s._engine.get_state()
        state = (st.delt, st.time_delta_sum, st.time_passed, st.tau0, st.t0, st.computed_steps, st.skip_check, st.stop_reason)
        s.solve_or_resume(3)
        out = (state, s.solution.timedata.data().copy(), s._engine.get_U(), s.solution.computed_steps)
        threshold = s.params.threshold
        s.close(fetch_U=False)
        return seen, out, threshold

    mo, got, t = run(lambda s: s.morphology())
    U, ref, _ = run(lambda s: s._engine.get_U())
    assert np.array_equal(mo.words, morphology.quad_counts(U, t)) and 0 < mo.n_A < N * N
    assert got[0] == ref[0] and got[3] == ref[3]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


# ---------------------------------------------------------------------------
# 5. batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(256, 'fast'), (136, 'chirp')])
def test_batch_equals_the_single_solvers_and_leaves_the_members_alone(gpu, N, engine):
    B = 3
    ps = tgs._members(N, B, 100)                         # (three members with their own A0, A1 and seed)
    assert len({p.func_A0(p.temp) for p in ps}) == B
    for m, p in enumerate(ps):
        p.threshold = p.XXX + 1e-3 * (m - 1)             # ... and their own threshold
    ts = [p.threshold for p in ps]
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    mos = bs.morphology()                                # member = -1, every member's own threshold
    assert len(mos) == B and [mo.threshold for mo in mos] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    for m in range(B):
        assert np.array_equal(mos[m].words, morphology.quad_counts(fields[m], ts[m])), m
        assert np.array_equal(bs.morphology(m).words, mos[m].words), m               # member = m
        assert np.array_equal(bs.solvers[m].morphology().words, mos[m].words), m     # through the member's Solver
        assert 0 < mos[m].n_A < N * N
    assert not np.array_equal(mos[0].words, mos[1].words)
    same = bs.morphology(threshold=ts[1])                # one threshold for all
    assert np.array_equal(same[1].words, mos[1].words)
    assert np.array_equal(same[0].words, morphology.quad_counts(fields[0], ts[1]))
    assert np.array_equal(bs.morphology(2, threshold=ts).words, mos[2].words)
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert np.array_equal(s.morphology().words, mos[m].words), m
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
# 6. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    s = tgs.solver(128, 4, 'fast')
    eng = s._get_engine()
    out = np.zeros(_lib.CHS_MORPH_WORDS, dtype=np.int64)
    ms = np.zeros(1)
    assert gpu.chs_morphology(eng._h, 0.5, _lib._i64ptr(out)) == _lib.CHS_ESTATE            # no field yet
    assert gpu.chs_morphology_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE            # no look yet
    with pytest.raises(AssertionError):
        s.morphology()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert gpu.chs_morphology(eng._h, bad, _lib._i64ptr(out)) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    assert gpu.chs_morphology(eng._h, 0.5, None) == _lib.CHS_EINVAL
    assert gpu.chs_morphology(None, 0.5, _lib._i64ptr(out)) == _lib.CHS_EINVAL
    assert gpu.chs_morphology_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_morphology_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE            # none of them was a look
    assert gpu.chs_morphology(eng._h, 0.5, _lib._i64ptr(out)) == _lib.CHS_OK
    assert gpu.chs_morphology_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    t = np.array([0.5, 0.5])
    outs = np.zeros((2, _lib.CHS_MORPH_WORDS), dtype=np.int64)
    assert gpu.chs_batch_morphology(b._h, -1, _lib._dptr(t), _lib._i64ptr(outs)) == _lib.CHS_ESTATE   # no fields yet
    bs.prepare()
    for member in (2, -2, 65536):
        assert gpu.chs_batch_morphology(b._h, member, _lib._dptr(t), _lib._i64ptr(outs)) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_morphology(b._h, -1, None, _lib._i64ptr(outs)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_morphology(b._h, -1, _lib._dptr(np.array([0.5, np.nan])), _lib._i64ptr(outs)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_morphology(b._h, 1, _lib._dptr(np.array([np.nan])), _lib._i64ptr(outs)) == _lib.CHS_EINVAL
    assert gpu.chs_batch_morphology(b._h, -1, _lib._dptr(t), _lib._i64ptr(outs)) == _lib.CHS_OK
    assert outs[:, :6].sum(axis=1).tolist() == [129 * 129] * 2
    with pytest.raises(ValueError):
        bs.morphology(threshold=[0.5])
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 7. experiment
# ---------------------------------------------------------------------------
def test_experiment_morphology_batch_equals_member_path(gpu, tmp_path, capsys):
    """`-N 136 -R 4 --batch 2 --morphology` and the same with `--concurrent 1` write identical -morphology.csv, their
    -results.csv is byte for byte that of a run without the flag, and without the flag no such file appears."""
    base = ['-N', '136', '-R', '4', '-n', '80']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--concurrent', '1', '--morphology', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '2', '--morphology', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    one, batch = open(tmp_path / 'one-morphology.csv').read(), open(tmp_path / 'batch-morphology.csv').read()
    assert one == batch
    lines = one.splitlines()
    assert lines[0] == 'id,threshold,n_A,SA,perimeter,perimeter_inner,euler8,euler4' and len(lines) == 5
    for i, ln in enumerate(lines[1:]):
        rid, t, n_A, SA, per, per_in, e8, e4 = ln.split(',')
        assert int(rid) == i and 0 < int(n_A) < 136 * 136 and float(SA) == int(n_A) / (136 * 136)
        assert 0 < int(per_in) <= int(per) and int(e8) <= int(e4)
    assert not (tmp_path / 'plain-morphology.csv').exists()
    plain = open(tmp_path / 'plain-results.csv', 'rb').read()
    assert plain == open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()
