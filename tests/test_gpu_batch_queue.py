"""GPU tests (``-m gpu``) of the seat queue: ``BatchSolver(params_list, seats=S)`` -- S seats launched every step, a
member that stops or has done its call hands its seat to the next one on the device (chs_batch_step_n_queued) --
against the unqueued batch (``BatchSolver`` without seats) on the same members.

The queue launches the unqueued batch's kernels over the seats, and a seat changes hands in front of an even step only
(so that every member walks its column tiles in the order it does there), so against the unqueued batch EVERYTHING is
bit for bit, in fp64 and fp32: all nine timedata columns, U, the state tuple, the Solution counters, the stop steps
(``assert_identical``).  Against single handles the allowance of test_gpu_batch.py applies (``assert_same``: E and E2
to E2_RTOL = 1e-14, everything else bit for bit).  ``members`` / ``snap`` / ``assert_same`` are test_gpu_batch.py's,
copied."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, experiment as ex
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import KAPPA, make, relerr, seed_step

pytestmark = pytest.mark.gpu


def members(N, B, ntmax, **kw):
    """B parameter sets of one ensemble: A0/A1 factors of make_rand_values (uniform source)."""
    init = make(N, ntmax, 'fast', **kw)
    init.file_id = 'batch'
    ep = ex.ExperimentParams()
    ep.runs = B
    rv, al, n = ex.make_rand_values(ep)
    assert n == B
    return [ex.run_params(init, i, rv, al)[0] for i in range(B)]


def snap(solver):
    """Everything a call leaves behind: rows, field, device state, Solution counters."""
    sol = solver.solution
    st = solver._engine.get_state()
    return dict(rows=sol.timedata.data().copy(), U=np.array(sol.U, copy=True),
                state=(st.delt, st.time_delta_sum, st.time_passed, st.tau0, st.t0, st.computed_steps, st.skip_check,
                       st.stop_reason),
                counters=(sol.computed_steps, sol.tau0, sol.t0, sol.stop_reason))


E2_RTOL = 1e-14     # (test_gpu_batch.py: the single handle's record is compiled into another kernel)
E_COLS = (1, 2)


def assert_same(a, b, what=''):
    """A batch member against its single handle."""
    assert a['rows'].shape == b['rows'].shape, what
    other = [c for c in range(9) if c not in E_COLS]
    assert np.array_equal(a['rows'][:, other], b['rows'][:, other]), (what, relerr(a['rows'][:, 1:], b['rows'][:, 1:]))
    for c in E_COLS:
        assert np.allclose(a['rows'][:, c], b['rows'][:, c], rtol=E2_RTOL, atol=0), (what, c, relerr(a['rows'][:, c], b['rows'][:, c]))
    assert np.array_equal(a['U'], b['U']), (what, relerr(a['U'], b['U']))
    assert a['state'] == b['state'], what
    assert a['counters'] == b['counters'], what


def assert_identical(a, b, what=''):
    """A queue member against the same member of the unqueued batch: bit for bit, every column."""
    assert a['rows'].shape == b['rows'].shape, (what, a['rows'].shape, b['rows'].shape)
    assert np.array_equal(a['rows'], b['rows'], equal_nan=True), (what, [c for c in range(9) if not np.array_equal(
        a['rows'][:, c], b['rows'][:, c], equal_nan=True)])
    assert np.array_equal(a['U'], b['U'], equal_nan=True), what
    assert a['state'] == b['state'], (what, a['state'], b['state'])
    assert a['counters'] == b['counters'], (what, a['counters'], b['counters'])


def _arg(solver, steps):
    """The solve_or_resume argument that makes `steps` iterations (the first call after prepare runs one fewer)."""
    if steps is None or steps == 0:
        return steps
    return steps + (1 if solver.solution.computed_steps == 1 else 0)


def batch_runs(params_list, calls, seats=None, seeds=None):
    """One BatchSolver (a queue with `seats`), the calls in turn; calls[c] = steps per member (a list), one count for
    all, or None.  Returns snaps[m][c]."""
    bs = BatchSolver(params_list, seats=seats)
    bs.prepare()
    if seeds is not None:
        for m, s in enumerate(bs.solvers):
            seed_step(s, seeds[m])
    snaps = [[] for _ in params_list]
    for n in calls:
        per = list(n) if isinstance(n, (list, tuple)) else [n] * len(params_list)
        bs.solve_or_resume([_arg(s, k) for s, k in zip(bs.solvers, per)])
        for m, s in enumerate(bs.solvers):
            snaps[m].append(snap(s))
    bs.close()
    return snaps


def single_runs(params_list, calls):
    out = []
    for m, p in enumerate(params_list):
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        snaps = []
        for n in calls:
            k = n[m] if isinstance(n, (list, tuple)) else n
            if k != 0:      # (a member that sits a batched call out is not called at all)
                s.solve_or_resume(_arg(s, k))
            snaps.append(snap(s))
        s.close()
        out.append(snaps)
    return out


def assert_queue_equals(got, ref, what=''):
    assert len(got) == len(ref)
    for m in range(len(ref)):
        for c in range(len(ref[m])):
            assert_identical(got[m][c], ref[m][c], f"{what} member {m} call {c}")


# ---------------------------------------------------------------------------
# 1. ragged call lengths, N=128 fp64, R=7
# ---------------------------------------------------------------------------
RAGGED = ([5, 2, 9, 1, 4, 0, 3], [2, 2, 0, 3, 1, 4, 2])   # a one-step member, members that sit a call out
_RAGGED = {}


def ragged_members():
    return members(128, 7, 400)


def ragged_reference():
    """The unqueued batch on the ragged case, computed once for the tests that compare with it."""
    if 'ref' not in _RAGGED:
        _RAGGED['ref'] = batch_runs(ragged_members(), RAGGED)
    return _RAGGED['ref']


def test_ragged_call_lengths_two_seats(gpu):
    """R=7, seats=2: the members' calls end at global steps the host does not know (the last-step pair), a member does
    one step, one sits the call out.  Bit for bit the unqueued batch; against single handles test_gpu_batch's
    allowance."""
    got, ref = batch_runs(ragged_members(), RAGGED, seats=2), ragged_reference()
    assert_queue_equals(got, ref, 'seats=2')
    assert [got[m][0]['rows'].shape[0] for m in range(7)] == [1 + n for n in RAGGED[0]]
    assert [got[m][1]['rows'].shape[0] for m in range(7)] == [1 + a + b for a, b in zip(*RAGGED)]
    one = single_runs(ragged_members(), RAGGED)
    for m in range(7):
        for c in range(2):
            assert_same(got[m][c], one[m][c], f"member {m} call {c} against its single handle")
    assert not np.array_equal(got[0][1]['U'], got[1][1]['U'])   # the members are different runs


@pytest.mark.parametrize('seats', [1, 7, 16])
def test_ragged_one_seat_and_seats_for_all(gpu, seats):
    """seats=1: one member after the other; seats=7 and 16 (>= R): everybody seated from the start, as unqueued."""
    assert_queue_equals(batch_runs(ragged_members(), RAGGED, seats=seats), ragged_reference(), f"seats={seats}")


def test_two_runs_give_identical_snapshots(gpu):
    a, b = batch_runs(ragged_members(), RAGGED, seats=2), batch_runs(ragged_members(), RAGGED, seats=3)
    c = batch_runs(ragged_members(), RAGGED, seats=2)
    assert_queue_equals(a, c, 'second run')
    assert_queue_equals(a, b, 'three seats')


def test_small_poll_batches(gpu, monkeypatch):
    """CHS_BATCH_STEPS=4, calls of 10-30 steps: the polls and the row copies fall across the seat changes; the rows
    come out complete and in order."""
    calls = ([25, 12, 30, 11, 20, 0, 17], [10, 30, 0, 13, 21, 14, 12])
    ref = batch_runs(ragged_members(), calls)
    monkeypatch.setenv('CHS_BATCH_STEPS', '4')
    got = batch_runs(ragged_members(), calls, seats=2)
    got3 = batch_runs(ragged_members(), calls, seats=3)
    monkeypatch.delenv('CHS_BATCH_STEPS')
    assert_queue_equals(got, ref, 'CHS_BATCH_STEPS=4')
    assert_queue_equals(got3, ref, 'CHS_BATCH_STEPS=4, three seats')
    for m in range(7):
        steps = got[m][1]['rows'][:, 0]
        assert steps.shape[0] == 1 + calls[0][m] + calls[1][m] and np.array_equal(steps, np.arange(steps.shape[0]))


# ---------------------------------------------------------------------------
# 2. stop rules
# ---------------------------------------------------------------------------
def test_per_member_time_limits_n256(gpu):
    """N=256, R=5, seats=2, time limits as in test_per_member_time_limit_n256: members 0, 1 and 3 stop after 7, 3 and
    0 steps of the first call (9 steps; member 3's limit is below one step: it halts in its `pre_only` tail and never
    takes a seat), member 2 after 12 steps -- inside the resumed call --, member 4 never.  A stopped member's field is
    rebuilt from hat_U while its seat has long been somebody else's."""
    def limited():
        ps = members(256, 5, 300)
        step_s = ps[0].delt / ps[0].M_tilde
        for p, k in zip(ps, (7.5, 3.5, 12.5, 0.5, 1e6)):
            p.time_max = k * step_s / 60.0
        return ps
    calls = (9, 8)
    got, ref = batch_runs(limited(), calls, seats=2), batch_runs(limited(), calls)
    assert_queue_equals(got, ref)
    assert [got[m][0]['counters'][3] for m in range(5)] == ['time-limit', 'time-limit', 'None', 'time-limit', 'None']
    assert [got[m][1]['counters'][3] for m in range(5)] == ['time-limit'] * 4 + ['None']
    n0 = [got[m][0]['rows'].shape[0] for m in range(5)]
    assert n0[3] < n0[1] < n0[0] < n0[2] == n0[4] == 10, n0
    n1 = [got[m][1]['rows'].shape[0] for m in range(5)]
    assert n1[:2] == n0[:2] and n1[3] == n0[3] and n0[2] < n1[2] < n1[4] == 18, n1
    one = single_runs(limited(), calls)
    for m in range(5):
        for c in range(2):
            assert_same(got[m][c], one[m][c], f"member {m} call {c} against its single handle")


def test_per_member_energy_stop_n512(gpu):
    """The members of test_per_member_energy_stop_n512 (N=512, energy rule armed, the last one ends at ntmax 600) in
    two seats, then a resumed call."""
    def ens():
        ps = members(512, 6, 2500, full_sim=False)
        ps[5].ntmax = 600
        return ps
    calls = (None, 100)
    got, ref = batch_runs(ens(), calls, seats=2), batch_runs(ens(), calls)
    assert_queue_equals(got, ref)
    first = [got[m][0] for m in range(6)]
    stops = [f['counters'][0] for f in first if f['counters'][3] == 'energy']
    assert len(stops) >= 2 and len(set(stops)) >= 2, [f['counters'] for f in first]
    assert first[5]['counters'][3] == 'None'


# ---------------------------------------------------------------------------
# 3. fp32, adaptive
# ---------------------------------------------------------------------------
def test_fp32_n256(gpu):
    """fp32, N=256, R=5, seats=2, 40 steps: the same batched fp32 kernels, bit for bit the unqueued fp32 batch."""
    ps = lambda: members(256, 5, 100, dtype='float32')
    calls = ([40, 40, 40, 40, 40], [3, 0, 7, 2, 1])
    assert_queue_equals(batch_runs(ps(), calls, seats=2), batch_runs(ps(), calls), 'fp32')


@pytest.mark.parametrize('N, seeds', [(256, (499, 500, 499, 498)), (128, (499, 500, 499))])
def test_adaptive_members(gpu, N, seeds):
    """An adaptive queue, members seeded at steps 499 / 500 / 499 / 498, calls of 3, 4 and 5 steps, two seats: bit for
    bit the unqueued adaptive batch, `delt` included.  (N=128: the configuration without the fused adaptive row kernel,
    whose step-size sums come from a sweep of U member by member.)"""
    ps = lambda: members(N, len(seeds), 10 ** 6, adaptive_time=True, delt_max=4.9e-7 / N)
    calls = (3, 4, 5)
    got, ref = batch_runs(ps(), calls, seats=2, seeds=seeds), batch_runs(ps(), calls, seeds=seeds)
    assert_queue_equals(got, ref, f"adaptive N={N}")
    delts = [np.concatenate([got[m][c]['rows'][1:, 8] for c in range(3)]) for m in range(len(seeds))]
    assert all(len(np.unique(d)) >= 3 for d in delts), delts       # the step did adapt
    assert not np.array_equal(delts[0], delts[1])


# ---------------------------------------------------------------------------
# 4. NaN
# ---------------------------------------------------------------------------
def test_nan_member_frees_its_seat(gpu):
    """Member 1 steps from a field with one value 1.5 (test_nan_member_does_not_disturb_the_others): it alone reports
    NaN and frees its seat; the others are bit for bit what they are in the unqueued batch with the same NaN member."""
    def run(seats):
        ps = members(256, 4, 60)
        U_bad = np.full((256, 256), ps[1].XXX)
        U_bad[17, 33] = 1.5
        bs = BatchSolver(ps, seats=seats)
        bs.prepare()
        bs.solvers[1].solution.U = U_bad
        with pytest.raises(AssertionError, match='NaN'):
            bs.solve_or_resume()
        errors = list(bs.member_errors)
        status = (bs._batch.step_n([0] * 4) if seats is None else bs._batch.step_n_queued([0] * 4, seats))[1]
        snaps = [snap(s) for m, s in enumerate(bs.solvers) if m != 1]
        bs.close()
        return errors, status, snaps
    got, ref = run(2), run(None)
    assert got[0] == ref[0] == [1]
    assert got[1] == ref[1] == [_lib.CHS_OK] * 4
    for a, b in zip(got[2], ref[2]):
        assert_identical(a, b)
        assert a['rows'].shape[0] == 60 and np.all(np.isfinite(a['rows']))


def test_nan_status_and_arguments_through_the_c_abi(gpu):
    ps = members(256, 3, 10)
    U_bad = np.full((256, 256), ps[0].XXX)
    U_bad[0, 0] = 1.5
    b = _lib.Batch([chsimpy_amd.Solver(p)._consts() for p in ps], chsimpy_amd.Solution(ps[0]).lam)
    b.set_U(-1, np.full((256, 256), ps[0].XXX))
    b.prepare()
    with pytest.raises(_lib.EngineError, match='seats'):
        b.step_n_queued([5, 5, 5], 0)
    import ctypes as C
    n = (C.c_int64 * 3)(5, 5, 5)
    done, status = (C.c_int64 * 3)(), (C.c_int32 * 3)()
    assert b.lib.chs_batch_step_n_queued(b._h, 2, n, 1, done, status) == _lib.CHS_EINVAL
    assert 'flags' in b.lib.chs_last_error().decode()
    b.set_U(0, U_bad)
    rows, status = b.step_n_queued([5, 5, 5], 2)
    assert status == [_lib.CHS_ENAN, _lib.CHS_OK, _lib.CHS_OK]
    assert rows[1].shape == rows[2].shape == (5, 9) and np.all(np.isfinite(rows[1])) and np.all(np.isfinite(rows[2]))
    assert rows[0].shape[0] == 1 and np.isnan(rows[0][-1, 1:]).any()
    buf = np.empty((9, 9))
    assert b.lib.chs_batch_member_rows(b._h, 1, buf.ctypes.data_as(C.POINTER(C.c_double)), 6) == _lib.CHS_EINVAL
    assert b.lib.chs_batch_member_rows(b._h, 3, buf.ctypes.data_as(C.POINTER(C.c_double)), 1) == _lib.CHS_EINVAL
    b.close()


# ---------------------------------------------------------------------------
# 5. ensemble
# ---------------------------------------------------------------------------
def test_experiment_queue_writes_the_results_of_the_member_path(gpu, tmp_path, capsys):
    """`python -m chsimpy_amd.experiment -N 128 -R 12 --batch 4 --queue` (the module's main, in this process; energy
    stop, ntmax 3000 as in test_run_ensemble_batch_equals_member_path): its -results.csv is byte for byte that of
    `--concurrent 1`."""
    base = ['-N', '128', '-R', '12', '-n', '3000', '-K', repr(KAPPA)]
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'one')])
    ex.main(base + ['--batch', '4', '--queue', '--file-id', str(tmp_path / 'queue')])
    assert 'not taken' not in capsys.readouterr().out
    one, queue = open(tmp_path / 'one-results.csv', 'rb').read(), open(tmp_path / 'queue-results.csv', 'rb').read()
    assert len(one.splitlines()) == 13
    assert one == queue


def test_experiment_queue_measurements_equal_the_member_path(gpu, tmp_path, capsys):
    """The same ensemble with every measurement flag: `--batch 4 --queue` looks at its members behind the call, those that
    stopped early and handed their seat on included, and writes the five files the member path writes, byte for byte;
    -results.csv likewise."""
    flags = [m.flag for m in ex.MEASUREMENTS]
    assert flags == ['--domain-size', '--morphology', '--droplets', '--widths', '--chords']
    base = ['-N', '128', '-R', '12', '-n', '3000', '-K', repr(KAPPA)] + flags
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '4', '--queue', '--file-id', str(tmp_path / 'queue')])
    assert 'not taken' not in capsys.readouterr().out
    for m in ex.MEASUREMENTS:
        one = open(tmp_path / f'one-{m.suffix}.csv', 'rb').read()
        assert len(one.splitlines()) == 13 and one.splitlines()[0].decode() == ','.join(m.cols), m.key
        assert one == open(tmp_path / f'queue-{m.suffix}.csv', 'rb').read(), m.key
    one = open(tmp_path / 'one-results.csv', 'rb').read()
    assert len(one.splitlines()) == 13 and one == open(tmp_path / 'queue-results.csv', 'rb').read()
