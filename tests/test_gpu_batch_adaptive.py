"""GPU tests (``-m gpu``) of the adaptive batch: B members that all adapt their time step (solver.py:177-193), advanced
by one launch per step kernel, against the same members run one by one (``Solver`` with ``rederive_hat=True``) and
against the oracle.  The pattern and the comparison are those of test_gpu_batch.py (``assert_same``: everything bit for
bit except E and E2, which agree to 1e-14): the batched row kernel writes the same partial column sums as the single
handle's, and the batched reduction adds them up in the single handle's order.

The rule fires on every second step beyond step 500 only, so the runs are seeded at step 499 / 500
(gpu_helpers.seed_step) with ``delt_max = 4.9e-7 / N``, the value the other adaptive tests use: the step then grows
from 3e-8 by a quarter of the distance at every firing."""
import ctypes as C

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, experiment as ex
from chsimpy_amd.batch import BatchSolver
from oracle import chs_oracle as orc
from gpu_helpers import make, relerr, seed_step, log_line
from test_gpu_batch import members, snap, assert_same

pytestmark = pytest.mark.gpu

CALLS = (3, 4, 2, 5)       # a call boundary on every alignment of the firing pattern
SEEDS = (499, 500, 499)    # firing steps on opposite parities inside one launch


def adaptive_members(N, B, **kw):
    return members(N, B, 10 ** 6, adaptive_time=True, delt_max=4.9e-7 / N, **kw)


def single_runs(params_list, calls, seeds=None):
    out = []
    for m, p in enumerate(params_list):
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        if seeds is not None:
            seed_step(s, seeds[m])
        snaps = []
        for n in calls:
            s.solve_or_resume(n[m] if isinstance(n, (list, tuple)) else n)
            snaps.append(snap(s))
        s.close()
        out.append(snaps)
    return out


def batch_runs(params_list, calls, seeds=None):
    bs = BatchSolver(params_list)
    bs.prepare()
    if seeds is not None:
        for m, s in enumerate(bs.solvers):
            seed_step(s, seeds[m])
    snaps = [[] for _ in params_list]
    for n in calls:
        bs.solve_or_resume(list(n) if isinstance(n, (list, tuple)) else n)
        for m, s in enumerate(bs.solvers):
            snaps[m].append(snap(s))
    bs.close()
    return snaps


_SINGLE = {}


def seeded_reference(N):
    """The single-handle runs of the every-size case, computed once per size (two tests compare with N=128's)."""
    if N not in _SINGLE:
        _SINGLE[N] = single_runs(adaptive_members(N, 3), CALLS, SEEDS)
    return _SINGLE[N]


def assert_batch_equals(got, ref, what=''):
    for m in range(len(ref)):
        for c in range(len(ref[m])):
            assert_same(got[m][c], ref[m][c], f"{what} member {m} call {c}")


# ---------------------------------------------------------------------------
# 1. every batched size, fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', [128, 256, 512, 1024, 2048])
def test_every_size_bitwise_equal_to_single_handles(gpu, N):
    """B=3 seeded at 499 / 500 / 499, calls of (3, 4, 2, 5) steps: the five transform configurations (N=128 takes the
    integrand's sums from a sweep of U as its single handle does, the others from the fused row kernel; N=2048 adds
    them up in two passes over the columns).  Bit for bit, the delt column and the state included."""
    ps = adaptive_members(N, 3)
    got, ref = batch_runs(ps, CALLS, SEEDS), seeded_reference(N)
    assert_batch_equals(got, ref, f"N={N}")
    delts = [np.concatenate([got[m][c]['rows'][:, 8] for c in range(len(CALLS))]) for m in range(3)]
    for m in range(3):
        assert len(np.unique(delts[m])) >= 3, (m, delts[m])      # the step did adapt
    assert not np.array_equal(delts[0], delts[2])                # ... each member's in its own way
    assert not np.array_equal(delts[0], delts[1])


# ---------------------------------------------------------------------------
# 2. crossing step 500 inside a call, unseeded
# ---------------------------------------------------------------------------
def test_crossing_step_500_inside_a_call(gpu):
    ps = adaptive_members(128, 4)
    calls = (510, 12)
    got, ref = batch_runs(ps, calls), single_runs(ps, calls)
    assert_batch_equals(got, ref)
    for m in range(4):
        d = got[m][0]['rows'][:, 8]
        assert len(np.unique(d[:499])) == 1 and len(np.unique(d)) >= 3


# ---------------------------------------------------------------------------
# 3. against the oracle
# ---------------------------------------------------------------------------
def test_seeded_member_against_oracle(gpu):
    """Member 2 of a seeded N=256, B=4 batch against the oracle seeded the same way: test_b4_member_against_oracle's
    comparisons with the delt column, rtol 1e-9."""
    N = 256
    ps = adaptive_members(N, 4)
    bs = BatchSolver(ps)
    bs.prepare()
    for s in bs.solvers:
        seed_step(s, 499)
    p = ps[2]
    o = orc.OracleSolver(orc.make_params(N, 10 ** 6, func_A0=p.func_A0, func_A1=p.func_A1, adaptive_time=True,
                                         delt_max=4.9e-7 / N))
    o.prepare()
    seed_step(o, 499)
    for n in CALLS:
        sol = bs.solve_or_resume(n)[2]
        o.solve_or_resume(n)
        td, to = sol.timedata.data(), o.timedata.data()
        assert td.shape == to.shape
        assert np.array_equal(td[:, 0], to[:, 0])
        for c in (1, 2, 3, 4, 5, 6, 7, 8):
            assert np.allclose(td[:, c], to[:, c], rtol=1e-9, atol=1e-300), (n, c, relerr(td[:, c], to[:, c]))
        assert np.allclose(sol.U, o.U, rtol=1e-9, atol=0), (n, relerr(sol.U, o.U))
        assert sol.computed_steps == o.computed_steps and sol.stop_reason == o.stop_reason
        assert sol.tau0 == o.tau0 and sol.t0 == pytest.approx(o.t0, rel=1e-12)
        assert bs.solvers[2].delt == pytest.approx(o.delt, rel=1e-12)
    assert len(np.unique(to[1:, 8])) >= 4
    bs.close()


# ---------------------------------------------------------------------------
# 4. time limit under an adaptive step
# ---------------------------------------------------------------------------
def test_time_limit_stops_members_mid_call(gpu):
    """N=256, B=4, full_sim=False, time_max=0.7 min, seeded at 499, calls (3, 12): on the oracle the members end at
    computed_steps 506, 505, 509, 506, all by the time limit and all inside the second call (their steps adapt
    differently) -- each is frozen while the others go on and its field is rebuilt from hat_U."""
    ps = adaptive_members(256, 4, full_sim=False, time_max=0.7)
    calls = (3, 12, 5)
    seeds = (499,) * 4
    got, ref = batch_runs(ps, calls, seeds), single_runs(ps, calls, seeds)
    assert [got[m][1]['counters'][0] for m in range(4)] == [506, 505, 509, 506]
    assert [got[m][1]['counters'][3] for m in range(4)] == ['time-limit'] * 4
    assert_batch_equals(got, ref)
    for m in range(4):
        # a further call completes no step
        assert got[m][2]['counters'][0] == got[m][1]['counters'][0]
        assert got[m][2]['rows'].shape[0] == got[m][1]['rows'].shape[0]


# ---------------------------------------------------------------------------
# 5. sit-out and polling
# ---------------------------------------------------------------------------
def test_zero_step_member_sits_out(gpu):
    ps = adaptive_members(256, 3)
    bs = BatchSolver(ps)
    bs.prepare()
    for s in bs.solvers:
        seed_step(s, 499)
    bs.solve_or_resume(4)
    before = snap(bs.solvers[1])
    bs.solve_or_resume([6, 0, 6])
    after = snap(bs.solvers[1])
    got = [snap(s) for s in bs.solvers]
    bs.close()
    assert np.array_equal(before['U'], after['U']) and before['state'] == after['state']
    assert before['counters'] == after['counters'] and np.array_equal(before['rows'], after['rows'])
    ref = single_runs([ps[0], ps[2]], (4, 6), (499, 499))
    assert_same(got[0], ref[0][1], 'member 0')
    assert_same(got[2], ref[1][1], 'member 2')


def test_small_step_batches_give_the_same_result(gpu, monkeypatch):
    """CHS_BATCH_STEPS=2: the states are polled behind every second step; the every-size case at N=128 again."""
    monkeypatch.setenv('CHS_BATCH_STEPS', '2')
    got = batch_runs(adaptive_members(128, 3), CALLS, SEEDS)
    monkeypatch.delenv('CHS_BATCH_STEPS')
    assert_batch_equals(got, seeded_reference(128), 'CHS_BATCH_STEPS=2')


# ---------------------------------------------------------------------------
# 6. fp32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', [512, 2048])
def test_fp32_within_the_engines_own_error(gpu, N):
    """fp32, B=2, seeded at 499, 12 steps.  The batched fp32 row kernel contracts a few multiply/add pairs differently
    from the single handle's (test_gpu_batch.test_fp32_n1024), so the comparison is not bit for bit.  The bound is
    measured here: the distance of a single-handle fp32 run from the fp64 oracle (delt, E, U) is the engine's own
    fp32 error, and the batch may be 4 times that far from the single handle -- a wrong column sum shows at the 1e-2
    level of delt.  The steps and the counters are exact."""
    ps = adaptive_members(N, 2, dtype='float32')
    calls, seeds = (12,), (499, 499)
    got, ref = batch_runs(ps, calls, seeds), single_runs(ps, calls, seeds)
    # the engine's own fp32 error: member 0's single-handle run against the fp64 oracle (one oracle run: at N=2048 it
    # is what the test's time goes into; the members differ in A0 / A1 by a few per cent, not in how fp32 rounds)
    o = orc.OracleSolver(orc.make_params(N, 10 ** 6, func_A0=ps[0].func_A0, func_A1=ps[0].func_A1, adaptive_time=True,
                                         delt_max=4.9e-7 / N))
    o.prepare()
    seed_step(o, 499)
    o.solve_or_resume(12)
    to = o.timedata.data()
    quantities = lambda r: dict(delt=r['rows'][:, 8], E=r['rows'][:, 1], U=r['U'].astype(np.float64))
    s0 = quantities(ref[0][0])
    assert s0['delt'].shape == to[:, 8].shape and ref[0][0]['counters'][0] == o.computed_steps
    own = dict(delt=relerr(s0['delt'], to[:, 8]), E=relerr(s0['E'], to[:, 1]), U=relerr(s0['U'], o.U))
    for m in range(2):
        a, b = got[m][0], ref[m][0]
        assert a['rows'].shape == b['rows'].shape
        assert np.array_equal(a['rows'][:, 0], b['rows'][:, 0])
        assert a['counters'][0] == b['counters'][0] and a['counters'][3] == b['counters'][3]
        assert len(np.unique(b['rows'][1:, 8])) >= 4
        qa, qb = quantities(a), quantities(b)
        for name in ('delt', 'E', 'U'):
            dist = relerr(qa[name], qb[name])
            line = (f"batch adaptive fp32 N={N} {name}: single handle (member 0) against the fp64 oracle "
                    f"{own[name]:.3e}, batch member {m} against its single handle {dist:.3e}")
            print(line)
            log_line(line)
            assert dist <= 4 * own[name], line


# ---------------------------------------------------------------------------
# 7. C ABI
# ---------------------------------------------------------------------------
def test_create_through_the_c_abi(gpu):
    lib = _lib.load()
    p = make(256, 10, 'fast')
    lam = np.ascontiguousarray(chsimpy_amd.Solution(p).lam, dtype=np.float64)
    base = chsimpy_amd.Solver(p)._consts()

    def create(cs):
        arr = (_lib.chs_consts * len(cs))(*cs)
        h = C.c_void_p()
        rc = lib.chs_batch_create(arr, len(cs), lam.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
        if h.value:
            lib.chs_batch_destroy(h)
        return rc, lib.chs_last_error().decode()

    def adaptive(on):
        c = _lib.chs_consts.from_buffer_copy(base)
        c.adaptive_time = 1 if on else 0
        return c

    rc, msg = create([adaptive(True), adaptive(True)])
    assert rc == _lib.CHS_OK, msg
    rc, msg = create([adaptive(True), adaptive(False)])
    assert rc == _lib.CHS_EINVAL and 'adaptive' in msg and 'member 1' in msg
    rc, msg = create([adaptive(False), adaptive(False), adaptive(True)])
    assert rc == _lib.CHS_EINVAL and 'adaptive' in msg and 'member 2' in msg


# ---------------------------------------------------------------------------
# 8. ensemble
# ---------------------------------------------------------------------------
def test_run_ensemble_batch_equals_member_path(gpu, tmp_path, capsys):
    """run_ensemble(batch=4) against run_ensemble(concurrent=1): 8 adaptive members at N=128, 520 steps."""
    p = make(128, 520, 'fast', adaptive_time=True, delt_max=4.9e-7 / 128)
    p.file_id = str(tmp_path / 'e')
    ep = ex.ExperimentParams()
    ep.runs = 8
    ref = ex.run_ensemble(p, ep, concurrent=1)
    got = ex.run_ensemble(p, ep, batch=4)
    assert 'not taken' not in capsys.readouterr().out
    assert len(got) == len(ref) == 8
    for a, b in zip(got, ref):
        assert a[6] == b[6] and a[8] == b[8] and a[9] == b[9]          # tau0, itargmax, id exact
        assert np.allclose(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), rtol=1e-12, atol=0,
                           equal_nan=True), (a, b)
