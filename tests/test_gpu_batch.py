"""GPU tests (``-m gpu``) of the batch: B members advanced by one launch per step kernel against the same members
run one by one (``Solver`` with ``rederive_hat=True``: every call a literal solve_or_resume, as every batched call
is), bit for bit -- the batched kernels run the single handle's kernel bodies and reduction trees (E and E2:
see E2_RTOL)."""
import ctypes as C

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, experiment as ex
from chsimpy_amd.batch import BatchSolver
from oracle import chs_oracle as orc
from gpu_helpers import make, relerr

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


def single_runs(params_list, calls, U_inits=None):
    out = []
    for m, p in enumerate(params_list):
        s = chsimpy_amd.Solver(p, None if U_inits is None else U_inits[m])
        s.rederive_hat = True
        s.prepare()
        snaps = []
        for n in calls:
            n = n[m] if isinstance(n, (list, tuple)) else n
            s.solve_or_resume(n)
            snaps.append(snap(s))
        s.close()
        out.append(snaps)
    return out


def batch_runs(params_list, calls, U_inits=None):
    bs = BatchSolver(params_list, U_inits)
    bs.prepare()
    snaps = [[] for _ in params_list]
    for n in calls:
        bs.solve_or_resume(list(n) if isinstance(n, (list, tuple)) else n)
        for m, s in enumerate(bs.solvers):
            snaps[m].append(snap(s))
    bs.close()
    return snaps


# The columns that are not bit for bit: E2 (timedata column 2), and E (column 1) which adds E2, may differ in their last
# bit in a few rows.  The single handle computes the record of most steps in the bookkeeping workgroup that rides in
# the next step's k_col, the batch in a tail kernel of its own: the same source (chs_tail.h: step_tail_body) compiled
# into different kernels, where the compiler may fuse the products of the gradient-energy sums into FMAs differently.
# Everything the run goes on from -- U, the state, the stop steps, the other columns -- is bit for bit equal.
E2_RTOL = 1e-14
E_COLS = (1, 2)


def assert_same(a, b, what=''):
    assert a['rows'].shape == b['rows'].shape, what
    other = [c for c in range(9) if c not in E_COLS]
    assert np.array_equal(a['rows'][:, other], b['rows'][:, other]), (what, relerr(a['rows'][:, 1:], b['rows'][:, 1:]))
    for c in E_COLS:
        assert np.allclose(a['rows'][:, c], b['rows'][:, c], rtol=E2_RTOL, atol=0), (what, c, relerr(a['rows'][:, c], b['rows'][:, c]))
    assert np.array_equal(a['U'], b['U']), (what, relerr(a['U'], b['U']))
    assert a['state'] == b['state'], what
    assert a['counters'] == b['counters'], what


def test_b4_n128_bitwise_equal_to_single_handles(gpu):
    """B=4 at N=128 fp64, full_sim: 300 steps in one call, then a call of 50."""
    ps = members(128, 4, 400)
    calls = (300, 50)
    got, ref = batch_runs(ps, calls), single_runs(ps, calls)
    for m in range(4):
        for c in range(len(calls)):
            assert_same(got[m][c], ref[m][c], f"member {m} call {c}")
    assert got[0][0]['rows'][-1, 1] != got[1][0]['rows'][-1, 1]   # the members are different runs


def test_b4_member_against_oracle(gpu):
    """Member 2 of the B=4 batch above against the oracle run with the same factors (gpu_helpers.compare_run's
    comparisons, rtol 1e-9)."""
    ps = members(128, 4, 300)
    bs = BatchSolver(ps)
    bs.prepare()
    sol = bs.solve_or_resume()[2]
    p = ps[2]
    o = orc.OracleSolver(orc.make_params(128, 300, func_A0=p.func_A0, func_A1=p.func_A1))
    o.prepare()
    o.solve_or_resume()
    td, to = sol.timedata.data(), o.timedata.data()
    assert td.shape == to.shape
    assert np.array_equal(td[:, 0], to[:, 0])
    for c in (1, 2, 3, 4, 5, 6, 7, 8):
        assert np.allclose(td[:, c], to[:, c], rtol=1e-9, atol=1e-300), (c, relerr(td[:, c], to[:, c]))
    assert np.allclose(sol.U, o.U, rtol=1e-9, atol=0), relerr(sol.U, o.U)
    assert sol.computed_steps == o.computed_steps and sol.stop_reason == o.stop_reason
    assert sol.tau0 == o.tau0 and sol.t0 == pytest.approx(o.t0, rel=1e-12)
    bs.close()


def test_per_member_energy_stop_n512(gpu):
    """N=512 fp64, B=6, energy rule armed: members stop at different steps, the last one (ntmax 600) not at all;
    then a resumed call."""
    ps = members(512, 6, 2500, full_sim=False)
    ps[5].ntmax = 600
    calls = (None, 100)
    got, ref = batch_runs(ps, calls), single_runs(ps, calls)
    for m in range(6):
        for c in range(len(calls)):
            assert_same(got[m][c], ref[m][c], f"member {m} call {c}")
    first = [got[m][0] for m in range(6)]
    stops = [f['counters'][0] for f in first if f['counters'][3] == 'energy']
    assert len(stops) >= 2 and len(set(stops)) >= 2, [f['counters'] for f in first]
    assert first[5]['counters'][3] == 'None'


def test_per_member_time_limit_n256(gpu):
    """N=256, B=3, three time limits, one of them never reached within the call."""
    ps = members(256, 3, 300)
    step_s = ps[0].delt / ps[0].M_tilde
    for p, k in zip(ps, (60.5, 140.5, 1e6)):
        p.time_max = k * step_s / 60.0
    calls = (300, 40)
    got, ref = batch_runs(ps, calls), single_runs(ps, calls)
    for m in range(3):
        for c in range(len(calls)):
            assert_same(got[m][c], ref[m][c], f"member {m} call {c}")
    assert [got[m][0]['counters'][3] for m in range(3)] == ['time-limit', 'time-limit', 'None']
    assert got[0][0]['rows'].shape[0] < got[1][0]['rows'].shape[0] < got[2][0]['rows'].shape[0]


def test_fp32_n1024(gpu):
    """fp32, N=1024, B=3, 200 steps.  Not bit for bit: in the batched instantiation of the fused fp32 row kernel the
    compiler contracts a few more multiply/subtract pairs into packed FMAs (118 against 112 v_pk_fma_f32 -- the source
    is the same), so the members part from their single runs at fp32 rounding from the second step on.  Checked: the
    first step bit for bit, then the whole run to fp32 accuracy, the time bookkeeping exactly."""
    ps = members(1024, 3, 200, dtype='float32')
    one_b, one_s = batch_runs(ps, (2,)), single_runs(ps, (2,))
    for m in range(3):
        assert_same(one_b[m][0], one_s[m][0], f"member {m}, one step")
    got, ref = batch_runs(ps, (200,)), single_runs(ps, (200,))
    for m in range(3):
        a, b = got[m][0], ref[m][0]
        assert a['rows'].shape == b['rows'].shape
        assert np.array_equal(a['rows'][:, [0, 4, 8]], b['rows'][:, [0, 4, 8]])
        assert np.allclose(a['rows'], b['rows'], rtol=1e-4, atol=0), relerr(a['rows'][:, 1:], b['rows'][:, 1:])
        assert np.allclose(a['U'], b['U'], rtol=1e-5, atol=0), relerr(a['U'], b['U'])
        assert a['state'] == b['state'] and a['counters'] == b['counters']


def test_largest_grid_n2048(gpu):
    """configs[4]'s grid size: N=2048 fp64, B=5, 20 steps."""
    ps = members(2048, 5, 20)
    got, ref = batch_runs(ps, (20,)), single_runs(ps, (20,))
    for m in range(5):
        assert_same(got[m][0], ref[m][0], f"member {m}")


def test_nan_member_does_not_disturb_the_others(gpu):
    """Member 1 steps from a field with one value 1.5 (assigned after prepare, whose record of it would be NaN
    already): log(U/(1-U)) is NaN in step 1 -- a numeric state of the run, not a device fault.  It alone reports
    NaN; the others are bit for bit their single runs."""
    ps = members(256, 3, 60)
    U_bad = np.full((256, 256), ps[1].XXX)
    U_bad[17, 33] = 1.5
    bs = BatchSolver(ps)
    bs.prepare()
    bs.solvers[1].solution.U = U_bad
    with pytest.raises(AssertionError, match='NaN'):
        bs.solve_or_resume()
    assert list(bs.member_errors) == [1]
    # the C ABI's per-member status
    status = bs._batch.step_n([0, 0, 0])[1]
    assert status == [_lib.CHS_OK] * 3
    got = [snap(s) for s in bs.solvers]
    bs.close()
    ref = single_runs([ps[0], ps[2]], (None,))
    assert_same(got[0], ref[0][0], 'member 0')
    assert_same(got[2], ref[1][0], 'member 2')


def test_nan_status_through_the_c_abi(gpu):
    ps = members(256, 2, 10)
    U_bad = np.full((256, 256), ps[0].XXX)
    U_bad[0, 0] = 1.5
    b = _lib.Batch([chsimpy_amd.Solver(p)._consts() for p in ps], chsimpy_amd.Solution(ps[0]).lam)
    b.set_U(-1, np.full((256, 256), ps[0].XXX))
    b.prepare()
    b.set_U(0, U_bad)
    rows, status = b.step_n([5, 5])
    assert status == [_lib.CHS_ENAN, _lib.CHS_OK]
    assert rows[1].shape == (5, 9) and np.all(np.isfinite(rows[1]))
    assert rows[0].shape[0] == 1 and np.isnan(rows[0][-1, 1:]).any()
    b.close()


def test_zero_step_member_sits_out(gpu):
    ps = members(256, 3, 100)
    bs = BatchSolver(ps)
    bs.prepare()
    bs.solve_or_resume(30)
    before = snap(bs.solvers[1])
    bs.solve_or_resume([50, 0, 50])
    after = snap(bs.solvers[1])
    got = [snap(s) for s in bs.solvers]
    bs.close()
    assert np.array_equal(before['U'], after['U']) and before['state'] == after['state']
    assert before['counters'] == after['counters'] and np.array_equal(before['rows'], after['rows'])
    ref = single_runs([ps[0], ps[2]], (30, 50))
    assert_same(got[0], ref[0][1], 'member 0')
    assert_same(got[2], ref[1][1], 'member 2')


def test_small_poll_batches_with_stops_and_ragged_calls(gpu, monkeypatch):
    """The plain, fixed-step batch through its polls: N=128 fp64, B=4, time limits that stop member 0 at about step 20
    and would stop member 2 at about step 33, two calls of per-member lengths [40, 12, 0, 25] and [10, 10, 5, 0], once
    with CHS_BATCH_STEPS=3 (a poll behind every third step, rows copied out as they complete) and once without (no
    poll at all).  The two runs are equal in every bit, the E columns included, and both are their single handles.
    A member with a zero-step call sits it out (test_zero_step_member_sits_out): member 2 takes no step in the first
    call, so its limit cannot have stopped it by then and its stop reason there is 'None'; member 0, past its limit,
    is stopped in front of the first step of its second call."""
    ps = members(128, 4, 400)
    step_s = ps[0].delt / ps[0].M_tilde
    for m, k in ((0, 20.5), (2, 33.5)):
        ps[m].time_max = k * step_s / 60.0
    calls = ([40, 12, 0, 25], [10, 10, 5, 0])
    monkeypatch.setenv('CHS_BATCH_STEPS', '3')
    small = batch_runs(ps, calls)
    monkeypatch.delenv('CHS_BATCH_STEPS')
    whole = batch_runs(ps, calls)
    for m in range(4):
        for c in range(2):
            a, b = small[m][c], whole[m][c]
            assert np.array_equal(a['rows'], b['rows']) and np.array_equal(a['U'], b['U']), (m, c)
            assert a['state'] == b['state'] and a['counters'] == b['counters'], (m, c)
    # the single handles make the calls in which their member takes steps
    ref = [single_runs([ps[m]], [n for n in (calls[0][m], calls[1][m]) if n > 0])[0] for m in range(4)]
    for got in (small, whole):
        for m in (0, 1):
            for c in range(2):
                assert_same(got[m][c], ref[m][c], f"member {m} call {c}")
        assert_same(got[2][1], ref[2][0], 'member 2 call 1')
        assert_same(got[3][0], ref[3][0], 'member 3 call 0')
        # the call a member sits out leaves it as it was: member 2 as prepared, member 3 as its first call left it
        assert got[2][0]['rows'].shape == (1, 9)
        a, b = got[3][1], got[3][0]
        assert np.array_equal(a['rows'], b['rows']) and np.array_equal(a['U'], b['U'])
        assert a['state'] == b['state'] and a['counters'] == b['counters']
        assert [got[m][0]['counters'][3] for m in range(4)] == ['time-limit', 'None', 'None', 'None']
        assert 15 <= got[0][0]['rows'].shape[0] <= 25


def test_run_ensemble_batch_equals_member_path(gpu, tmp_path):
    """run_ensemble(batch=4) against run_ensemble(concurrent=1): 8 runs at N=256, energy stop, post-processing on."""
    p = make(256, 3000, 'fast', full_sim=False)
    p.file_id = str(tmp_path / 'e')
    ep = ex.ExperimentParams()
    ep.runs = 8
    ref = ex.run_ensemble(p, ep, concurrent=1)
    got = ex.run_ensemble(p, ep, batch=4)
    assert len(got) == len(ref) == 8
    for a, b in zip(got, ref):
        assert a[6] == b[6] and a[8] == b[8] and a[9] == b[9]          # tau0, tsep, id exact
        assert np.allclose(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), rtol=1e-12, atol=0,
                           equal_nan=True), (a, b)


def test_create_rejections_through_the_c_abi(gpu):
    lib = _lib.load()
    p = make(256, 10, 'fast')
    lam = np.ascontiguousarray(chsimpy_amd.Solution(p).lam, dtype=np.float64)
    base = chsimpy_amd.Solver(p)._consts()

    def create(cs, n_lam=256):
        arr = (_lib.chs_consts * len(cs))(*cs)
        h = C.c_void_p()
        lam_ = lam if n_lam == 256 else np.ascontiguousarray(chsimpy_amd.utils.eigenvalues_1d(n_lam))
        rc = lib.chs_batch_create(arr, len(cs), lam_.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
        if h.value:
            lib.chs_batch_destroy(h)
        return rc, lib.chs_last_error().decode()

    def mod(**kw):
        c = _lib.chs_consts.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    rc, msg = create([base, mod(adaptive_time=1)])
    assert rc == _lib.CHS_EINVAL and 'adaptive' in msg
    rc, msg = create([base, mod(N=512)])
    assert rc == _lib.CHS_EINVAL and 'N' in msg
    rc, msg = create([mod(N=4096)], n_lam=4096)
    assert rc == _lib.CHS_EINVAL and '2048' in msg
    rc, msg = create([mod(engine=_lib.CHS_ENGINE_DIRECT)])
    assert rc == _lib.CHS_EINVAL and 'fast' in msg
    rc, msg = create([base, base])
    assert rc == _lib.CHS_OK, msg
