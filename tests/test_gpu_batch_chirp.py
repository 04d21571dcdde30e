"""GPU tests (``-m gpu``) of the chirp batch: B members of a grid size the chirp engine runs, advanced by one launch
set of the chirp step's 13 kernels, against the same members as single ``Solver``s with ``engine='chirp'`` and
``rederive_hat=True`` (every call a literal solve_or_resume, as every batched call is).

Equality is bit for bit in fp64 AND fp32 -- all nine timedata columns, U, the state tuple and the Solution counters:
the batched kernels are the single handle's kernels with the member's record in place of the arguments (one body, the
same block shapes, bands and reduction trees), so no column needs a tolerance here (tests/test_gpu_batch.py's E2_RTOL is
the fast batch's, whose tail is another kernel than the single handle's)."""
import ctypes as C

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, experiment as ex
from chsimpy_amd.batch import BatchSolver, batch_engine
from oracle import chs_oracle as orc
from gpu_helpers import RTOL, log_line, make, relerr

pytestmark = pytest.mark.gpu


def members(N, B, ntmax, engine='chirp', **kw):
    """B parameter sets of one ensemble: A0/A1 factors of make_rand_values (uniform source)."""
    init = make(N, ntmax, engine, **kw)
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


def single_runs(params_list, calls, U_inits=None, engines=None):
    out = []
    for m, p in enumerate(params_list):
        s = chsimpy_amd.Solver(p, None if U_inits is None else U_inits[m])
        s.rederive_hat = True
        s.prepare()
        if engines is not None:
            engines.append(s._engine.engine)
        snaps = []
        for n in calls:
            n = n[m] if isinstance(n, (list, tuple)) else n
            s.solve_or_resume(n)
            snaps.append(snap(s))
        s.close()
        out.append(snaps)
    return out


def batch_runs(params_list, calls, U_inits=None, engines=None):
    bs = BatchSolver(params_list, U_inits)
    bs.prepare()
    if engines is not None:
        engines.append(bs._batch.engine)      # what the device batch's members report (chs_batch_engine)
    snaps = [[] for _ in params_list]
    for n in calls:
        bs.solve_or_resume(list(n) if isinstance(n, (list, tuple)) else n)
        for m, s in enumerate(bs.solvers):
            snaps[m].append(snap(s))
    bs.close()
    return snaps


def assert_same(a, b, what=''):
    """bit for bit: every timedata column, the field, the state and the counters"""
    assert a['rows'].shape == b['rows'].shape, (what, a['rows'].shape, b['rows'].shape)
    for c in range(9):
        assert np.array_equal(a['rows'][:, c], b['rows'][:, c]), (what, 'column', c, relerr(a['rows'][:, c], b['rows'][:, c]))
    assert np.array_equal(a['U'], b['U']), (what, 'U', relerr(a['U'], b['U']))
    assert a['state'] == b['state'], (what, a['state'], b['state'])
    assert a['counters'] == b['counters'], (what, a['counters'], b['counters'])


# N, B, engine, calls, member settings: the smallest shapes at which each path of the line kernel's launch can go wrong
SHAPES = [
    (24, 5, 'chirp', (20, 3), {}),      # P=64: 32 lines per workgroup, one partial workgroup per member
    (100, 3, 'chirp', (40, 7), {}),     # P=256: 13 workgroups per member, the last with 4 of 8 lines; N no multiple of the 32-wide tile
    (129, 2, 'auto', (10,), {}),        # P=512; 'auto' resolves to chirp
    (1025, 2, 'chirp', (3,), {}),       # P=4096: the 512-thread launch of the MAXT = 1024 instantiation
    (2049, 2, 'chirp', (2,), {}),       # P=8192: 1024 threads, 132 KiB of LDS
    # the batched float launches of 512 and 1024 threads (the single handles they are compared with meet scipy and the
    # oracle at these sizes in tests/test_gpu_chirp.py and tests/test_gpu_chirp_sizes.py)
    (1025, 2, 'chirp', (3,), dict(dtype='float32')),
    (2049, 2, 'chirp', (2,), dict(dtype='float32')),
]


@pytest.mark.parametrize('N, B, engine, calls, kw', SHAPES,
                         ids=[f"N{s[0]}" + ''.join(f"-{v}" for v in s[4].values()) for s in SHAPES])
def test_bitwise_equal_to_single_chirp_handles(gpu, N, B, engine, calls, kw):
    ps = members(N, B, sum(calls) + 2, engine, **kw)
    engines, of_batch = [], []
    got, ref = batch_runs(ps, calls, engines=of_batch), single_runs(ps, calls, engines=engines)
    # the members of the device batch report the engine a single handle of them runs, and the host rule says the same
    assert of_batch == ['chirp'], of_batch
    assert engines == ['chirp'] * B and batch_engine(ps[0]) == 'chirp', engines
    for m in range(B):
        for c in range(len(calls)):
            assert_same(got[m][c], ref[m][c], f"N={N} {kw} member {m} call {c}")
        assert got[m][-1]['rows'].shape[0] == 1 + sum(calls) - 1   # (the first call after prepare runs nsteps-1 iterations)
    assert got[0][0]['rows'][-1, 1] != got[1][0]['rows'][-1, 1]   # the members are different runs


def test_member_against_oracle(gpu):
    """Member 1 of the N=100, B=3 batch, 60 steps, against the CPU oracle run with the same factors."""
    ps = members(100, 3, 60)
    bs = BatchSolver(ps)
    bs.prepare()
    sol = bs.solve_or_resume()[1]
    p = ps[1]
    o = orc.OracleSolver(orc.make_params(100, 60, func_A0=p.func_A0, func_A1=p.func_A1))
    o.prepare()
    o.solve_or_resume()
    td, to = sol.timedata.data(), o.timedata.data()
    assert td.shape == to.shape
    assert np.array_equal(td[:, 0], to[:, 0])
    for c in (1, 2, 3, 4, 5, 6, 7, 8):
        assert np.allclose(td[:, c], to[:, c], rtol=RTOL, atol=1e-300), (c, relerr(td[:, c], to[:, c]))
    assert np.allclose(sol.U, o.U, rtol=RTOL, atol=0), relerr(sol.U, o.U)
    assert sol.computed_steps == o.computed_steps and sol.stop_reason == o.stop_reason
    assert sol.tau0 == o.tau0 and sol.t0 == pytest.approx(o.t0, rel=1e-12)
    bs.close()


ENERGY_STOPS = [68, 105, 85, 75]   # computed_steps at which the CPU oracle stops these four members


@pytest.fixture(scope='module')
def energy_singles(gpu):
    """the four members of the energy-rule tests as single chirp handles: computed once, read by both tests"""
    ps = members(72, 4, 4000, full_sim=False, delt=2e-6)
    return ps, single_runs(ps, (None, 30))


@pytest.mark.parametrize('batch_steps', [None, '4'], ids=['one-poll-size', 'CHS_BATCH_STEPS=4'])
def test_per_member_energy_stop(gpu, energy_singles, monkeypatch, batch_steps):
    """N=72, B=4, energy rule armed (full_sim=False, delt=2e-6, ntmax=4000): every member stops at its own step, the
    launches go on for the others.  With CHS_BATCH_STEPS=4 there is a poll behind every fourth step: rows are copied
    out while the call runs, launches are issued behind halted members, and the call ends once the polls have seen
    everyone stopped.  Then a resumed call of 30 steps."""
    ps, ref = energy_singles
    if batch_steps:
        monkeypatch.setenv('CHS_BATCH_STEPS', batch_steps)
    got = batch_runs(ps, (None, 30))
    stops = [got[m][0]['counters'][0] for m in range(4)]
    assert stops == [ref[m][0]['counters'][0] for m in range(4)]
    assert stops == ENERGY_STOPS, stops
    assert len(set(stops)) == 4
    assert [got[m][0]['counters'][3] for m in range(4)] == ['energy'] * 4
    for m in range(4):
        for c in range(2):
            assert_same(got[m][c], ref[m][c], f"member {m} call {c}")


def test_per_member_time_limit(gpu):
    """N=100, B=4: four time limits -- below the first step (k_pre stops the member before it has taken a step: no row,
    the field untouched), two in mid-call, one never reached.  Then a second call."""
    ps = members(100, 4, 120)
    step_s = ps[0].delt / ps[0].M_tilde
    for p, k in zip(ps, (0.5, 30.5, 70.5, 1e6)):
        p.time_max = k * step_s / 60.0
    calls = (100, 20)
    got, ref = batch_runs(ps, calls), single_runs(ps, calls)
    for m in range(4):
        for c in range(len(calls)):
            assert_same(got[m][c], ref[m][c], f"member {m} call {c}")
    assert [got[m][0]['counters'][3] for m in range(4)] == ['time-limit', 'time-limit', 'time-limit', 'None']
    n = [got[m][0]['rows'].shape[0] for m in range(4)]
    assert n[0] == 1 and n[0] < n[1] < n[2] < n[3] == 100, n


def test_ragged_calls_and_a_member_that_sits_out(gpu):
    """N=40, B=4, calls of per-member lengths [0, 1, 5, 12] and [3, 0, 2, 1]: a member with a zero-step call keeps its
    state, record and field; the others are their single handles, which make the calls in which their member steps."""
    ps = members(40, 4, 100)
    calls = ([0, 1, 5, 12], [3, 0, 2, 1])
    bs = BatchSolver(ps)
    bs.prepare()
    prepared = [snap(s) for s in bs.solvers]
    bs.solve_or_resume(list(calls[0]))
    first = [snap(s) for s in bs.solvers]
    bs.solve_or_resume(list(calls[1]))
    second = [snap(s) for s in bs.solvers]
    bs.close()
    for a, b in ((prepared[0], first[0]), (first[1], second[1])):     # the calls that members 0 and 1 sit out
        assert np.array_equal(a['rows'], b['rows']) and np.array_equal(a['U'], b['U'])
        assert a['state'] == b['state'] and a['counters'] == b['counters']
    ref = [single_runs([ps[m]], [k for k in (calls[0][m], calls[1][m]) if k > 0])[0] for m in range(4)]
    assert_same(second[0], ref[0][0], 'member 0 call 1')
    assert_same(first[1], ref[1][0], 'member 1 call 0')
    for m in (2, 3):
        assert_same(first[m], ref[m][0], f"member {m} call 0")
        assert_same(second[m], ref[m][1], f"member {m} call 1")


def test_nan_member_does_not_disturb_the_others(gpu):
    """Member 1 steps from a field with one value 1.5 (assigned after prepare): log(U/(1-U)) is NaN in step 1 -- a
    numeric state of the run, not a device fault.  It alone reports NaN; the others are bit for bit their singles."""
    N = 100
    ps = members(N, 3, 30)
    U_bad = np.full((N, N), ps[1].XXX)
    U_bad[17, 33] = 1.5
    bs = BatchSolver(ps)
    bs.prepare()
    bs.solvers[1].solution.U = U_bad
    with pytest.raises(AssertionError, match='NaN'):
        bs.solve_or_resume()
    assert list(bs.member_errors) == [1]
    status = bs._batch.step_n([0, 0, 0])[1]
    assert status == [_lib.CHS_OK] * 3
    got = [snap(s) for s in bs.solvers]
    bs.close()
    for m in (0, 2):
        assert np.all(np.isfinite(got[m]['rows']))
    ref = single_runs([ps[0], ps[2]], (None,))
    assert_same(got[0], ref[0][0], 'member 0')
    assert_same(got[2], ref[1][0], 'member 2')


def test_fp32_bitwise_equal_to_single_chirp_handles(gpu):
    """fp32, N=100, B=3, 30 steps: the shared kernel bodies deliver bit for bit here too.  The distances from the fp64
    oracle (the batch's and the single handle's are the same numbers) go to the parity log."""
    ps = members(100, 3, 30, dtype='float32')
    got, ref = batch_runs(ps, (30,)), single_runs(ps, (30,))
    for m in range(3):
        assert_same(got[m][0], ref[m][0], f"fp32 member {m}")
    p = ps[0]
    o = orc.OracleSolver(orc.make_params(100, 30, func_A0=p.func_A0, func_A1=p.func_A1))
    o.prepare()
    o.solve_or_resume()
    to = o.timedata.data()
    for name, run in (('batch', got[0][0]), ('single', ref[0][0])):
        cols = ' '.join(f"col{c} {relerr(run['rows'][:, c], to[:, c]):.2e}" for c in (1, 2, 5, 6, 7))
        log_line(f"chirp fp32 N=100 B=3 30 steps, {name} member 0 against the fp64 oracle: U {relerr(run['U'], o.U):.2e} {cols}")


def test_rejections_through_the_c_abi(gpu):
    lib = _lib.load()
    lam_of = lambda p: np.ascontiguousarray(chsimpy_amd.Solution(p).lam, dtype=np.float64)

    def create(cs, lam):
        arr = (_lib.chs_consts * len(cs))(*cs)
        h = C.c_void_p()
        rc = lib.chs_batch_create(arr, len(cs), lam.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
        if h.value:
            lib.chs_batch_destroy(h)
        return rc, lib.chs_last_error().decode()

    p = make(100, 10, 'chirp')
    base = chsimpy_amd.Solver(p)._consts()
    adaptive = _lib.chs_consts.from_buffer_copy(base)
    adaptive.adaptive_time = 1
    rc, msg = create([base, base], lam_of(p))
    assert rc == _lib.CHS_OK, msg
    rc, msg = create([base, adaptive, adaptive], lam_of(p))
    assert rc == _lib.CHS_EINVAL and 'adaptive' in msg and 'member 1' in msg
    p136 = make(136, 10, 'chirp')
    chirp136 = chsimpy_amd.Solver(p136)._consts()
    auto136 = _lib.chs_consts.from_buffer_copy(chirp136)
    auto136.engine = _lib.CHS_ENGINE_AUTO
    rc, msg = create([auto136, chirp136], lam_of(p136))                  # two spellings of one resolved engine
    assert rc == _lib.CHS_OK, msg
    fast136 = _lib.chs_consts.from_buffer_copy(chirp136)
    fast136.engine = _lib.CHS_ENGINE_FAST
    rc, msg = create([chirp136, fast136], lam_of(p136))
    assert rc == _lib.CHS_EINVAL and 'engine' in msg and 'member 1' in msg
    auto100 = _lib.chs_consts.from_buffer_copy(base)
    auto100.engine = _lib.CHS_ENGINE_AUTO
    rc, msg = create([auto100], lam_of(p))
    assert rc == _lib.CHS_EINVAL and '2048' in msg                       # 'auto' at N=100 is the direct engine
    p256 = make(256, 10, 'chirp')
    rc, msg = create([chsimpy_amd.Solver(p256)._consts()], lam_of(p256))
    assert rc == _lib.CHS_EINVAL and 'fast engine only' in msg

    b = _lib.Batch([base, base], lam_of(p))
    assert b.engine == 'chirp'
    b.set_U(-1, np.full((100, 100), p.XXX))
    b.prepare()
    n = (C.c_int64 * 2)(5, 5)
    done, status = (C.c_int64 * 2)(), (C.c_int32 * 2)()
    assert lib.chs_batch_step_n_queued(b._h, 2, n, 0, done, status) == _lib.CHS_EINVAL
    assert 'queue' in lib.chs_last_error().decode()
    rows, st = b.step_n([5, 5])                                          # the batch is still good for a plain call
    assert st == [_lib.CHS_OK] * 2 and rows[0].shape == rows[1].shape == (5, 9)
    b.close()


def test_experiment_cli_batch_equals_member_path(gpu, tmp_path, capsys):
    """python -m chsimpy_amd.experiment -N 136 -R 6 --batch 3 writes the results file of --concurrent 1 byte for byte
    (N=136 under 'auto' is a chirp size) and no longer says that the batch was not taken."""
    base = ['-N', '136', '-R', '6', '-n', '80']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '3', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    assert open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()
    assert 'batch_per_rank, 3' in open(tmp_path / 'batch-metadata.csv').read()
