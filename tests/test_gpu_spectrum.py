"""GPU tests (``-m gpu``) of the radially averaged structure factor computed on the device
(chs_structure_factor / chs_batch_structure_factor, chsimpy_amd/csrc/chs_spectrum.hip).

Reference: ``scipy.fft.dctn(U - U.mean(), norm='ortho')`` in float64 of the field as downloaded with ``get_U`` -- the
exact values the device holds, also for fp32 -- binned with ``spectrum.bin_of``.

Tolerance, derived: the suite's transform tolerance tau for the engine and element type bounds the error of every
coefficient by delta = tau * max|C_ref|; a bin of n_b modes with the power Ssum_ref then moves by at most
    2 * delta * sqrt(n_b * Ssum_ref) + n_b * delta**2        (Cauchy-Schwarz over the bin's modes)
and bin 0, whose only mode counts as 0, is exactly 0 on both sides.  The worst ratio of error to bound of every case is
logged (profiles/spectrum_parity_margins.txt).
"""
import functools
import os

import numpy as np
import pytest
from scipy import fft as sfft

import chsimpy_amd
from chsimpy_amd import _lib, experiment as ex, spectrum
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import log_line, make, relerr, seed_step

pytestmark = pytest.mark.gpu

# The transform tolerances of the existing dctn tests, as a fraction of the largest coefficient:
TAU_F64 = 1e-12          # tests/test_gpu_parity.py: test_dctn_matches_scipy (direct, fast); tests/test_gpu_chirp.py (chirp)
TAU_F32_FAST = 2e-5      # tests/test_gpu_parity.py: test_fp32_dctn
TAU_F32_CHIRP = 4e-6     # tests/test_gpu_chirp.py: FP32_TOL (N <= 1000)


def tau_of(engine, dtype):
    if dtype == 'float64':
        return TAU_F64
    return TAU_F32_CHIRP if engine == 'chirp' else TAU_F32_FAST


@functools.lru_cache(maxsize=None)
def sizes(N):
    return spectrum.bin_sizes(N)


def reference(U):
    C = sfft.dctn(np.asarray(U, dtype=np.float64) - U.mean(), norm='ortho', workers=max(1, min(8, os.cpu_count() or 1)))
    return spectrum.bin_power(C), float(np.max(np.abs(C)))


def bound_of(ref, cmax, tau, N):
    n = sizes(N).astype(np.float64)
    delta = tau * cmax
    return 2.0 * delta * np.sqrt(n * ref) + n * delta * delta


def check(ssum, U, tau, what):
    """Every bin within the bound; returns the worst ratio of error to bound."""
    N = U.shape[0]
    ref, cmax = reference(U)
    assert ssum.shape == ref.shape == (spectrum.bin_count(N),)
    assert ssum.dtype == np.float64
    assert ssum[0] == 0.0 and ref[0] == 0.0
    bound = bound_of(ref, cmax, tau, N)
    err = np.abs(ssum - ref)
    ratio = float(np.max(err[1:] / bound[1:]))
    log_line(f"spectrum {what}: worst |Ssum - ref| / bound = {ratio:.3e} (tau {tau:g}, max|C| {cmax:.3e}, "
             f"k1 {spectrum.StructureFactor(ssum, N).k1:.6g} ref {spectrum.StructureFactor(ref, N).k1:.6g})")
    assert np.all(err <= bound), (what, ratio, int(np.argmax(err / np.maximum(bound, 1e-300))))
    return ratio


def solver(N, ntmax, engine, dtype='float64', U_init=None, **kw):
    return chsimpy_amd.Solver(make(N, ntmax, engine, dtype=dtype, **kw), U_init)


# ---------------------------------------------------------------------------
# 1. single modes: layout and binning
# ---------------------------------------------------------------------------
MODE_CASES = [(128, 'fast', 'float64'), (128, 'fast', 'float32'), (100, 'chirp', 'float64'), (24, 'direct', 'float64'),
              (301, 'chirp', 'float64')]   # 301: ragged edges in every 32-wide tile, an odd N (no 16-byte rows)


@pytest.mark.parametrize("N,engine,dtype", MODE_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in MODE_CASES])
@pytest.mark.parametrize("which", ['3-7', 'edge'])
def test_single_modes_land_in_their_bins(gpu, N, engine, dtype, which):
    """U = 0.5 + a cos(pi p (x+1/2)/N) cos(pi q (y+1/2)/N) + a' (a second mode at another radius): Ssum is a^2 N^2 / 4
    in bin_of(p, q), a'^2 N^2 / 4 in the second mode's bin, and every other bin stays below n_b delta^2."""
    p, q = (3, 7) if which == '3-7' else (N - 1, 1)
    p2, q2 = 10, 2
    a, a2 = 0.01, 0.005
    x = (np.arange(N) + 0.5) / N
    U = (0.5 + a * np.outer(np.cos(np.pi * p * x), np.cos(np.pi * q * x))
         + a2 * np.outer(np.cos(np.pi * p2 * x), np.cos(np.pi * q2 * x)))
    s = solver(N, 2, engine, dtype, U_init=U)
    s.prepare()
    assert s._engine.engine == engine
    sf = s.structure_factor()
    Ud = s._engine.get_U()
    tau = tau_of(engine, dtype)
    check(sf.Ssum, Ud, tau, f"modes ({p},{q})+({p2},{q2}) N={N} {engine} {dtype}")
    b1, b2 = spectrum.bin_of(p, q), spectrum.bin_of(p2, q2)
    assert b1 != b2
    want = np.zeros(spectrum.bin_count(N))
    want[b1], want[b2] = a * a * N * N / 4, a2 * a2 * N * N / 4
    # Against the analytic spectrum the same bound with a larger delta: the field the device holds is the analytic one
    # up to the rounding of its storage (|U| <= 0.515) and of the centred field (|U - mean| <= 0.015), half an ulp each
    # per element, and an orthonormal transform moves no coefficient by more than the 2-norm of that: N * 0.53 * ulp/2.
    half_ulp = 2.0 ** -53 if dtype == 'float64' else 2.0 ** -24
    delta = tau * (a * N / 2) + N * 0.53 * half_ulp
    n = sizes(N).astype(np.float64)
    bound = 2.0 * delta * np.sqrt(n * want) + n * delta * delta
    err = np.abs(sf.Ssum - want)
    assert np.all(err <= bound), (int(np.argmax(err / bound)), float(np.max(err / bound)))
    assert sf.N == N and sf.ell == 2 * N / sf.k1 and sf.ell_phys == sf.ell * s.solution.delx
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random and evolved fields against the reference
# ---------------------------------------------------------------------------
FIELD_CASES = [(128, 'fast', 'float64', 40), (128, 'fast', 'float32', 40), (256, 'fast', 'float64', 40),
               (256, 'fast', 'float32', 40), (129, 'auto', 'float64', 40), (1025, 'chirp', 'float64', 40),
               (2048, 'fast', 'float32', 0),    # the 8-column tile configuration of the fast engine
               (4096, 'fast', 'float64', 0)]    # the headline size: 1024 tiles, the most bins of the fp64 step's sizes


@pytest.mark.parametrize("N,engine,dtype,steps", FIELD_CASES, ids=[f"N{c[0]}-{c[2]}" for c in FIELD_CASES])
def test_fields_against_scipy(gpu, N, engine, dtype, steps):
    s = solver(N, steps + 1, engine, dtype)
    s.prepare()
    eng = s._engine.engine
    assert eng == ('chirp' if N in (129, 1025) else 'fast')
    tau = tau_of(eng, dtype)
    check(s.structure_factor().Ssum, s._engine.get_U(), tau, f"start field N={N} {eng} {dtype}")
    if steps:
        s.solve_or_resume()
        assert s.solution.computed_steps == steps + 1
        sf = s.structure_factor()
        check(sf.Ssum, s._engine.get_U(), tau, f"after {steps} steps N={N} {eng} {dtype}")
        assert 0 < sf.k1 < N and sf.ell > 2
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp'), (4096, 'fast')])
def test_two_calls_give_the_same_bits(gpu, N, engine):
    s = solver(N, 8, engine)
    s.prepare()
    a = s.structure_factor().Ssum
    b = s.structure_factor().Ssum
    assert np.array_equal(a, b)
    s.solve_or_resume(4)
    c = s.structure_factor().Ssum
    d = s.structure_factor().Ssum
    assert np.array_equal(c, d) and not np.array_equal(a, c)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. observing does not change the run
# ---------------------------------------------------------------------------
def _observed_run(N, engine, calls, look, seed=None, **kw):
    s = solver(N, 1000, engine, **kw)
    s.rederive_hat = False
    s.prepare()
    if seed is not None:
        seed_step(s, seed)
    look(s)
    out = []
    for n in calls:
        s.solve_or_resume(n)
        look(s)
        st = s._engine.get_state()
        out.append((s.solution.timedata.data().copy(),
                    (st.delt, st.time_delta_sum, st.time_passed, st.tau0, st.t0, st.computed_steps, st.skip_check, st.stop_reason)))
    U = s._engine.get_U()
    s.close(fetch_U=False)
    return out, U


OBSERVE_CASES = [(128, 'fast', (7, 6, 5), None, {}),            # the continuing loop: T1, hat_U, partial sums carried
                 (4096, 'fast', (3, 2, 2), None, {}),           # the gated configuration, other buffers
                 (100, 'chirp', (7, 6, 5), None, {}),
                 # (delt_max as the seeded adaptive runs of tests/test_gpu_issue_modes.py have it: the default lets the field leave (0, 1))
                 (128, 'fast', (7, 6, 5), 499, dict(adaptive_time=True, delt_max=4.9e-7 / 128))]


@pytest.mark.parametrize("N,engine,calls,seed,kw", OBSERVE_CASES,
                         ids=[f"N{c[0]}-{c[1]}" + ('-adaptive' if c[4] else '') for c in OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with structure_factor() between them against the same calls with get_U() between them: all nine record
    columns, the state and the final field, bit for bit."""
    got, Ug = _observed_run(N, engine, calls, lambda s: s.structure_factor(), seed, **kw)
    ref, Ur = _observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), (c, relerr(rg[:, c], rr[:, c]))
        assert sg == sr
    assert got[-1][0].shape[0] == 1 + sum(calls) - (1 if seed is None else 0)   # (the first call after prepare: nsteps-1)
    assert np.array_equal(Ug, Ur)


@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_a_look_behind_a_stopped_call(gpu, N, engine):
    """A call that the time limit ended leaves the device's halt flag set, at which the transform kernels return at
    once: the look takes it down for its own launches and puts it back.  The spectrum is that of the field the call
    left, the state is what it was, and the resumed call (which stops again without a step) gives what it gives behind
    a get_U."""
    kw = dict(time_max=30 * 3e-8 / 1.71e-8 / 60)      # ~30 steps of simulated time (tests/test_gpu_parity.py: test_time_limit_stop)

    def run(look):
        s = solver(N, 500, engine, **kw)
        s.prepare()
        s.solve_or_resume()
        assert s.solution.stop_reason == 'time-limit' and s.solution.computed_steps < 40
        seen = look(s)
        st = s._engine.get_state()
        state = (st.delt, st.time_delta_sum, st.time_passed, st.tau0, st.t0, st.computed_steps, st.skip_check, st.stop_reason)
        s.solve_or_resume(3)
        out = (state, s.solution.timedata.data().copy(), s._engine.get_U(), s.solution.computed_steps)
        s.close(fetch_U=False)
        return seen, out

    sf, got = run(lambda s: s.structure_factor())
    U, ref = run(lambda s: s._engine.get_U())
    check(sf.Ssum, U, TAU_F64, f"behind a time-limit stop N={N} {engine}")
    assert got[0] == ref[0] and got[3] == ref[3]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


# ---------------------------------------------------------------------------
# 5. batch
# ---------------------------------------------------------------------------
def _members(N, B, ntmax):
    init = make(N, ntmax, 'auto')
    init.file_id = 'spectrum'
    ep = ex.ExperimentParams()
    ep.runs = B
    rv, al, n = ex.make_rand_values(ep)
    ps = [ex.run_params(init, i, rv, al)[0] for i in range(B)]
    for m, p in enumerate(ps):
        p.seed = 2023 + 7 * m
    return ps


def _batch_snap(bs):
    out = []
    for s in bs.solvers:
        st = s._engine.get_state()
        out.append((s.solution.timedata.data().copy(), s._engine.get_U(),
                    (st.delt, st.time_delta_sum, st.time_passed, st.tau0, st.t0, st.computed_steps, st.skip_check, st.stop_reason)))
    return out


@pytest.mark.parametrize("N,engine", [(256, 'fast'), (136, 'chirp')])
def test_batch_equals_the_single_solvers_and_leaves_the_members_alone(gpu, N, engine):
    B = 3
    ps = _members(N, B, 100)
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    sfs = bs.structure_factor()
    assert len(sfs) == B
    for m in range(B):                                   # member = -1 against member by member
        assert np.array_equal(bs.structure_factor(m).Ssum, sfs[m].Ssum), m
    assert not np.array_equal(sfs[0].Ssum, sfs[1].Ssum)  # different runs
    bs.solve_or_resume(5)
    looked = _batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert np.array_equal(s.structure_factor().Ssum, sfs[m].Ssum), m
        s.close(fetch_U=False)
    ref = BatchSolver(ps)                                # the members' next call without the look
    ref.prepare()
    ref.solve_or_resume(20)
    ref.solve_or_resume(5)
    plain = _batch_snap(ref)
    ref.close(fetch_U=False)
    for m in range(B):
        assert np.array_equal(looked[m][0], plain[m][0]) and np.array_equal(looked[m][1], plain[m][1]), m
        assert looked[m][2] == plain[m][2], m


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_wrong_bin_count_and_missing_field(gpu):
    s = solver(128, 4, 'fast')
    eng = s._get_engine()
    nb = spectrum.bin_count(128)
    assert gpu.chs_structure_factor_bins(128) == nb
    buf = np.zeros(nb + 1)
    assert gpu.chs_structure_factor(eng._h, _lib._dptr(buf), nb) == _lib.CHS_ESTATE     # no field yet
    with pytest.raises(AssertionError):
        s.structure_factor()
    s.prepare()
    assert gpu.chs_structure_factor(eng._h, _lib._dptr(buf), nb + 1) == _lib.CHS_EINVAL
    msg = gpu.chs_last_error().decode()
    assert str(nb) in msg and 'expected' in msg, msg
    assert gpu.chs_structure_factor(eng._h, _lib._dptr(buf), nb) == _lib.CHS_OK
    ms = s._engine.structure_factor_ms()
    assert ms.shape == (3,) and np.all(ms >= 0.0)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 7. experiment
# ---------------------------------------------------------------------------
def test_experiment_domain_sizes_batch_equals_member_path(gpu, tmp_path, capsys):
    """`-N 136 -R 4 --batch 2 --domain-size` and the same with `--concurrent 1` write identical -domains.csv, and their
    -results.csv is byte for byte that of a run without the flag."""
    base = ['-N', '136', '-R', '4', '-n', '80']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--concurrent', '1', '--domain-size', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '2', '--domain-size', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    one, batch = open(tmp_path / 'one-domains.csv').read(), open(tmp_path / 'batch-domains.csv').read()
    assert one == batch
    lines = one.splitlines()
    assert lines[0] == 'id,k1,ell,ell_phys' and len(lines) == 5
    for i, ln in enumerate(lines[1:]):
        rid, k1, ell, ell_phys = ln.split(',')
        assert int(rid) == i and 0 < float(k1) < 136 and float(ell) == 2 * 136 / float(k1) and float(ell_phys) > 0
    assert not (tmp_path / 'plain-domains.csv').exists()
    plain = open(tmp_path / 'plain-results.csv', 'rb').read()
    assert plain == open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()
