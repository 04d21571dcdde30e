"""GPU parity tests (``-m gpu``) of every issue mode of the fused step (``chs_fast_step``, ``run_steps``) against
the oracle, at the (N, dtype) cells production reaches.  DESIGN.md section 6 maps mode x (N, dtype) to the tests.

* adaptive dt with a stop rule armed (time limit far away, or ``full_sim=False``): every firing step goes through
  the gated tail (no quiet step, no ``lam_by_colmin``), seeded at step 499 and cut into calls of every alignment;
* adaptive dt with the time limit reached inside a call after re-evaluations (``chs_fast_recover_u``), resumed;
* adaptive dt with the energy stop after step 500, unseeded;
* the same under the production switches CHS_LAM_BY_COLMIN=0, CHS_ADAPT_SPARSE=0, CHS_ADAPT_SWEEP=1;
* fp32 fixed dt against the oracle at N = 256 ... 8192, and with stop rules armed (hat flip, gate, recover_u);
* the transforms through ``Engine.dctn`` on single DCT basis modes;
* the field of every step of one-step continuing calls against the oracle's ``record=`` hook.

Each docstring names the branch of ``chs_fast_step`` the test reaches, the margin measured on the MI355X
(``parity.log``, copied to profiles/) and the oracle's cost on the GPU box (about 0.1 us per grid point and step).
"""
import numpy as np
import pytest
from scipy import fft as sfft

import chsimpy_amd
from oracle import chs_oracle as orc
from gpu_helpers import RTOL, compare_fields, compare_snapshots, drive, fmt_errs, log_line, make

pytestmark = pytest.mark.gpu

M_TILDE = 1.71e-8
CHUNKS = (1, 2, 1, 3, 1, 1, 4, 2)           # from step 499: a call boundary on every alignment of the firing pattern
RTOL_LONG = 1e-8                             # long runs through the spinodal growth (test_gpu_fast_modes.py)
RTOL_SPEC = 1e-8
# fp32 against the fp64 oracle: the largest error of every compared quantity, measured per case on the MI355X (parity.log;
# keys of fmt_errs), and each tolerance 5x that (f32_tols).  The spectral error (spectral_err: the non-constant modes of
# dctn(U - U_oracle) over std(U_oracle)) is large in fp32 and grows with N: every fp32 transform carries the constant mode
# N * mean(U), whose rounding (ulp 5e-4 at N=8192, a fifth of std(U)) leaks into the other modes.
_F32_KEYS = ('U', 'col1', 'col2', 'col3', 'col4', 'col5', 'col6', 'col7', 'col8', 'delt', 'spec', 'tds')
F32_MEASURED = {(case, N): dict(zip(_F32_KEYS, v)) for (case, N), v in {
    #                        U        E        E2       SA       domtime  Ra       L2       PS       delt     delt     spec     tds
    ('armed', 2048):        (7.36e-7, 3.77e-8, 2.60e-5, 1.25e-4, 1.59e-6, 1.46e-5, 7.94e-6, 1.83e-5, 5.56e-6, 5.44e-6, 3.95e-1, 4.77e-6),
    ('time_limit', 8192):   (1.02e-6, 3.76e-8, 8.70e-5, 5.39e-4, 5.14e-7, 3.69e-5, 7.94e-6, 3.80e-5, 2.05e-6, 4.31e-6, 3.31, 2.47e-6),
    ('fixed', 256):         (6.34e-7, 3.81e-8, 9.29e-6, 6.10e-5, 0.0, 1.15e-5, 8.77e-6, 5.21e-6, 0.0, 0.0, 4.47e-3, 0.0),
    ('fixed', 1024):        (4.13e-7, 3.80e-8, 5.44e-5, 7.82e-5, 0.0, 3.80e-5, 9.66e-6, 2.75e-5, 0.0, 0.0, 3.17e-2, 0.0),
    ('fixed', 4096):        (4.11e-7, 3.78e-8, 2.89e-5, 5.94e-5, 0.0, 2.49e-5, 7.94e-6, 1.46e-5, 0.0, 0.0, 2.88e-1, 0.0),
    ('fixed', 8192):        (6.62e-7, 3.76e-8, 1.84e-5, 4.06e-4, 0.0, 1.49e-5, 7.94e-6, 8.92e-6, 0.0, 0.0, 2.83, 0.0),
    ('time_limit_fixed', 256):  (5.19e-7, 3.77e-8, 6.50e-7, 1.53e-5, 0.0, 4.73e-6, 8.58e-6, 2.87e-7, 0.0, 0.0, 4.67e-3, 0.0),
    ('time_limit_fixed', 4096): (4.23e-7, 3.78e-8, 2.14e-5, 5.43e-5, 0.0, 2.12e-5, 7.94e-6, 1.11e-5, 0.0, 0.0, 3.26e-1, 0.0),
}.items()}


def f32_tols(case, N):
    """compare_snapshots tolerances of an fp32 case: 5x each measured error; floors for what was measured exact: SA (a
    count) two points, the fp64 time bookkeeping and the columns derived from it 1e-12."""
    m = F32_MEASURED[(case, N)]
    floor = {3: 2.0 / N ** 2, 4: 1e-12, 8: 1e-12}
    return dict(rtol=0.0, rtol_cols={c: max(5 * m[f'col{c}'], floor.get(c, 0.0)) for c in range(1, 9)},
                rtol_U=5 * m['U'], rtol_spec=5 * m['spec'],
                rtol_time=max(5 * max(m['tds'], m['delt']), 1e-12))


_ORACLE = {}


def oracle_snaps(N, chunks, seed=None, **kw):
    """The oracle's snapshots of one configuration, computed once per module: several tests compare engine runs in
    different modes (stop rule armed or not, production switches) with the same expectation.  Only one N >= 4096
    entry is kept (a field of N=4096 is 134 MB)."""
    key = (N, tuple(chunks), seed, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        if N >= 4096:
            for k in [k for k in _ORACLE if k[0] >= 4096]:
                del _ORACLE[k]
        _ORACLE[key] = drive(orc.OracleSolver(orc.make_params(N, 10 ** 6, **kw)), chunks, seed)[0]
    return _ORACLE[key]


def engine_snaps(N, chunks, seed=None, dtype='float64', **kw):
    s = chsimpy_amd.Solver(make(N, 10 ** 6, 'fast', dtype=dtype, **kw))
    snaps = drive(s, chunks, seed)[0]
    assert s._engine.engine == 'fast'
    s.close(fetch_U=False)
    return snaps


def tols(dtype, case, N):
    return f32_tols(case, N) if dtype == 'float32' else dict(rtol=RTOL, rtol_spec=RTOL_SPEC)


# ---------------------------------------------------------------------------
# A. adaptive dt with a stop rule armed
# ---------------------------------------------------------------------------
ARMED = [(1024, 'float64'), (2048, 'float32'), (4096, 'float64')]
# a stop rule armed that never fires: a time limit far away (full_sim=True), or the energy rule (full_sim=False, its
# check off as in every run seeded at step 499)
ARMS = {'time_max_far': dict(full_sim=True, time_max=1e4), 'full_sim_false': dict(full_sim=False)}


def _armed_case(N, dtype, arm):
    dmax = 4.9e-7 / N
    want = oracle_snaps(N, CHUNKS, 499, adaptive_time=True, delt_max=dmax)
    got = engine_snaps(N, CHUNKS, 499, dtype, adaptive_time=True, delt_max=dmax, **ARMS[arm])
    assert len(np.unique(want[-1]['rows'][1:, 8])) >= 4          # the rule fired several times
    return compare_snapshots(got, want, **tols(dtype, 'armed', N))


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("N,dtype", ARMED)
def test_adaptive_stop_armed_never_reached_every_alignment(gpu, N, dtype, arm):
    """Adaptive dt with a stop rule armed that never fires, seeded at step 499, calls of 1, 2, 1, 3, 1, 1, 4, 2 steps.
    With a time limit or full_sim=False there is no quiet step and no lam_by_colmin: every step of a call but its
    last defers its tail as a GATED rider of the next k_col (gate_wait), the firing ones behind
    chs_launch_colmin_rows (fused adaptive row kernel) -- a branch the full_sim=True tests never take at N >= 1024.
    Counters, time bookkeeping, record (delt column included) and U after every call against the oracle's chunks:
    fp64 at rtol 1e-9, fp32 at the stated fp32 tolerances.  Oracle: 15 steps (N=4096: 24 s, once for both arms)."""
    worst = _armed_case(N, dtype, arm)
    log_line(f"issue modes: adaptive, stop armed ({arm}), N={N} {dtype}, chunks {CHUNKS} from 499: {fmt_errs(worst)}")


# time_max (minutes) between the time_delta_sum of records 505 and 506 of the seeded adaptive run (oracle, half a
# step on either side): the limit ends the first call at step 506 -- a firing step, after the firings of 502 and
# 504 -- and every resumed call fires again and stops without a step (solver.py:185-199)
TIME_MAX_506 = {1024: 0.5327081496499861, 4096: 0.5350707949101017, 8192: 0.5352198798977204}
TL_CASES = [(1024, 'float64'), (4096, 'float64'), (8192, 'float32')]
TL_CHUNKS = (10, 1, 3)


def _time_limit_case(N, dtype):
    kw = dict(adaptive_time=True, delt_max=4.9e-7 / N if N < 8192 else 6e-11, full_sim=False,
              time_max=TIME_MAX_506[N])
    want = oracle_snaps(N, TL_CHUNKS, 499, **kw)
    got = engine_snaps(N, TL_CHUNKS, 499, dtype, **kw)
    assert [(w['steps'], w['stop']) for w in want] == [(506, 'time-limit')] * 3
    assert len(np.unique(want[0]['rows'][1:, 8])) == 3 and want[1]['delt'] != want[0]['delt']
    return compare_snapshots(got, want, **tols(dtype, 'time_limit', N))


@pytest.mark.parametrize("N,dtype", TL_CASES)
def test_adaptive_time_limit_mid_call_after_reevaluations(gpu, N, dtype):
    """Adaptive dt, full_sim=False plus a time limit, seeded at step 499: a call of 10 steps that the limit ends at
    step 506 (records 499..505), after the rule fired at 502 and 504 and re-evaluated delt at 506 itself; U rebuilt
    from hat_U (chs_fast_recover_u: the fused adaptive row kernel keeps U in registers).  Then resumed calls of 1 and
    3 steps: each re-evaluates delt from the stopped field (step 506 is even), adds it to time_delta_sum and stops
    without a step.  Stop step, stop_reason, time_delta_sum, time_passed, delt, record and U after every call.
    Oracle: 8 steps (N=8192: about a minute)."""
    worst = _time_limit_case(N, dtype)
    log_line(f"issue modes: adaptive time limit at 506, N={N} {dtype}, chunks {TL_CHUNKS}: {fmt_errs(worst)}")


# (N, delt, delt_max, stop step): full_sim=False, adaptive, from the default start field.  Chosen on the oracle: the
# energy rule stops the run in steps 520-800, after dozens of re-evaluations; conditioning (one-ulp perturbation of
# U_init -> change of the stopping field): N=128 1.8e-13, N=1024 7.4e-14
ENERGY_STOPS = [(128, 2.5e-7, 8e-9, 653), (1024, 3e-8, 4.9e-7 / 1024, 719)]


@pytest.mark.parametrize("N,delt,dmax,stop", ENERGY_STOPS)
def test_adaptive_energy_stop_beyond_step_500(gpu, N, delt, dmax, stop):
    """The reference's default mode with --adaptive-time: full_sim=False, the energy rule stopping the run beyond
    step 500 while delt adapts.  N=128 sweeps U for the integrand (k_mu), N=1024 takes the fused adaptive row kernel
    with the gated tail and chs_fast_recover_u.  One call to the stop, then resumed calls of 1, 5 and 30 steps
    (solver.py:159), all against the oracle at RTOL_LONG (L2 at 400x, as test_energy_stop_full_sim_false_fast_engine).
    Oracle: the run to the stop plus 36 steps."""
    kw = dict(full_sim=False, adaptive_time=True, delt=delt, delt_max=dmax)
    chunks = (6000, 1, 5, 30)
    want = oracle_snaps(N, chunks, **kw)
    got = engine_snaps(N, chunks, **kw)
    assert want[0]['stop'] == 'energy' and want[0]['steps'] == want[0]['tau0'] == stop
    assert len(np.unique(want[0]['rows'][:, 8])) > 3
    worst = compare_snapshots(got, want, rtol=RTOL_LONG, rtol_cols={6: 400 * RTOL_LONG}, rtol_time=1e-9,
                              rtol_spec=RTOL_LONG)
    log_line(f"issue modes: adaptive energy stop at {stop}, N={N} delt={delt} delt_max={dmax}, chunks {chunks}: "
             f"{fmt_errs(worst)}")


SWITCHES = ['CHS_LAM_BY_COLMIN=0', 'CHS_ADAPT_SPARSE=0', 'CHS_ADAPT_SWEEP=1']


@pytest.mark.parametrize("case", ['time_max_far', 'full_sim_false', 'time_limit'])
@pytest.mark.parametrize("switch", SWITCHES)
def test_adaptive_stop_rules_under_production_switches(gpu, switch, case, monkeypatch):
    """The N=1024 fp64 cases of the two tests above again with a production switch set (and no engine pool, so that
    the switch is read by a fresh engine): CHS_LAM_BY_COLMIN=0 (coefficients never set by the reduction),
    CHS_ADAPT_SPARSE=0 (the reduction issued and the tail gated on every step, csHost not used), CHS_ADAPT_SWEEP=1
    (the separate sweep of U instead of the fused adaptive row kernel: U stored every step, no recover_u).  Same
    oracle expectation.  Oracle: shared with the tests above."""
    k, v = switch.split('=')
    monkeypatch.setenv(k, v)
    monkeypatch.setenv('CHS_ENGINE_POOL', '0')
    worst = _time_limit_case(1024, 'float64') if case == 'time_limit' else _armed_case(1024, 'float64', case)
    log_line(f"issue modes: N=1024 fp64 {case} under {switch}: {fmt_errs(worst)}")


# ---------------------------------------------------------------------------
# B. fp32 stepping against the fp64 oracle
# ---------------------------------------------------------------------------
F32_FIXED = [(256, 200), (1024, 200), (4096, 12), (8192, 4)]


@pytest.mark.parametrize("N,nt", F32_FIXED)
def test_fp32_fixed_dt_vs_oracle(gpu, N, nt):
    """fp32, fixed dt, full_sim=True, one call: the deferred ungated tail on the fp32 instantiations of the fused
    kernels at N = 256 and 1024 (wave-local / one-tile columns) and N = 4096 and 8192 (the headline kernels).  Record,
    counters and U against the fp64 oracle.  Oracle: N=1024 20 s, N=4096 20 s, N=8192 27 s."""
    want = oracle_snaps(N, (nt,))
    got = engine_snaps(N, (nt,), dtype='float32')
    worst = compare_snapshots(got, want, **f32_tols('fixed', N))
    log_line(f"issue modes: fp32 fixed dt N={N} {nt} steps vs oracle: {fmt_errs(worst)}")


@pytest.mark.parametrize("N", [256, 4096])
def test_fp32_time_limit_mid_call(gpu, N):
    """fp32, full_sim=False plus a time limit of 8.5 steps: calls of 4 and 3 steps, a call of 10 that the limit ends
    after 2 and a resumed call that completes nothing.  N=256: the two-buffer hat_U flip (the tail stays deferred,
    run_steps points hat_U at the buffer of the last completed step); N=4096: the gated tail and chs_fast_recover_u.
    The stop step matches exactly (the time bookkeeping is fp64).  Oracle: 9 steps (N=4096: 15 s)."""
    kw = dict(full_sim=False, time_max=8.5 * 3e-8 / M_TILDE / 60)
    chunks = (4, 3, 10, 2)
    want = oracle_snaps(N, chunks, **kw)
    got = engine_snaps(N, chunks, dtype='float32', **kw)
    assert [(w['steps'], w['stop']) for w in want] == [(4, 'None'), (7, 'None'), (9, 'time-limit'), (9, 'time-limit')]
    worst = compare_snapshots(got, want, **f32_tols('time_limit_fixed', N))
    log_line(f"issue modes: fp32 time limit mid-call N={N}, chunks {chunks}: {fmt_errs(worst)}")


# ---------------------------------------------------------------------------
# C. the transforms (Engine.dctn: the entry kernels) on single DCT basis modes
# ---------------------------------------------------------------------------
def _basis(N, k):
    """Column k of the orthonormal DCT-III matrix: the field whose dct (norm='ortho') is the unit impulse e_k.  The
    angle pi k (2n+1) / (2N) is reduced modulo 2 pi in integers first: formed in floating point it reaches pi N/2, and
    its rounding alone (1.7e-12 of the largest entry at N=4096) would be more than the transform's error."""
    n = np.arange(N, dtype=np.int64)
    m = (k * (2 * n + 1)) % (4 * N)
    c = np.cos(np.pi * m / (2 * N)) * np.sqrt(2.0 / N)
    return c / np.sqrt(2.0) if k == 0 else c


@pytest.mark.parametrize("dtype", ['float64', 'float32'])
@pytest.mark.parametrize("N", [128, 256, 512, 1024, 2048, 4096, 8192])
def test_dctn_single_basis_modes(gpu, N, dtype):
    """Forward dctn of the basis mode (k, l) is the unit impulse at (k, l), the inverse of that impulse is the mode,
    for k, l in {0, 1, N/16-1, N/16, N/2-1, N/2, N-1} (all pairs up to N=1024, the diagonal and a shifted diagonal
    above); a constant field and the alternating +-1 field against scipy in float64.  A permutation or sign error
    shared by the forward and the inverse transform (which Parseval and the round trip both let through) moves the
    impulse.  Tolerances relative to the largest entry: fp64 1e-12, fp32 4e-6 (measured up to 1.4e-6)."""
    tol = 1e-12 if dtype == 'float64' else 4e-6
    s = chsimpy_amd.Solver(make(N, 2, 'fast', dtype=dtype), np.full((N, N), 0.5))
    eng = s._get_engine()
    assert eng.engine == 'fast'
    K = [0, 1, N // 16 - 1, N // 16, N // 2 - 1, N // 2, N - 1]
    pairs = [(k, l) for k in K for l in K] if N <= 1024 else \
        [(k, k) for k in K] + [(k, K[(i + 3) % len(K)]) for i, k in enumerate(K)]
    ef = ei = 0.0
    for k, l in pairs:
        B = np.outer(_basis(N, k), _basis(N, l))
        Y = eng.dctn(B)
        Y[k, l] -= 1.0
        ef = max(ef, float(np.max(np.abs(Y))))
        assert ef < tol, (k, l, ef, np.unravel_index(np.argmax(np.abs(Y)), Y.shape))
        E = np.zeros((N, N))
        E[k, l] = 1.0
        Z = eng.dctn(E, inverse=True)
        ei = max(ei, float(np.max(np.abs(Z - B)) / np.max(np.abs(B))))
        assert ei < tol, (k, l, ei)
    one = np.full((N, N), 1.0)
    alt = np.where((np.arange(N)[:, None] + np.arange(N)[None, :]) % 2 == 0, 1.0, -1.0)
    ec = 0.0
    for X in (one, alt):
        T = sfft.dctn(X, norm='ortho', workers=8)
        ec = max(ec, float(np.max(np.abs(eng.dctn(X) - T)) / np.max(np.abs(T))))
        ec = max(ec, float(np.max(np.abs(eng.dctn(T, inverse=True) - X))))
        assert ec < tol, ec
    log_line(f"issue modes: dctn basis modes N={N} {dtype} ({len(pairs)} pairs): forward {ef:.2e} inverse {ei:.2e} "
             f"constant/alternating {ec:.2e}")
    s.close()


# ---------------------------------------------------------------------------
# D. the field of every step, fixed dt, fp64
# ---------------------------------------------------------------------------
_PER_STEP = {}


def oracle_per_step(N, nt):
    """(snapshot, {computed_steps: U}) of ONE oracle call of nt steps from the default start field at fixed dt (`drive`
    with record=True).  At N >= 4096 it is kept for the process: tests/test_gpu_profile_steps.py holds a profiled call
    followed by an ordinary one to the same run and drops the entry when it is done (its fields are 134 MB each)."""
    if (N, nt) in _PER_STEP:
        return _PER_STEP[(N, nt)]
    snaps, fields = drive(orc.OracleSolver(orc.make_params(N, 10 ** 6)), (nt + 1,), record=True)
    if N >= 4096:
        _PER_STEP.clear()
        _PER_STEP[(N, nt)] = (snaps[0], fields)
    return snaps[0], fields


@pytest.mark.parametrize("N,nt", [(128, 50), (1024, 20), (4096, 8)])
def test_per_step_field_of_one_step_continuing_calls(gpu, N, nt):
    """Fixed dt, full_sim=True, one-step calls Engine.step_n(1): every call but the first continues the device loop
    (hat_U, T1 and sum(mu^2) taken over, the deferred tail's partial sets alternating), and its single step is both
    the first and the last of a call.  The field after each call against the field the oracle's record= hook saw
    inside ONE call, matched by computed_steps (the first solve_or_resume runs nsteps-1 steps, solver.py:160-163):
    rtol 1e-9 pointwise and in spectrum.  Oracle: nt steps (N=4096: 13 s)."""
    s = chsimpy_amd.Solver(make(N, 10 ** 6, 'fast'))
    s.prepare()
    eng = s._engine
    got = {}
    for _ in range(nt):
        rows, rc = eng.step_n(1)
        assert rc == 0 and rows.shape == (1, 9)
        got[int(eng.get_state().computed_steps)] = eng.get_U()
    s.close(fetch_U=False)
    want = oracle_per_step(N, nt)[1]
    assert sorted(want) == list(range(2, nt + 2))
    worst = compare_fields(got, want, rtol=RTOL, rtol_spec=RTOL_SPEC)
    log_line(f"issue modes: per-step U, N={N} fp64, {nt} one-step calls: {fmt_errs(worst)}")
