"""GPU tests (``-m gpu``) of ``chs_profile_steps`` (``Engine.profile_steps``), the call behind the roofline figure of
bench.py: nsteps steps with every kernel slot timed by HIP events on the engine's stream, the record thrown away.

A profiled call takes an issue plan production never uses otherwise (chs_step_host.h: no warm entry, no riding tail --
the bookkeeping is a launch of its own behind every row kernel -- ``keepResident`` off, ``decide`` off), so nothing else
in the suite holds it to the oracle.  Here: the loop state and the field behind a profiled call, the ordinary call that
follows it (which has to enter cold and finds partial sums, ``hat_valid`` and ``resident`` as the profiled call left
them), an adaptive and a stopped profiled call, the numbers it returns and its argument checks.  The oracle and the
comparison helpers are those of tests/test_gpu_issue_modes.py (about 0.1 us per grid point and step)."""
import math

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib
from gpu_helpers import RTOL, fmt_errs, log_line, make, relerr, seed_step, spectral_err
import test_gpu_issue_modes as tim

pytestmark = pytest.mark.gpu

SLOT_MU, SLOT_PRE, SLOT_FWD, SLOT_SPEC, SLOT_INV, SLOT_DIAG, SLOT_FIN, SLOT_MISC = range(_lib.CHS_NKERNELS)
K = 3                                         # steps of the ordinary call behind a profiled one
# sum(ms) - last_step_ms() of a profiled call was measured on the MI355X over the cases of
# test_the_numbers_a_profiled_call_returns and N = 4096, three calls each: -0.24 ... -1.02 ms, never positive (the call's
# own interval also holds its entry and the gaps between the launches; profiles/looks_large_sizes.txt).  So the test
# asserts sum(ms) <= last_step_ms() with no allowance.


def engine_of(N, engine, dtype='float64', seed=None, **kw):
    s = chsimpy_amd.Solver(make(N, 10 ** 6, engine, dtype=dtype, **kw))
    s.prepare()
    if seed is not None:
        seed_step(s, seed)
    assert s._engine.engine == engine
    return s, s._engine


def state_of(eng):
    st = eng.get_state()
    return dict(steps=int(st.computed_steps), stop=_lib.STOP_NAMES[st.stop_reason], tau0=st.tau0, skip=bool(st.skip_check),
                t0=float(st.t0), tds=float(st.time_delta_sum), tp=float(st.time_passed), delt=float(st.delt))


def compare_state_and_field(g, U, w, rtol_U=RTOL, rtol_spec=RTOL, rtol_time=1e-12):
    """What compare_snapshots asks of a call's end, without the record: the counters exactly, the time bookkeeping to
    rtol_time, the field pointwise and in spectrum.  Returns the errors."""
    worst = {}
    for k in ('steps', 'stop', 'tau0', 'skip'):
        assert g[k] == w[k], (k, g[k], w[k])
    for k in ('t0', 'tds', 'tp', 'delt'):
        worst[k] = abs(g[k] - w[k]) / max(abs(w[k]), 1e-300)
        assert worst[k] <= rtol_time, (k, g[k], w[k], worst[k])
    worst['U'], worst['spec'] = relerr(U, w['U']), spectral_err(U, w['U'])
    assert worst['U'] <= rtol_U, ('U', worst['U'])
    assert worst['spec'] <= rtol_spec, ('U spectrum', worst['spec'])
    return worst


def compare_rows(rows, want, rtol=RTOL):
    """The record rows of a call against the oracle's rows of the same steps, as compare_snapshots compares them."""
    assert rows.shape == want.shape, (rows.shape, want.shape)
    assert np.array_equal(rows[:, 0], want[:, 0])
    worst = {}
    for c in range(1, 9):
        e = relerr(rows[:, c], want[:, c]) if c != 3 else float(np.max(np.abs(rows[:, c] - want[:, c])))
        worst[f'col{c}'] = e
        assert e <= rtol, (f'record column {c}', e)
    return worst


def check_numbers(eng, ms, calls, n):
    """What every profiled call returns: a name for every slot that was timed, finite times, and the slot intervals as
    disjoint pieces of the stream between the call's own two events.  Returns sum(ms) - last_step_ms()."""
    names = eng.kernel_names()
    assert ms.shape == calls.shape == (_lib.CHS_NKERNELS,) and len(names) == _lib.CHS_NKERNELS
    for i in range(_lib.CHS_NKERNELS):
        assert calls[i] >= 0 and math.isfinite(ms[i]) and ms[i] >= 0.0, (i, calls[i], ms[i])
        assert calls[i] == 0 or names[i], (i, names[i], calls[i])
        assert calls[i] > 0 or ms[i] == 0.0, (i, ms[i])
    total = eng.last_step_ms()
    assert math.isfinite(total) and total > 0.0
    excess = float(ms.sum()) - total
    log_line(f"profile steps: N={eng.N} {eng.engine} n={n}: sum(ms) {float(ms.sum()):.6f} call {total:.6f} excess {excess:.3e} ms; "
             f"calls {calls.tolist()}")
    return excess


# ---------------------------------------------------------------------------
# 1. state and field behind a profiled call; the call after it
# ---------------------------------------------------------------------------
CASES = [(128, 'fast', 'float64', 20), (1024, 'fast', 'float64', 12), (100, 'chirp', 'float64', 12),
         (24, 'direct', 'float64', 12), (256, 'fast', 'float32', 12)]


def _tols(N, dtype):
    if dtype == 'float32':
        t = tim.f32_tols('fixed', N)
        return dict(rtol_U=t['rtol_U'], rtol_spec=t['rtol_spec'], rtol_time=t['rtol_time'])
    return {}


@pytest.mark.parametrize("N,engine,dtype,n", CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_state_and_field_behind_a_profiled_call(gpu, N, engine, dtype, n):
    """prepare(), then profile_steps(n): computed_steps, stop_reason, tau0 and skip_check are the oracle's behind the same
    n steps, t0, time_delta_sum, time_passed and delt to 1e-12, the field to RTOL pointwise and in spectrum (fp32: the
    fixed-dt tolerances of N = 256).  Oracle: n + 3 steps, shared with the test below."""
    want = tim.oracle_snaps(N, (n + 1, K))[0]
    s, eng = engine_of(N, engine, dtype)
    ms, calls = eng.profile_steps(n)
    assert want['steps'] == n + 1 and want['stop'] == 'None'
    worst = compare_state_and_field(state_of(eng), eng.get_U(), want, **_tols(N, dtype))
    check_numbers(eng, ms, calls, n)
    log_line(f"profile steps: state and field N={N} {engine} {dtype} n={n}: {fmt_errs(worst)}")
    s.close(fetch_U=False)


FOLLOW = [(128, 'fast', 20), (1024, 'fast', 12), (100, 'chirp', 12), (24, 'direct', 12)]


@pytest.mark.parametrize("rederive", [False, True], ids=['default', 'rederive-hat'])
@pytest.mark.parametrize("N,engine,n", FOLLOW, ids=[f"N{c[0]}-{c[1]}" for c in FOLLOW])
def test_the_call_behind_a_profiled_call(gpu, N, engine, n, rederive):
    """profile_steps(n), then an ordinary step_n(3) with the default flags and with CHS_STEP_REDERIVE_HAT: the profiled
    call left no riding tail, the partial sums in one set and `resident` off, so the call enters cold; its three record
    rows, the state and the field behind it are the oracle's for those steps."""
    snaps = tim.oracle_snaps(N, (n + 1, K))
    s, eng = engine_of(N, engine)
    eng.profile_steps(n)
    rows, rc = eng.step_n(K, rederive_hat=rederive)
    assert rc == _lib.CHS_OK and rows.shape == (K, 9)
    worst = compare_rows(rows, snaps[1]['rows'][-K:])
    assert snaps[1]['rows'].shape[0] == 1 + n + K
    worst.update(compare_state_and_field(state_of(eng), eng.get_U(), snaps[1]))
    rows2, rc = eng.step_n(2)                            # ... and leaves the loop where a further call continues
    assert rc == _lib.CHS_OK and rows2.shape == (2, 9) and rows2[0, 0] == rows[-1, 0] + 1
    log_line(f"profile steps: the call behind, N={N} {engine} rederive={rederive}: {fmt_errs(worst)}")
    s.close(fetch_U=False)


def test_profiled_then_ordinary_steps_at_4096(gpu):
    """What bench.py does in order at the headline size: N = 4096 fp64, 6 profiled steps, then 2 ordinary ones.  The
    field behind the profiled call against the oracle's field of that step; rows, state and field behind the ordinary
    call against the end of the oracle's 8-step run -- the run test_per_step_field_of_one_step_continuing_calls pays for
    (13 s when this test runs alone), at that test's tolerances: RTOL pointwise, RTOL_SPEC in spectrum (spectral_err is N/2
    times sharper than the pointwise error; measured 1.6e-9 here)."""
    N, n, k = 4096, 6, 2
    snap, fields = tim.oracle_per_step(N, n + k)
    s, eng = engine_of(N, 'fast')
    ms, calls = eng.profile_steps(n)
    got = state_of(eng)
    assert got['steps'] == n + 1 and got['stop'] == 'None'
    U = eng.get_U()
    eu, es = relerr(U, fields[n + 1]), spectral_err(U, fields[n + 1])
    assert eu <= RTOL and es <= tim.RTOL_SPEC, (eu, es)
    assert calls[SLOT_SPEC] == n and calls[SLOT_INV] == n
    check_numbers(eng, ms, calls, n)
    del U
    rows, rc = eng.step_n(k)
    assert rc == _lib.CHS_OK and snap['rows'].shape[0] == 1 + n + k
    worst = compare_rows(rows, snap['rows'][-k:])
    worst.update(compare_state_and_field(state_of(eng), eng.get_U(), snap, rtol_spec=tim.RTOL_SPEC))
    log_line(f"profile steps: N={N} fp64, {n} profiled then {k} ordinary: U behind the profile {eu:.2e} spec {es:.2e}; {fmt_errs(worst)}")
    s.close(fetch_U=False)
    tim._PER_STEP.clear()


# ---------------------------------------------------------------------------
# 2. adaptive; a stop inside the call
# ---------------------------------------------------------------------------
def test_adaptive_profiled_call(gpu):
    """N = 1024 fp64 seeded at step 499, adaptive: under a profile `decide` is off and every firing step reduces and
    launches its tail.  delt, state and field behind profile_steps(8) against the oracle.  Oracle: 8 steps."""
    N, n = 1024, 8
    kw = dict(adaptive_time=True, delt_max=4.9e-7 / N)
    want = tim.oracle_snaps(N, (n,), 499, **kw)[0]
    assert want['steps'] == 499 + n and len(np.unique(want['rows'][1:, 8])) >= 3       # the rule fired
    s, eng = engine_of(N, 'fast', seed=499, **kw)
    ms, calls = eng.profile_steps(n)
    worst = compare_state_and_field(state_of(eng), eng.get_U(), want)
    assert state_of(eng)['delt'] != make(N, 2).delt
    check_numbers(eng, ms, calls, n)
    assert calls[SLOT_SPEC] == n
    log_line(f"profile steps: adaptive N={N} from 499, n={n}: {fmt_errs(worst)}")
    s.close(fetch_U=False)


def test_a_stop_inside_a_profiled_call(gpu):
    """N = 256 fp64, full_sim=False and the time limit of test_fp32_time_limit_mid_call (8.5 steps): profile_steps(10)
    ends at step 9 with `time-limit` like the oracle's call, and the field is that of the last completed step."""
    N = 256
    kw = dict(full_sim=False, time_max=8.5 * 3e-8 / tim.M_TILDE / 60)
    want = tim.oracle_snaps(N, (11,), **kw)[0]
    assert (want['steps'], want['stop']) == (9, 'time-limit')
    s, eng = engine_of(N, 'fast', **kw)
    ms, calls = eng.profile_steps(10)
    worst = compare_state_and_field(state_of(eng), eng.get_U(), want)
    check_numbers(eng, ms, calls, 10)
    log_line(f"profile steps: time limit inside the call N={N}: {fmt_errs(worst)}")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. the numbers it returns
# ---------------------------------------------------------------------------
NUMBERS = [(128, 'fast', 20), (1024, 'fast', 12), (100, 'chirp', 12), (24, 'direct', 12)]


@pytest.mark.parametrize("N,engine,n", NUMBERS, ids=[f"N{c[0]}-{c[1]}" for c in NUMBERS])
def test_the_numbers_a_profiled_call_returns(gpu, N, engine, n):
    """Slot names, finite times, the counts of a fixed-dt call -- one column pass per step, at least one row kernel per
    step -- a second call that counts from zero again, and sum(ms) against the call's own time."""
    s, eng = engine_of(N, engine)
    ms, calls = eng.profile_steps(n)
    excess = check_numbers(eng, ms, calls, n)
    assert calls[SLOT_SPEC] == n
    if engine == 'fast':
        names = eng.kernel_names()
        assert names[SLOT_SPEC] == 'k_col' and names[SLOT_MU] == 'k_row_fwd (prologue)' and names[SLOT_INV] == 'k_row_inv (fused)'
        assert calls[SLOT_MU] + calls[SLOT_INV] + calls[SLOT_DIAG] >= n and calls[SLOT_FWD] == 0
        # (chs_fast_step under a profile: the first step's k_pre, then k_col, the row kernel and the tail of every step)
        assert calls[SLOT_INV] == calls[SLOT_FIN] == n and calls[SLOT_PRE] == 1
    else:                                                # (one_step of the natural engines: seven launches a step)
        for slot in (SLOT_MU, SLOT_PRE, SLOT_FWD, SLOT_INV, SLOT_DIAG, SLOT_FIN):
            assert calls[slot] == n, (slot, calls[slot])
        assert calls[SLOT_MISC] == 0
    ms2, calls2 = eng.profile_steps(n)                   # counts and times start from zero
    assert np.array_equal(calls2, calls), (calls, calls2)
    excess = max(excess, check_numbers(eng, ms2, calls2, n))
    assert excess <= 0.0, excess
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------
def test_arguments(gpu):
    N = 128
    s = chsimpy_amd.Solver(make(N, 10 ** 6, 'fast'))
    eng = s._get_engine()
    ms = np.full(_lib.CHS_NKERNELS, -1.0)
    calls = np.full(_lib.CHS_NKERNELS, -1, dtype=np.int64)
    m, c = _lib._dptr(ms), _lib._i64ptr(calls)
    assert gpu.chs_profile_steps(None, 1, m, c) == _lib.CHS_EINVAL
    assert gpu.chs_profile_steps(eng._h, 1, None, c) == _lib.CHS_EINVAL
    assert gpu.chs_profile_steps(eng._h, 1, m, None) == _lib.CHS_EINVAL
    assert 'null' in gpu.chs_last_error().decode()
    assert gpu.chs_profile_steps(eng._h, 1, m, c) == _lib.CHS_ESTATE               # not prepared
    with pytest.raises(AssertionError):
        eng.profile_steps(1)
    s.prepare()
    before, U = state_of(eng), eng.get_U()
    assert gpu.chs_profile_steps(eng._h, 0, m, c) == _lib.CHS_OK                   # no steps: nothing counted, nothing moved
    assert not calls.any() and not ms.any()
    assert state_of(eng) == before and np.array_equal(eng.get_U(), U)
    assert gpu.chs_profile_steps(eng._h, -3, m, c) == _lib.CHS_OK and not calls.any()
    assert state_of(eng) == before
    ms2, calls2 = eng.profile_steps(2)                   # ... and the handle steps on from there
    assert calls2[SLOT_SPEC] == 2 and state_of(eng)['steps'] == before['steps'] + 2
    s.close(fetch_U=False)
