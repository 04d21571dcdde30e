"""GPU tests (``-m gpu``) of the engine pool: ``chs_destroy`` parks an engine, ``chs_create`` takes a parked engine of the
same (device, N, dtype, transform engine, eigenvalue table) into use again through ``rearm()`` (chs_api.hip), a hand-kept
list of resets of a struct with about ninety members.  Every ensemble member after a rank's first few, every member of a
batch and every repeated ``Solver`` of a process runs on such an engine.

What is held here: a run on a re-armed engine is the run on an engine created with the pool empty -- every record row,
the field, every word of ``chs_get_state`` (at creation and behind every call), the host generator's state, every look's
result and the errors a handle without a look answers with -- whatever the engine's previous life left behind: an armed
adaptive step, a stop after an odd number of steps, NaN in every buffer, jitter from either generator, a profiled call,
a resident loop, looks of every kind with a kept tracking frame, a batch.  Same library, same device, same launches:
every comparison is ``==`` / ``np.array_equal``, there is no tolerance in this file but the one of the oracle check,
which excludes a reference that is wrong in the same way.  Then the pool's own rules: match key, eviction, size cap,
the environment switch, threads.

Found by this file (profiles/pool_rearm.txt has the resets it was shown to bite on):
  - ``rearm()`` did not forget the structure factor: ``chs_structure_factor_last_ms`` of a re-armed handle answered with
    the previous run's times (test_every_previous_life_then_every_run[F64-looks-V5] and every ``-V5`` case behind a
    previous life with looks)."""
import threading

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib
from gpu_helpers import KAPPA, RTOL, compare_snapshots, fmt_errs, log_line, make, seed_step, snapshot
import test_gpu_issue_modes as tim

pytestmark = pytest.mark.gpu

M_TILDE = tim.M_TILDE
POOL_MAX = 4                                   # CHS_POOL_MAX (chs_api.hip)

# name: (engine, dtype, N) -- the smallest sizes at which each code path exists
CONFIGS = {
    'F64': ('fast', 'float64', 128),           # smallest fast grid; stop rules run the two-buffer hat_U flip
    'F32': ('fast', 'float32', 256),           # packed core
    'G64': ('fast', 'float64', 4096),          # the gate with fixed dt exists from 4096 only; 128 MiB field, still pooled
    'C64': ('chirp', 'float64', 100),          # the reference's smoke size
    'C32': ('chirp', 'float32', 129),          # odd N, fp32 plan
    'D64': ('direct', 'float64', 24),
    'D32': ('direct', 'float32', 24),
}


def _delt_max(cfg):
    """delt_dyn is a column sum and grows with N (test_adaptive_time_fast_engine): the fast grids scale delt_max, the
    natural-order engines' small grids keep the reference's."""
    engine, _, N = CONFIGS[cfg]
    return dict(delt_max=4.9e-7 / N) if engine == 'fast' else {}


def _state(eng):
    st = eng.get_state()
    return {f[0]: getattr(st, f[0]) for f in st._fields_}


def _rng(s):
    return None if s._pcg is None else s._pcg.bit_generator.state


_LIVE = []


def _reset_pool():
    """An empty pool, whatever an earlier test that failed left open (an engine it leaked would be parked whenever the
    garbage collector finds it, in the middle of a later test's counts)."""
    while _LIVE:
        s = _LIVE.pop()
        if hasattr(s, 'solvers'):
            s.close(fetch_U=False)
        elif getattr(s, '_engine', None) is not None:
            s._engine.close()
            s._engine = None
    _lib.pool_clear()
    assert _lib.pool_count() == 0


def _open(p, U_init=None, takes=None):
    """A Solver with its engine forced.  takes=True: a parked engine was taken; False: none was."""
    s = chsimpy_amd.Solver(p, U_init)
    _LIVE.append(s)
    before = _lib.pool_count()
    s._get_engine()
    if takes is not None:
        assert _lib.pool_count() == before - (1 if takes else 0), (before, _lib.pool_count(), takes)
    return s


def same(a, b, path='snapshot'):
    """a == b all the way down: arrays array_equal (NaN equal to NaN), scalars ==, objects by their attributes."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray), path
        assert a.shape == b.shape and a.dtype == b.dtype, (path, a.shape, b.shape, a.dtype, b.dtype)
        eq = np.array_equal(a, b, equal_nan=True) if a.dtype.kind in 'fc' else np.array_equal(a, b)
        assert eq, (path, int(np.sum(a != b)), 'elements differ')
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (path, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            same(a[k], b[k], f'{path}[{k!r}]')
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), (path, a, b)
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f'{path}[{i}]')
    elif hasattr(a, '__dict__') and not isinstance(a, type):
        assert type(a) is type(b), (path, type(a), type(b))
        same(vars(a), vars(b), path + '.')
    elif isinstance(a, float) and a != a:
        assert isinstance(b, float) and b != b, (path, a, b)
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


# ---------------------------------------------------------------------------
# victims: the run that is compared
# ---------------------------------------------------------------------------
VICTIMS = ('V1', 'V2', 'V3', 'V4', 'V5', 'V6')
# V1 fixed dt, full_sim, calls of 5 + 4       V2 full_sim=False, a time limit that stops inside the second call
# V3 adaptive, seeded at 499, 8 steps         V4 jitter 0.02 from the device generator, 6 steps in two calls
# V5 V1, then every look with default arguments
# V6 the C ABI without the Solver: prepare, chs_step_n(4), chs_profile_steps(3) and never a chs_set_jitter_* call (the
#    Solver sets the jitter before every call, which hides a jitter left armed)
_CHUNKS = {'V1': (5, 4), 'V2': (5, 4), 'V3': (8,), 'V4': (4, 3), 'V5': (5, 4)}


def victim_params(cfg, v, seed=2023):
    engine, dtype, N = CONFIGS[cfg]
    kw = dict(dtype=dtype, seed=seed)
    if v == 'V2':
        kw.update(full_sim=False, time_max=6.5 * 3e-8 / M_TILDE / 60)       # 4 steps, then the limit behind 2 more
    if v == 'V3':
        kw.update(adaptive_time=True, **_delt_max(cfg))
    if v == 'V4':
        kw.update(jitter=0.02)
    return make(N, 10 ** 6, engine, **kw)


LOOK_MS = ('structure_factor_ms', 'morphology_ms', 'components_ms', 'distance_ms', 'chords_ms', 'composition_ms',
           'two_point_ms', 'contour_ms', 'shapes_ms', 'track_ms', 'thickness_ms', 'geodesic_ms')
LOOK_FETCHES = (('components_table',), ('components_labels',), ('distance_hist',), ('distance_map',), ('thickness_hist',),
                ('thickness_map',), ('geodesic_hist',), ('geodesic_profile',), ('geodesic_map',), ('chords_hist',),
                ('composition_hist', 15), ('two_point_counts', 4), ('contour_hist', 64), ('contour_map',),
                ('shapes_table',), ('track_pairs',))


def _without_a_look(eng):
    """What a handle answers before its first look: every *_last_ms (all twelve) and every fetch of a table, histogram,
    map, labels or pairs raises 'no ... so far'.  Returns the messages."""
    out = {}
    for call in [(n,) for n in LOOK_MS] + list(LOOK_FETCHES):
        with pytest.raises(AssertionError) as e:
            getattr(eng, call[0])(*call[1:])
        assert 'so far' in str(e.value), (call, str(e.value))
        out[call[0]] = str(e.value)
    return out


def _looks_default(s):
    out = {'none_before': _without_a_look(s._engine)}
    first = s.track()
    assert first.have_prev is False or first.have_prev == 0           # the first track() finds no frame
    out['track_first'] = first
    for name in ('structure_factor', 'morphology', 'composition', 'two_point', 'contour', 'chords', 'components',
                 'distance', 'thickness', 'geodesic', 'shapes', 'track'):
        out[name] = getattr(s, name)()
    assert out['track'].have_prev
    return out


def run_victim(s, v):
    """The victim's run on the Solver s, whose engine exists: everything that is compared."""
    eng = s._engine
    out = dict(engine=eng.engine, created=_state(eng), calls=[], states=[], rng=[_rng(s)])
    if v == 'V6':
        s.prepare()
        rows, rc = eng.step_n(4)
        assert rc == _lib.CHS_OK and rows.shape == (4, 9)
        out['states'].append(_state(eng))
        _, calls = eng.profile_steps(3)
        out.update(rows=rows, profile_calls=calls, U=eng.get_U())
        out['states'].append(_state(eng))
        assert out['states'][-1]['computed_steps'] == 8
        return out
    s.prepare()
    if v == 'V3':
        seed_step(s, 499)
    for c in _CHUNKS[v]:
        s.solve_or_resume(c)
        out['calls'].append(snapshot(s))
        out['states'].append(_state(eng))
        out['rng'].append(_rng(s))
    last = out['calls'][-1]
    if v in ('V1', 'V5'):
        assert (last['steps'], last['stop']) == (9, 'None')
    if v == 'V2':
        assert out['calls'][0]['steps'] == 5 and (last['steps'], last['stop']) == (7, 'time-limit')
    if v == 'V3':
        assert last['steps'] == 507 and len(np.unique(last['rows'][1:, 8])) >= 2          # the rule fired
    if v == 'V4':
        assert last['steps'] == 7
    if v == 'V5':
        out['looks'] = _looks_default(s)
    return out


_FRESH = {}


def fresh(cfg, v, seed=2023):
    """The victim on an engine created with the pool empty, once per (config, victim, seed)."""
    key = (cfg, v, seed)
    if key not in _FRESH:
        _reset_pool()
        s = _open(victim_params(cfg, v, seed), takes=False)
        assert s._engine.engine == CONFIGS[cfg][0]
        _FRESH[key] = run_victim(s, v)
        s.close()
    return _FRESH[key]


def final_U(snap):
    return snap['U'] if 'U' in snap else snap['calls'][-1]['U']


# ---------------------------------------------------------------------------
# dirty runs: named by what they leave behind.  Other constants than any victim's; N and with it the eigenvalue table
# stay.  Each returns its final field, and parks its engine.
# ---------------------------------------------------------------------------
D_DELT, D_MT = 2e-8, 2.3e-8


def dirty_params(cfg, **kw):
    engine, dtype, N = CONFIGS[cfg]
    base = dict(dtype=dtype, seed=7, kappa_tilde=KAPPA * 1.3, delt=D_DELT, threshold=0.87, M_tilde=D_MT)
    base.update(kw)
    return make(N, 10 ** 6, engine, **base)


def _park(s, U=None):
    U = np.array(s.solution.U if U is None else U)
    s.close()
    return U


def d_adaptive_armed(cfg, takes=None, s=None):
    """Leaves dPartColRows, gateSeq, nColMinCur, an adapted delt / lam and csHost."""
    own = s is None
    if own:
        s = _open(dirty_params(cfg, adaptive_time=True, full_sim=False, **_delt_max(cfg)), takes=takes)
        s.prepare()
    seed_step(s, 499)
    sol = s.solve_or_resume(8)
    assert sol.computed_steps == 507 and len(np.unique(sol.timedata.data()[1:, 8])) >= 2     # 500 .. 506: re-evaluated
    return _park(s) if own else None


def d_stopped_odd(cfg, takes=None):
    """Leaves swapped hat_U buffers, halt, stop_reason and a U rebuilt from hat_U."""
    s = _open(dirty_params(cfg, full_sim=False, time_max=3.5 * D_DELT / D_MT / 60), takes=takes)
    s.prepare()
    sol = s.solve_or_resume(10)
    assert (sol.computed_steps, sol.stop_reason) == (4, 'time-limit')       # three completed steps
    return _park(s)


def d_nan(cfg, takes=None):
    """The start field of test_nan_raises_assertion_like_the_reference and two steps on from it (nan_flag, NaN through the
    step's buffers and hat_U), then NaN put into U, MU, T1 and T2 outright."""
    N = CONFIGS[cfg][2]
    U0 = np.full((N, N), 0.875)
    U0[3, 4] = 1.5
    s = _open(dirty_params(cfg), U0, takes=takes)
    with pytest.raises(AssertionError):
        s.prepare()
    eng = s._engine
    rows, rc = eng.step_n(2)
    assert rc == _lib.CHS_ENAN                                       # nan_flag; the step's transforms ran on NaN
    # (the fused fp64 row kernel does not store the field of a step that stops: U itself may still be finite here.)
    # Whatever the engine's kernels left out: a NaN field, and a transform of one through MU, T1 and T2
    nan = np.full((N, N), np.nan)
    assert np.isnan(eng.dctn(nan)).all()
    eng.set_U(nan)
    U = eng.get_U()
    assert np.isnan(U).all()
    s._engine.close()
    s._engine = None
    return U


def d_jitter(cfg, takes=None, device=(False, True)):
    """Leaves dNoise, jitter, jitterPcg and pcgState."""
    s = _open(dirty_params(cfg, jitter=0.02), takes=takes)
    s.prepare()
    for k, dev in enumerate(device):
        s.device_rng = dev
        s.solve_or_resume(4 if k == 0 else 3)
    assert s.solution.computed_steps == 1 + 3 * len(device)
    return _park(s)


def d_jitter_host(cfg, takes=None):
    return d_jitter(cfg, takes, (False,))


def d_jitter_pcg(cfg, takes=None):
    return d_jitter(cfg, takes, (True,))


def _profiled(s):
    ms, calls = s._engine.profile_steps(3)
    assert calls[3] == 3                                             # SLOT_SPEC: one column pass per step


def d_profiled(cfg, takes=None):
    """Leaves the step timer's event pool filled and the issue plan of a profiled call behind."""
    s = _open(dirty_params(cfg), takes=takes)
    s.prepare()
    _profiled(s)
    return _park(s, s._engine.get_U())


def d_resident_odd(cfg, takes=None):
    """Leaves resident, hat_valid, an odd stepCount, and parity wherever it ends."""
    s = _open(dirty_params(cfg), takes=takes)
    s.prepare()
    s.solve_or_resume(4)
    s.solve_or_resume(4)
    assert s.solution.computed_steps == 8                            # 3 + 4 steps
    return _park(s)


def _looks_non_default(s):
    t = 0.8751
    s.structure_factor()
    s.morphology(t)
    s.composition(t, bins=9, range=(0.86, 0.89), quantiles=(0.25,))
    s.two_point(t, rmax=5)
    s.contour(t, bins=16, kmax=0.5, map=True)
    s.chords(t)
    s.components(t, connectivity=8, side='above', labels=True)
    s.distance(t, side='above', map=True)
    s.thickness(t, side='above', map=True)
    s.geodesic(t, connectivity=4, side='above', source='left', map=True)
    s.shapes(t, connectivity=8, side='above')
    a = s.track(t, keep=True)
    s.solve_or_resume(1)
    b = s.track(t, keep=True)                                        # a frame and a pair table exist
    assert not a.have_prev and b.have_prev and s._engine._tr_pairs > 0
    for n in LOOK_MS:
        assert getattr(s._engine, n)() is not None


def d_looks(cfg, takes=None):
    """Leaves the buffers, results and times of every look, and a kept tracking frame."""
    s = _open(dirty_params(cfg), takes=takes)
    s.prepare()
    s.solve_or_resume(11)
    _looks_non_default(s)
    return _park(s)


def d_everything(cfg, takes=None):
    """All of the above on one engine: what is compatible in one life of a handle (its constants are fixed at creation)
    chained there, the lives chained through the pool -- each takes the engine the one before parked.  NaN goes last."""
    s = _open(dirty_params(cfg, adaptive_time=True, full_sim=False, **_delt_max(cfg)), takes=takes)
    s.prepare()
    d_adaptive_armed(cfg, s=s)
    _looks_non_default(s)
    _profiled(s)
    s.close()
    for life in (d_jitter, d_resident_odd, d_stopped_odd, d_nan):
        assert _lib.pool_count() == 1
        U = life(cfg, takes=True)
    return U


DIRTY = dict(adaptive_armed=d_adaptive_armed, stopped_odd=d_stopped_odd, nan=d_nan, jitter_host=d_jitter_host,
             jitter_pcg=d_jitter_pcg, profiled=d_profiled, resident_odd=d_resident_odd, looks=d_looks,
             everything=d_everything)
MIRROR = dict(V1='resident_odd', V2='stopped_odd', V3='adaptive_armed', V4='jitter_pcg', V5='looks', V6='jitter_pcg')


def rearmed(cfg, dirty, v, seed=2023):
    """The victim on the engine the dirty run parked.  Returns (victim's snapshot, dirty run's final field)."""
    _reset_pool()
    dU = DIRTY[dirty](cfg, takes=False)
    assert _lib.pool_count() == 1
    s = _open(victim_params(cfg, v, seed), takes=True)
    assert _lib.pool_count() == 0                 # the parked engine was taken: no new one was quietly built
    snap = run_victim(s, v)
    s.close()
    assert _lib.pool_count() == 1
    return snap, dU


def check_pair(cfg, dirty, v):
    want = fresh(cfg, v)
    got, dU = rearmed(cfg, dirty, v)
    # negative control: the previous life left something that could have shown
    assert not np.array_equal(dU, final_U(want))
    same(got, want)


# ---------------------------------------------------------------------------
# 1. the matrix
# ---------------------------------------------------------------------------
MATRIX = [('F64', d, v) for d in DIRTY for v in VICTIMS]
for _c in ('F32', 'C64', 'C32', 'D64', 'D32'):
    MATRIX += [(_c, 'everything', v) for v in VICTIMS] + [(_c, MIRROR[v], v) for v in VICTIMS]
# the gate of N = 4096 and chs_fast_recover_u; nothing else at this size
MATRIX += [('G64', 'stopped_odd', 'V1'), ('G64', 'stopped_odd', 'V2'), ('G64', 'adaptive_armed', 'V3')]


@pytest.mark.parametrize("cfg,dirty,v", MATRIX, ids=['-'.join(m) for m in MATRIX])
def test_every_previous_life_then_every_run(gpu, cfg, dirty, v):
    """A run on the engine that `dirty` parked is the run on an engine created with the pool empty, in every compared
    bit, and the dirty run's final field is not the victim's."""
    check_pair(cfg, dirty, v)


@pytest.mark.parametrize("cfg", ['F64', 'G64', 'C64', 'D64'])
def test_the_fresh_run_is_the_oracles(gpu, cfg):
    """fresh(config, V1) against the oracle with compare_snapshots at the suite's RTOL = 1e-9: the reference of this
    file is not wrong the way a re-armed engine could be.  (The fp32 fresh runs are held in test_gpu_issue_modes.py.)
    N = 4096: spectral_err is N / 2 times sharper than the pointwise error, and the suite holds every N = 4096 run to
    RTOL pointwise and RTOL_SPEC = 1e-8 in spectrum (test_gpu_issue_modes.py, test_gpu_profile_steps.py: 1.6e-9 measured
    over 8 steps); so does this one (measured here: U 1.7e-15 pointwise, 2.1e-9 in spectrum)."""
    N = CONFIGS[cfg][2]
    want = tim.oracle_snaps(N, _CHUNKS['V1'])
    kw = dict(rtol_spec=tim.RTOL_SPEC) if N >= 4096 else {}
    worst = compare_snapshots(fresh(cfg, 'V1')['calls'], want, rtol=RTOL, **kw)
    log_line(f"pool: fresh V1 against the oracle, {cfg}: {fmt_errs(worst)}")
    for key in [k for k in tim._ORACLE if k[0] >= 4096]:             # (a field of N = 4096 is 134 MB, kept per call)
        del tim._ORACLE[key]


@pytest.mark.parametrize("cfg", ['F64', 'C64'])
def test_twice_rearmed(gpu, cfg):
    """everything, V1, stopped_odd, V1 again: one engine through four lives, the count after every close and create."""
    want = fresh(cfg, 'V1')
    _reset_pool()
    d_everything(cfg, takes=False)
    assert _lib.pool_count() == 1
    for k in range(2):
        s = _open(victim_params(cfg, 'V1'), takes=True)
        assert _lib.pool_count() == 0
        got = run_victim(s, 'V1')
        s.close()
        assert _lib.pool_count() == 1
        same(got, want, f'life {2 * k + 2}')
        if k == 0:
            d_stopped_odd(cfg, takes=True)
            assert _lib.pool_count() == 1


def test_a_rearmed_handle_has_no_field_and_is_not_prepared(gpu):
    """Before chs_set_U a handle from the pool answers like a new one: no field to fetch, to prepare or to look at, and
    no prepared loop to step."""
    def answers(s):
        eng, out = s._engine, []
        for call in (eng.get_U, eng.prepare, lambda: eng.step_n(1), lambda: eng.morphology(0.875), eng.get_mu,
                     lambda: eng.profile_steps(1)):
            with pytest.raises(AssertionError) as e:                 # CHS_ESTATE
                call()
            out.append(str(e.value))
        return out
    _reset_pool()
    s = _open(victim_params('F64', 'V1'), takes=False)
    want = answers(s)
    s._engine.close()
    _reset_pool()
    d_everything('F64', takes=False)
    s = _open(victim_params('F64', 'V1'), takes=True)
    assert answers(s) == want
    s._engine.close()


# ---------------------------------------------------------------------------
# 2. batches
# ---------------------------------------------------------------------------
def test_engines_parked_by_a_batch_serve_single_runs(gpu):
    """The members of an adaptive B = 3 batch are parked by batch_free with their stream swapped back: three single V1
    Solvers each take one (3 -> 0) and equal the fresh run."""
    want = fresh('F64', 'V1')
    _reset_pool()
    ps = [dirty_params('F64', adaptive_time=True, seed=20 + m, **_delt_max('F64')) for m in range(3)]
    bs = chsimpy_amd.BatchSolver(ps)
    _LIVE.append(bs)
    bs.prepare()
    for s in bs.solvers:
        seed_step(s, 499)
    sols = bs.solve_or_resume(8)
    assert all(sol.computed_steps == 507 for sol in sols)
    assert len(np.unique(sols[0].timedata.data()[1:, 8])) >= 2
    dU = np.array(sols[0].U)
    bs.close()
    assert _lib.pool_count() == 3
    singles = []
    for k in range(3):
        singles.append(_open(victim_params('F64', 'V1'), takes=True))
        assert _lib.pool_count() == 2 - k
    assert not np.array_equal(dU, final_U(want))
    for k, s in enumerate(singles):
        same(run_victim(s, 'V1'), want, f'single {k}')
    for s in singles:
        s.close()
    assert _lib.pool_count() == 3


def _batch_run(cfg, parked):
    """A B = 2 batch of V1-like members (two seeds), created with `parked` engines in the pool."""
    ps = [victim_params(cfg, 'V1', seed) for seed in (2023, 11)]
    bs = chsimpy_amd.BatchSolver(ps)
    _LIVE.append(bs)
    assert _lib.pool_count() == parked
    bs._get_batch()
    assert _lib.pool_count() == 0                                    # (a parked engine became one member)
    assert bs._batch.engine == CONFIGS[cfg][0]
    bs.prepare()
    out = []
    for c in _CHUNKS['V1']:
        bs.solve_or_resume(c)
        out.append([dict(snap=snapshot(s), state=_state(s._engine)) for s in bs.solvers])
    bs.close()
    assert _lib.pool_count() == 2
    return out


_BATCH = {}


@pytest.mark.parametrize("dirty", ['everything', 'resident_odd'])
@pytest.mark.parametrize("cfg", ['F64', 'C64'])
def test_a_batch_takes_a_parked_single_engine(gpu, cfg, dirty):
    """One engine parked by a single run -- `everything`, or `resident_odd`, which parks it with `resident` and
    `hat_valid` set: a B = 2 batch takes it for one member (1 -> 0) and equals the same batch built on an empty pool.
    F64: the fast batch; C64: the chirp batch."""
    if cfg not in _BATCH:
        _reset_pool()
        _BATCH[cfg] = _batch_run(cfg, 0)
    want = _BATCH[cfg]
    _reset_pool()
    dU = DIRTY[dirty](cfg, takes=False)
    assert _lib.pool_count() == 1
    got = _batch_run(cfg, 1)
    assert not np.array_equal(dU, want[-1][0]['snap']['U'])
    same(got, want)


# ---------------------------------------------------------------------------
# 3. the pool's own rules
# ---------------------------------------------------------------------------
def _small(N, engine, dtype='float64', takes=None):
    s = _open(make(N, 5, engine, dtype=dtype), takes=takes)
    return s


def _close(s):
    s.prepare()
    s.close(fetch_U=False)


def test_match_key(gpu):
    """Device, N, dtype, transform engine and eigenvalue table make the key: nothing else takes a parked engine."""
    _reset_pool()
    _close(_small(100, 'chirp', takes=False))
    assert _lib.pool_count() == 1
    d = _small(100, 'direct', takes=False)                           # another transform engine
    assert _lib.pool_count() == 1
    _close(d)
    assert _lib.pool_count() == 2
    f = _small(100, 'chirp', 'float32', takes=False)                 # another dtype
    assert _lib.pool_count() == 2
    _close(f)
    assert _lib.pool_count() == 3
    n = _small(101, 'chirp', takes=False)                            # another N
    assert _lib.pool_count() == 3
    _close(n)
    assert _lib.pool_count() == 4
    a = _small(100, 'auto', takes=True)                              # 'auto' below N = 129 is the direct engine
    assert _lib.pool_count() == 3 and a._get_engine().engine == 'direct'
    ref = chsimpy_amd.Solver(make(100, 5, 'chirp'))
    lam = np.array(ref.solution.lam, dtype=np.float64)
    lam[3] = np.nextafter(lam[3], np.inf)                            # one entry of the table, one ulp
    e = _lib.Engine(ref._consts(), lam)
    assert _lib.pool_count() == 3 and e.engine == 'chirp'
    c = _small(100, 'chirp', takes=True)                             # ... and the same table takes it
    assert _lib.pool_count() == 2 and c._engine.engine == 'chirp'
    e.close()
    assert _lib.pool_count() == 3
    _close(a)
    assert _lib.pool_count() == 4
    _close(c)
    assert _lib.pool_count() == POOL_MAX
    _reset_pool()


def test_eviction_is_least_recently_parked(gpu):
    """Five chirp engines of different N parked: four stay, the first-parked one is gone."""
    _reset_pool()
    sizes = (20, 21, 22, 23, 25)
    for k, N in enumerate(sizes):
        _close(_small(N, 'chirp', takes=False))
        assert _lib.pool_count() == min(k + 1, POOL_MAX)
    first = _small(sizes[0], 'chirp', takes=False)                   # gone: a new one is created
    assert _lib.pool_count() == POOL_MAX
    second = _small(sizes[1], 'chirp', takes=True)
    assert _lib.pool_count() == POOL_MAX - 1
    first._engine.close()
    assert _lib.pool_count() == POOL_MAX
    second._engine.close()
    assert _lib.pool_count() == POOL_MAX
    _reset_pool()


def test_an_engine_above_the_field_cap_is_freed(gpu):
    """fast fp32 N = 8192: a field of 256 MiB > CHS_POOL_FIELD_BYTES (160 MiB) is freed on close."""
    _reset_pool()
    _close(_small(100, 'chirp', takes=False))
    assert _lib.pool_count() == 1
    s = _open(make(8192, 3, 'fast', dtype='float32'), takes=False)
    s.prepare()
    sol = s.solve_or_resume(3)                                       # two steps
    assert sol.computed_steps == 3
    s.close(fetch_U=False)
    assert _lib.pool_count() == 1
    _reset_pool()


def test_the_environment_switch(gpu, monkeypatch):
    """CHS_ENGINE_POOL=0: close parks nothing, create takes nothing."""
    _reset_pool()
    monkeypatch.setenv('CHS_ENGINE_POOL', '0')
    _close(_small(100, 'chirp', takes=False))
    assert _lib.pool_count() == 0
    monkeypatch.delenv('CHS_ENGINE_POOL')
    _close(_small(100, 'chirp', takes=False))
    assert _lib.pool_count() == 1
    monkeypatch.setenv('CHS_ENGINE_POOL', '0')
    s = _small(100, 'chirp', takes=False)
    assert _lib.pool_count() == 1
    _close(s)
    assert _lib.pool_count() == 1
    monkeypatch.delenv('CHS_ENGINE_POOL')
    _reset_pool()


def test_threads_create_and_destroy_concurrently(gpu):
    """experiment.py's pattern: three threads, four F64 members each with their own seeds and a mix of V1 / V2 / V4,
    pool on.  Every member equals its sequential fresh run; at most CHS_POOL_MAX engines stay parked."""
    jobs = [[(('V1', 'V2', 'V4')[(t + i) % 3], 100 + 4 * t + i) for i in range(4)] for t in range(3)]
    want = {(v, seed): fresh('F64', v, seed) for job in jobs for v, seed in job}
    _reset_pool()
    got, errors = {}, []

    def work(job):
        try:
            for v, seed in job:
                s = _open(victim_params('F64', v, seed))
                got[(v, seed)] = run_victim(s, v)
                s.close()
        except BaseException as e:                                   # noqa: B902 -- handed to the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(job,)) for job in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    assert 1 <= _lib.pool_count() <= POOL_MAX
    assert sorted(got) == sorted(want)
    for key in want:
        same(got[key], want[key], f'member {key}')
    _reset_pool()
