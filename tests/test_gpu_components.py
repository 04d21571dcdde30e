"""GPU tests (``-m gpu``) of the connected components of the thresholded field labelled on the device (chs_components /
chs_batch_components, chsimpy_amd/csrc/chs_components.hip).

Reference: ``scipy.ndimage.label`` with the 4- or 8-structure on the foreground of the field as downloaded with
``get_U`` -- the exact values the device holds, also for fp32 -- its labels renumbered by ascending `first`, areas from
np.bincount, boxes from ndimage.find_objects (tests/test_components_host.py: reference, check_look).  Everything is
integer: every comparison is for equality of summary, table and labels.

``TR x TC`` is the tile a workgroup labels in LDS (``_lib.CC_TILE``); the pattern sizes are the smallest at which each
phase can still go wrong: one workgroup, one below / equal to / one above a tile, more than two tiles a side."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, components, experiment as ex, morphology
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import make
import test_gpu_spectrum as tgs
import test_components_host as host
import test_morphology_host as mh

pytestmark = pytest.mark.gpu

T = host.T
TILE = host.tile_from_header()        # (the library's own is checked against it below)
SIDES = ('below', 'above')


def engine_of(N, engine, dtype='float64'):
    s = chsimpy_amd.Solver(make(N, 2, engine, dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == engine
    return s, eng


def dev_look(eng, t, conn, side, table=True, labels=True):
    words, tab, lab = eng.components_look(t, conn, components.side_code(side), table, labels)
    return components.Components(words, eng.N, t, conn, side, table=tab, labels=lab)


def fg_of(Ud, t, side):
    X = np.nan_to_num(Ud, nan=np.inf) < t
    return X if side == 'below' else ~X


# ---------------------------------------------------------------------------
# 1. patterns
# ---------------------------------------------------------------------------
def test_the_tile_is_the_headers(gpu):
    assert _lib.CC_TILE == TILE


@pytest.mark.parametrize("N", host.tile_sizes(TILE))
def test_patterns_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')

    def look(U, t, conn, side):
        if look.U is not U:
            eng.set_U(U)
            look.U = U
        return dev_look(eng, t, conn, side)
    look.U = None
    for name, U, want in host.patterns(N, TILE):
        host.check_pattern(look, name, U, want, N)
    for name, U, t, _ in mh.hand_made(N):               # the threshold, NaN and one-ulp fields, on both sides
        for conn in (4, 8):
            for side in SIDES:
                host.check_look(look(U, t, conn, side), fg_of(U, t, side), conn, f"{name} N={N} {conn} {side}")
    s.close(fetch_U=False)


def test_patterns_on_the_device_fp32(gpu):
    N = max(TILE) + 1                                    # (no multiple of four: the element loads; two tiles a side)
    s, eng = engine_of(N, 'chirp', 'float32')

    def look(U, t, conn, side):
        if look.U is not U:
            eng.set_U(U)
            look.U = U
            assert np.array_equal(eng.get_U() < t, U < t)
        return dev_look(eng, t, conn, side)
    look.U = None
    for name, U, want in host.patterns(N, TILE):
        host.check_pattern(look, name, U, want, N)
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. random fields: every load path, engine and element type
# ---------------------------------------------------------------------------
RANDOM_CASES = [(8, 'chirp', 'float64'), (100, 'chirp', 'float32'), (129, 'chirp', 'float32'), (512, 'fast', 'float32'),
                (513, 'chirp', 'float64'), (100, 'direct', 'float64')]


@pytest.mark.parametrize("N,engine,dtype", RANDOM_CASES, ids=[f"N{c[0]}-{c[1]}-{c[2]}" for c in RANDOM_CASES])
def test_random_fields(gpu, N, engine, dtype):
    s, eng = engine_of(N, engine, dtype)
    rng = np.random.default_rng(11 * N + len(engine))
    for conn in (4, 8):
        for density in (0.3, 0.5, 0.593 if conn == 4 else 0.407):
            U = mh.field_of(rng.random((N, N)) < density)
            k = max(2, N // 16)
            U[rng.integers(0, N, k), rng.integers(0, N, k)] = T     # a few pixels at the threshold: background below
            eng.set_U(U)
            Ud = eng.get_U()
            assert np.array_equal(Ud == T, U == T)
            for side in SIDES:
                co = dev_look(eng, T, conn, side)
                host.check_look(co, fg_of(Ud, T, side), conn, f"N={N} {engine} {dtype} {density} {conn} {side}")
                assert co.count > 0
    assert eng.components_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. every XCD at work
# ---------------------------------------------------------------------------
def test_a_large_random_field(gpu):
    """4096 tiles on every XCD, at the site-percolation threshold: clusters of every size, chains across many tiles."""
    N = 4096
    s, eng = engine_of(N, 'fast')
    U = mh.field_of(np.random.default_rng(4096).random((N, N)) < 0.593)
    eng.set_U(U)
    co = dev_look(eng, T, 4, 'below', labels=False)
    host.check_look(co, U < T, 4, 'N=4096 0.593')
    assert co.count > 100000 and co.largest > 100000
    s.close(fetch_U=False)


def test_a_large_serpentine(gpu):
    """One component whose chain runs through every one of 33 x 33 tiles, fp32, element loads, connectivity 8."""
    N = 2049
    s, eng = engine_of(N, 'chirp', 'float32')
    ii, jj = np.indices((N, N))
    X = (ii % 2 == 0) | ((ii % 2 == 1) & (jj == np.where((ii // 2) % 2 == 0, N - 1, 0)))
    eng.set_U(mh.field_of(X))
    co = dev_look(eng, T, 8, 'below')
    assert co.count == 1 and co.spanning == 1 and co.area == int(X.sum())
    host.check_look(co, X, 8, 'serpentine N=2049')
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. the Euler identities against the morphology of the same handle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_euler_identities_after_a_run(gpu, N, engine):
    steps = 40
    s = tgs.solver(N, steps + 1, engine)
    s.prepare()
    sol = s.solve_or_resume()
    assert s._engine.engine == engine and sol.computed_steps == steps + 1
    mo = s.morphology()
    look = {(c, sd): s.components(connectivity=c, side=sd, labels=True) for c in (4, 8) for sd in SIDES}
    assert mo.euler8 == look[8, 'below'].count - look[4, 'above'].inner
    assert mo.euler4 == look[4, 'below'].count - look[8, 'above'].inner
    for c in (4, 8):
        assert look[c, 'below'].area == mo.n_A and 0 < mo.n_A < N * N
        assert look[c, 'below'].area + look[c, 'above'].area == N * N
        for sd in SIDES:
            co = look[c, sd]
            assert co.threshold == s.params.threshold and co.N == N and co.delx == sol.delx
            host.check_look(co, fg_of(sol.U, s.params.threshold, sd), c, f"after a run N={N} {c} {sd}")
            assert np.array_equal(co.radius_eq, np.sqrt(co.areas / np.pi) * sol.delx)
    lower = s.components(s.params.threshold - 1e-3, table=False)          # an explicit threshold, summary only
    assert lower.areas is None and lower.labels is None and lower.area <= mo.n_A
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 5. determinism; a look changes nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp'), (1024, 'fast')])
def test_two_looks_give_the_same_bits(gpu, N, engine):
    s = tgs.solver(N, 8, engine)
    s.prepare()
    s.solve_or_resume(4)
    t = float(np.median(s._engine.get_U()))              # a two-phase picture whatever the run has done so far
    a, b = s.components(t, labels=True), s.components(t, labels=True)
    assert a.count > 1 and np.array_equal(a.words, b.words) and np.array_equal(a.table, b.table) and np.array_equal(a.labels, b.labels)
    c = s.components(t, connectivity=8, labels=True)
    assert c.count <= a.count and c.area == a.area
    s.close(fetch_U=False)


@pytest.mark.parametrize("N,engine,calls,seed,kw", tgs.OBSERVE_CASES,
                         ids=[f"N{c[0]}-{c[1]}" + ('-adaptive' if c[4] else '') for c in tgs.OBSERVE_CASES])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with components() between them against the same calls with get_U() between them: all nine record columns,
    the state and the final field, bit for bit."""
    got, Ug = tgs._observed_run(N, engine, calls, lambda s: s.components(), seed, **kw)
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
    """A call that the time limit ended leaves the device's halt flag set.  The look does not read it: the components are
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

    co, got, t = run(lambda s: s.components(labels=True))
    U, ref, _ = run(lambda s: s._engine.get_U())
    host.check_look(co, U < t, 4, f"behind a stopped call N={N}")
    assert 0 < co.area < N * N
    assert got[0] == ref[0] and got[3] == ref[3]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


# ---------------------------------------------------------------------------
# 6. batches
# ---------------------------------------------------------------------------
def _same(a, b):
    return (np.array_equal(a.words, b.words) and np.array_equal(a.table, b.table)
            and (a.labels is None or b.labels is None or np.array_equal(a.labels, b.labels)))


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
    cos = bs.components(labels=True)                     # every member at its own threshold
    assert len(cos) == B and [co.threshold for co in cos] == ts
    fields = [s._engine.get_U() for s in bs.solvers]
    for m in range(B):
        host.check_look(cos[m], fields[m] < ts[m], 4, f"member {m}")
        assert _same(bs.components(m, labels=True), cos[m]), m                  # member = m
        assert _same(bs.solvers[m].components(labels=True), cos[m]), m          # through the member's Solver
        assert 0 < cos[m].area < N * N
    assert not np.array_equal(cos[0].words, cos[1].words)
    same = bs.components(threshold=ts[1], connectivity=8, side='above')          # one threshold for all
    for m in range(B):
        host.check_look(same[m], ~(fields[m] < ts[1]), 8, f"member {m} above")
    assert _same(bs.components(2, threshold=ts), cos[2])
    with pytest.raises(ValueError):
        bs.components(threshold=[0.5])
    bs.solve_or_resume(5)
    looked = tgs._batch_snap(bs)
    bs.close(fetch_U=False)
    for m, p in enumerate(ps):                           # the three single Solvers run the same way
        s = chsimpy_amd.Solver(p)
        s.rederive_hat = True
        s.prepare()
        s.solve_or_resume(20)
        assert _same(s.components(labels=True), cos[m]), m
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
# 7. errors
# ---------------------------------------------------------------------------
def test_errors(gpu):
    s = tgs.solver(128, 4, 'fast')
    eng = s._get_engine()
    out = np.zeros(_lib.CHS_CC_WORDS, dtype=np.int64)
    lab = np.zeros((128, 128), dtype=np.int32)
    tab = np.zeros((128 * 128, _lib.CHS_CC_COLS), dtype=np.int32)
    ms = np.zeros(1)
    o, l, tb = _lib._i64ptr(out), _lib._i32ptr(lab), _lib._i32ptr(tab)
    assert gpu.chs_components(eng._h, 0.5, 4, 0, o) == _lib.CHS_ESTATE                       # no field yet
    for call in (lambda: gpu.chs_components_table(eng._h, 0, tb), lambda: gpu.chs_components_labels(eng._h, l),
                 lambda: gpu.chs_components_last_ms(eng._h, _lib._dptr(ms))):
        assert call() == _lib.CHS_ESTATE                                                    # no look yet
    with pytest.raises(AssertionError):
        s.components()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert gpu.chs_components(eng._h, bad, 4, 0, o) == _lib.CHS_EINVAL
        assert 'finite' in gpu.chs_last_error().decode()
    for conn in (0, 6, -4, 16):
        assert gpu.chs_components(eng._h, 0.5, conn, 0, o) == _lib.CHS_EINVAL
        assert 'connectivity' in gpu.chs_last_error().decode()
    for side in (2, -1):
        assert gpu.chs_components(eng._h, 0.5, 4, side, o) == _lib.CHS_EINVAL
    assert gpu.chs_components(eng._h, 0.5, 4, 0, None) == _lib.CHS_EINVAL
    assert gpu.chs_components(None, 0.5, 4, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_components_table(None, 0, tb) == _lib.CHS_EINVAL
    assert gpu.chs_components_labels(None, l) == _lib.CHS_EINVAL
    assert gpu.chs_components_last_ms(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_components_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE             # none of them was a look
    assert gpu.chs_components_labels(eng._h, l) == _lib.CHS_ESTATE
    assert gpu.chs_components(eng._h, float(np.median(eng.get_U())), 4, 0, o) == _lib.CHS_OK
    C = int(out[0])
    assert C > 0 and gpu.chs_components_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for rows in (C - 1, C + 1, -1):
        assert gpu.chs_components_table(eng._h, rows, tb) == _lib.CHS_EINVAL
    assert gpu.chs_components_table(eng._h, C, None) == _lib.CHS_EINVAL
    assert gpu.chs_components_labels(eng._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_components_table(eng._h, C, tb) == _lib.CHS_OK and gpu.chs_components_labels(eng._h, l) == _lib.CHS_OK
    assert lab.max() == C - 1 and int(tab[:C, 1].sum()) == int(out[1])
    with pytest.raises(ValueError):
        s.components(connectivity=5)
    with pytest.raises(ValueError):
        s.components(side='left')
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_components(b._h, 0, 0.5, 4, 0, o) == _lib.CHS_ESTATE                # no fields yet
    assert gpu.chs_batch_components_table(b._h, 0, tb) == _lib.CHS_ESTATE
    assert gpu.chs_batch_components_labels(b._h, l) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, -2, 65536):
        assert gpu.chs_batch_components(b._h, member, 0.5, 4, 0, o) == _lib.CHS_EINVAL, member
    assert gpu.chs_batch_components(b._h, 1, float('nan'), 4, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components(b._h, 1, 0.5, 5, 0, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components(b._h, 1, 0.5, 8, 3, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components(b._h, 1, 0.5, 8, 1, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components(None, 1, 0.5, 8, 1, o) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components_table(None, 0, tb) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components_labels(None, l) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components_table(b._h, 0, tb) == _lib.CHS_ESTATE                    # none of them was a look
    assert gpu.chs_batch_components(b._h, 1, 0.5, 8, 1, o) == _lib.CHS_OK
    C = int(out[0])
    assert gpu.chs_batch_components_table(b._h, C + 1, tb) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components_table(b._h, C, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components_labels(b._h, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_components_table(b._h, C, tb) == _lib.CHS_OK and gpu.chs_batch_components_labels(b._h, l) == _lib.CHS_OK
    assert out[1] == int((~(bs.solvers[1]._engine.get_U() < 0.5)).sum())
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 8. experiment
# ---------------------------------------------------------------------------
def test_experiment_droplets_batch_equals_member_path(gpu, tmp_path, capsys):
    """`-N 136 -R 4 -n 80 --droplets` one by one and with `--batch 2` write identical -droplets.csv, their -results.csv
    is byte for byte that of a run without the flag, and without the flag no such file appears."""
    base = ['-N', '136', '-R', '4', '-n', '80']
    ex.main(base + ['--concurrent', '1', '--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--concurrent', '1', '--droplets', '--file-id', str(tmp_path / 'one')])
    capsys.readouterr()
    ex.main(base + ['--batch', '2', '--droplets', '--file-id', str(tmp_path / 'batch')])
    assert 'not taken' not in capsys.readouterr().out
    one, batch = open(tmp_path / 'one-droplets.csv').read(), open(tmp_path / 'batch-droplets.csv').read()
    assert one == batch
    lines = one.splitlines()
    assert lines[0] == ','.join(ex.DROPLETS_COLS) and len(lines) == 5
    for i, ln in enumerate(lines[1:]):
        f = ln.split(',')
        rid, t, conn, cb, lb, sb, mb, ca, la, sa, ma = f
        assert int(rid) == i and int(conn) == 4 and int(cb) >= 1 and int(ca) >= 1
        assert 1 <= int(lb) <= float(mb) * int(cb) < 136 * 136 and 1 <= int(la) <= float(ma) * int(ca) < 136 * 136
        assert round(float(mb) * int(cb)) + round(float(ma) * int(ca)) == 136 * 136      # the two sides fill the grid
        assert int(sb) <= int(cb) and int(sa) <= int(ca)
    assert not (tmp_path / 'plain-droplets.csv').exists()
    plain = open(tmp_path / 'plain-results.csv', 'rb').read()
    assert plain == open(tmp_path / 'one-results.csv', 'rb').read() == open(tmp_path / 'batch-results.csv', 'rb').read()
