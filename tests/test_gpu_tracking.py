"""GPU tests (``-m gpu``) of the droplet tracking on the device (chs_track / chs_batch_track,
chsimpy_amd/csrc/chs_track.hip).

Reference: the numpy model ``tracking.pair_table`` / ``tracking.words_of`` on the fields as downloaded with ``get_U`` at
both looks -- the exact values the device holds, also for fp32 -- with the label images of ``scipy.ndimage.label``
renumbered by ascending `first` (tests/test_components_host.py: reference); tests/test_tracking_host.py holds the model
against plain loops.  Every cell is an integer and every accumulation an integer add: every comparison is for equality
of words, pair table, shape table and component table.

The sizes are the smallest at which each path of the passes can still go wrong: one workgroup, one below / equal to /
one above a tile, more than two tiles a side.  The kernels read int32 images only, so there is no streamed path and no
size above the cache bound."""
import numpy as np
import pytest

from chsimpy_amd import _lib, components, shapes, tracking
from chsimpy_amd.batch import BatchSolver
from gpu_helpers import log_line
import test_gpu_components as tgc
import test_gpu_shapes as tgsh
import test_gpu_spectrum as tgs
import test_components_host as cchost
import test_morphology_host as mh
import test_shapes_host as shost
import test_tracking_host as host

pytestmark = pytest.mark.gpu

T = mh.T
TILE = cchost.tile_from_header()
SIDES = shost.SIDES
engine_of = tgc.engine_of
PATTERNS = 8            # the first few of cchost.patterns: empty, full, the four corners, the two diagonals
W = tracking


class Tracker:
    """Track looks on one engine against the model: fields uploaded once and compared as downloaded, the model's frame
    kept beside the device's."""

    def __init__(self, eng):
        self.eng, self.U, self.Ud, self.frame, self.models = eng, None, None, None, {}

    def put(self, U):
        if self.U is not U:
            self.eng.set_U(U)
            self.U, self.Ud = U, self.eng.get_U()
        return self

    def reset(self):
        self.eng.track_reset()
        self.frame = None

    def model(self, t, conn, side):
        key = (id(self.U), t, conn, side)
        if key not in self.models:
            self.models[key] = (self.U,) + tuple(tgsh.model_of(self.Ud, t, conn, side))   # (U held: its id stays its own)
        return self.models[key][1:]

    def look(self, t, conn, side, keep=True, what=''):
        words, pairs, tab, cctab = self.eng.track_look(t, conn, components.side_code(side), keep)
        what = f"{what} {conn} {side} keep={keep}"
        assert words.dtype == np.int64 and words.shape == (W.CHS_TR_WORDS,) and pairs.dtype == np.int64 and pairs.shape[1] == 3
        mw, mtab, mcctab, labels = self.model(t, conn, side)
        want = W.words_of(mw, self.frame, labels)
        assert np.array_equal(words, want), (what, words, want)
        if self.frame is None:
            assert pairs.shape == (0, 3), what
        else:
            mp = W.pair_table(self.frame, labels)
            assert pairs.shape == mp.shape and np.array_equal(pairs, mp), (what, pairs.shape, mp.shape)
        assert np.array_equal(tab, mtab) and np.array_equal(cctab, mcctab), what
        if keep:
            self.frame = labels
        return words, pairs


def all_ordered_pairs(tr, fields, what):
    """Every ordered pair (A, B) of `fields`, both connectivities and sides: A is kept, every B looks at it with keep=0."""
    for conn in (4, 8):
        for side in SIDES:
            for na, A in fields:
                tr.reset()
                w, _ = tr.put(A).look(T, conn, side, True, f"{what} {na}")
                assert w[W.CHS_TR_HAVE_PREV] == 0
                for nb, B in fields:
                    w, _ = tr.put(B).look(T, conn, side, False, f"{what} {na} -> {nb}")
                    assert w[W.CHS_TR_HAVE_PREV] == 1


# ---------------------------------------------------------------------------
# 1. sizes, patterns and events
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", cchost.tile_sizes(TILE))
def test_patterns_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    tr = Tracker(eng)
    all_ordered_pairs(tr, [(name, U) for name, U, _ in cchost.patterns(N, TILE)[:PATTERNS]], f"N={N}")
    s.close(fetch_U=False)


def test_patterns_on_the_device_fp32(gpu):
    N = max(TILE) + 1
    s, eng = engine_of(N, 'chirp', 'float32')
    tr = Tracker(eng)
    all_ordered_pairs(tr, [(name, U) for name, U, _ in cchost.patterns(N, TILE)[:PATTERNS]], "fp32")
    s.close(fetch_U=False)


@pytest.mark.parametrize("N", [n for n in cchost.tile_sizes(TILE) if n >= host.EVENT_MIN_N])
def test_hand_made_events_on_the_device(gpu, N):
    s, eng = engine_of(N, 'chirp')
    tr = Tracker(eng)
    for name, Xp, Xn, want in host.event_pairs(N):
        Up, Un = mh.field_of(Xp), mh.field_of(Xn)
        for conn in (4, 8):
            tr.reset()
            tr.put(Up).look(T, conn, 'below', True, name)
            prev = tgsh.dev_look(eng, T, conn, 'below', labels=False)
            words, pairs = tr.put(Un).look(T, conn, 'below', True, name)
            now = tgsh.dev_look(eng, T, conn, 'below', labels=False)       # (a shapes look does not disturb the frame)
            t = W.Track(words, pairs, prev, now)
            full = dict.fromkeys(W.KINDS, 0)
            full.update(want)
            assert t.counts() == full, (name, conn)
            b = t.area_budget()
            assert b['vanished'] + b['born'] + b['exchanged'] == b['total'] == int(Xn.sum()) - int(Xp.sum())
    s.close(fetch_U=False)


def test_far_more_keys_in_a_tile_than_slots(gpu):
    """Horizontal against vertical one-pixel stripes at 2 tile + 2, connectivity 4: a full tile holds 32 x 32 + 32 + 32
    keys, more than the sweep's LDS slots, and every counted pixel is a run of its own -- most contributions take the
    global path."""
    N = 2 * max(TILE) + 2
    s, eng = engine_of(N, 'chirp')
    Xp, Xn = host.stripes_pair(N)
    tr = Tracker(eng)
    tr.put(mh.field_of(Xp)).look(T, 4, 'below', True, 'stripes')
    words, pairs = tr.put(mh.field_of(Xn)).look(T, 4, 'below', False, 'stripes')
    h = N // 2
    assert words[W.CHS_TR_PAIRS] == h * h + 2 * h == pairs.shape[0] and words[W.CHS_TR_HEADS] == 3 * h * h
    assert words[W.CHS_TR_SLOTS] == W.slots_of(3 * h * h) and words[W.CHS_TR_OVERLAP] == h * h
    words, pairs = tr.look(T, 4, 'above', False, 'stripes, the other side')
    assert words[W.CHS_TR_HAVE_PREV] == 1 and pairs.shape[0] == words[W.CHS_TR_PAIRS] > 0
    s.close(fetch_U=False)


def test_every_pixel_a_head_and_a_row(gpu):
    """A checkerboard against its complement at connectivity 4: N^2 one-pixel keys."""
    N = 2 * max(TILE) + 2
    s, eng = engine_of(N, 'chirp')
    ii, jj = np.indices((N, N))
    X = (ii + jj) % 2 == 0
    tr = Tracker(eng)
    tr.put(mh.field_of(X)).look(T, 4, 'below', True, 'checkerboard')
    words, pairs = tr.put(mh.field_of(~X)).look(T, 4, 'below', True, 'checkerboard')
    assert words[W.CHS_TR_PAIRS] == words[W.CHS_TR_HEADS] == N * N == pairs.shape[0] and np.all(pairs[:, 2] == 1)
    assert words[W.CHS_TR_OVERLAP] == 0 and words[W.CHS_TR_LOST] == words[W.CHS_TR_GAINED] == N * N // 2
    assert words[W.CHS_TR_SLOTS] == W.slots_of(N * N) == 65536
    words, pairs = tr.look(T, 4, 'below', True, 'the complement against itself')     # the table shrinks again
    assert words[W.CHS_TR_PAIRS] == N * N // 2 and np.array_equal(pairs[:, 0], pairs[:, 1])
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 2. the life of the frame
# ---------------------------------------------------------------------------
def test_frame_life(gpu):
    N = 100
    s, eng = engine_of(N, 'chirp')
    rng = np.random.default_rng(21)
    A, B, C = (shost.special_field(N, rng) for _ in range(3))
    tr = Tracker(eng)
    w, p = tr.put(A).look(T, 4, 'below', True, 'first')
    assert w[W.CHS_TR_HAVE_PREV] == 0 and not np.any(w[17:]) and p.shape == (0, 3)
    first = tr.frame
    # keep=0 leaves the frame: a third look still compares against the first
    w, _ = tr.put(B).look(T, 4, 'below', False, 'second')
    assert w[W.CHS_TR_HAVE_PREV] == 1 and tr.frame is first
    w3, p3 = tr.put(C).look(T, 4, 'below', False, 'third')
    assert w3[W.CHS_TR_PREV_COUNT] == first.max() + 1 and w3[W.CHS_TR_PAIRS] > 10
    # a components and a shapes look in between, with other arguments, do not disturb it; steps and set_U neither
    eng.components(0.3, 8, components.side_code('above'))
    eng.shapes(0.7, 8, components.side_code('above'))
    eng.set_U(B)
    eng.set_U(C)
    w4, p4 = tr.look(T, 4, 'below', False, 'third again')
    assert np.array_equal(w4, w3) and np.array_equal(p4, p3)
    # a different (threshold, connectivity, side) from frame to look is allowed
    for t, conn, side in ((0.3, 8, 'below'), (0.6, 4, 'above'), (T, 8, 'above')):
        w, _ = tr.look(t, conn, side, False, 'other arguments')
        assert w[W.CHS_TR_PREV_COUNT] == first.max() + 1
    tr.look(0.3, 8, 'above', True, 'other arguments, kept')
    w, _ = tr.put(A).look(T, 4, 'below', True, 'against the frame of other arguments')
    assert w[W.CHS_TR_HAVE_PREV] == 1
    # reset drops the frame; the last pair table stays fetchable
    before = eng.track_pairs()
    eng.track_reset()
    assert np.array_equal(eng.track_pairs(), before)
    tr.frame = None
    w, p = tr.look(T, 4, 'below', False, 'after the reset')
    assert w[W.CHS_TR_HAVE_PREV] == 0 and p.shape == (0, 3)
    w, _ = tr.look(T, 4, 'below', False, 'keep=0 without a frame keeps none')
    assert w[W.CHS_TR_HAVE_PREV] == 0
    assert eng.track_ms() >= 0.0 and eng.shapes_ms() >= 0.0 and eng.components_ms() >= 0.0
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 3. an evolved field
# ---------------------------------------------------------------------------
def test_an_evolved_field(gpu):
    N, steps, more = 256, 2000, 200
    s = tgs.solver(N, steps + more + 1, 'fast')
    s.prepare()
    s.solve_or_resume(steps + 1)
    assert s._engine.engine == 'fast' and s.solution.computed_steps == steps + 1
    t = s.params.threshold
    U1 = s._engine.get_U()
    # (one phase is the connected matrix, the other one the droplets in its holes: track the droplets)
    side = max(SIDES, key=lambda sd: int(tgsh.model_of(U1, t, 4, sd)[0][0]))
    code = components.side_code(side)
    first = s.track(side=side)
    assert not first.have_prev and first.now.count > 100
    s.solve_or_resume(more)
    U2 = s._engine.get_U()
    tr = s.track(side=side, keep=False)
    assert tr.have_prev and (tr.steps_prev, tr.steps_now) == (steps + 1, steps + more + 1) and tr.time_now > tr.time_prev > 0
    assert not np.array_equal(U1, U2)
    m1, m2 = tgsh.model_of(U1, t, 4, side), tgsh.model_of(U2, t, 4, side)
    assert np.array_equal(tr.words, W.words_of(m2[0], m1[3], m2[3])) and np.array_equal(tr.pairs, W.pair_table(m1[3], m2[3]))
    for sh, m in ((tr.prev, m1), (tr.now, m2)):
        assert np.array_equal(sh.words, m[0]) and np.array_equal(sh.table, m[1]) and np.array_equal(sh.components.table, m[2])
    assert tr.prev is first.now and tr.now.delx == s.solution.delx
    c, g, b = tr.counts(), tr.growth(), tr.area_budget()
    assert c['continued'] > 100 and c['continued'] == len(g['a']) and b['vanished'] + b['born'] + b['exchanged'] == b['total']
    assert g['dt'] == tr.time_now - tr.time_prev and np.all(np.isfinite(g['radius_rate']))
    # the same look again, and the same sequence of looks again on the downloaded fields: the same bits
    again = s.track(side=side, keep=False)
    assert np.array_equal(again.words, tr.words) and np.array_equal(again.pairs, tr.pairs)
    eng = s._engine
    eng.track_reset()
    eng.set_U(U1)
    w1 = eng.track(t, 4, code, True)
    eng.set_U(U2)
    w2, p2, tab2, _ = eng.track_look(t, 4, code, False)
    assert np.array_equal(w1, first.words) and np.array_equal(w2, tr.words) and np.array_equal(p2, tr.pairs)
    assert np.array_equal(tab2, tr.now.table)
    log_line(f"tracking: evolved N={N}, steps {steps} -> {steps + more}: {tr.prev.count} -> {tr.now.count} droplets, {tr.n_pairs} pairs, "
             f"{tr.n_heads} heads, {tr.n_slots} slots, {c}; track {eng.track_ms():.4f} ms, shapes {eng.shapes_ms():.4f} ms, "
             f"components {eng.components_ms():.4f} ms")
    s.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 4. the run does not notice
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine,calls,seed,kw", tgsh.OBSERVED, ids=[f"N{c[0]}-{c[1]}" for c in tgsh.OBSERVED])
def test_a_look_between_calls_does_not_change_the_run(gpu, N, engine, calls, seed, kw):
    """Calls with track() between them against the same calls with get_U() between them: all nine record columns, the
    state and the final field, bit for bit."""
    seen = []
    got, Ug = tgs._observed_run(N, engine, calls, lambda s: seen.append(s.track(connectivity=8).have_prev), seed, **kw)
    ref, Ur = tgs._observed_run(N, engine, calls, lambda s: s._engine.get_U(), seed, **kw)
    assert seen == [False] + [True] * len(calls)
    for (rg, sg), (rr, sr) in zip(got, ref):
        assert rg.shape == rr.shape
        for c in range(9):
            assert np.array_equal(rg[:, c], rr[:, c]), c
        assert sg == sr
    assert np.array_equal(Ug, Ur)


# ---------------------------------------------------------------------------
# 5. codes and states
# ---------------------------------------------------------------------------
def test_errors_are_those_of_shapes(gpu):
    s = tgs.solver(128, 4, 'fast')
    eng = s._get_engine()
    out = np.zeros(_lib.CHS_TR_WORDS, dtype=np.int64)
    sho = np.zeros(_lib.CHS_SH_WORDS, dtype=np.int64)
    rows = np.zeros((128 * 128, 3), dtype=np.int64)
    ms = np.zeros(1)
    o, so, rw = _lib._i64ptr(out), _lib._i64ptr(sho), _lib._i64ptr(rows)

    def both(*args):
        """The code of chs_track, which must be that of chs_shapes with the same arguments."""
        rt = gpu.chs_track(eng._h, *args, 1, o)
        assert rt == gpu.chs_shapes(eng._h, *args, so)
        return rt

    assert both(0.5, 4, 0) == _lib.CHS_ESTATE                                               # no field yet
    assert gpu.chs_track_pairs(eng._h, 0, rw) == _lib.CHS_ESTATE                            # no look yet
    assert gpu.chs_track_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE
    assert gpu.chs_track_reset(eng._h) == _lib.CHS_OK                                       # (nothing to drop)
    with pytest.raises(AssertionError):
        s.track()
    s.prepare()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert both(bad, 4, 0) == _lib.CHS_EINVAL and 'finite' in gpu.chs_last_error().decode()
    for conn in (0, 6, -4, 16):
        assert both(0.5, conn, 0) == _lib.CHS_EINVAL and 'connectivity' in gpu.chs_last_error().decode()
    for side in (2, -1):
        assert both(0.5, 4, side) == _lib.CHS_EINVAL
    assert both(float('nan'), 5, 2) == _lib.CHS_EINVAL and 'finite' in gpu.chs_last_error().decode()   # the same order
    assert gpu.chs_track(eng._h, 0.5, 4, 0, 1, None) == _lib.CHS_EINVAL
    assert gpu.chs_track(eng._h, float('nan'), 4, 0, 1, None) == _lib.CHS_EINVAL and 'null' in gpu.chs_last_error().decode()
    assert gpu.chs_track(None, 0.5, 4, 0, 1, o) == _lib.CHS_EINVAL and gpu.chs_track_pairs(None, 0, rw) == _lib.CHS_EINVAL
    assert gpu.chs_track_reset(None) == _lib.CHS_EINVAL
    assert gpu.chs_track_last_ms(eng._h, None) == _lib.CHS_EINVAL and gpu.chs_track_last_ms(None, _lib._dptr(ms)) == _lib.CHS_EINVAL
    assert gpu.chs_track_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_ESTATE                  # none of them was a look
    assert gpu.chs_track_pairs(eng._h, 0, rw) == _lib.CHS_ESTATE
    t = float(np.median(eng.get_U()))
    assert gpu.chs_track(eng._h, t, 4, 0, 1, o) == _lib.CHS_OK and out[W.CHS_TR_HAVE_PREV] == 0
    assert gpu.chs_track_pairs(eng._h, 0, rw) == _lib.CHS_OK and gpu.chs_track_pairs(eng._h, 1, rw) == _lib.CHS_EINVAL
    s.solve_or_resume(3)
    assert gpu.chs_track(eng._h, t, 4, 0, 1, o) == _lib.CHS_OK and out[W.CHS_TR_HAVE_PREV] == 1
    P = int(out[W.CHS_TR_PAIRS])
    assert P > 0 and gpu.chs_track_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] >= 0.0
    for n in (P - 1, P + 1, -1):
        assert gpu.chs_track_pairs(eng._h, n, rw) == _lib.CHS_EINVAL
    assert gpu.chs_track_pairs(eng._h, P, None) == _lib.CHS_EINVAL
    # a refused call leaves the last pair table, the last time and the frame
    last, kept = ms[0], out.copy()
    assert gpu.chs_track(eng._h, float('inf'), 4, 0, 1, o) == _lib.CHS_EINVAL and gpu.chs_track(eng._h, t, 5, 0, 1, o) == _lib.CHS_EINVAL
    assert gpu.chs_track_pairs(eng._h, P, rw) == _lib.CHS_OK
    assert int(rows[:P, 2].sum()) == int(out[W.CHS_TR_OVERLAP] + out[W.CHS_TR_LOST] + out[W.CHS_TR_GAINED])
    assert gpu.chs_track_last_ms(eng._h, _lib._dptr(ms)) == _lib.CHS_OK and ms[0] == last
    assert gpu.chs_track(eng._h, t, 4, 0, 0, o) == _lib.CHS_OK and out[W.CHS_TR_HAVE_PREV] == 1
    assert out[W.CHS_TR_PREV_COUNT] == kept[0] and out[W.CHS_TR_LOST] == out[W.CHS_TR_GAINED] == 0   # the frame is the last look's
    with pytest.raises(ValueError):
        s.track(connectivity=5)
    with pytest.raises(ValueError):
        s.track(side='left')
    with pytest.raises(ValueError):
        s.track()                                            # a frame this Solver did not take
    assert not s.track(reset=True).have_prev and s.track().have_prev
    s.close(fetch_U=False)

    bs = BatchSolver(tgs._members(128, 2, 10))
    b = bs._get_batch()
    assert gpu.chs_batch_track(b._h, 0, 0.5, 4, 0, 1, o) == _lib.CHS_ESTATE == gpu.chs_batch_shapes(b._h, 0, 0.5, 4, 0, so)
    assert gpu.chs_batch_track_pairs(b._h, 0, rw) == _lib.CHS_ESTATE
    bs.prepare()
    for member in (2, -1, 65536):
        assert gpu.chs_batch_track(b._h, member, 0.5, 4, 0, 1, o) == _lib.CHS_EINVAL, member
        assert gpu.chs_batch_track_reset(b._h, member) == _lib.CHS_EINVAL, member
    for args in ((float('nan'), 4, 0), (0.5, 5, 0), (0.5, 8, 3)):
        assert gpu.chs_batch_track(b._h, 1, *args, 1, o) == _lib.CHS_EINVAL == gpu.chs_batch_shapes(b._h, 1, *args, so)
    assert gpu.chs_batch_track(b._h, 1, 0.5, 8, 1, 1, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_track(None, 1, 0.5, 8, 1, 1, o) == _lib.CHS_EINVAL and gpu.chs_batch_track_pairs(None, 0, rw) == _lib.CHS_EINVAL
    assert gpu.chs_batch_track_reset(None, 0) == _lib.CHS_EINVAL and gpu.chs_batch_track_reset(b._h, 1) == _lib.CHS_OK
    assert gpu.chs_batch_track_pairs(b._h, 0, rw) == _lib.CHS_ESTATE                         # none of them was a look
    assert gpu.chs_batch_track(b._h, 1, 0.5, 8, 1, 1, o) == _lib.CHS_OK and out[W.CHS_TR_HAVE_PREV] == 0
    assert gpu.chs_batch_track(b._h, 1, 0.5, 8, 1, 1, o) == _lib.CHS_OK and out[W.CHS_TR_HAVE_PREV] == 1
    P = int(out[W.CHS_TR_PAIRS])
    assert gpu.chs_batch_track_pairs(b._h, P + 1, rw) == _lib.CHS_EINVAL and gpu.chs_batch_track_pairs(b._h, P, None) == _lib.CHS_EINVAL
    assert gpu.chs_batch_track_pairs(b._h, P, rw) == _lib.CHS_OK and np.array_equal(rows[:P, 0], rows[:P, 1])
    bs.close(fetch_U=False)


# ---------------------------------------------------------------------------
# 6. batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,engine", [(128, 'fast'), (100, 'chirp')])
def test_batch_members_keep_their_own_frames(gpu, N, engine):
    """Two members tracked alternately: each look equals the member's single handle on the same fields."""
    B = 2
    ps = tgs._members(N, B, 100)
    for p in ps:
        p.engine = engine
    bs = BatchSolver(ps)
    bs.prepare()
    assert bs._batch.engine == engine
    bs.solve_or_resume(20)
    singles = [engine_of(N, engine) for _ in range(B)]
    ts = None
    for step in range(3):
        fields = [s._engine.get_U() for s in bs.solvers]
        if ts is None:
            ts = [float(np.median(f)) for f in fields]        # a two-phase picture of every member
        for m in (0, 1) if step != 1 else (1, 0):             # alternately, in changing order
            tr = bs.track(m, threshold=ts, connectivity=8)
            eng = singles[m][1]
            eng.set_U(fields[m])
            w, p, tab, cctab = eng.track_look(ts[m], 8, 0, True)
            assert np.array_equal(tr.words, w) and np.array_equal(tr.pairs, p), (step, m)
            assert np.array_equal(tr.now.table, tab) and np.array_equal(tr.now.components.table, cctab), (step, m)
            assert tr.have_prev == (step > 0) and tr.now.count > 1
            if step > 0:
                assert tr.prev_count == tr.prev.count and tr.n_pairs >= max(tr.prev.count, tr.now.count)
        bs.solve_or_resume(10)
    both = bs.track(threshold=ts, connectivity=8, keep=False)                  # all members, member by member
    assert len(both) == B and all(t.have_prev for t in both) and not np.array_equal(both[0].pairs, both[1].pairs)
    one = bs.track(0, threshold=ts, connectivity=8, keep=False, reset=True)    # the reset is that member's alone
    assert not one.have_prev and bs.track(1, threshold=ts, connectivity=8, keep=False).have_prev
    for s, _ in singles:
        s.close(fetch_U=False)
    bs.close(fetch_U=False)
