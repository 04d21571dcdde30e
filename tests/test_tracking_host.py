"""Host side of the droplet tracking (chsimpy_amd/tracking.py): the numpy model of the pair table and of the head count
against plain Python loops, the families of the link graph against scipy's connected components, hand-made pairs of
looks with known events, the stripes whose row and head counts are computed here, the area budget, the growth of a disc,
the consistency checks of `Track`, the header's constants and prototypes.  No device.

`event_pairs`, `stripes_pair`, `label_image` and `loop_pairs` are shared with tests/test_gpu_tracking.py, which puts the
same fields on the device.  Everything in the tables is an integer: every comparison of them is for equality."""
import os
import re

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from chsimpy_amd import _lib, components, shapes, tracking
import test_components_host as cchost
import test_morphology_host as mh
import test_shapes_host as shost

ROOT = cchost.ROOT
T = mh.T
EVENT_MIN_N = 48


def label_image(X, connectivity):
    """The number image of the boolean image X: scipy's labelling renumbered by ascending `first`."""
    return cchost.reference(X, connectivity)[0]


def loop_pairs(frame, now):
    """(rows, heads) of two number images by plain loops over the pixels."""
    N = frame.shape[0]
    count, nheads = {}, 0
    for i in range(N):
        for j in range(N):
            key = (int(frame[i, j]), int(now[i, j]))
            if key == (-1, -1):
                continue
            count[key] = count.get(key, 0) + 1
            left = j > 0 and (int(frame[i, j - 1]), int(now[i, j - 1])) == key
            up = i > 0 and (int(frame[i - 1, j]), int(now[i - 1, j])) == key
            if not left and not up:
                nheads += 1
    rows = np.array([(a, b, n) for (a, b), n in sorted(count.items())], dtype=np.int64).reshape(-1, 3)
    return rows, nheads


def event_pairs(N):
    """Hand-made pairs of looks with known events: a list of (name, X_prev, X_now, {kind: families} at connectivity 4)."""
    assert N >= EVENT_MIN_N
    disc = shost.disc
    empty = np.zeros((N, N), dtype=bool)
    two = disc(N, 12, 12, 6) | disc(N, 34, 30, 9)
    out = [('identical', two, two, dict(continued=2)),
           ('shifted', disc(N, 20, 20, 8), disc(N, 20, 22, 8), dict(continued=1)),
           ('merged', disc(N, 20, 12, 6) | disc(N, 20, 28, 6), disc(N, 20, 12, 8) | disc(N, 20, 28, 8), dict(merged=1)),
           ('vanished', two, disc(N, 34, 30, 9), dict(continued=1, vanished=1)),
           ('born', disc(N, 34, 30, 9), two, dict(continued=1, born=1))]
    bell = disc(N, 20, 10, 7) | disc(N, 20, 34, 7)
    bar = empty.copy()
    bar[19:22, 10:35] = True
    cut = bell | bar
    cut[:, 22] = False
    out.append(('split', bell | bar, cut, dict(split=1)))
    out.append(('from-empty', empty, two, dict(born=2)))
    out.append(('to-empty', two, empty, dict(vanished=2)))
    out.append(('empty-empty', empty, empty, dict()))
    return out


def stripes_pair(N):
    """Horizontal against vertical one-pixel stripes."""
    ii, jj = np.indices((N, N))
    return ii % 2 == 0, jj % 2 == 0


def model_track(Xp, Xn, conn=4, **kw):
    return tracking.look(mh.field_of(Xp), mh.field_of(Xn), T, conn, 'below', **kw)


# ---------------------------------------------------------------------------
# 1. the model against plain loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_pair_table_and_heads_against_loops(seed):
    rng = np.random.default_rng(900 + seed)
    for N in (2 + seed, int(rng.integers(2, 34)), int(rng.integers(2, 34))):
        for conn in (4, 8):
            dp, dn = rng.choice([0.0, 0.2, 0.45, 0.6, 0.8, 1.0], 2)
            frame = label_image(rng.random((N, N)) < dp, conn)
            now = label_image(rng.random((N, N)) < dn, conn)
            rows, nheads = loop_pairs(frame, now)
            got = tracking.pair_table(frame, now)
            assert got.dtype == np.int64 and got.shape == rows.shape and np.array_equal(got, rows), (N, conn)
            assert tracking.heads(frame, now) == nheads and rows.shape[0] <= nheads
            w = tracking.words_of(np.zeros(17, dtype=np.int64), frame, now)
            assert w[tracking.CHS_TR_PAIRS] == rows.shape[0] and w[tracking.CHS_TR_HEADS] == nheads
            assert w[tracking.CHS_TR_OVERLAP] == np.count_nonzero((frame >= 0) & (now >= 0))
            assert w[tracking.CHS_TR_LOST] == np.count_nonzero((frame >= 0) & (now < 0))
            assert w[tracking.CHS_TR_GAINED] == np.count_nonzero((frame < 0) & (now >= 0))
            assert w[tracking.CHS_TR_PREV_COUNT] == frame.max(initial=-1) + 1 and w[tracking.CHS_TR_HAVE_PREV] == 1


@pytest.mark.parametrize("N", [8, 63, 65, 130])
def test_pairs_never_exceed_heads_on_noise(N):
    """The bound that sizes the device's hash table, on noise at four densities and both connectivities."""
    rng = np.random.default_rng(N)
    for density in (0.2, 0.4, 0.593, 0.8):
        for conn in (4, 8):
            frame = label_image(rng.random((N, N)) < density, conn)
            now = label_image(rng.random((N, N)) < density, conn)
            P, h = tracking.pair_table(frame, now).shape[0], tracking.heads(frame, now)
            assert 0 < P <= h <= N * N and tracking.slots_of(h) >= max(2 * h, 1024)


def test_slots():
    assert [tracking.slots_of(h) for h in (0, 1, 512, 513, 1024, 1025, 12675)] == [1024, 1024, 1024, 2048, 2048, 4096, 32768]


def test_stripes_against_stripes():
    """Horizontal against vertical one-pixel stripes at N = 130, connectivity 4: 65 x 65 crossings, 65 + 65 remainders;
    every counted pixel is a head."""
    N = 130
    Xp, Xn = stripes_pair(N)
    frame, now = label_image(Xp, 4), label_image(Xn, 4)
    rows, nheads = loop_pairs(frame, now)
    assert rows.shape[0] == 65 * 65 + 65 + 65 == 4355 and nheads == 3 * 65 * 65 == 12675
    got = tracking.pair_table(frame, now)
    assert np.array_equal(got, rows) and tracking.heads(frame, now) == 12675
    assert np.all(got[(got[:, 0] >= 0) & (got[:, 1] >= 0), 2] == 1) and np.all(got[(got[:, 0] < 0) | (got[:, 1] < 0), 2] == 65)
    tr = model_track(Xp, Xn)
    assert tr.counts() == dict(vanished=0, born=0, continued=0, merged=0, split=0, mixed=1)


# ---------------------------------------------------------------------------
# 2. families against scipy
# ---------------------------------------------------------------------------
def scipy_families(tr, min_overlap=1):
    t = tr.links(min_overlap)
    ca, cb = tr.prev.count, tr.now.count
    g = coo_matrix((np.ones(len(t)), (t[:, 0], ca + t[:, 1])), shape=(ca + cb, ca + cb))
    _, lab = connected_components(g, directed=False)
    fam = {}
    for node, l in enumerate(lab):
        fam.setdefault(l, ([], []))[0 if node < ca else 1].append(node if node < ca else node - ca)
    return sorted((tuple(p), tuple(q)) for p, q in fam.values())


@pytest.mark.parametrize("seed", range(6))
def test_families_against_scipy(seed):
    rng = np.random.default_rng(40 + seed)
    N = int(rng.integers(12, 40))
    for conn in (4, 8):
        tr = tracking.look(rng.random((N, N)), rng.random((N, N)), float(rng.choice([0.3, 0.45, 0.6])), conn, 'below')
        for mo in (1, 2, 3):
            fams = tr.families(mo)
            assert sorted((f.prev, f.now) for f in fams) == scipy_families(tr, mo)
            assert sorted(k for f in fams for k in f.prev) == list(range(tr.prev.count))
            assert sorted(k for f in fams for k in f.now) == list(range(tr.now.count))
            for f in fams:
                np_, nn = len(f.prev), len(f.now)
                want = {(1, 0): 'vanished', (0, 1): 'born', (1, 1): 'continued'}.get((np_, nn))
                if want is None:
                    want = 'merged' if nn == 1 else 'split' if np_ == 1 else 'mixed'
                assert f.kind == want and np_ + nn >= 1
            b = tr.area_budget(mo)
            assert b['vanished'] + b['born'] + b['exchanged'] == b['total'] == int(tr.now.area.sum()) - int(tr.prev.area.sum())
            assert b['vanished'] <= 0 <= b['born'] and sum(tr.counts(mo).values()) == len(fams)
        for k in range(tr.now.count):
            pre = tr.predecessors(k)
            assert int(pre[:, 1].sum()) + int(tr.pairs[(tr.pairs[:, 0] < 0) & (tr.pairs[:, 1] == k), 2].sum()) == tr.now.area[k]
        for k in range(tr.prev.count):
            suc = tr.successors(k)
            assert int(suc[:, 1].sum()) + int(tr.pairs[(tr.pairs[:, 0] == k) & (tr.pairs[:, 1] < 0), 2].sum()) == tr.prev.area[k]


# ---------------------------------------------------------------------------
# 3. hand-made events
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [EVENT_MIN_N, 65])
def test_hand_made_events(N):
    for name, Xp, Xn, want in event_pairs(N):
        tr = model_track(Xp, Xn)
        full = dict.fromkeys(tracking.KINDS, 0)
        full.update(want)
        assert tr.counts() == full, name
        assert tr.have_prev and tr.prev_count == tr.prev.count
        assert tr.overlap == int((Xp & Xn).sum()) and tr.lost == int((Xp & ~Xn).sum()) and tr.gained == int((~Xp & Xn).sum()), name
        b = tr.area_budget()
        assert b['vanished'] + b['born'] + b['exchanged'] == b['total'] == int(Xn.sum()) - int(Xp.sum()), name
        if name == 'identical':
            assert np.array_equal(tr.pairs[:, 0], tr.pairs[:, 1]) and np.array_equal(tr.pairs[:, 2], tr.prev.area)
            assert all(f.prev == f.now for f in tr.families())
        if name == 'shifted':
            assert np.array_equal(tr.pairs[:, :2], [[-1, 0], [0, -1], [0, 0]]) and tr.pairs[0, 2] == tr.pairs[1, 2]
            g = tr.growth()
            assert np.array_equal(g['shift'], [[0.0, 2.0]]) and g['d_area'][0] == 0 and np.isnan(g['area_rate'][0])
        if name == 'merged':
            assert tr.families()[0] == tracking.Family('merged', (0, 1), (0,)) and len(tr.predecessors(0)) == 2
        if name == 'split':
            assert tr.families()[0] == tracking.Family('split', (0,), (0, 1)) and len(tr.successors(0)) == 2
            assert tr.lost == 3 and tr.gained == 0
        if name == 'vanished':
            assert b['vanished'] == -int(shost.disc(N, 12, 12, 6).sum()) and b['exchanged'] == 0
        if name == 'born':
            assert b['born'] == int(shost.disc(N, 12, 12, 6).sum()) and b['exchanged'] == 0
        if name in ('from-empty', 'empty-empty'):
            assert tr.prev.count == 0 and tr.overlap == 0 and tr.lost == 0
        if name == 'empty-empty':
            assert tr.pairs.shape == (0, 3) and tr.families() == [] and tr.n_slots == 1024


def test_growth_of_a_disc_whose_radius_grows_by_one():
    N, r = 64, 10
    Xp, Xn = shost.disc(N, 30, 31, r), shost.disc(N, 30, 31, r + 1)
    tr = model_track(Xp, Xn, delx=0.5, steps=(100, 300), times=(1.0, 3.0))
    g = tr.growth()
    a0, a1 = int(Xp.sum()), int(Xn.sum())
    assert tr.counts()['continued'] == 1 and len(g['a']) == 1 and g['dt'] == 2.0 and (tr.steps_prev, tr.steps_now) == (100, 300)
    assert g['area_prev'][0] == a0 and g['area_now'][0] == a1 and g['d_area'][0] == a1 - a0 == tr.gained and tr.lost == 0
    assert g['area_rate'][0] == (a1 - a0) / 2.0
    r0, r1 = np.sqrt(a0 / np.pi) * 0.5, np.sqrt(a1 / np.pi) * 0.5
    assert g['radius_eq_prev'][0] == r0 and g['radius_eq_now'][0] == r1 and g['radius_rate'][0] == (r1 - r0) / 2.0
    assert 0.4 < g['d_radius_eq'][0] < 0.6                          # one pixel of delx = 0.5
    assert np.array_equal(g['shift'], [[0.0, 0.0]]) and g['distance'][0] == 0.0
    assert g['d_mean_u'][0] == 0.0 and g['mean_u_rate'][0] == 0.0   # (every foreground pixel holds the same value)


# ---------------------------------------------------------------------------
# 4. the Track object
# ---------------------------------------------------------------------------
def test_a_first_look_has_nothing_to_link():
    tr = tracking.look(None, mh.field_of(shost.disc(48, 20, 20, 8)), T)
    assert not tr.have_prev and tr.prev is None and tr.pairs.shape == (0, 3) and 'no frame' in repr(tr)
    assert not np.any(tr.words[17:])
    for call in (tr.links, tr.families, tr.counts, tr.growth, tr.area_budget, lambda: tr.predecessors(0)):
        with pytest.raises(ValueError):
            call()


def test_the_constructor_rejects_what_no_true_table_holds():
    _, Xp, Xn, _ = event_pairs(48)[2]
    tr = model_track(Xp, Xn)
    ok = lambda w=tr.words, p=tr.pairs, prev=tr.prev, now=tr.now: tracking.Track(w, p, prev, now)
    ok()
    for r in range(tr.pairs.shape[0]):
        for c in range(3):
            for d in (-1, 1):
                p = tr.pairs.copy()
                p[r, c] += d
                with pytest.raises(ValueError):
                    ok(p=p)
    with pytest.raises(ValueError):
        ok(p=tr.pairs[::-1])
    with pytest.raises(ValueError):
        ok(p=tr.pairs[:-1])
    for k in range(17, 25):
        w = tr.words.copy()
        w[k] += 1
        if k == tracking.CHS_TR_HEADS:                      # (one head more is no contradiction; fewer heads than pairs are)
            w[k] = tr.n_pairs - 1
        with pytest.raises(ValueError):
            ok(w=w)
    w = tr.words.copy()
    w[0] += 1
    with pytest.raises(ValueError):
        ok(w=w)
    with pytest.raises(ValueError):
        ok(prev=None)
    with pytest.raises(ValueError):
        ok(w=tr.words[:24])
    with pytest.raises(ValueError):
        tracking.pair_table(np.zeros((4, 4), dtype=int), np.zeros((4, 5), dtype=int))
    with pytest.raises(ValueError):
        tracking.pair_table(np.full((4, 4), -2), np.zeros((4, 4), dtype=int))


# ---------------------------------------------------------------------------
# 5. header and binding
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_TR_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_TR_WORDS'] == tracking.CHS_TR_WORDS == _lib.CHS_TR_WORDS == len(tracking.WORDS) == 25
    assert tracking.WORDS[:17] == shapes.WORDS
    for i, w in enumerate(tracking.WORDS[17:], start=17):
        assert defs['CHS_TR_' + w.upper()] == getattr(tracking, 'CHS_TR_' + w.upper()) == i
    from chsimpy_amd import _build
    src = open(os.path.join(_build.CSRC, 'chs_track.hip')).read()
    assert int(re.search(r'#define\s+TR_MIN_SLOTS\s+(\d+)', src).group(1)) == tracking.MIN_SLOTS
    assert os.path.join(_build.CSRC, 'chs_track.hip') in _build.source_files()


TR_SYMBOLS = ['chs_track', 'chs_track_pairs', 'chs_track_reset', 'chs_track_last_ms', 'chs_batch_track', 'chs_batch_track_pairs',
              'chs_batch_track_reset']


@pytest.mark.parametrize("name", TR_SYMBOLS)
def test_the_prototypes_match_the_header(hip_lib, name):
    cchost.test_the_prototypes_match_the_header(hip_lib, name)


def test_the_member_of_a_batch_answers_the_track_calls():
    from chsimpy_amd.batch import _Member
    assert {'track', 'track_look'} <= set(_Member._LOOKS)
    for cls in (_lib.Engine, _lib.Batch):
        assert all(hasattr(cls, n) for n in ('track', 'track_look', 'track_pairs', 'track_reset'))
