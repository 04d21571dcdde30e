"""Host side of the connected components of the thresholded field (chsimpy_amd/components.py): the numpy model against
scipy.ndimage.label, hand-made patterns with known answers, the two Euler identities against the bit-quad counts, the
consistency checks of `Components`, the header's constants and prototypes, the host model of the kernels' phases
(tests/cc_model.cpp, built with the address and undefined-behaviour sanitizers) and the experiment's --droplets on a dry
run.  No device.

`reference`, `patterns` and `check_look` are shared with tests/test_gpu_components.py, which puts the same fields on the
device.  Everything is integer: every comparison is for equality."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from chsimpy_amd import _lib, components, morphology
import test_morphology_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG, BG, T = mh.FG, mh.BG, mh.T
STRUCTURE = {4: mh.FOUR, 8: mh.EIGHT}


def tile_from_header():
    """(CHS_CC_TR, CHS_CC_TC) of chs_cc_host.h: the tile extents, without loading the library."""
    from chsimpy_amd import _build
    hdr = open(os.path.join(_build.CSRC, 'chs_cc_host.h')).read()
    return tuple(int(re.search(r'#define\s+%s\s+(\d+)\b' % k, hdr).group(1)) for k in ('CHS_CC_TR', 'CHS_CC_TC'))


def tile_sizes(tile):
    """The N at which each phase can still go wrong: one workgroup, below / at / above one tile, more than two tiles."""
    tr, tc = tile
    return [8, min(tr, tc) - 1, max(tr, tc), max(tr, tc) + 1, 2 * max(tr, tc) + 1]


def reference(X, connectivity):
    """(labels int32 [N][N], table int32 [C][6]) of the boolean image X from scipy.ndimage.label, its labels renumbered
    by ascending `first` (scipy's own order is not relied on), the areas from np.bincount, the boxes from
    ndimage.find_objects."""
    X = np.asarray(X, dtype=bool)
    N = X.shape[0]
    lab, C = ndimage.label(X, structure=STRUCTURE[connectivity])
    labels = np.full((N, N), -1, dtype=np.int32)
    table = np.zeros((C, components.CHS_CC_COLS), dtype=np.int32)
    if C == 0:
        return labels, table
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first = np.full(C + 1, N * N, dtype=np.int64)
    first[flat[idx[::-1]]] = idx[::-1]                     # (descending index: the smallest is written last)
    order = np.argsort(first[1:], kind='stable')           # scipy's label order[k] + 1 becomes number k
    number = np.empty(C + 1, dtype=np.int64)
    number[0] = -1
    number[order + 1] = np.arange(C)
    labels[:] = number[lab]
    areas = np.bincount(flat, minlength=C + 1)
    boxes = np.array([(si.start, si.stop - 1, sj.start, sj.stop - 1) for si, sj in ndimage.find_objects(lab)])
    table[:, 0] = first[1:][order]
    table[:, 1] = areas[1:][order]
    table[:, 2:] = boxes[order]
    return labels, table


def check_look(co, X, connectivity, what=''):
    """A `Components` with table (and labels, where fetched) against the scipy reference of the boolean image X."""
    N = X.shape[0]
    labels, table = reference(X, connectivity)
    want = components.summary_of(table, N)
    assert co.words.dtype == np.int64 and np.array_equal(co.words, want), (what, co.words, want)
    assert co.area == int(X.sum())
    if co.table is not None:
        assert co.table.dtype == np.int32 and np.array_equal(co.table, table), what
    if co.labels is not None:
        assert co.labels.dtype == np.int32 and np.array_equal(co.labels, labels), what
    return want


def model_look(U, t, connectivity, side):
    labels, table = components.label(U, t, connectivity, side)
    N = np.asarray(U).shape[0]
    return components.Components(components.summary_of(table, N), N, t, connectivity, side, table=table, labels=labels)


def patterns(N, tile):
    """Hand-made fields with known answers: a list of (name, U, {word: (value at connectivity 4, value at 8)}) for the
    side below the threshold T (``count_above``: the count of the complement)."""
    assert N >= 8
    tt = max(tile)
    B = tt if N > tt else N // 2                     # a tile border where the grid has one
    out = []

    def add(name, X, **want):
        out.append((name, mh.field_of(X), {k: (v if isinstance(v, tuple) else (v, v)) for k, v in want.items()}))

    empty = np.zeros((N, N), dtype=bool)
    ii, jj = np.indices((N, N))
    add('empty', empty, count=0, area=0, largest=0, spanning=0, inner=0, largest_first=-1, count_above=1)
    add('full', ~empty, count=1, area=N * N, largest=N * N, spanning=1, inner=0, largest_first=0, count_above=0)
    for i, j in ((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)):
        X = empty.copy()
        X[i, j] = True
        add(f'corner-{i}-{j}', X, count=1, area=1, spanning=0, inner=0, largest_first=i * N + j, count_above=1)
    add('diagonal', ii == jj, count=(N, 1), area=N, largest=(1, N), spanning=(0, 1), largest_first=0)
    add('anti-diagonal', ii + jj == N - 1, count=(N, 1), area=N, largest=(1, N), spanning=(0, 1), largest_first=N - 1)
    half = (N * N + 1) // 2
    add('checkerboard', (ii + jj) % 2 == 0, count=(half, 1), area=half, largest=(1, half), largest_first=0,
        count_above=(N * N - half, 1))
    add('comb', (ii == N - 1) | (jj % 2 == 0), count=1, spanning=1, area=(N - 1) * ((N + 1) // 2) + N, largest_first=0)
    X = (ii % 2 == 0) | ((ii % 2 == 1) & (jj == np.where((ii // 2) % 2 == 0, N - 1, 0)))
    add('serpentine', X, count=1, spanning=1, area=N * ((N + 1) // 2) + N // 2, largest_first=0)
    rings = empty.copy()
    offsets = list(range(0, (N - 1) // 2 + 1, 2))
    for o in offsets:
        rings[o:N - o, o:N - o] = True
        if N - 2 * o > 2:
            rings[o + 1:N - o - 1, o + 1:N - o - 1] = False
    add('rings', rings, count=len(offsets), inner=len(offsets) - 1, spanning=1, largest=4 * N - 4, largest_first=0)
    X = rings.copy()                                 # the spiral: every ring opened below its corner, joined to the next
    for o in offsets:
        if N - 2 * o >= 3:
            X[o + 1, o] = False
        if N - 2 * o >= 5:
            X[o + 2, o + 1] = True
    add('spiral', X, count=1, spanning=1, count_above=1, largest_first=0)
    add('stripes', jj % 2 == 0, count=(N + 1) // 2, spanning=(N + 1) // 2, largest=N, largest_first=0, inner=0)
    for name, pix, count in (('pair-h', ((5, B - 1), (5, B)), 1), ('pair-v', ((B - 1, 6), (B, 6)), 1),
                             ('pair-d', ((B - 1, B - 1), (B, B)), (2, 1)), ('pair-a', ((B - 1, B), (B, B - 1)), (2, 1))):
        X = empty.copy()
        for i, j in pix:
            X[i, j] = True
        add(name, X, count=count, area=2, spanning=0)      # (the complement: left to scipy -- pair-a cuts a grid corner off)
    return out


def check_pattern(look, name, U, want, N):
    """`look(U, t, connectivity, side)` -> Components with table and labels: the known answers, then scipy."""
    for c, conn in enumerate((4, 8)):
        below = look(U, T, conn, 'below')
        for k, v in want.items():
            if k != 'count_above':
                assert getattr(below, k) == v[c], (name, N, conn, k, getattr(below, k), v[c])
        check_look(below, U < T, conn, f"{name} N={N} {conn} below")
        above = look(U, T, conn, 'above')
        if 'count_above' in want:
            assert above.count == want['count_above'][c], (name, N, conn, above.count)
        check_look(above, ~(U < T), conn, f"{name} N={N} {conn} above")
        assert below.area + above.area == N * N


# ---------------------------------------------------------------------------
# the numpy model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.5, 0.593, 0.7])
@pytest.mark.parametrize("N", [8, 33, 100])
def test_model_against_scipy(N, density):
    rng = np.random.default_rng(1000 * N + int(1000 * density))
    U = mh.field_of(rng.random((N, N)) < density)
    for conn in (4, 8):
        for side in ('below', 'above'):
            X = (U < T) if side == 'below' else ~(U < T)
            assert np.array_equal(components.foreground(U, T, side), X)
            co = model_look(U, T, conn, side)
            check_look(co, X, conn, f"N={N} {density} {conn} {side}")
            assert co.count > 0 and co.connectivity == conn and co.side == side


@pytest.mark.parametrize("N", tile_sizes(tile_from_header()))
def test_patterns_with_known_answers(N):
    for name, U, want in patterns(N, tile_from_header()):
        check_pattern(model_look, name, U, want, N)


@pytest.mark.parametrize("N", [8, 33])
def test_threshold_nan_and_one_ulp_fields(N):
    """The fields of test_morphology_host.hand_made: a pixel at the threshold and a NaN pixel are background below and
    foreground above; one ulp decides."""
    for name, U, t, _ in mh.hand_made(N):
        Xb = np.nan_to_num(U, nan=np.inf) < t
        for conn in (4, 8):
            check_look(model_look(U, t, conn, 'below'), Xb, conn, name)
            check_look(model_look(U, t, conn, 'above'), ~Xb, conn, name)
        if name == 'nan-pixel':
            assert not components.foreground(U, t, 'below')[3, 4] and components.foreground(U, t, 'above')[3, 4]
        if name == 'one-ulp':
            assert model_look(U, t, 4, 'below').area == 1 and model_look(U, t, 4, 'above').area == N * N - 1


@pytest.mark.parametrize("density", [0.3, 0.5, 0.593, 0.8])
@pytest.mark.parametrize("N", [8, 33, 100])
def test_euler_identities(N, density):
    """euler8 = COUNT(below, 8) - INNER(above, 4) and euler4 = COUNT(below, 4) - INNER(above, 8)."""
    rng = np.random.default_rng(77 * N + int(1000 * density))
    U = mh.field_of(rng.random((N, N)) < density)
    mo = morphology.Morphology(morphology.quad_counts(U, T), N, T)
    look = {(c, s): model_look(U, T, c, s) for c in (4, 8) for s in ('below', 'above')}
    assert mo.euler8 == look[8, 'below'].count - look[4, 'above'].inner
    assert mo.euler4 == look[4, 'below'].count - look[8, 'above'].inner
    assert look[4, 'below'].area == look[8, 'below'].area == mo.n_A


def test_components_object():
    U = mh.field_of(np.random.default_rng(5).random((33, 33)) < 0.4)
    labels, table = components.label(U, T, 4, 'below')
    words = components.summary_of(table, 33)
    co = components.Components(words, 33, T, 4, 'below', table=table, labels=labels, delx=0.25)
    assert co.count == len(co.areas) == len(co.first) == len(co.bbox) and co.bbox.shape[1] == 4
    assert co.mean_area == co.area / co.count and co.weighted_mean_area == co.sumsq / co.area
    assert np.array_equal(co.radius_eq, np.sqrt(co.areas / np.pi) * 0.25)
    hist, edges = co.size_histogram(bins=[1, 2, 4, 8, 1000])
    assert hist.sum() == co.count and np.array_equal(hist, np.histogram(table[:, 1], bins=[1, 2, 4, 8, 1000])[0])
    assert co.largest == table[:, 1].max() and co.largest_first == table[table[:, 1] == co.largest, 0].min()
    bare = components.Components(words, 33, T, 8, 'above')
    assert bare.areas is None and bare.first is None and bare.bbox is None and bare.labels is None and bare.radius_eq is None
    assert bare.connectivity == 8 and bare.side == 'above'
    with pytest.raises(ValueError):
        bare.size_histogram()
    zero = components.Components(components.summary_of(np.zeros((0, 6)), 8), 8, T)
    assert zero.count == 0 and zero.mean_area == 0.0 and zero.weighted_mean_area == 0.0 and zero.largest_first == -1
    # the consistency checks
    bad = table.copy()
    bad[0, 1] += 1
    with pytest.raises(ValueError, match='add up'):
        components.Components(words, 33, T, table=bad)
    with pytest.raises(ValueError, match='rows'):
        components.Components(words, 33, T, table=table[:-1])
    with pytest.raises(ValueError, match='increasing'):
        components.Components(words, 33, T, table=table[::-1])
    with pytest.raises(ValueError):
        components.Components(words[:6], 33, T)
    with pytest.raises(ValueError):
        components.Components(words, 33, T, labels=labels[:-1])


def test_bad_arguments():
    U = np.zeros((8, 8))
    for kw in (dict(connectivity=6), dict(connectivity=True), dict(side='left'), dict(side=2)):
        with pytest.raises(ValueError):
            components.label(U, 0.5, **kw)
    with pytest.raises(ValueError):
        components.label(U, float('nan'))
    with pytest.raises(ValueError):
        components.label(np.zeros((8, 9)), 0.5)
    with pytest.raises(ValueError):
        components.Components(np.zeros(7, dtype=np.int64), 8, 0.5, connectivity=5)
    assert components.side_code('above') == components.side_code(1) == 1 and components.side_code('below') == 0


# ---------------------------------------------------------------------------
# header, binding, host model of the kernels, experiment
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_CC_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_CC_WORDS'] == components.CHS_CC_WORDS == _lib.CHS_CC_WORDS == len(components.WORDS) == 7
    assert defs['CHS_CC_COLS'] == components.CHS_CC_COLS == _lib.CHS_CC_COLS == len(components.COLS) == 6
    for i, w in enumerate(components.WORDS):
        assert defs['CHS_CC_' + w.upper()] == getattr(components, 'CHS_CC_' + w.upper()) == i
    assert defs['CHS_CC_BELOW'] == components.CHS_CC_BELOW == _lib.CHS_CC_BELOW == 0
    assert defs['CHS_CC_ABOVE'] == components.CHS_CC_ABOVE == _lib.CHS_CC_ABOVE == 1
    codes = dict(re.findall(r'#define\s+(CHS_E[A-Z]+)\s+\((-\d+)\)', hdr))
    assert int(codes['CHS_ECHECK']) == _lib.CHS_ECHECK == min(int(v) for v in codes.values()) == -len(codes)


_CTYPES = dict(mh._CTYPES)
_CTYPES['int32_t*'] = ctypes.POINTER(ctypes.c_int32)
_CTYPES['int64_t'] = ctypes.c_int64
CC_SYMBOLS = ['chs_components', 'chs_components_table', 'chs_components_labels', 'chs_components_last_ms', 'chs_components_tile',
              'chs_batch_components', 'chs_batch_components_table', 'chs_batch_components_labels']


@pytest.mark.parametrize("name", CC_SYMBOLS)
def test_the_prototypes_match_the_header(hip_lib, name):
    """The argument and return types the binding declares are those of the prototype in include/chs_hip.h."""
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'^\s*(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr, flags=re.M)
    assert m, f"{name}: no prototype in the header"
    ret, args = m.group(1), [a.strip() for a in m.group(2).split(',')]
    want = []
    for a in args:
        a = re.sub(r'\[\w*\]$', '*', a)
        t = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)\s*\w*\s*(\*?)$', a)
        assert t, a
        want.append(_CTYPES[t.group(1) + ('*' if (t.group(2) or t.group(3)) else '')])
    fn = getattr(hip_lib, name)
    assert name in _lib.SYMBOLS
    assert list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert ctypes.sizeof(fn.restype) == ctypes.sizeof(_CTYPES[ret])


def test_the_tile_of_the_library_is_the_headers(hip_lib):
    assert _lib.CC_TILE == _lib.components_tile() == tile_from_header()
    assert hip_lib.chs_components_tile(None, None) == _lib.CHS_EINVAL


def test_host_model_of_the_kernels_phases(tmp_path):
    """tests/cc_model.cpp: phases 1 to 4 through the functions the kernels use (chs_cc_host.h), pixels in scrambled
    orders and with stale loads, every pattern, both connectivities and sides, N in {8, T-1, T, T+1, 2T+1}, against a
    flood fill -- under the address and undefined-behaviour sanitizers."""
    from chsimpy_amd import _build
    exe = str(tmp_path / 'cc_model')
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I' + _build.CSRC,
                    os.path.join(ROOT, 'tests', 'cc_model.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and '\n0 failures' in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert int(re.search(r'(\d+) checks', r.stdout).group(1)) > 1000
    # the header is host code: nothing of HIP in it, and the program includes that header alone
    hdr = open(os.path.join(_build.CSRC, 'chs_cc_host.h')).read()
    assert not re.search(r'#include\s*[<"](hip/|chs_common|chs_fast|chs_cx)', hdr)
    prog = open(os.path.join(ROOT, 'tests', 'cc_model.cpp')).read()
    assert re.findall(r'#include\s*"([^"]+)"', prog) == ['chs_cc_host.h']
    # ... and the kernels take find, unite and the maps from it
    dev = open(os.path.join(_build.CSRC, 'chs_components.hip')).read()
    assert '#include "chs_cc_host.h"' in dev
    for fn in ('chs_cc::unite(', 'chs_cc::find(', 'chs_cc::tile_pairs(', 'chs_cc::border_pairs(', 'chs_cc::fg_of('):
        assert fn in dev, fn


def test_experiment_writes_the_droplets_file_on_a_dry_run(tmp_path):
    """--droplets adds <id>-droplets.csv and leaves the result files byte for byte what they are without it, member by
    member and in batches (members without device work: launcher, gather and writer alone)."""
    from chsimpy_amd import experiment
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'plain', '--morphology'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'drops', '--morphology', '--droplets'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'batch', '--batch', '2', '--droplets',
                         '--droplets-connectivity', '8'])
    finally:
        os.chdir(cwd)
    assert not (tmp_path / 'plain-droplets.csv').exists()
    assert not (tmp_path / 'batch-morphology.csv').exists()
    text = (tmp_path / 'drops-droplets.csv').read_text()
    lines = text.splitlines()
    assert lines[0] == ('id,threshold,connectivity,count_below,largest_below,spanning_below,mean_area_below,'
                        'count_above,largest_above,spanning_above,mean_area_above')
    assert lines[0] == ','.join(experiment.DROPLETS_COLS)
    assert [ln.split(',')[0] for ln in lines[1:]] == ['0', '1', '2']
    for ln in lines[1:]:
        f = ln.split(',')
        assert f[2] == '4' and int(f[3]) == int(f[0]) + 1 and float(f[6]) == 3.0 and '.' in f[6] and '.' not in f[3]
    batch = (tmp_path / 'batch-droplets.csv').read_text().splitlines()
    assert [ln.split(',')[2] for ln in batch[1:]] == ['8'] * 3
    assert [ln.split(',')[:2] + ln.split(',')[3:] for ln in batch] == [ln.split(',')[:2] + ln.split(',')[3:] for ln in lines]
    for kind in ('results.csv', 'results-agg.csv', 'morphology.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'drops-{kind}').read_bytes()
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'batch-{kind}').read_bytes()
    assert experiment.write_droplets(str(tmp_path / 'w'), [(0, 0.5, 4, 0, 0, 0, 0.0, 1, 256, 1, 256.0)]).endswith('w-droplets.csv')
    assert (tmp_path / 'w-droplets.csv').read_text().splitlines()[1] == '0,0.5,4,0,0,0,0.0,1,256,1,256.0'
