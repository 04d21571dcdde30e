"""Host side of the morphology of the thresholded field (chsimpy_amd/morphology.py): the bit-quad counts and what is
derived from them against scipy.ndimage's labelling and direct counts, hand-made fields with known answers, the ctypes
prototypes of the new entry points against include/chs_hip.h, and the experiment's --morphology on a dry run.  No device.

`hand_made(N)` is shared with tests/test_gpu_morphology.py, which puts the same fields on the device."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from chsimpy_amd import _lib, morphology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FG, BG, T = 0.2, 0.8, 0.5        # a foreground value, a background value, the threshold between them
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
EIGHT = np.ones((3, 3), dtype=int)


def field_of(mask):
    return np.where(np.asarray(mask, dtype=bool), FG, BG)


def euler_by_labelling(X):
    """(euler8, euler4) of the boolean image X from connected components: foreground components minus holes, a hole
    being a background component that does not reach the padding ring, in the complementary connectivity."""
    X = np.asarray(X, dtype=bool)
    bg = ~np.pad(X, 1, constant_values=False)
    c8 = ndimage.label(X, structure=EIGHT)[1]
    c4 = ndimage.label(X, structure=FOUR)[1]
    h4 = ndimage.label(bg, structure=FOUR)[1] - 1     # (the ring's component is no hole)
    h8 = ndimage.label(bg, structure=EIGHT)[1] - 1
    return c8 - h4, c4 - h8


def unlike_pairs(X):
    """4-adjacent pixel pairs inside the grid with one pixel in the foreground and one in the background."""
    X = np.asarray(X, dtype=bool)
    return int(np.count_nonzero(X[1:, :] != X[:-1, :])) + int(np.count_nonzero(X[:, 1:] != X[:, :-1]))


def check_against_direct_counts(words, X, N):
    """The seven words and everything derived from them against the direct counts on the boolean image X."""
    mo = morphology.Morphology(words, N, T, delx=0.25)
    assert mo.Q0 + mo.Q1 + mo.Q2 + mo.QD + mo.Q3 + mo.Q4 == (N + 1) ** 2
    assert (mo.Q1 - mo.Q3 - 2 * mo.QD) % 4 == 0 and (mo.Q1 - mo.Q3 + 2 * mo.QD) % 4 == 0
    assert mo.n_A == int(X.sum()) and mo.SA == int(X.sum()) / (N * N)
    border = int(X[0].sum()) + int(X[-1].sum()) + int(X[:, 0].sum()) + int(X[:, -1].sum())
    assert mo.border == border
    assert mo.perimeter_inner == unlike_pairs(X)
    assert mo.perimeter == unlike_pairs(np.pad(X, 1, constant_values=False)) == mo.perimeter_inner + border
    assert (mo.euler8, mo.euler4) == euler_by_labelling(X)
    assert mo.interface_phys == mo.perimeter_inner * 0.25
    return mo


@pytest.mark.parametrize("density", [0.2, 0.5, 0.7])
@pytest.mark.parametrize("N", [8, 33, 100])
def test_quad_counts_against_labelling_and_direct_counts(N, density):
    rng = np.random.default_rng(1000 * N + int(100 * density))
    for _ in range(3):
        X = rng.random((N, N)) < density
        words = morphology.quad_counts(field_of(X), T)
        assert words.dtype == np.int64 and words.shape == (morphology.CHS_MORPH_WORDS,)
        check_against_direct_counts(words, X, N)


def hand_made(N):
    """Hand-made fields with known answers: a list of (name, U, threshold, {attribute: value})."""
    assert N >= 8
    out = []

    def add(name, U, want, t=T):
        out.append((name, np.array(U, dtype=np.float64), t, want))

    empty = np.zeros((N, N), dtype=bool)
    zero = dict(Q0=(N + 1) ** 2, Q1=0, Q2=0, QD=0, Q3=0, Q4=0, border=0, n_A=0, perimeter=0, perimeter_inner=0, euler8=0,
                euler4=0)
    add('empty', field_of(empty), zero)
    add('full', field_of(~empty), dict(n_A=N * N, perimeter=4 * N, perimeter_inner=0, euler8=1, euler4=1, border=4 * N,
                                       Q1=4, Q2=4 * (N - 1), QD=0, Q3=0, Q4=(N - 1) ** 2))
    for i, j in ((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)):
        X = empty.copy()
        X[i, j] = True
        add(f'corner-{i}-{j}', field_of(X), dict(n_A=1, Q1=4, Q2=0, QD=0, Q3=0, Q4=0, border=2, perimeter=4, perimeter_inner=2,
                                                 euler8=1, euler4=1))
    ii, jj = np.indices((N, N))
    X = (ii + jj) % 2 == 0
    n_A = (N * N + 1) // 2
    # every inner pair is unlike; the background is one 8-connected piece with the ring (no hole for euler4), and every
    # background pixel off the border is a 4-connected hole of the one 8-connected foreground (euler8)
    add('checkerboard', field_of(X), dict(n_A=n_A, perimeter_inner=2 * N * (N - 1), euler4=n_A, euler8=1 - ((N - 2) ** 2) // 2,
                                          Q4=0, Q3=0, QD=(N - 1) ** 2))
    X = empty.copy()
    X[2:5, 2:5] = True
    X[3, 3] = False
    add('ring', field_of(X), dict(n_A=8, perimeter=16, perimeter_inner=16, border=0, euler8=0, euler4=0))
    X = empty.copy()
    X[2, 2] = X[3, 3] = True
    add('two-at-a-corner', field_of(X), dict(n_A=2, QD=1, Q1=6, perimeter=8, euler8=1, euler4=2))
    add('all-at-the-threshold', np.full((N, N), T), zero)
    U = field_of(~empty)
    U[3, 3] = T                                    # equal to the threshold: background, a hole of one pixel
    U[0, 5] = T                                    # and a notch in the border row
    add('pixels-at-the-threshold', U, dict(n_A=N * N - 2, euler8=0, euler4=0, border=4 * N - 1, perimeter_inner=7,
                                           perimeter=4 * N - 1 + 7))
    U = field_of(~empty)
    U[3, 4] = np.nan                               # NaN: background
    add('nan-pixel', U, dict(n_A=N * N - 1, euler8=0, euler4=0, border=4 * N, perimeter_inner=4, perimeter=4 * N + 4))
    U = field_of(empty)
    U[N - 1, 2] = np.nextafter(T, 0.0)             # one ulp below the threshold: foreground
    U[N - 1, 3] = np.nextafter(T, 1.0)             # one ulp above: background
    add('one-ulp', U, dict(n_A=1, border=1, perimeter=4, perimeter_inner=3, euler8=1, euler4=1))
    return out


def check_hand_made(words, N, t, want, name):
    mo = morphology.Morphology(words, N, t)
    for k, v in want.items():
        assert getattr(mo, k) == v, (name, N, k, getattr(mo, k), v)
    return mo


@pytest.mark.parametrize("N", [8, 33, 129])
def test_hand_made_fields(N):
    for name, U, t, want in hand_made(N):
        words = morphology.quad_counts(U, t)
        check_hand_made(words, N, t, want, name)
        if name != 'one-ulp':                       # (all others separate at T the way field_of does)
            check_against_direct_counts(words, np.nan_to_num(U, nan=BG) < t, N)


def test_the_comparison_is_done_in_double_on_the_stored_element():
    """An fp32 field is widened, not the threshold narrowed: 0.1f = 0.100000001490116... is not below 0.1."""
    U = np.full((8, 8), BG, dtype=np.float32)
    U[1, 1] = np.float32(0.1)
    assert morphology.Morphology(morphology.quad_counts(U, 0.1), 8, 0.1).n_A == 0
    assert morphology.Morphology(morphology.quad_counts(U, float(np.float32(0.1))), 8, 0.1).n_A == 0     # equal: background
    assert morphology.Morphology(morphology.quad_counts(U, 0.1000001), 8, 0.1).n_A == 1


def test_bad_arguments():
    with pytest.raises(ValueError):
        morphology.quad_counts(np.zeros((8, 8)), float('nan'))
    with pytest.raises(ValueError):
        morphology.quad_counts(np.zeros((8, 9)), 0.5)
    with pytest.raises(ValueError):
        morphology.Morphology(np.zeros(6, dtype=np.int64), 8, 0.5)
    with pytest.raises(ValueError):
        morphology.Morphology(np.zeros(7, dtype=np.int64), 8, 0.5)      # the classes do not add up to 81
    assert morphology.Morphology([81, 0, 0, 0, 0, 0, 0], 8, 0.5).interface_phys is None


def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_MORPH_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_MORPH_WORDS'] == morphology.CHS_MORPH_WORDS == _lib.CHS_MORPH_WORDS == len(morphology.WORDS) == 7
    for i, w in enumerate(morphology.WORDS):
        assert defs['CHS_MORPH_' + w.upper()] == getattr(morphology, 'CHS_MORPH_' + w.upper()) == i


_CTYPES = {'chs_handle': ctypes.c_void_p, 'chs_batch': ctypes.c_void_p, 'double*': ctypes.POINTER(ctypes.c_double),
           'int64_t*': ctypes.POINTER(ctypes.c_int64), 'double': ctypes.c_double, 'int32_t': ctypes.c_int32, 'int': ctypes.c_int}


@pytest.mark.parametrize("name", ['chs_morphology', 'chs_batch_morphology', 'chs_morphology_last_ms'])
def test_the_prototypes_match_the_header(hip_lib, name):
    """The argument and return types the binding declares are those of the prototype in include/chs_hip.h."""
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'^\s*(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr, flags=re.M)
    assert m, f"{name}: no prototype in the header"
    ret, args = m.group(1), [a.strip() for a in m.group(2).split(',')]
    want = []
    for a in args:
        a = re.sub(r'\[\w*\]$', '*', a)                       # int64_t out[CHS_MORPH_WORDS] -> int64_t out*
        t = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)\s*\w*\s*(\*?)$', a)
        assert t, a
        want.append(_CTYPES[t.group(1) + ('*' if (t.group(2) or t.group(3)) else '')])
    fn = getattr(hip_lib, name)
    assert name in _lib.SYMBOLS
    assert list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert fn.restype in (_CTYPES[ret], ctypes.c_int)
    assert ctypes.sizeof(fn.restype) == ctypes.sizeof(_CTYPES[ret])


def test_experiment_writes_the_morphology_file_on_a_dry_run(tmp_path):
    """--morphology adds <id>-morphology.csv and leaves the result files byte for byte what they are without it, alone
    and beside --domain-size, member by member and in batches (members without device work: launcher, gather and writer
    alone)."""
    from chsimpy_amd import experiment
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'plain', '--domain-size'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'morph', '--domain-size', '--morphology'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'batch', '--batch', '2', '--morphology'])
    finally:
        os.chdir(cwd)
    assert not (tmp_path / 'plain-morphology.csv').exists()
    assert not (tmp_path / 'batch-domains.csv').exists()
    text = (tmp_path / 'morph-morphology.csv').read_text()
    assert text == (tmp_path / 'batch-morphology.csv').read_text()
    lines = text.splitlines()
    assert lines[0] == 'id,threshold,n_A,SA,perimeter,perimeter_inner,euler8,euler4'
    assert [ln.split(',')[0] for ln in lines[1:]] == ['0', '1', '2']
    for ln in lines[1:]:
        rid, t, n_A, SA, per, per_in, e8, e4 = ln.split(',')
        assert float(SA) == int(n_A) / 256 and int(per) >= int(per_in) and (int(e8), int(e4)) == (1 - int(rid),) * 2
    for kind in ('results.csv', 'results-agg.csv', 'domains.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'morph-{kind}').read_bytes()
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'batch-{kind}').read_bytes()
