"""CPU tests of the composition look (chsimpy_amd/composition.py): the order-preserving key, the numpy models against
numpy's own sort and histogram, the `Composition` object on hand-made words, the header's constants and prototypes, and
the experiment's --composition on a dry run.  No device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, composition as cmp, experiment as ex
import test_morphology_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 0.875

# (N, dtype) of the reference's histogram: the start field of a run, solver.py:78-82
UHIST_CASES = [(8, np.float64), (100, np.float64), (129, np.float32), (513, np.float64)]


def start_field(N, dtype, nbins=15):
    return (0.875 + 0.01 * (np.random.default_rng(17 * N + nbins).random((N, N)) - 0.5)).astype(dtype)


def tile_from_source():
    """(elems_per_thread, threads, max_groups, digit_bits) as chs_composition.hip defines them."""
    src = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_composition.hip')).read()
    return tuple(int(re.search(r'#define\s+' + k + r'\s+(\d+)\b', src).group(1))
                 for k in ('CMP_EPT', 'CMP_THREADS', 'CMP_MAX_GROUPS', 'CMP_DIGIT_BITS'))


def special_field(N, dtype=np.float64):
    """+-0, +-inf, a NaN of each sign, denormals, negative values and values above 1 in a field of noise."""
    rng = np.random.default_rng(N)
    U = (rng.random((N, N)) * 3.0 - 1.0).astype(dtype)
    tiny = np.finfo(dtype).tiny
    flat = U.ravel()
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, tiny / 4, -tiny / 4, tiny, -tiny, -2.5, 7.0, T]
    flat[rng.choice(flat.size, len(vals), replace=False)] = np.array(vals, dtype=dtype)
    neg_nan = np.array([np.nan], dtype=dtype)
    neg_nan.view(np.uint64 if dtype == np.float64 else np.uint32)[0] |= (1 << (63 if dtype == np.float64 else 31))
    flat[np.flatnonzero(np.isnan(flat))[0]] = neg_nan[0]          # (whatever -np.nan is: one NaN has its sign bit set)
    return U


# ---------------------------------------------------------------------------
# the key
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_key_is_monotone_over_a_ladder(dtype):
    fi = np.finfo(dtype)
    den = fi.smallest_subnormal
    ladder = np.array([-np.inf, -fi.max, -1.5, -1.0, -fi.tiny, -den * 3, -den, -0.0, 0.0, den, den * 3, fi.tiny, 0.5,
                       np.nextafter(dtype(0.5), dtype(1)), 1.0, 1.5, fi.max, np.inf], dtype=dtype)
    keys = cmp.key_of(ladder)
    assert keys.dtype == (np.uint64 if dtype == np.float64 else np.uint32)
    assert np.all(keys[1:] > keys[:-1])
    assert int(keys[8]) - int(keys[7]) == 1                       # -0.0 and +0.0 are neighbours
    ut = keys.dtype.type
    nans = np.array([np.nan, np.nan], dtype=dtype)
    nans.view(ut)[1] |= ut(1) << ut(8 * nans.itemsize - 1)        # a NaN of each sign
    assert np.signbit(nans[1]) and not np.signbit(nans[0])
    nk = cmp.key_of(nans)
    assert nk[0] == nk[1] == ~ut(0) and nk[0] > keys[-1]
    with pytest.raises(ValueError):
        cmp.key_of(np.zeros(3, dtype=np.int32))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_select_model_is_numpys_sort(dtype):
    for N in (8, 33):
        U = special_field(N, dtype)
        want = np.sort(U.ravel()).astype(np.float64)
        ranks = [0, 1, N * N // 2, N * N - 2, N * N - 1, 1] + list(range(2, N * N - 2, 7))
        got = cmp.select_model(U, ranks)
        assert got.dtype == np.float64
        assert np.array_equal(got, want[ranks], equal_nan=True)
        assert np.isnan(got[3]) and np.isnan(got[4]) and got[0] == -np.inf    # NaN of either sign sorts last


# ---------------------------------------------------------------------------
# the histogram
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [15, 256, 4096])
@pytest.mark.parametrize("N,dtype", UHIST_CASES, ids=[f"N{n}-{np.dtype(d).name}" for n, d in UHIST_CASES])
def test_histogram_model_is_numpys_histogram(N, dtype, nbins):
    """The reference's Uhist (plotview.py:159-167) at 15 bins, and the widest table: no pixel moves across an edge."""
    U = start_field(N, dtype, nbins)
    lo, hi, scale = cmp.range_model(U, nbins)
    assert (lo, hi) == (float(U.min()), float(U.max())) and scale == nbins / (hi - lo)
    got = cmp.histogram_model(U, nbins, lo, hi, scale)
    assert got.dtype == np.int64 and got.shape == (nbins,) and int(got.sum()) == N * N
    assert np.array_equal(got, np.histogram(U.astype(np.float64), bins=nbins)[0])


def test_histogram_model_range_outliers_and_a_constant_field():
    U = special_field(16)
    lo, hi, scale = cmp.range_model(U, 7, (0.0, 1.0))
    assert (lo, hi, scale) == (0.0, 1.0, 7.0)
    h = cmp.histogram_model(U, 7, lo, hi, scale)
    w = cmp.words_model(U, T, lo=lo, hi=hi)
    assert int(h.sum()) + w['n_under'] + w['n_over'] + w['n_nan'] == 256
    assert w['n_nan'] == 2 and w['n_inf'] == 2 and w['n_under'] > 1 and w['n_over'] > 1
    x = U[np.isfinite(U) & (U >= 0) & (U <= 1)]
    assert np.array_equal(h, np.histogram(x, bins=7, range=(0.0, 1.0))[0])
    # the field's own range leaves out the infinite pixels: -inf is under, +inf over
    lo, hi, scale = cmp.range_model(U, 4)
    assert (lo, hi) == (-2.5, 7.0)
    w = cmp.words_model(U, T, lo=lo, hi=hi)
    assert (w['n_under'], w['n_over'], w['min'], w['max']) == (1, 1, -2.5, 7.0)
    assert int(cmp.histogram_model(U, 4, lo, hi, scale).sum()) == 256 - 4
    # hi == lo: scale 0, everything in bin 0
    C = np.full((8, 8), 0.3)
    assert cmp.range_model(C, 15) == (0.3, 0.3, 0.0)
    assert cmp.histogram_model(C, 15, 0.3, 0.3, 0.0).tolist() == [64] + [0] * 14
    # no finite pixel
    E = np.full((8, 8), np.nan)
    E[0, 0] = np.inf
    lo, hi, scale = cmp.range_model(E, 3)
    assert math.isnan(lo) and math.isnan(hi) and scale == 0.0
    assert cmp.histogram_model(E, 3, lo, hi, scale).tolist() == [0, 0, 0]
    w = cmp.words_model(E, T, lo=lo, hi=hi)
    assert (w['n_nan'], w['n_inf'], w['n_under'], w['n_over']) == (63, 1, 0, 1) and math.isnan(w['min']) and math.isnan(w['center'])


def test_words_model():
    U = np.array([[0.25, 0.75], [1.0, np.nan]])
    w = cmp.words_model(U, 0.75)
    assert (w['n_total'], w['n_nan'], w['n_inf'], w['n_below']) == (4, 1, 0, 1)          # 0.75 is not below 0.75
    assert float(w['sum']) == 2.0 and float(w['sum_below']) == 0.25 and w['center'] == 2.0 / 3.0
    d = np.array([0.25, 0.75, 1.0], dtype=np.longdouble) - np.longdouble(2.0 / 3.0)
    for p in (2, 3, 4):
        assert abs(float(w[f'm{p}'] - (d ** p).sum())) < 1e-18 and float(w[f'abs{p}']) >= abs(float(w[f'm{p}']))
    assert cmp.words_model(U, 0.75, center=0.5)['center'] == 0.5
    assert cmp.quantile_rank(0.5, 3) == 1 and cmp.quantile_rank(1.0, 3) == 2 and cmp.quantile_rank(0.05, 100) == 4
    with pytest.raises(ValueError):
        cmp.quantile_rank(1.5, 3)


# ---------------------------------------------------------------------------
# the object
# ---------------------------------------------------------------------------
def hand_words():
    """N = 4: ten pixels at 0.25, four at 0.75, one NaN, one +inf; threshold 0.5, four bins over [0, 1]."""
    iw = [16, 1, 1, 10, 0, 1, 4]
    c = (10 * 0.25 + 4 * 0.75) / 14
    m = [10 * (0.25 - c) ** p + 4 * (0.75 - c) ** p for p in (2, 3, 4)]
    fw = [0.25, 0.75, 5.5, 2.5, c] + m + [0.0, 1.0, 4.0]
    return iw, fw, [0, 10, 0, 4]


def test_composition_object():
    iw, fw, hist = hand_words()
    co = cmp.Composition(iw, fw, 4, 0.5, hist=hist, quantiles={0.5: 0.25}, delx=0.5)
    assert (co.n, co.n_nan, co.n_inf, co.n_finite, co.n_below, co.under, co.over, co.nbins) == (16, 1, 1, 14, 10, 0, 1, 4)
    assert (co.min, co.max, co.mean) == (0.25, 0.75, fw[4]) and co.SA == 10 / 16
    assert co.mean_below == 0.25 and co.mean_above == 0.75
    assert co.var == fw[5] / 14 and co.skewness == (fw[6] / 14) / co.var ** 1.5 and co.kurtosis == (fw[7] / 14) / co.var ** 2
    assert co.skewness > 0 and co.edges.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert co.peaks() == (0.375, 0.875) and co.quantiles == {0.5: 0.25} and co.hist.dtype == np.int64
    assert 'SA=0.625' in repr(co)
    bare = cmp.Composition(iw, fw, 4, 0.5)
    assert bare.hist is None and bare.peaks() == (None, None) and bare.quantiles == {}
    one_sided = cmp.Composition(iw, fw, 4, 0.0, hist=hist)
    assert one_sided.peaks() == (None, 0.375)
    # a field without a finite pixel
    nan = float('nan')
    e = cmp.Composition([16, 16, 0, 0, 0, 0, 4], [nan, nan, 0.0, 0.0, nan, 0.0, 0.0, 0.0, nan, nan, 0.0], 4, 0.5, hist=[0] * 4)
    assert e.mean is None and e.var is None and e.skewness is None and e.mean_below is None and e.mean_above is None
    assert e.edges is None and e.peaks() == (None, None) and e.SA == 0.0
    for bad_iw, bad_fw, bad_hist in [(iw[:6], fw, None), (iw, fw[:10], None), ([15] + iw[1:], fw, None),
                                     (iw, fw, [0, 10, 0, 5]), (iw, fw, [0, 10, 4]), (iw[:6] + [0], fw, None),
                                     (iw, [0.25, 0.75, 5.5, 2.5, 0.8] + fw[5:], None), ([16, 9, 8] + iw[3:], fw, None)]:
        with pytest.raises(ValueError):
            cmp.Composition(bad_iw, bad_fw, 4, 0.5, hist=bad_hist)


def test_bad_arguments():
    for bins in (0, 4097, 1.5, True):
        with pytest.raises(ValueError):
            cmp.check_bins(bins)
    assert cmp.check_bins(1) == 1 and cmp.check_bins(4096) == 4096
    for rng in ((1.0, 0.0), (0.0, math.inf), (math.nan, 1.0), (-math.inf, 0.0)):
        with pytest.raises(ValueError):
            cmp.check_range(rng)
    assert cmp.check_range((0, 1)) == (0.0, 1.0) and all(math.isnan(v) for v in cmp.check_range(None))
    with pytest.raises(ValueError):
        cmp.histogram_model(np.zeros((3, 4)), 4, 0.0, 1.0, 4.0)


# ---------------------------------------------------------------------------
# header, binding, experiment
# ---------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+(CHS_CMP_[A-Z_0-9]+)\s+(\d+)\b', hdr)}
    assert defs['CHS_CMP_IWORDS'] == cmp.CHS_CMP_IWORDS == _lib.CHS_CMP_IWORDS == len(cmp.IWORDS) == 7
    assert defs['CHS_CMP_FWORDS'] == cmp.CHS_CMP_FWORDS == _lib.CHS_CMP_FWORDS == len(cmp.FWORDS) == 11
    assert defs['CHS_CMP_MAX_BINS'] == cmp.CHS_CMP_MAX_BINS == _lib.CHS_CMP_MAX_BINS == 4096
    assert defs['CHS_CMP_MAX_RANKS'] == cmp.CHS_CMP_MAX_RANKS == _lib.CHS_CMP_MAX_RANKS == 8
    for i, w in enumerate(cmp.IWORDS):
        assert defs['CHS_CMP_' + w.upper()] == getattr(cmp, 'CHS_CMP_' + w.upper()) == i
    for i, w in enumerate(cmp.FWORDS):
        assert defs['CHS_CMP_' + w.upper()] == getattr(cmp, 'CHS_CMP_' + w.upper()) == i
    ept, threads, groups, bits = tile_from_source()
    assert threads % 64 == 0 and ept % 4 == 0 and bits == 11 and 8 * (1 << bits) * 4 <= 64 * 1024
    assert (16384 ** 2) // groups < 2 ** 32                          # a workgroup's counts fit 32 bits
    E, D = _lib.composition_sum_terms(4096, (ept, threads, groups, bits))
    assert (E, D) == (ept * -(-4096 * 4096 // (ept * threads * groups)), 8 + 11)
    assert _lib.composition_sum_terms(8, (ept, threads, groups, bits))[0] == ept


_CTYPES = dict(mh._CTYPES)
_CTYPES['int32_t*'] = ctypes.POINTER(ctypes.c_int32)
CMP_SYMBOLS = ['chs_composition', 'chs_composition_hist', 'chs_composition_select', 'chs_composition_last_ms',
               'chs_composition_tile', 'chs_batch_composition', 'chs_batch_composition_hist', 'chs_batch_composition_select',
               'chs_batch_composition_last_ms']


@pytest.mark.parametrize("name", CMP_SYMBOLS)
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


def test_entry_points_that_need_no_device(hip_lib):
    assert _lib.composition_tile() == tile_from_source()
    w = ctypes.c_int32(0)
    assert hip_lib.chs_composition_tile(None, None, None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_composition_tile(ctypes.byref(w), ctypes.byref(w), ctypes.byref(w), None) == _lib.CHS_EINVAL
    iw, fw = np.zeros(7, dtype=np.int64), np.zeros(11)
    nan = float('nan')
    assert hip_lib.chs_composition(None, 0.5, 15, nan, nan, _lib._i64ptr(iw), _lib._dptr(fw)) == _lib.CHS_EINVAL
    assert hip_lib.chs_composition_hist(None, 15, _lib._i64ptr(iw)) == _lib.CHS_EINVAL
    assert hip_lib.chs_composition_select(None, 1, _lib._i64ptr(iw), _lib._dptr(fw)) == _lib.CHS_EINVAL
    assert hip_lib.chs_composition_last_ms(None, None) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_composition(None, 0, 0.5, 15, nan, nan, _lib._i64ptr(iw), _lib._dptr(fw)) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_composition_hist(None, 15, _lib._i64ptr(iw)) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_composition_select(None, 0, 1, _lib._i64ptr(iw), _lib._dptr(fw)) == _lib.CHS_EINVAL
    assert hip_lib.chs_batch_composition_last_ms(None, ctypes.byref(ctypes.c_double(0))) == _lib.CHS_EINVAL


def test_the_record_is_a_measurement_of_its_own_tuple():
    assert [m.key for m in ex.FIELD_MEASUREMENTS] == ['composition'] and ex.ALL_MEASUREMENTS == ex.MEASUREMENTS + ex.FIELD_MEASUREMENTS
    m = ex.FIELD_MEASUREMENTS[0]
    assert isinstance(m, ex.Measurement) and m.flag == '--composition' and m.suffix == 'composition'
    assert m.cols == ex.COMPOSITION_COLS == ('id', 'threshold', 'n_nan', 'min', 'max', 'mean', 'var', 'SA', 'mean_below',
                                             'mean_above', 'q05', 'q50', 'q95')
    assert m.int_cols == {'id', 'n_nan'} and m.rows_of_batch is None
    p = chsimpy_amd.Parameters()
    p.N = 16
    assert len(m.dry_row(2, p, {})) == len(m.cols) - 1
    known = ex.arg_parser()._option_string_actions
    assert known['--composition'].dest == 'composition'
    assert len({x.key for x in ex.ALL_MEASUREMENTS}) == len({x.suffix for x in ex.ALL_MEASUREMENTS}) == 6


@pytest.mark.parametrize('batch', [[], ['--batch', '2']], ids=['one_by_one', 'batch2'])
def test_experiment_writes_the_composition_file_on_a_dry_run(tmp_path, batch):
    """--composition adds <id>-composition.csv; a dry run with the five old flags, with or without it, writes the bytes
    it writes alone (members without device work: launcher, gather and writer alone)."""
    old = [m.flag for m in ex.MEASUREMENTS]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        base = ['-N', '16', '-R', '3', '--dry-run'] + batch
        ex.main(base + ['--file-id', 'bare'])
        ex.main(base + ['--file-id', 'old'] + old)
        ex.main(base + ['--file-id', 'new', '--composition'])
        ex.main(base + ['--file-id', 'all', '--composition'] + old)
    finally:
        os.chdir(cwd)
    assert not (tmp_path / 'bare-composition.csv').exists() and not (tmp_path / 'old-composition.csv').exists()
    text = (tmp_path / 'new-composition.csv').read_text()
    assert (tmp_path / 'all-composition.csv').read_text() == text
    lines = text.splitlines()
    assert lines[0] == 'id,threshold,n_nan,min,max,mean,var,SA,mean_below,mean_above,q05,q50,q95' and len(lines) == 4
    for i, ln in enumerate(lines[1:]):
        f = ln.split(',')
        assert len(f) == 13 and f[0] == str(i) and f[2] == str(i) and float(f[3]) == 0.125 and float(f[4]) == 0.875 + 0.001 * i
        assert float(f[6]) == 0.1 / (i + 1) and [float(v) for v in f[10:]] == [0.126, 0.5, 0.874]
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'new-{kind}').read_bytes() == (tmp_path / f'bare-{kind}').read_bytes()
        assert (tmp_path / f'all-{kind}').read_bytes() == (tmp_path / f'bare-{kind}').read_bytes()
    for m in ex.MEASUREMENTS:
        assert (tmp_path / f'all-{m.suffix}.csv').read_bytes() == (tmp_path / f'old-{m.suffix}.csv').read_bytes()
        assert not (tmp_path / f'new-{m.suffix}.csv').exists()
    nan = float('nan')
    assert ex.write_composition(str(tmp_path / 'w'), [(4, 0.5, 0, 0.1, 0.9, 0.5, 0.01, 0.25, nan, 0.6, 0.1, 0.5, 0.9)]).endswith(
        'w-composition.csv')
    assert (tmp_path / 'w-composition.csv').read_text().splitlines()[1] == '4,0.5,0,0.1,0.9,0.5,0.01,0.25,nan,0.6,0.1,0.5,0.9'
