"""Host side of the radially averaged structure factor (chsimpy_amd/spectrum.py): the binning rule, the bin counts,
the moments, and the ctypes prototypes of the new entry points against include/chs_hip.h.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

from chsimpy_amd import _lib, spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", [8, 100, 129, 512])
def test_bin_of_is_the_nearest_integer_to_the_radius(N):
    """Integer rule against np.rint(np.hypot(i, j)) for all modes: equal because no tie exists (b + 1/2 squared is no
    integer), so the float route cannot round the other way at these sizes."""
    k = np.arange(N)
    got = spectrum.bin_of(k[:, None], k[None, :])
    want = np.rint(np.hypot(k[:, None], k[None, :])).astype(np.int64)
    assert got.shape == (N, N) and np.array_equal(got, want)
    s = k[:, None] ** 2 + k[None, :] ** 2
    assert np.all((s == 0) | ((got * got - got < s) & (s <= got * got + got)))
    assert np.array_equal(got, spectrum.bin_map(N))
    assert spectrum.bin_of(0, 0) == 0 and spectrum.bin_of(3, 4) == 5 and spectrum.bin_of(1, 1) == 1


@pytest.mark.parametrize("N", [8, 100, 129, 512])
def test_bin_sizes_count_every_mode(N):
    n = spectrum.bin_sizes(N)
    assert n.dtype == np.int64 and n.shape == (spectrum.bin_count(N),)
    assert n.sum() == N * N
    assert n[0] == 1 and n[1] == 3 and n[-1] >= 1    # (0,0) | (0,1), (1,0), (1,1) | the corner


def test_bin_count():
    """nb = the integer nearest to (N-1) * sqrt(2), plus one: 9.90 -> 10, 179.6 -> 180, 5791.2 -> 5791, 11583.8 -> 11584."""
    assert [spectrum.bin_count(N) for N in (8, 128, 4096, 8192)] == [11, 181, 5792, 11585]
    for N in (8, 128, 4096, 8192):
        assert spectrum.bin_count(N) == spectrum.bin_of(N - 1, N - 1) + 1


def test_structure_factor_moments_on_a_hand_made_ssum():
    N = 8
    nb = spectrum.bin_count(N)
    ssum = np.zeros(nb)
    ssum[2], ssum[4] = 3.0, 1.0
    ssum[0] = 123.0      # bin 0 and the bins beyond N-1 take no part in k1
    ssum[9] = 50.0
    sf = spectrum.StructureFactor(ssum, N, delx=0.5)
    assert sf.N == 8
    assert sf.k1 == (2 * 3.0 + 4 * 1.0) / 4.0 == 2.5
    assert sf.ell == 2 * 8 / 2.5
    assert sf.ell_phys == sf.ell * 0.5
    assert np.array_equal(sf.n, spectrum.bin_sizes(N))
    assert np.array_equal(sf.S, ssum / spectrum.bin_sizes(N))
    assert spectrum.StructureFactor(ssum, N).ell_phys is None
    assert np.isnan(spectrum.StructureFactor(np.zeros(nb), N).k1)
    with pytest.raises(ValueError):
        spectrum.StructureFactor(np.zeros(nb + 1), N)


def test_bin_power_is_the_sum_of_squares_per_bin():
    N = 24
    C = np.random.default_rng(3).standard_normal((N, N))
    got = spectrum.bin_power(C)
    bins = spectrum.bin_map(N)
    for b in (0, 1, 5, 17, spectrum.bin_count(N) - 1):
        sel = bins == b
        want = float((C[sel] ** 2).sum()) - (C[0, 0] ** 2 if b == 0 else 0.0)
        assert got[b] == pytest.approx(want, rel=1e-14, abs=1e-300)
    assert got[0] == 0.0


_CTYPES = {'chs_handle': ctypes.c_void_p, 'chs_batch': ctypes.c_void_p, 'double*': ctypes.POINTER(ctypes.c_double),
           'int32_t': ctypes.c_int32, 'int': ctypes.c_int}


@pytest.mark.parametrize("name", ['chs_structure_factor_bins', 'chs_structure_factor', 'chs_batch_structure_factor',
                                  'chs_structure_factor_last_ms'])
def test_the_prototypes_match_the_header(hip_lib, name):
    """The argument and return types the binding declares are those of the prototype in include/chs_hip.h."""
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'^\s*(\w+)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr, flags=re.M)
    assert m, f"{name}: no prototype in the header"
    ret, args = m.group(1), [a.strip() for a in m.group(2).split(',')]
    want = []
    for a in args:
        a = re.sub(r'\[\d*\]$', '*', a)                       # double ms[3] -> double ms*
        t = re.match(r'^(?:const\s+)?(\w+)\s*(\*?)\s*\w*\s*(\*?)$', a)
        assert t, a
        want.append(_CTYPES[t.group(1) + ('*' if (t.group(2) or t.group(3)) else '')])
    fn = getattr(hip_lib, name)
    assert name in _lib.SYMBOLS
    assert list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert fn.restype in (_CTYPES[ret], ctypes.c_int)
    assert ctypes.sizeof(fn.restype) == ctypes.sizeof(_CTYPES[ret])


def test_bins_entry_point_agrees_with_the_host_rule(hip_lib):
    """chs_structure_factor_bins needs no device."""
    for N in (8, 24, 100, 128, 129, 301, 1025, 4096, 8192):
        assert hip_lib.chs_structure_factor_bins(N) == spectrum.bin_count(N)
    assert hip_lib.chs_structure_factor_bins(0) == _lib.CHS_EINVAL


def test_experiment_writes_the_domain_file_on_a_dry_run(tmp_path):
    """--domain-size adds <id>-domains.csv and leaves the three result files byte for byte what they are without it
    (members without device work: launcher, gather and writer alone)."""
    from chsimpy_amd import experiment
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'plain'])
        experiment.main(['-N', '16', '-R', '3', '--dry-run', '--file-id', 'plain2', '--domain-size'])
    finally:
        os.chdir(cwd)
    assert not (tmp_path / 'plain-domains.csv').exists()
    lines = (tmp_path / 'plain2-domains.csv').read_text().splitlines()
    assert lines[0] == 'id,k1,ell,ell_phys' and [ln.split(',')[0] for ln in lines[1:]] == ['0', '1', '2']
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'plain-{kind}').read_bytes() == (tmp_path / f'plain2-{kind}').read_bytes()
