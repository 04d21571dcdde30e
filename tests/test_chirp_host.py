"""CPU tests of the chirp engine (CHS_ENGINE_CHIRP, chsimpy_amd/csrc/chs_chirp.hip): the numpy model of its index maps
(tools/chirp_model.py) against scipy, its host tables (chs_chirp_host.h) against their definitions, the constants of
header and binding, and the batch's unchanged refusal.  Nothing here touches a device."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import fftpack

import chsimpy_amd
from chsimpy_amd import _lib, batch as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12   # of the largest entry: the project's fp64 transform tolerance (tests/test_gpu_parity.py)


def _model():
    spec = importlib.util.spec_from_file_location('chirp_model', os.path.join(ROOT, 'tools', 'chirp_model.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


cm = _model()


# every P = 16 ... 8192, and both ends of the ranges of P = 128, 1024 and 4096 (the plans (2, 1), (3, 1) and (3, 0))
@pytest.mark.parametrize('N, P', [(8, 16), (9, 32), (24, 64), (100, 256), (127, 256), (129, 512), (1000, 2048),
                                  (2049, 8192), (4096, 8192), (40, 128), (64, 128), (65, 256), (301, 1024),
                                  (512, 1024), (513, 2048), (1025, 4096), (2048, 4096)])
def test_plan_takes_the_smallest_power_of_two(N, P):
    pl = cm.plan(N)
    assert pl['P'] == P and 1 << pl['logP'] == P
    assert 3 * pl['nt'] + (pl['rl'] or 3) == pl['logP']
    f = cm.freq_of_pos(pl, np.arange(P))
    assert sorted(f) == list(range(P))


def test_the_models_pass_view_is_the_kernels_position_map():
    """The passes of the model work on a reshaped view of the line; the kernel computes positions from lane and
    register number.  The two are the same map, and every pass touches every position once."""
    for N in (8, 9, 24, 100, 129, 1000, 40, 301, 1025, 2049):
        pl = cm.plan(N)
        P = pl['P']
        lds = np.arange(P)[None, :]
        for ls in [pl['logP'] - 3 - 3 * i for i in range(pl['nt'])] + [0]:
            pos = cm.positions(pl, ls)                      # [lane, register]
            assert sorted(pos.ravel()) == list(range(P))
            v = cm._view(lds, ls)[0]                        # [t >> ls, q, t & mask]
            t = np.arange(P // 8)
            for q in range(8):
                assert np.array_equal(v[t >> ls, q, t & ((1 << ls) - 1)], pos[:, q])


@pytest.mark.parametrize('N', [8, 9, 24, 100, 127, 129, 1000, 2049, 40, 64, 301, 1025])
def test_model_matches_scipy_forward_and_inverse(N):
    """The device's dataflow restated in numpy: reorder for odd and even N, padding, the digit-reversed Bhat order with
    the chosen radices, the inverse pairing -- forward and inverse, rows and columns."""
    rng = np.random.default_rng(N)
    tb = cm.tables(N)
    x = rng.standard_normal((N, N))
    y = fftpack.dctn(x, norm='ortho')
    got = cm.dct2d(x, tb)
    assert np.max(np.abs(got - y)) <= TOL * np.max(np.abs(y)), np.max(np.abs(got - y)) / np.max(np.abs(y))
    back = cm.dct2d(y, tb, inverse=True)
    want = fftpack.idctn(y, norm='ortho')
    assert np.max(np.abs(back - want)) <= TOL * np.max(np.abs(want)), np.max(np.abs(back - want)) / np.max(np.abs(want))


@pytest.mark.parametrize('N', [9, 100])
def test_model_single_basis_modes(N):
    """A single cosine mode goes to a unit impulse and back: a permutation or sign error common to both directions
    would pass a round trip, not this."""
    tb = cm.tables(N)
    n = np.arange(N)
    for k in (0, 1, N // 2, N - 1):
        f = np.sqrt((1.0 if k == 0 else 2.0) / N)
        mode = f * np.cos(np.pi * k * (2 * n + 1) / (2 * N))
        X = cm.lines(mode[None, :], tb)[0]
        e = np.zeros(N)
        e[k] = 1.0
        assert np.max(np.abs(X - e)) <= TOL, (k, np.max(np.abs(X - e)))
        assert np.max(np.abs(cm.lines(e[None, :], tb, inverse=True)[0] - mode)) <= TOL, k


def test_model_in_complex64_stays_within_the_fp32_tolerance():
    """Tables rounded once to float, arithmetic in complex64: the fp32 engine's tolerance (4e-6) holds with room at
    N = 100, and the model stays under the 2e-5 cap of the bound that takes over above N = 1000."""
    N = 100
    tb = cm.tables(N, np.complex64)
    x = np.random.default_rng(1).standard_normal((N, N))
    y = fftpack.dctn(x, norm='ortho')
    assert cm.dct2d(x, tb).dtype == np.float32
    assert np.max(np.abs(cm.dct2d(x, tb) - y)) <= 4e-6 * np.max(np.abs(y))
    # N = 1025 (P = 4096, three exchange passes): above N = 1000 the bound of the GPU test is twice this model's own
    # error and never above 2e-5, the project's fp32 transform tolerance (tests/test_gpu_parity.py: test_fp32_dctn).
    # The model itself has to stay under that cap, in both directions, on the GPU test's input.
    N = 1025
    tb = cm.tables(N, np.complex64)
    x = np.random.default_rng(N).standard_normal((N, N))
    y = fftpack.dctn(x, norm='ortho')
    ef = float(np.max(np.abs(cm.dct2d(x, tb) - y)) / np.max(np.abs(y)))
    ei = float(np.max(np.abs(cm.dct2d(y, tb, inverse=True) - x)) / np.max(np.abs(x)))
    assert ef <= 2e-5, f"complex64 model N={N}: forward {ef:.3e} of the largest entry"
    assert ei <= 2e-5, f"complex64 model N={N}: inverse {ei:.3e} of the largest entry"


@pytest.fixture(scope='module')
def tables_exe(tmp_path_factory):
    """tests/chirp_tables.cpp, host C++ only, built with the address and undefined-behaviour sanitizers."""
    from chsimpy_amd import _build
    exe = str(tmp_path_factory.mktemp('chirp') / 'chirp_tables')
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Wall',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I' + _build.CSRC,
                    os.path.join(ROOT, 'tests', 'chirp_tables.cpp'), '-o', exe], check=True)
    return exe


def test_host_tables_against_direct_evaluation(tables_exe):
    """tests/chirp_tables.cpp: every table of chs_chirp_host.h for N in {9, 100, 129, 250} against long double
    evaluation of its definition (Bhat: the O(P^2) sum), the position map against a naive decimation-in-frequency
    network."""
    from chsimpy_amd import _build
    r = subprocess.run([tables_exe], capture_output=True, text=True)
    assert r.returncode == 0 and '\n0 failures' in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    # the header is host code: nothing of HIP in it
    hdr = open(os.path.join(_build.CSRC, 'chs_chirp_host.h')).read()
    assert not re.search(r'#include\s*[<"](hip/|chs_common|chs_fast|chs_cx)', hdr)
    # the program includes that header alone
    prog = open(os.path.join(ROOT, 'tests', 'chirp_tables.cpp')).read()
    assert re.findall(r'#include\s*"([^"]+)"', prog) == ['chs_chirp_host.h']


@pytest.mark.parametrize('N', [9, 100, 129, 40, 301])
def test_model_tables_are_the_headers_tables(tables_exe, N):
    """The plan and every table of chs_chirp_host.h, rounded to double and printed by `chirp_tables --dump N`, against
    the model's own (tools/chirp_model.py).  Both evaluate the chirp, the factors and the twiddles in extended precision
    and round once: they may differ by the last bit (4 ulp of the table's largest entry allowed).  Bhat comes from a
    long double FFT in the header and from numpy's double FFT in the model: 1e-13 of its largest entry."""
    r = subprocess.run([tables_exe, '--dump', str(N)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    tb = cm.tables(N)
    pl = tb['plan']
    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == 'plan':
            assert [int(v) for v in f[1:]] == [pl['P'], pl['logP'], pl['nt'], pl['rl']]
        else:
            got.setdefault(f[0], []).append((int(f[1]), complex(float(f[2]), float(f[3]))))
    assert sorted(got) == ['bhat', 'fin', 'fout', 'iin', 'iout', 'tw']
    for name, rows in got.items():
        assert [i for i, _ in rows] == list(range(len(tb[name]))), name
        hdr = np.array([v for _, v in rows])
        tol = 1e-13 if name == 'bhat' else 4 * np.finfo(np.float64).eps
        err = np.max(np.abs(hdr - tb[name])) / np.max(np.abs(tb[name]))
        assert err <= tol, (name, err)


def test_model_bhat_is_the_dft_of_b_at_freq_of_pos():
    """Bhat of the model at position p is the plain DFT sum of b over P at frequency freq_of_pos(p)."""
    tb = cm.tables(129)
    pl = tb['plan']
    N, P = 129, pl['P']
    n = np.arange(N)
    w = np.exp(-1j * np.pi * ((n * n) % (2 * N)) / N)
    b = np.zeros(P, dtype=complex)
    b[:N] = np.conj(w)
    b[P - n[1:]] = np.conj(w[1:])
    k = cm.freq_of_pos(pl, np.arange(P))
    direct = np.array([np.sum(b * np.exp(-2j * np.pi * np.arange(P) * f / P)) for f in k]) / P
    assert np.max(np.abs(direct - tb['bhat'])) < 1e-13


def test_engine_constants_of_header_and_binding():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    assert re.search(r'#define\s+CHS_ENGINE_CHIRP\s+3\b', hdr)
    assert _lib.ENGINES['chirp'] == 3 and _lib.CHS_ENGINE_CHIRP == 3
    m = re.search(r'#define\s+CHS_CHIRP_AUTO_MIN_N\s+(\d+)\b', hdr)
    assert m and int(m.group(1)) == _lib.CHS_CHIRP_AUTO_MIN_N
    assert _lib.CHS_CHIRP_AUTO_MIN_N >= 129      # N = 64 and N = 100 under 'auto' stay on the direct engine
    assert _lib.ENGINES == {'auto': 0, 'direct': 1, 'fast': 2, 'chirp': 3}


def test_a_batch_still_runs_the_fast_engine_only():
    p = chsimpy_amd.Parameters()
    p.N, p.kappa_tilde, p.engine = 256, 3e-4, 'chirp'
    why = bt.scope_error(p)
    assert why and 'fast engine only' in why
    with pytest.raises(ValueError, match='fast engine only'):
        bt.validate([p])
