"""GPU tests of the chirp engine (CHS_ENGINE_CHIRP, chsimpy_amd/csrc/chs_chirp.hip): the transform for any N in
[8, 4096] against scipy and on single basis modes, and the step loop it carries -- every stop rule, adaptive dt, jitter,
chunked calls, fp32 -- against the oracle, with the tolerances of the direct and fast engines' tests."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.fftpack as scifft

import chsimpy_amd
from chsimpy_amd import _lib
from oracle import chs_oracle as orc

pytestmark = pytest.mark.gpu

from gpu_helpers import RTOL, compare_run, compare_snapshots, drive, fmt_errs, log_line, make, relerr  # noqa: E402


def _basis(N, k):
    """Column k of the orthonormal DCT-III matrix (the angle reduced modulo 2 pi in integers)."""
    n = np.arange(N)
    m = (k * (2 * n + 1)) % (4 * N)
    c = np.cos(np.pi * m / (2 * N)) * np.sqrt(2.0 / N)
    return c / np.sqrt(2.0) if k == 0 else c


def _model():
    """tools/chirp_model.py: the engine's dataflow in numpy; in complex64 it is the yardstick of the fp32 transform above
    N = 1000."""
    spec = importlib.util.spec_from_file_location(
        'chirp_model', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'chirp_model.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


FP32_TOL = 4e-6        # N <= 1000: the complex64 model stays under it with room (<= 2.7e-6)
FP32_CAP = 2e-5        # the project's fp32 transform tolerance (tests/test_gpu_parity.py: test_fp32_dctn)

# Every plan (logP, nt, rl) of chirp_plan, P = 16 ... 8192, in both types.
# 127: 2N-1 = 253 fills P = 256; 129: the first N of P = 512; 2049: the first N of the largest P; 4096: the last N
# P = 128 (2, 1): N = 40 a partial last workgroup (8 of 16 lines), N = 64 fills P
# P = 1024 (3, 1): N = 301 odd, 1 of 2 lines in the last workgroup, N = 512 fills P (a power of two, even-N Makhoul map)
# P = 4096 (3, 0): N = 1025 the first N of the 512-thread launch, N = 2048 fills P
@pytest.mark.parametrize("dtype,N", [('float64', N) for N in (8, 9, 24, 100, 127, 129, 1000, 2049, 4096)] +
                         [('float32', N) for N in (9, 100, 129, 1000)] +
                         [('float64', N) for N in (40, 64, 301, 512, 1025, 2048)] +
                         [('float32', N) for N in (8, 24, 40, 301, 1025, 2049)])
def test_dctn_matches_scipy(gpu, dtype, N):
    """fp64: 1e-12 of the largest entry.  fp32: 4e-6 up to N = 1000; above, the algorithm alone outgrows that (the
    complex64 model: 4.4e-6 at N = 2048, 7.1e-6 at N = 4095), so the bound of each direction is twice the error of the
    model in that direction on the same input, and never above 2e-5.  Twice, because the kernel contracts to FMA and
    orders the radix-8 butterflies differently from numpy's complex64 arithmetic, with the same number of roundings."""
    s = chsimpy_amd.Solver(make(N, 2, 'chirp', dtype=dtype))
    eng = s._get_engine()
    assert eng.engine == 'chirp'
    X = np.random.default_rng(N).standard_normal((N, N))
    Yr = scifft.dctn(X, norm='ortho')
    tolf = toli = 1e-12 if dtype == 'float64' else FP32_TOL
    model = ''
    if dtype == 'float32' and N > 1000:
        cm = _model()
        tb = cm.tables(N, np.complex64)
        mf = float(np.max(np.abs(cm.dct2d(X, tb) - Yr)) / np.max(np.abs(Yr)))
        mi = float(np.max(np.abs(cm.dct2d(Yr, tb, inverse=True) - X)) / np.max(np.abs(X)))
        tolf, toli = min(2 * mf, FP32_CAP), min(2 * mi, FP32_CAP)
        model = f"; complex64 model forward {mf:.3e} inverse {mi:.3e}, bounds {tolf:.3e} {toli:.3e}"
    ef = float(np.max(np.abs(eng.dctn(X) - Yr)) / np.max(np.abs(Yr)))
    ei = float(np.max(np.abs(eng.dctn(Yr, inverse=True) - X)) / np.max(np.abs(X)))
    log_line(f"chirp dctn N={N} {dtype}: forward {ef:.3e} inverse {ei:.3e} of the largest entry{model}")
    assert ef < tolf, (ef, tolf)
    assert ei < toli, (ei, toli)
    s.close()


def test_n_above_the_range_is_refused(gpu):
    with pytest.raises(_lib.EngineError, match=r'chirp engine needs N in \[8, 4096\]'):
        chsimpy_amd.Solver(make(4097, 2, 'chirp'))._get_engine()


@pytest.mark.parametrize("N", [100, 129, 40, 1025])
def test_dctn_single_basis_modes(gpu, N):
    """Forward dctn of the basis mode (k, l) is the unit impulse at (k, l), the inverse of the impulse is the mode: a
    permutation or sign error common to both directions moves the impulse.  N = 40 (P = 128) and N = 1025 (P = 4096,
    16 mode pairs) are plans that no other size here runs."""
    s = chsimpy_amd.Solver(make(N, 2, 'chirp'), np.full((N, N), 0.5))
    eng = s._get_engine()
    assert eng.engine == 'chirp'
    K = [0, 1, N // 2 - 1, N // 2, N - 2, N - 1] if N < 1025 else [0, 1, N // 2, N - 1]
    ef = ei = 0.0
    for k in K:
        for l in K:
            B = np.outer(_basis(N, k), _basis(N, l))
            Y = eng.dctn(B)
            Y[k, l] -= 1.0
            ef = max(ef, float(np.max(np.abs(Y))))
            assert ef < 1e-12, (k, l, ef, np.unravel_index(np.argmax(np.abs(Y)), Y.shape))
            E = np.zeros((N, N))
            E[k, l] = 1.0
            Z = eng.dctn(E, inverse=True)
            ei = max(ei, float(np.max(np.abs(Z - B)) / np.max(np.abs(B))))
            assert ei < 1e-12, (k, l, ei)
    log_line(f"chirp basis modes N={N}: forward {ef:.3e} inverse {ei:.3e}")
    s.close()


@pytest.mark.parametrize("N,nt", [(24, 60), (100, 60), (129, 30)])
def test_steps_against_the_oracle(gpu, N, nt):
    compare_run(make(N, nt, 'chirp'), {})


@pytest.mark.parametrize("N,delt,stop_step", [(100, 1e-6, 313), (72, 2e-6, 79)])
def test_energy_stop(gpu, N, delt, stop_step):
    """The energy rule (full_sim=False) ends the run on the device; at N=100 behind the first 256-step issue batch of
    an armed stop rule, with empty launches behind the halt that every chirp kernel has to sit out."""
    sol, o = compare_run(make(N, 4000, 'chirp', full_sim=False, delt=delt), dict(full_sim=False, delt=delt))
    assert o.stop_reason == 'energy' and o.computed_steps == stop_step, (o.stop_reason, o.computed_steps)
    assert sol.computed_steps == stop_step


def test_adaptive_time(gpu):
    """adaptive_time (solver.py:177-193) seeded at step 499, where the rule begins to fire: the column-sum minimum of
    the natural-order engines' pre-step."""
    chunks, kw = (3, 4, 2), dict(adaptive_time=True)
    s = chsimpy_amd.Solver(make(100, 600, 'chirp', **kw))
    got = drive(s, chunks, seed=499)[0]
    assert s._engine.engine == 'chirp'
    s.close()
    want = drive(orc.OracleSolver(orc.make_params(100, 600, **kw)), chunks, seed=499)[0]
    assert len({w['delt'] for w in want}) > 1        # delt did move
    worst = compare_snapshots(got, want, rtol=1e-9)
    log_line(f"chirp adaptive N=100 seeded at 499, chunks {chunks}: {fmt_errs(worst)}")


def test_jitter_noise_drawn_on_the_device_continues_the_host_stream(gpu):
    N, nt = 100, 25
    runs = {}
    for dev in (True, False):
        s = chsimpy_amd.Solver(make(N, nt, 'chirp', jitter=0.02))
        s.device_rng = dev
        s.prepare()
        s.solve_or_resume(10)
        sol = s.solve_or_resume(nt - 10)
        assert s._engine.engine == 'chirp'
        runs[dev] = (sol.U.copy(), sol.timedata.data().copy(), s._pcg.bit_generator.state['state']['state'])
        s.close()
    assert runs[True][2] == runs[False][2]                      # generator state
    assert np.array_equal(runs[True][1], runs[False][1])        # every recorded scalar
    assert np.array_equal(runs[True][0], runs[False][0])        # the field
    compare_run(make(N, 12, 'chirp', jitter=0.001), dict(jitter=0.001))


def test_resume_chunks_match_oracle_chunks(gpu):
    s = chsimpy_amd.Solver(make(100, 0, 'chirp'))
    o = orc.OracleSolver(orc.make_params(100, 0))
    s.prepare(); o.prepare()
    for chunk in (5, 7, 1, 12):
        sol = s.solve_or_resume(chunk)
        o.solve_or_resume(chunk)
        assert sol.computed_steps == o.computed_steps
        assert np.allclose(sol.U, o.U, rtol=RTOL, atol=0)
    assert np.allclose(sol.timedata.data(), o.timedata.data(), rtol=RTOL, atol=1e-300)
    s.close()


def test_fp32_run_is_as_close_to_the_oracle_as_the_direct_engines(gpu):
    """N=100, 60 steps in float32: the chirp engine's distance from the fp64 oracle, in U and in every record column,
    is at most 4x the direct engine's own (the convention of tests/test_gpu_batch_adaptive.py).  The direct engine
    accumulates its products in fp64 and rounds coefficient by coefficient, so its own distance is small; the chirp
    kernel sends the constant part of a line round the convolution for that reason (chs_chirp.hip).  Both distances
    are logged."""
    N, nt = 100, 60
    o = orc.OracleSolver(orc.make_params(N, nt))
    o.prepare()
    o.solve_or_resume()
    to = o.timedata.data()
    dist = {}
    for engine in ('chirp', 'direct'):
        s = chsimpy_amd.Solver(make(N, nt, engine, dtype='float32'))
        s.prepare()
        sol = s.solve_or_resume()
        assert s._engine.engine == engine
        td = sol.timedata.data()
        assert td.shape == to.shape and np.array_equal(td[:, 0], to[:, 0])
        d = {'U': relerr(sol.U, o.U)}
        for c in range(1, 9):
            d[f'col{c}'] = relerr(td[:, c], to[:, c]) if c != 3 else float(np.max(np.abs(td[:, c] - to[:, c])))
        dist[engine] = d
        log_line(f"fp32 N={N} {nt} steps {engine} vs fp64 oracle: {fmt_errs(d)}")
        s.close()
    for k, own in dist['direct'].items():
        assert dist['chirp'][k] <= 4 * own, (k, dist['chirp'][k], own)


def test_auto_resolution(gpu):
    """'auto': the fast engine where it exists, the chirp engine from CHS_CHIRP_AUTO_MIN_N (129: measured, DESIGN.md
    section 3a) to 4096, the direct engine below and above."""
    first = _lib.CHS_CHIRP_AUTO_MIN_N
    while first & (first - 1) == 0:
        first += 1
    assert 129 <= first <= 4096
    want = {64: 'direct', 100: 'direct', 128: 'fast', 512: 'fast', first: 'chirp', 1000: 'chirp', 4097: 'direct'}
    for N, engine in want.items():
        s = chsimpy_amd.Solver(make(N, 2))
        assert s._get_engine().engine == engine, (N, s._get_engine().engine)
        s.close()


def test_a_pooled_engine_repeats_its_run_bit_for_bit(gpu):
    _lib.pool_clear()
    runs = []
    for _ in range(2):
        s = chsimpy_amd.Solver(make(100, 20, 'chirp'))
        s.prepare()
        sol = s.solve_or_resume()
        runs.append((sol.U.copy(), sol.timedata.data().copy()))
        s.close()
        assert _lib.pool_count() == 1          # parked, and taken into use again by the second run
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
