"""GPU tests of the chirp engine's step loop at the grid sizes where the launch shapes of the natural-order pointwise
kernels change (chsimpy_amd/csrc/chs_pointwise.hip, chs_chirp_kernels.h).  Only the chirp engine takes these kernels to
large N (the direct engine is O(N^3) and is tested at N <= 128), and at N <= 129 (tests/test_gpu_chirp.py) every one of
them has a single column block:

  N = 301    k_diag with blockIdx.y = 1 and 45 columns in its last column block (partDiag index, nDiagBlocks);
             k_chirp_transpose with 10 x 10 tiles and a ragged edge of 13; adaptive: two k_colmin_slices blocks, the
             second of 45 columns, five k_colsum_slices column blocks, the last ragged
  N = 1025   the first N at which k_spectral's cap of 4096 blocks bites and its grid-stride loop goes round again
             (1025^2 > 4096 * 256); P = 4096, the 512-thread line kernel; five k_diag column blocks, the last of one column
  N = 2049   P = 8192, the 1024-thread line kernel; nine k_diag column blocks

A wrong index in any of these still gives finite rows and a smooth field: the runs are compared with the oracle, the
fp64 ones at the project's 1e-9 in every record column, U, the counters, t0 and time_passed."""
import numpy as np
import pytest

import chsimpy_amd
from oracle import chs_oracle as orc

pytestmark = pytest.mark.gpu

from gpu_helpers import RTOL, compare_run, compare_snapshots, drive, fmt_errs, log_line, make, relerr  # noqa: E402


def _runs_chirp(p):
    s = chsimpy_amd.Solver(p)
    engine = s._get_engine().engine
    s.close()
    return engine == 'chirp'


@pytest.mark.parametrize("N,nt", [(301, 20), (1025, 4), (2049, 3)])
def test_steps_against_the_oracle(gpu, N, nt):
    p = make(N, nt, 'chirp')
    assert _runs_chirp(p)
    compare_run(p, {}, rtol=RTOL)


def test_fp32_steps_against_the_oracle_n1025(gpu):
    """N=1025, 3 steps in float32 against the fp64 oracle, with the project's fp32 step tolerances
    (tests/test_gpu_parity.py: test_fp32_fast_engine_small_grids_vs_oracle): U rtol 2e-4, E rtol 1e-5, PS rtol 2e-3
    from row 1 on, mean(U) rel 2e-6; the step column, computed_steps and stop_reason exact.  The oracle stepped with the
    complex64 model of the transform lands at U 1.4e-7, E 2e-11, PS 1.4e-7, mass 1e-8: the algorithm is well inside.
    The direct engine's distances at this size are logged next to the chirp engine's; their ratio is not asserted
    (nobody has measured it here)."""
    N, nt = 1025, 3
    o = orc.OracleSolver(orc.make_params(N, nt))
    o.prepare()
    o.solve_or_resume()
    to = o.timedata.data()
    for engine in ('chirp', 'direct'):
        s = chsimpy_amd.Solver(make(N, nt, engine, dtype='float32'))
        s.prepare()
        sol = s.solve_or_resume()
        assert s._engine.engine == engine
        td = sol.timedata.data()
        d = {'U': relerr(sol.U, o.U), 'mass': abs(float(sol.U.mean()) / float(o.U.mean()) - 1.0)}
        for c in range(1, 9):
            d[f'col{c}'] = relerr(td[:, c], to[:, c]) if c != 3 else float(np.max(np.abs(td[:, c] - to[:, c])))
        log_line(f"fp32 N={N} {nt} steps {engine} vs fp64 oracle: {fmt_errs(d)}")
        if engine == 'chirp':
            assert td.shape == to.shape and np.array_equal(td[:, 0], to[:, 0])
            assert sol.computed_steps == o.computed_steps and sol.stop_reason == o.stop_reason
            assert np.allclose(sol.U, o.U, rtol=2e-4, atol=0), d['U']
            assert np.allclose(td[:, 1], to[:, 1], rtol=1e-5, atol=0), d['col1']       # E
            assert np.allclose(td[1:, 7], to[1:, 7], rtol=2e-3, atol=0), relerr(td[1:, 7], to[1:, 7])   # PS
            assert sol.U.mean() == pytest.approx(o.U.mean(), rel=2e-6), d['mass']     # mass conservation in fp32
        s.close()


def test_adaptive_time_n301(gpu):
    """tests/test_gpu_chirp.py: test_adaptive_time at N=301, seeded at step 499 where the rule begins to fire.  delt_dyn
    is a column SUM and grows with N: delt_max = 4.9e-7 / N, the scaling of test_adaptive_time_fast_engine (on the CPU
    oracle delt goes 3e-8 -> 1.139e-7 -> 1.408e-7 over the three calls)."""
    N, chunks = 301, (3, 4, 2)
    kw = dict(adaptive_time=True, delt_max=4.9e-7 / N)
    s = chsimpy_amd.Solver(make(N, 600, 'chirp', **kw))
    got = drive(s, chunks, seed=499)[0]
    assert s._engine.engine == 'chirp'
    s.close()
    want = drive(orc.OracleSolver(orc.make_params(N, 600, **kw)), chunks, seed=499)[0]
    assert len({w['delt'] for w in want}) > 1        # delt did move
    worst = compare_snapshots(got, want, rtol=1e-9)
    log_line(f"chirp adaptive N={N} seeded at 499, chunks {chunks}: {fmt_errs(worst)}")
