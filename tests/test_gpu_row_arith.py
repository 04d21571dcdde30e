"""GPU tests of the arithmetic of the row kernels and of the transform core they share with k_col:
the radix-8 / radix-16 butterflies whose odd eighth roots are folded into the following additions
(chs_fast_core.h: bfly2_rot, dft4_rot), the energy density and EnergieEut from shared intermediates
(chs_math.h: chs_energy_mu_from_logs) and the table-driven log with its integer index and domain word
(chs_log_unit_tab_f64).  Shapes: the smallest that reach each changed path."""
import numpy as np
import pytest
from scipy import fft as scifft

import chsimpy_amd
from chsimpy_amd import _lib

pytestmark = pytest.mark.gpu

from gpu_helpers import RTOL, compare_run, log_line, make  # noqa: E402

# what tools/row_arith_model.py prints for the ramp field (profiles/row_arith_parity_margins.txt): the largest relative
# difference of the modelled energy density / EnergieEut of one grid point from the oracle's numpy expressions
RAMP_MODEL_MAX_REL = 2.754e-11
RAMP_RTOL = max(4 * RAMP_MODEL_MAX_REL, RTOL)


# N = 256: the first plan with a radix-8 pass (4*8*4); N = 2048: the plan with a radix-16 pass (8*16*8), in both types
@pytest.mark.parametrize("dtype,N", [('float64', 256), ('float64', 2048), ('float32', 256), ('float32', 2048)])
def test_transforms_match_scipy(gpu, dtype, N):
    """fp64: 1e-12 of the largest entry (test_gpu_parity.py: test_dctn_matches_scipy); fp32: 2e-5 (test_fp32_dctn)."""
    s = chsimpy_amd.Solver(make(N, 2, 'fast', dtype=dtype), np.full((N, N), 0.5))
    eng = s._get_engine()
    assert eng.engine == 'fast'
    X = np.random.default_rng(N).standard_normal((N, N))
    if dtype == 'float32':
        X = X.astype(np.float32).astype(np.float64)
    tol = 1e-12 if dtype == 'float64' else 2e-5
    Yr = scifft.dctn(X, norm='ortho', workers=8)
    ef = float(np.max(np.abs(eng.dctn(X) - Yr)) / np.max(np.abs(Yr)))
    ei = float(np.max(np.abs(eng.dctn(Yr, inverse=True) - X)) / np.max(np.abs(X)))
    log_line(f"row arith dctn N={N} {dtype}: forward {ef:.3e} inverse {ei:.3e} of the largest entry (bound {tol:.0e})")
    s.close()
    assert ef < tol, ef
    assert ei < tol, ei


@pytest.mark.parametrize("ntmax", [1, 40])
def test_n256_steps_vs_oracle(gpu, ntmax):
    """One literal call of 1 and of 40 steps at N=256: every record column and the final U within gpu_helpers.RTOL."""
    compare_run(make(256, ntmax, 'fast'), {})


def ramp_field(N):
    """Every row runs from 1e-6 to 1 - 1e-6 (so every lane meets every magnitude of U and 1-U), with the usual
    uniform noise of relative size 0.01 scaled by the distance to the nearer end: the field stays inside (0, 1)."""
    rng = np.random.default_rng(7)
    r = np.broadcast_to(np.linspace(1e-6, 1 - 1e-6, N)[None, :], (N, N))
    return r + 0.01 * (rng.random((N, N)) - 0.5) * np.minimum(r, 1 - r)


def test_n256_ramp_to_both_ends_vs_oracle(gpu):
    """U = 1e-6 .. 1-1e-6, where U log U + (1-U) log(1-U) cancels worst, one 1-step call.  Bound: the CPU model of the
    kernel's formulas (tools/row_arith_model.py, exact fma) differs from the oracle's expressions by at most 2.754e-11
    (EnergieEut at its zero crossing; energy density 4.3e-16) over that ramp; four times that is 1.1e-10, below the
    existing tolerance 1e-9, which therefore holds as the floor."""
    assert RAMP_RTOL == RTOL
    compare_run(make(256, 1, 'fast'), {}, U_init=ramp_field(256), rtol=RAMP_RTOL)


@pytest.mark.parametrize("bad", [1.0, -0.25])
def test_field_outside_the_unit_interval_gives_the_nan_record(gpu, bad):
    """One grid point at 1.0 (log(1-U) of zero) or at a negative value, N=128, a 3-step call.  As the existing tests
    assert it (test_gpu_parity.py: test_nan_raises_assertion_like_the_reference, test_gpu_batch.py:
    test_nan_status_through_the_c_abi): a field that is bad at prepare() raises the reference's assertion; one that
    turns bad afterwards ends the call with CHS_ENAN and a single row that holds the NaN."""
    N = 128
    good = np.full((N, N), 0.875)
    U_bad = good.copy()
    U_bad[5, 77] = bad
    s = chsimpy_amd.Solver(make(N, 3, 'fast'), U_bad)
    with pytest.raises(AssertionError):
        s.prepare()
        s.solve_or_resume()
    s.close()
    s = chsimpy_amd.Solver(make(N, 3, 'fast'), good)
    s.prepare()
    eng = s._get_engine()
    eng.set_U(U_bad)
    rows, rc = eng.step_n(3)
    s.close()
    assert rc == _lib.CHS_ENAN
    assert rows.shape[0] == 1 and np.isnan(rows[-1, 1:]).any()


def test_n4096_three_steps_vs_oracle(gpu):
    """The headline size: three steps of the fused pipeline (k_row_fwd2, k_col, the fused k_row_inv) against the oracle."""
    compare_run(make(4096, 3, 'fast'), {})
