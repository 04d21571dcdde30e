"""The comparison helpers of tests/gpu_helpers.py (compare_snapshots, compare_fields), which the issue-mode GPU tests
use, must reject a subtly wrong solver.  Here they compare the oracle with mutated copies of itself at N=64/128 (no
GPU): each mutation must fail each helper, and an unmutated copy must pass both."""
import numpy as np
import pytest
import scipy.fftpack as scifft

from oracle import chs_oracle as orc
from gpu_helpers import compare_fields, compare_snapshots, drive


class Mutant(orc.OracleSolver):
    """OracleSolver.solve_or_resume with one of four subtle errors switched on:
    'seig'  -- one Seig entry off by 1e-7 relative;
    'odd'   -- delt re-evaluated on odd steps instead of even ones;
    'limit' -- the time limit checked after the update of U instead of before it;
    'stop'  -- after an energy stop, U of the following step returned instead of that of the stopping step."""

    def __init__(self, params, mutation):
        super().__init__(params)
        self.mutation = mutation
        if mutation == 'seig':
            self.Seig = self.Seig.copy()
            self.Seig[-2, -3] *= 1 + 1e-7   # (a high wavenumber, see CASES)

    def solve_or_resume(self, nsteps=None, record=None):
        m = self.mutation
        p = self.params
        N = p.N
        if nsteps is None:
            nsteps = max(p.ntmax, 0)
        time_limit = p.time_max * 60 if (p.time_max is not None and p.time_max > 0) else None
        Seig, CHeig = self.Seig, self.CHeig
        U = self.U
        hat_U = scifft.dctn(U, norm='ortho')
        itbegin = 1 if self.computed_steps == 1 else 0
        for it in range(itbegin, nsteps):
            EnergieEut = self.mu(U)
            parity = 1 if m == 'odd' else 0
            if p.adaptive_time and self.computed_steps > 500 and np.remainder(self.computed_steps, 2) == parity:
                delt_dyn = np.linalg.norm(p.delt_max / np.sqrt(1 + 500 / 8 * np.abs(EnergieEut) ** 2), ord=-1)
                delt_new = max(p.delt, delt_dyn)
                self.delt = 0.75 * self.delt + 0.25 * delt_new if delt_new / self.delt > 1.15 else delt_new
                CHeig, Seig = orc.get_coefficients(N, self.kappa_tilde, self.delt, self.delx2)
            self.time_delta_sum += self.delt
            self.time_passed = self.time_delta_sum / p.M_tilde
            over = time_limit is not None and self.time_passed > time_limit
            if over and m != 'limit':
                self.stop_reason = 'time-limit'
                break
            hat_U = (hat_U + Seig * scifft.dctn(EnergieEut, norm='ortho')) / CHeig
            U = scifft.idctn(hat_U, norm='ortho')
            if over:
                self.stop_reason = 'time-limit'
                break
            E, E2 = self._energies(U)
            PS, Ra = self._stats(U)
            self.timedata.insert(it=self.computed_steps, delt=self.delt, E=E, E2=E2, SA=np.sum(U < p.threshold) / N ** 2,
                                 domtime=self.time_passed ** (1 / 3), Ra=Ra, L2=np.linalg.norm(EnergieEut) / N ** 2, PS=PS)
            self.computed_steps += 1
            if record is not None:
                record(self.computed_steps - 1, U)
            if not self.skip_check and self.timedata.energy_falls(self.computed_steps - 1):
                self.tau0 = self.computed_steps
                self.t0 = self.time_passed
                if not p.full_sim:
                    self.stop_reason = 'energy'
                    if m == 'stop':
                        hat_U = (hat_U + Seig * scifft.dctn(self.mu(U), norm='ortho')) / CHeig
                        U = scifft.idctn(hat_U, norm='ortho')
                    break
                self.skip_check = True
        self.U = U
        return self


# mutation -> (N, oracle parameters, chunks, seeded step): a run in which the mutated code path matters.  'seig': the
# entry sits at a high wavenumber, where Seig * dctn(mu) is a few per cent of hat_U per step; the error it leaves in U
# is 1e-12 pointwise (below any tolerance) but 2e-8 of the fluctuation scale in that mode: what catches it is the
# spectral comparison (gpu_helpers.spectral_err).  An entry at a low wavenumber, where Seig is ~1e-6 of that, leaves
# 2e-11 in the spectrum, below the 1e-9 of the fp64 tests.
CASES = {
    'seig': (128, dict(), (12, 1, 7), None),
    'odd': (64, dict(adaptive_time=True), (3, 4, 2), 499),
    'limit': (64, dict(full_sim=False, time_max=8.5 * 3e-8 / 1.71e-8 / 60), (4, 10, 2), None),
    'stop': (128, dict(full_sim=False, delt=1e-6), (200, 1, 3), None),
}


def _runs(mutation, mutant):
    N, kw, chunks, seed = CASES[mutation]
    p = orc.make_params(N, 10 ** 6, **kw)
    o = Mutant(p, mutation if mutant else None)
    return drive(o, chunks, seed, record=True)


@pytest.fixture(scope='module')
def reference_runs():
    return {m: _runs(m, False) for m in CASES}


@pytest.mark.parametrize("mutation", list(CASES))
def test_unmutated_copy_passes_both_helpers(reference_runs, mutation):
    """The restated loop without a mutation is the oracle bit for bit (so that what fails below is the mutation)."""
    N, kw, chunks, seed = CASES[mutation]
    want = drive(orc.OracleSolver(orc.make_params(N, 10 ** 6, **kw)), chunks, seed, record=True)
    got = reference_runs[mutation]
    compare_snapshots(got[0], want[0], rtol=0, rtol_U=0, rtol_spec=0, rtol_time=0)
    compare_fields(got[1], want[1], rtol=0)


@pytest.mark.parametrize("mutation", list(CASES))
def test_compare_snapshots_rejects_mutation(reference_runs, mutation):
    """compare_snapshots at the tolerances of the fp64 GPU tests (rtol 1e-9)."""
    got = _runs(mutation, True)[0]
    with pytest.raises(AssertionError):
        compare_snapshots(got, reference_runs[mutation][0])


@pytest.mark.parametrize("mutation", list(CASES))
def test_compare_fields_rejects_mutation(reference_runs, mutation):
    """compare_fields (per-step fields matched by computed_steps) at rtol 1e-9."""
    got = _runs(mutation, True)[1]
    with pytest.raises(AssertionError):
        compare_fields(got, reference_runs[mutation][1])
