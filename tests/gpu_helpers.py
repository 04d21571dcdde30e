"""Shared helpers of the ``-m gpu`` parity tests: parameter construction and the run-against-the-oracle
comparison (timedata columns, final U, counters, stop reason)."""
import os

import numpy as np
import pytest

import chsimpy_amd
from oracle import chs_oracle as orc

KAPPA = 0.0002989112919661156
RTOL = 1e-9
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def make(N, ntmax, engine='auto', **kw):
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.engine = N, ntmax, True, KAPPA, engine
    for k, v in kw.items():
        setattr(p, k, v)
    if 'threshold' not in kw:
        p.threshold = p.XXX
    return p


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def log_line(text):
    """Measured parity margins go to gpurun_out/parity.log on the GPU box (copied to profiles/ at round end)."""
    d = os.path.join(os.path.dirname(os.path.dirname(__file__)), 'gpurun_out')
    if os.path.isdir(d):
        with open(os.path.join(d, 'parity.log'), 'a') as f:
            f.write(text.rstrip() + '\n')


def _log_parity(p, engine, eu, cols):
    d = os.path.join(os.path.dirname(os.path.dirname(__file__)), 'gpurun_out')
    if os.path.isdir(d):
        with open(os.path.join(d, 'parity.log'), 'a') as f:
            f.write(f"N={p.N} ntmax={p.ntmax} engine={engine} adaptive={p.adaptive_time} jitter={p.jitter} "
                    f"delt={p.delt}: max rel err U={eu:.3e} E={cols[0]:.3e} E2={cols[1]:.3e} Ra={cols[2]:.3e} "
                    f"L2={cols[3]:.3e} PS={cols[4]:.3e}\n")


def compare_run(p, okw, U_init=None, rtol=RTOL, cols=(1, 2, 3, 4, 5, 6, 7, 8)):
    s = chsimpy_amd.Solver(p, U_init)
    s.prepare()
    sol = s.solve_or_resume()
    o = orc.OracleSolver(orc.make_params(p.N, p.ntmax, **okw), U_init)
    o.prepare()
    o.solve_or_resume()
    td, to = sol.timedata.data(), o.timedata.data()
    assert td.shape == to.shape
    assert np.array_equal(td[:, 0], to[:, 0])
    for c in cols:
        assert np.allclose(td[:, c], to[:, c], rtol=rtol, atol=1e-300), (c, relerr(td[:, c], to[:, c]))
    _log_parity(p, s._engine.engine, relerr(sol.U, o.U), [relerr(td[:, c], to[:, c]) for c in (1, 2, 5, 6, 7)])
    assert np.allclose(sol.U, o.U, rtol=rtol, atol=0), relerr(sol.U, o.U)
    assert sol.computed_steps == o.computed_steps
    assert sol.stop_reason == o.stop_reason
    assert sol.tau0 == o.tau0 and sol.t0 == pytest.approx(o.t0, rel=1e-12)
    assert s.time_passed == pytest.approx(o.time_passed, rel=1e-12)
    s.close()
    return sol, o




# ---------------------------------------------------------------------------
# Run-against-run comparison used by test_gpu_issue_modes.py.  The helpers take plain snapshots, so that the same
# code compares the engine with the oracle on the GPU box and the oracle with mutated copies of itself on any machine
# (tests/test_issue_mode_helpers.py shows that they reject subtle errors).
# ---------------------------------------------------------------------------
def _fft_workers():
    return max(1, min(8, os.cpu_count() or 1))


def spectral_err(U, Uref):
    """max |dctn(U - Uref)| over the non-constant modes, relative to the fluctuation scale std(Uref).  U is ~0.875
    plus fluctuations of a few 1e-3, and a white field spreads one mode over all N^2 points: an error confined to
    one mode is N/2 times larger here than in the pointwise relative error of U.  (dctn is orthonormal, so
    std(Uref) is the RMS of the non-constant coefficients of Uref.)  The constant mode is N * mean(U): its relative
    error is that of the mean, which the pointwise comparison bounds; on the fluctuation scale it would only measure
    the rounding of the mass (fp32: 2e-6 of 0.875 times N)."""
    from scipy import fft
    D = fft.dctn(np.asarray(U, dtype=np.float64) - Uref, norm='ortho', workers=_fft_workers())
    D[0, 0] = 0.0
    return float(np.max(np.abs(D)) / np.std(Uref))


def snapshot(solver):
    """What a call leaves behind, from a chsimpy_amd.Solver or an oracle.chs_oracle.OracleSolver: counters, stop
    reason, tau0/t0, the time bookkeeping, the record and the field."""
    sol = getattr(solver, 'solution', solver)
    return dict(steps=int(sol.computed_steps), stop=sol.stop_reason, tau0=sol.tau0, t0=float(sol.t0),
                skip=bool(solver.skip_check), tds=float(solver.time_delta_sum), tp=float(solver.time_passed),
                delt=float(solver.delt), rows=np.array(sol.timedata.data(), dtype=np.float64),
                U=np.array(sol.U, dtype=np.float64))


def seed_step(solver, step):
    """Put the loop at computed_steps = step (the adaptive rule fires beyond step 500 only, solver.py:177) with the
    energy rule's check off (it indexes the record by step number, timedata.py:63): the engine through chs_set_state,
    the oracle by its attributes."""
    if hasattr(solver, '_engine'):
        eng = solver._engine
        st = eng.get_state()
        st.computed_steps = step
        st.skip_check = 1
        eng.set_state(st)
        solver._pull_state()
    else:
        solver.computed_steps = step
        solver.skip_check = True


def drive(solver, chunks, seed=None, record=False):
    """prepare(), optionally seed the step counter, then one solve_or_resume per chunk.  Returns the snapshot after
    every call and, with record=True, the field of every step by the computed_steps it leaves: the oracle's record
    hook for the steps inside a call, the field after the call for every call (so that a call that stops without
    completing a step is looked at too)."""
    solver.prepare()
    if seed is not None:
        seed_step(solver, seed)
    snaps, fields = [], {}
    hook = (lambda k, U: fields.__setitem__(k + 1, U.copy())) if (record and not hasattr(solver, '_engine')) else None
    for c in chunks:
        if hook is not None:
            solver.solve_or_resume(c, record=hook)
        else:
            solver.solve_or_resume(c)
        snaps.append(snapshot(solver))
        if record:
            fields[snaps[-1]['steps']] = snaps[-1]['U']
    return snaps, fields


def compare_snapshots(got, want, rtol=RTOL, rtol_cols=None, rtol_U=None, rtol_spec=None, rtol_time=1e-12):
    """Compare the snapshots of two runs call by call.  Exact: computed_steps, stop reason, tau0, skip_check and the
    record's step column.  rtol_time: t0, time_delta_sum, time_passed and delt; rtol (per column: rtol_cols): record
    columns E, E2, SA, domtime, Ra, L2, PS, delt; rtol_U: U pointwise; rtol_spec: spectral_err.  Raises
    AssertionError on the first difference; returns the largest error of each quantity seen."""
    rtol_cols = dict(rtol_cols or {})
    rtol_U = rtol if rtol_U is None else rtol_U
    rtol_spec = rtol_U if rtol_spec is None else rtol_spec
    assert len(got) == len(want)
    worst = {}

    def keep(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ('steps', 'stop', 'tau0', 'skip'):
            assert g[k] == w[k], (i, k, g[k], w[k])
        for k in ('t0', 'tds', 'tp', 'delt'):
            e = abs(g[k] - w[k]) / max(abs(w[k]), 1e-300)
            keep(k, e)
            assert e <= rtol_time, (i, k, g[k], w[k], e)
        assert g['rows'].shape == w['rows'].shape, (i, g['rows'].shape, w['rows'].shape)
        assert np.array_equal(g['rows'][:, 0], w['rows'][:, 0]), i
        for c in range(1, 9):
            e = relerr(g['rows'][:, c], w['rows'][:, c]) if c != 3 else \
                float(np.max(np.abs(g['rows'][:, c] - w['rows'][:, c])))
            keep(f'col{c}', e)
            assert e <= rtol_cols.get(c, rtol), (i, f'record column {c}', e)
        eu, es = relerr(g['U'], w['U']), spectral_err(g['U'], w['U'])
        keep('U', eu)
        keep('spec', es)
        assert eu <= rtol_U, (i, 'U', eu)
        assert es <= rtol_spec, (i, 'U spectrum', es)
    return worst


def compare_fields(got, want, rtol=RTOL, rtol_spec=None):
    """Per-step fields {computed_steps: U} of two runs: the same steps, every field within rtol pointwise and in
    spectrum.  Returns the largest errors."""
    rtol_spec = rtol if rtol_spec is None else rtol_spec
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    eu = es = 0.0
    for k in sorted(want):
        e1, e2 = relerr(got[k], want[k]), spectral_err(got[k], want[k])
        assert e1 <= rtol, (k, 'U', e1)
        assert e2 <= rtol_spec, (k, 'U spectrum', e2)
        eu, es = max(eu, e1), max(es, e2)
    return dict(U=eu, spec=es)


def fmt_errs(worst):
    return ' '.join(f"{k} {v:.2e}" for k, v in sorted(worst.items()))
