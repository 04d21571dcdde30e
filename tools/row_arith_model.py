#!/usr/bin/env python3
"""The executable model of the fp64 pointwise block of the row kernels (oracle/math_model.py: chs_log_unit_tab_f64 and
chs_energy_mu_from_logs of chsimpy_amd/csrc/chs_math.h, operation by operation with an exact fused multiply-add,
rounded once), set against the oracle's numpy expressions.  No GPU needed.

usage: tools/row_arith_model.py [points]
Prints the largest error of the modelled log in ulp, and the largest relative difference of the energy density and
of EnergieEut from the oracle's expressions over the ramp U = 1e-6 .. 1-1e-6 (where U log U + (1-U) log(1-U) cancels
worst) and over the usual field 0.875 +- 0.01 (profiles/row_arith_parity_margins.txt)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import chs_oracle as orc  # noqa: E402
from oracle.math_model import energy_mu, log_unit_tab  # noqa: E402  (the model itself: shared with the tests)


def margins(U, o):
    got = np.array([energy_mu(float(u), o) for u in U])
    Uinv = 1 - U
    eref = o.RT * (U * (np.log(U) - o.params.B) + Uinv * np.log(Uinv)) + (o.A0 + o.A1 * (Uinv - U)) * U * Uinv
    mref = o.mu(U)
    re = np.abs(got[:, 0] - eref) / np.abs(eref)
    rm = np.abs(got[:, 1] - mref) / np.abs(mref)
    # the recorded quantities are sums over the grid: E = mean(e), L2 = sum(mu^2)
    se = abs(got[:, 0].sum() - eref.sum()) / abs(eref.sum())
    sm = abs((got[:, 1] ** 2).sum() - (mref ** 2).sum()) / (mref ** 2).sum()
    return re.max(), rm.max(), se, sm


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    o = orc.OracleSolver(orc.make_params(64, 2))
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(n), 1 - rng.random(n) * 1e-3, 1 - rng.random(n) * 1e-9,
                        np.exp(rng.uniform(-700, 0, n)), np.linspace(0.99, 1.0, n),
                        np.arange(128, 257) / 256.0, (np.arange(128, 256) + 0.5) / 256.0,
                        np.nextafter((np.arange(128, 256) + 0.5) / 256.0, 0), 2.0 ** -np.arange(1, 1000, 7.0)])
    x = x[(x > 0) & (x <= 1)]
    got = np.array([log_unit_tab(float(v)) for v in x])
    ref = np.log(np.asarray(x, dtype=np.longdouble)).astype(np.float64)
    ok = ref != 0
    ulp = np.abs(got[ok] - ref[ok]) / np.spacing(np.abs(ref[ok]))
    print(f"log: {ok.sum()} points, max error {ulp.max():.3f} ulp; log(1) = {log_unit_tab(1.0)!r}")
    ramp = np.linspace(1e-6, 1 - 1e-6, n) + rng.uniform(-5e-7, 5e-7, n)
    usual = 0.875 + rng.uniform(-0.01, 0.01, n)
    for name, U in (('ramp 1e-6 .. 1-1e-6', ramp), ('usual 0.875 +- 0.01', usual)):
        e, m, se, sm = margins(U, o)
        print(f"{name}: {n} points, max rel diff from the oracle's expressions: E {e:.3e}  mu {m:.3e};"
              f"  of the sums: sum(E) {se:.3e}  sum(mu^2) {sm:.3e}")


if __name__ == '__main__':
    main()
