#!/usr/bin/env python3
"""The table behind chs_transport_iters_default: conjugate-gradient iterations of the numpy model
(chsimpy_amd/transport.py: the device's iteration and stopping logic) at tol = 1e-6 on fields the oracle has evolved for
STEPS steps, thresholded at their median, both sides, from the top and the left wall.  No device is needed.  Per case the
active pixels, D_eff / D_0, the iterations and iterations / N; at the end the largest ratio, of which the default factor
is to be at least twice.
usage: tools/transport_iters.py N STEPS [STEPS ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chsimpy_amd import components, transport  # noqa: E402
from oracle import chs_oracle as orc  # noqa: E402


def main():
    N = int(sys.argv[1])
    worst = 0.0
    done = 0
    s = orc.OracleSolver(orc.make_params(N, 1 << 30))
    s.prepare()
    for steps in sorted(int(a) for a in sys.argv[2:]):
        s.solve_or_resume(steps + 1 - done)
        done = steps + 1
        U = s.U
        t = float(np.median(U))
        for side in ('below', 'above'):
            X = components.foreground(U, t, side)
            for source in ('top', 'left'):
                S = transport.System(X, source)
                if not S.active.any():
                    print(f"N={N} steps={steps} {side:5s} {source:4s}: no spanning component", flush=True)
                    continue
                try:
                    _, w, v, _ = transport.solve(X, source, 1e-6, transport.MAX_FACTOR * transport.iters_default(N), system=S)
                except transport.IterationLimit as e:
                    print(f"N={N} steps={steps} {side:5s} {source:4s}: not accepted after {e.iters} iterations", flush=True)
                    worst = float('inf')
                    continue
                it = int(w[transport.CHS_TRN_ITERS])
                worst = max(worst, it / N)
                print(f"N={N} steps={steps} {side:5s} {source:4s}: active {int(w[1]):7d} of {int(w[0]):7d}  D_eff/D_0 "
                      f"{0.5 * (v[0] + v[1]):.6f}  iters {it:6d} = {it / N:5.2f} N  checks {int(w[8])}", flush=True)
    print(f"N={N}: the largest ratio {worst:.2f}; the default limit {transport.iters_default(N)} = {transport.iters_default(N) / N:.2f} N")


if __name__ == '__main__':
    main()
