#!/usr/bin/env python3
"""Device time of a look at the two-point correlation (Solver.two_point, chs_two_point_last_ms: device events around the
whole look) at rmax 16, 64 and 256, beside the look at the chord lengths on the same handle and field: 1 warm-up + 3 looks
each, on two fields -- the start field thresholded at its mean (noise) and the field after STEPS steps thresholded at its
mean (a two-phase picture).  The pair kernel's work does not depend on the field: (rmax + 1)(2 rmax + 1) displacements of
N^2 / 32 word pairs per phase.  One size per process.  Nothing asserts a time.
usage: tools/two_point_cost.py N [float64|float32] [STEPS]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402
from chsimpy_amd import two_point  # noqa: E402

RMAX = (16, 64, 256)


def looks(s, eng, t, what):
    N = s.params.N
    print(f"  {what}:")
    med = {}
    for rmax in RMAX:
        if rmax > two_point.max_r(N):
            continue
        tp_ms, ch = [], []
        for k in range(4):
            two = s.two_point(t, rmax=rmax, counts=(k == 3))
            tp_ms.append(eng.two_point_ms())
            s.chords(t, hist=False)
            ch.append(eng.chords_ms())
        f = lambda v: ' '.join(f"{x:.4f}" for x in v[1:])
        med[rmax] = float(np.median(tp_ms[1:]))
        words = 2 * (rmax + 1) * (2 * rmax + 1) * N * ((N + 31) // 32)            # word pairs the pair kernel visits
        z = two.first_zero('below')
        print(f"    rmax {rmax:3d}: two_point {f(tp_ms)}   chords {f(ch)}   (ms, after one warm-up look); "
              f"{words / med[rmax] * 1e-6:.1f} G word pairs / s; n_below {two.n('below')}, S2(0, 1) {two.S2('below', 0, 1):.4f}, "
              f"first zero {'none' if z is None else format(z / (s.solution.delx or 1.0), '.2f') + ' px'}", flush=True)
    return med


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, steps + 1, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    eng = s._get_engine()
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 3 looks, ms; tile {eng.two_point_tile()}")
    looks(s, eng, float(eng.get_U().mean()), 'the start field, at its mean')
    s.solve_or_resume()
    looks(s, eng, float(eng.get_U().mean()), f'after {steps} steps, at the mean')
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
