#!/usr/bin/env python3
"""Device time of a look at the distance transform (Solver.distance, chs_distance_last_ms: device events around the
whole look) beside the looks at the morphology and at the connected components on the same handle: 1 warm-up + 5 looks
each, on three fields -- the field after 40 steps of the default run thresholded at its median (a two-phase picture), a
random two-level field at density 0.593, and the worst case of the horizontal search: one background pixel in an
otherwise full grid.  One size per process.  Nothing asserts a time.
usage: tools/distance_cost.py N [float64|float32]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.4f} ({v.min():.4f} .. {v.max():.4f})"


def looks(s, eng, t, what):
    dt, cc, morph = [], [], []
    for k in range(6):
        di = s.distance(t)
        dt.append(eng.distance_ms())
        s.components(t, table=False)
        cc.append(eng.components_ms())
        s.morphology(t)
        morph.append(eng.morphology_ms())
    dt, cc, morph = np.array(dt[1:]), np.array(cc[1:]), np.array(morph[1:])
    print(f"  {what}: distance {fmt(dt)}   components {fmt(cc)}   morphology {fmt(morph)}   "
          f"distance / components {np.median(dt) / np.median(cc):.2f}   distance / morphology {np.median(dt) / np.median(morph):.1f}")
    print(f"    fg {di.fg}, r_max {di.r_max:.2f} at {di.argmax}, r2_mean {di.r2_mean:.2f}, r_floor_mean {di.r_floor_mean:.3f}, "
          f"q50 {di.quantile(0.5)}, q90 {di.quantile(0.9)}")


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, 41, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 5 looks: median (min .. max), ms")
    looks(s, eng, float(np.median(eng.get_U())), 'after 40 steps, at the median ')
    eng.set_U(np.where(np.random.default_rng(N).random((N, N)) < 0.593, 0.2, 0.8))
    looks(s, eng, 0.5, 'random, density 0.593         ')
    U = np.full((N, N), 0.2)
    U[0, 0] = 0.8
    eng.set_U(U)
    looks(s, eng, 0.5, 'one background pixel (worst)  ')
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
