#!/usr/bin/env python3
"""Device time of a look at the connected components (Solver.components, chs_components_last_ms) beside the look at the
morphology (chs_morphology_last_ms) on the same handle -- phase 1 of the labelling is the same read of U: 1 warm-up + 5
looks each, on the field after 40 steps of the default run (thresholded at its median: a two-phase picture) and on a
random two-level field at density 0.593.  One size per process.
usage: tools/components_cost.py N [float64|float32] [4|8]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.4f} ({v.min():.4f} .. {v.max():.4f})"


def looks(s, eng, t, conn, what):
    cc, morph = [], []
    for k in range(6):
        co = s.components(t, connectivity=conn, table=False)
        cc.append(eng.components_ms())
        s.morphology(t)
        morph.append(eng.morphology_ms())
    cc, morph = np.array(cc[1:]), np.array(morph[1:])
    print(f"  {what}: components {fmt(cc)}   morphology {fmt(morph)}   ratio {np.median(cc) / np.median(morph):.1f}")
    print(f"    count {co.count}, area {co.area}, largest {co.largest}, spanning {co.spanning}, inner {co.inner}")


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    conn = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, 41, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} {dtype} engine={eng.engine} connectivity={conn}: 1 warm-up, 5 looks: median (min .. max), ms")
    looks(s, eng, float(np.median(eng.get_U())), conn, 'after 40 steps, at the median')
    eng.set_U(np.where(np.random.default_rng(N).random((N, N)) < 0.593, 0.2, 0.8))
    looks(s, eng, 0.5, conn, 'random, density 0.593 ')
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
