#!/usr/bin/env python3
"""Device time of the sweep and the summary of a look at the droplet shapes (Solver.shapes, chs_shapes_last_ms) beside the
labelling it builds on (chs_components_last_ms of the same look) on the same handle: 1 warm-up + 7 looks, on the field
after `steps` steps of the default run at its own threshold -- both sides: one is the connected matrix, the other one the
droplets -- and on a random two-level field at density 0.593 (noise: at connectivity 4 every tile holds more labels than
slots).  One size per process.
usage: tools/shapes_cost.py N [float64|float32] [4|8] [steps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.4f} ({v.min():.4f} .. {v.max():.4f})"


def looks(s, eng, t, conn, side, what):
    sh_ms, cc_ms = [], []
    for k in range(8):
        sh = s.shapes(t, connectivity=conn, side=side)
        sh_ms.append(eng.shapes_ms())
        cc_ms.append(eng.components_ms())
    sh_ms, cc_ms = np.array(sh_ms[1:]), np.array(cc_ms[1:])
    print(f"  {what}: shapes {fmt(sh_ms)}   components {fmt(cc_ms)}   ratio {np.median(sh_ms) / np.median(cc_ms):.2f}")
    pop = sh.population()
    print(f"    count {sh.count}, area {int(sh.area.sum())}, holes {sh.total_holes}, inner {sh.inner_round}, "
          f"mean circularity {pop['mean_circularity']}, mean aspect {pop['mean_aspect']}")


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    conn = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, steps + 1, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} {dtype} engine={eng.engine} connectivity={conn}: 1 warm-up, 7 looks: median (min .. max), ms")
    looks(s, eng, p.threshold, conn, 'below', f'after {steps} steps, below the threshold')
    looks(s, eng, p.threshold, conn, 'above', f'after {steps} steps, above the threshold')
    eng.set_U(np.where(np.random.default_rng(N).random((N, N)) < 0.593, 0.2, 0.8))
    looks(s, eng, 0.5, conn, 'below', 'random, density 0.593, below        ')
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
