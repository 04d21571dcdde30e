#!/usr/bin/env python3
"""Device time of a skeleton look (Solver.skeleton, chs_skeleton_last_ms: device events around the whole look, the
distance look inside included), the time of its sub-iterations (chs_skeleton_thin_ms: all k_sk_thin launches and the
host's looks at the counter between them) and the distance look's own time: 1 warm-up + 3 looks each, on the field after
STEPS steps of the default run thresholded at its median, both sides, and -- with `full` -- on the full grid, which is
what needs the most sub-iterations of all fields found (about 2 N).  Per case SUBITERS, the limit, microseconds per
sub-iteration and the network's main words.  One size per process; the output of N = 512 (40 steps) and N = 4096 (40 and
2000 steps, full grid) in float64 is collected in profiles/skeleton.txt.  Nothing asserts a time.
usage: tools/skeleton_cost.py N STEPS [full] [float64|float32]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402
from chsimpy_amd import _lib  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.3f} ({v.min():.3f} .. {v.max():.3f})"


def looks(s, eng, t, side, what):
    ms, thin, dt = [], [], []
    for k in range(4):
        try:
            sk = s.skeleton(t, side=side, hist=True)
        except _lib.SkeletonLimitError as e:
            print(f"  {what} {side}: refused, a pixel was deleted in sub-iteration {e.subiters}, limit {e.limit}")
            return
        ms.append(eng.skeleton_ms())
        thin.append(eng.skeleton_thin_ms())
        s.distance(t, side=side, hist=False)
        dt.append(eng.distance_ms())
    ms, thin, dt = np.array(ms[1:]), np.array(thin[1:]), np.array(dt[1:])
    issued = -(-(sk.subiters + 4) // 32) * 32           # the host issues 32 at a time
    print(f"  {what} {side:5s}: look {fmt(ms)} ms   sub-iterations (k_sk_thin) {fmt(thin)} ms   distance look {fmt(dt)} ms "
          f"= {100 * np.median(dt) / np.median(ms):.0f} %")
    neck = 'none' if sk.neck_radius is None else f"{sk.neck_radius:.2f}"
    print(f"      SUBITERS {sk.subiters} of {sk.limit}, {min(issued, sk.limit)} issued, {1e3 * np.median(thin) / min(issued, sk.limit):.2f} us a "
          f"sub-iteration;  fg {sk.fg}, pixels {sk.pixels}, ends {sk.ends}, junctions {sk.junctions}, euler8 {sk.euler8}, "
          f"length/area {sk.length_per_area:.5f} per px, neck radius {neck} px")


def main():
    args = sys.argv[1:]
    full = 'full' in args
    args = [a for a in args if a != 'full']
    N, steps = int(args[0]), int(args[1])
    dtype = args[2] if len(args) > 2 else 'float64'
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, steps + 1, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 3 looks: median (min .. max); default limit "
          f"{_lib.skeleton_subiters_default(N)} sub-iterations")
    t = float(np.median(eng.get_U()))
    for side in ('below', 'above'):
        looks(s, eng, t, side, f"after {steps} steps, at the median")
    if full:
        eng.set_U(np.full((N, N), 0.2))
        looks(s, eng, 0.5, 'below', "full grid                    ")
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
