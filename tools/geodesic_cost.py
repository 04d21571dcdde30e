#!/usr/bin/env python3
"""Device time of a geodesic look (Solver.geodesic, chs_geodesic_last_ms: device events around the whole look, the
components look inside included), the time of its relaxation rounds (chs_geodesic_relax_ms: all k_geo_relax launches and
the host's looks at the round counter between them) and the components look's share: 1 warm-up + 3 looks each, on the
field after STEPS steps of the default run thresholded at its median -- both connectivities, source top and source left --
and on the one-pixel serpentine, which is what the default round limit admits.  Per case ROUNDS, the limit, the tortuosity
and the accessible fraction.  One size per process; the output of N = 512 (40 steps) and N = 4096 (2000 steps) in float64
is collected in profiles/geodesic.txt.  Nothing asserts a time.
usage: tools/geodesic_cost.py N STEPS [float64|float32]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402
from chsimpy_amd import _lib  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.3f} ({v.min():.3f} .. {v.max():.3f})"


def looks(s, eng, t, conn, source, what):
    ms, relax, cc = [], [], []
    for k in range(4):
        try:
            g = s.geodesic(t, connectivity=conn, source=source, hist=False, profile=False)
        except _lib.GeodesicLimitError as e:
            print(f"  {what} conn {conn} source {source}: refused after {e.rounds} rounds, limit {e.limit}")
            return
        ms.append(eng.geodesic_ms())
        relax.append(eng.geodesic_relax_ms())
        s.components(t, connectivity=conn, table=False)
        cc.append(eng.components_ms())
    ms, relax, cc = np.array(ms[1:]), np.array(relax[1:]), np.array(cc[1:])
    print(f"  {what} conn {conn} source {source:6s}: look {fmt(ms)} ms   rounds (k_geo_relax) {fmt(relax)} ms   components {fmt(cc)} ms "
          f"= {100 * np.median(cc) / np.median(ms):.0f} %")
    print(f"      ROUNDS {g.rounds} of {g.limit}, {1e3 * np.median(relax) / max(g.rounds, 1):.1f} us a round;  fg {g.fg}, reached "
          f"{g.reached} ({100 * g.accessible_fraction:.1f} %), cc {g.cc_reached} of {g.cc_count}, tortuosity {g.tortuosity:.4f}, "
          f"mean {g.mean_tortuosity:.4f}, max reach {g.max_reach:.0f} px")


def serpentine(N):
    X = np.zeros((N, N), dtype=bool)
    X[0::2] = True
    for k, i in enumerate(range(1, N, 2)):
        X[i, N - 1 if k % 2 == 0 else 0] = True
    return X


def main():
    N, steps = int(sys.argv[1]), int(sys.argv[2])
    dtype = sys.argv[3] if len(sys.argv) > 3 else 'float64'
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, steps + 1, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 3 looks: median (min .. max); default limit {_lib.geodesic_rounds_default(N)} rounds")
    t = float(np.median(eng.get_U()))
    for conn in (4, 8):
        for source in ('top', 'left'):
            looks(s, eng, t, conn, source, f"after {steps} steps, at the median")
    eng.set_U(np.where(serpentine(N), 0.2, 0.8))
    for conn in (4, 8):
        looks(s, eng, 0.5, conn, 'top', "serpentine                    ")
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
