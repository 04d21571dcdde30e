#!/usr/bin/env python3
"""Device time of a look at the contour (Solver.contour, chs_contour_last_ms: device events around the whole look), with
and without the map, beside the look at the morphology -- one sweep over the same bytes: the streaming floor -- on the
same handle: 1 warm-up + 3 looks each, the median, on three fields: the start field (noise: nearly every cell is crossed,
the worst case), the field after STEPS steps, and a constant field (no crossed cell: the sweep alone).  One size per
process.  Nothing asserts a time.
usage: tools/contour_cost.py N [float64|float32] [STEPS]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def looks(s, eng, what, t):
    ms = {k: [] for k in ('contour', 'contour + map', 'morphology')}
    for k in range(4):
        eng.contour(t, 64, 1.0)
        ms['contour'].append(eng.contour_ms())
        eng.contour(t, 64, 1.0, map=True)
        ms['contour + map'].append(eng.contour_ms())
        eng.morphology(t)
        ms['morphology'].append(eng.morphology_ms())
    eng.contour(t, 64, 1.0)                                # (hands the map's memory back)
    med = {k: float(np.median(v[1:])) for k, v in ms.items()}
    print(f"  {what}: " + '   '.join(f"{k} {' '.join(f'{x:.4f}' for x in v[1:])}" for k, v in ms.items())
          + f"   contour / morphology {med['contour'] / med['morphology']:.2f}", flush=True)
    c = s.contour(t)
    crossed = c.word('segments') - c.word('saddles')
    print(f"    {c!r}\n    crossed cells {crossed} of {(eng.N - 1) ** 2} ({crossed / (eng.N - 1) ** 2:.3f}), saddles "
          f"{c.word('saddles')}, under/over {c.word('hist_under')}/{c.word('hist_over')}, S_V {c.S_V:.5f}, rms curvature "
          f"{c.rms_curvature}", flush=True)
    return med


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, steps + 1, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    eng = s._get_engine()
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 3 looks, ms; tile {eng.contour_tile()}")
    looks(s, eng, 'the start field (noise) ', p.threshold)
    s.solve_or_resume()
    U = eng.get_U()
    looks(s, eng, f'after {steps} steps      ', float(np.median(U)))
    eng.set_U(np.full((N, N), p.XXX))
    looks(s, eng, 'a constant field        ', p.threshold - 0.1)
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
