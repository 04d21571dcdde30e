#!/usr/bin/env python3
"""Device time of a look at the chord lengths (Solver.chords, chs_chords_last_ms: device events around the whole look)
beside the looks at the distance transform and at the morphology on the same handle and field: 1 warm-up + 3 looks each,
on two fields -- the start field thresholded at its mean (noise: about N^2 / 2 chords per direction, almost all of them
1 to 3 pixels long) and the field after STEPS steps thresholded at its mean (a two-phase picture).  One size per process.
Nothing asserts a time.
usage: tools/chords_cost.py N [float64|float32] [STEPS]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def looks(s, eng, t, what):
    ch, dt, morph = [], [], []
    for k in range(4):
        co = s.chords(t, hist=False)
        ch.append(eng.chords_ms())
        s.distance(t, hist=False)
        dt.append(eng.distance_ms())
        s.morphology(t)
        morph.append(eng.morphology_ms())
    f = lambda v: ' '.join(f"{x:.4f}" for x in v[1:])
    print(f"  {what}: chords {f(ch)}   distance {f(dt)}   morphology {f(morph)}   (ms, after one warm-up look)")
    print("    " + '; '.join(f"{p} {d}: {co.count(p, d)} inner + {co.cut(p, d)} cut, mean {co.mean(p, d):.3f}, max {co.max(p, d)}"
                             for p in ('below', 'above') for d in ('rows', 'cols')), flush=True)
    return float(np.median(ch[1:]))


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
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 3 looks, ms")
    noise = looks(s, eng, float(eng.get_U().mean()), 'the start field, at its mean      ')
    s.solve_or_resume()
    evolved = looks(s, eng, float(eng.get_U().mean()), f'after {steps} steps, at the mean  ')
    print(f"  noise / evolved {noise / evolved:.1f}")
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
