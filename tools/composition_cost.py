#!/usr/bin/env python3
"""Device time of a look at the composition (Solver.composition, chs_composition_last_ms: device events around the whole
look) at 15 and 4096 bins and of a select of 3 and of 8 ranks, beside the look at the morphology -- one sweep over the
same bytes: the streaming floor; composition is two sweeps, a select six (fp64) or three (fp32) -- on the same handle:
1 warm-up + 3 looks each, on three fields: the start field (noise), the field after STEPS steps (two phases) and a
constant field (every lane of every wavefront in one bin, one digit).  One size per process.  Nothing asserts a time.
usage: tools/composition_cost.py N [float64|float32] [STEPS]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def looks(s, eng, what):
    t = s.params.threshold
    n2 = eng.N * eng.N
    ranks8 = [int(q * (n2 - 1)) for q in (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0)]
    ms = {k: [] for k in ('composition 15', 'composition 4096', 'select 3', 'select 8', 'morphology')}
    for k in range(4):
        eng.composition(t, 15)
        ms['composition 15'].append(eng.composition_ms())
        eng.composition(t, 4096)
        ms['composition 4096'].append(eng.composition_ms())
        eng.composition_select([ranks8[1], ranks8[3], ranks8[5]])
        ms['select 3'].append(eng.composition_ms())
        eng.composition_select(ranks8)
        ms['select 8'].append(eng.composition_ms())
        eng.morphology(t)
        ms['morphology'].append(eng.morphology_ms())
    print(f"  {what}: " + '   '.join(f"{k} {' '.join(f'{x:.4f}' for x in v[1:])}" for k, v in ms.items()), flush=True)
    co = s.composition(bins=15)
    print(f"    {co!r}\n    hist {co.hist.tolist()}", flush=True)
    return {k: float(np.median(v[1:])) for k, v in ms.items()}


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
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 3 looks, ms")
    noise = looks(s, eng, 'the start field (noise) ')
    s.solve_or_resume()
    looks(s, eng, f'after {steps} steps      ')
    eng.set_U(np.full((N, N), p.XXX))
    const = looks(s, eng, 'a constant field        ')
    print('  constant / noise: ' + '   '.join(f"{k} {const[k] / noise[k]:.2f}" for k in noise))
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
