#!/usr/bin/env python3
"""Device time of a look at the morphology (Solver.morphology, chs_morphology_last_ms) beside the three parts of
Solver.structure_factor (chs_structure_factor_last_ms) on the same handle: 1 warm-up + 5 looks each, on the field after
20 steps of the default run.  One size per process.
usage: tools/morphology_cost.py N [float64|float32]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    esz = 8 if dtype == 'float64' else 4
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, 21, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    morph, spec = [], []
    for k in range(6):
        mo = s.morphology()
        morph.append(eng.morphology_ms())
        s.structure_factor()
        spec.append(eng.structure_factor_ms().copy())
    morph, spec = np.array(morph[1:]), np.array(spec[1:])

    def fmt(v):
        return f"{np.median(v):.4f} ({v.min():.4f} .. {v.max():.4f})"
    tbs = N * N * esz / (np.median(morph) * 1e-3) / 1e12
    tbs_bins = N * N * esz / (np.median(spec[:, 2]) * 1e-3) / 1e12
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 5 looks: median (min .. max), ms")
    print(f"  morphology (k_morph_quads + k_morph_fin): {fmt(morph)}   N^2 sizeof(T) / time = {tbs:.2f} TB/s")
    print(f"  structure factor: sweeps {fmt(spec[:, 0])}  transform {fmt(spec[:, 1])}  binning {fmt(spec[:, 2])}"
          f"   binning: {tbs_bins:.2f} TB/s")
    print(f"  morphology / binning = {np.median(morph) / np.median(spec[:, 2]):.2f}")
    print(f"  n_A = {mo.n_A} (SA {mo.SA:.4f}), perimeter_inner = {mo.perimeter_inner}, euler8 = {mo.euler8}, euler4 = {mo.euler4}")
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
