#!/usr/bin/env python3
"""Device time of the overlap passes of a track look (Solver.track, chs_track_last_ms) beside the shape table and the
labelling of the same look (chs_shapes_last_ms, chs_components_last_ms) on the same handle: 1 warm-up + 7 looks with
keep=0 against one frame.  The frame is the field after `steps` steps of the default run at its own threshold, the look
the field after `more` further steps -- both sides: one is the connected matrix, the other one the droplets -- and then
one random two-level field at density 0.593 against another (noise: about N^2 / 2 heads, the hash table at its
largest).  One size per process.
usage: tools/track_cost.py N [float64|float32] [4|8] [steps] [more]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402
from chsimpy_amd import components, tracking  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.4f} ({v.min():.4f} .. {v.max():.4f})"


def looks(s, eng, U1, U2, t, conn, side, what, objects=True):
    """objects: through Solver.track, with the families of the last look; else the engine's words alone (noise: millions
    of droplets, whose host objects would take longer than everything else here)."""
    code = components.side_code(side)
    eng.set_U(U1)
    if objects:
        s.track(t, connectivity=conn, side=side, reset=True)
    else:
        eng.track_reset()
        eng.track(t, conn, code, True)
    eng.set_U(U2)
    ms = {'track': [], 'shapes': [], 'components': []}
    for k in range(8):
        if objects:
            tr = s.track(t, connectivity=conn, side=side, keep=False)
            w = tr.words
        else:
            w = eng.track(t, conn, code, False)
        for name in ms:
            ms[name].append(getattr(eng, name + '_ms')())
    ms = {k: np.array(v[1:]) for k, v in ms.items()}
    print(f"  {what}: track {fmt(ms['track'])}   shapes {fmt(ms['shapes'])}   components {fmt(ms['components'])}")
    W = tracking
    print(f"    droplets {w[W.CHS_TR_PREV_COUNT]} -> {w[0]}, pairs {w[W.CHS_TR_PAIRS]}, heads {w[W.CHS_TR_HEADS]}, "
          f"slots {w[W.CHS_TR_SLOTS]} ({16 * w[W.CHS_TR_SLOTS] / 2 ** 20:.2f} MiB), overlap {w[W.CHS_TR_OVERLAP]}, "
          f"lost {w[W.CHS_TR_LOST]}, gained {w[W.CHS_TR_GAINED]}" + (f", {tr.counts()}" if objects else ""))


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    conn = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    more = int(sys.argv[5]) if len(sys.argv) > 5 else 200
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, steps + more + 1, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume(steps + 1)
    eng = s._engine
    U1 = eng.get_U()
    s.solve_or_resume(more)
    U2 = eng.get_U()
    print(f"N={N} {dtype} engine={eng.engine} connectivity={conn}: frame after {steps} steps, look after {steps + more}; "
          f"1 warm-up, 7 looks: median (min .. max), ms")
    looks(s, eng, U1, U2, p.threshold, conn, 'below', 'below the threshold')
    looks(s, eng, U1, U2, p.threshold, conn, 'above', 'above the threshold')
    rng = np.random.default_rng(N)
    R1, R2 = (np.where(rng.random((N, N)) < 0.593, 0.2, 0.8) for _ in range(2))
    looks(s, eng, R1, R2, 0.5, conn, 'below', 'random, density 0.593  ', objects=False)
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
