#!/usr/bin/env python3
"""Device time of a transport look (Solver.transport, chs_transport_last_ms: device events around the whole look, the
components look inside included) and of its solve (chs_transport_solve_ms: all k_trn_ap / k_trn_update launches, the
host's looks at the scalars every 32 iterations and the closing sweeps): 1 warm-up + 3 looks each, on the field after
STEPS steps of the default run, the phase below the field's Q quantile for every Q given (default 0.5 and 0.6: at the
median a phase often does not span), from the top and the left wall.  Per case the active pixels, D_eff / D_0, the
tortuosity factor, ITERS, microseconds per iteration, and beside it the traffic floor of an iteration: 82 bytes per active
pixel -- k_trn_ap reads r, p and the pixel's byte and writes p and q (33), k_trn_update reads x, r, p, q and the byte and
writes x and r (49) -- over the bandwidth BW in TB/s (default 4.0; tools/membw.py measures it on the same box).  The halo
edges and the bytes of the pixels of an active tile that are not active are not in the floor.  One size per process; the
output of N = 512, 1024 and 2048 is collected in profiles/transport.txt.  Nothing asserts a time.
usage: tools/transport_cost.py N STEPS [BW] [Q ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402
from chsimpy_amd import _lib  # noqa: E402

BYTES = 82


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.3f} ({v.min():.3f} .. {v.max():.3f})"


def looks(s, eng, t, source, what, bw):
    ms, solve = [], []
    for k in range(4):
        try:
            tr = s.transport(t, source=source, profile=False)
        except _lib.TransportLimitError as e:
            print(f"  {what} {source:4s}: refused after {e.iters} iterations, limit {e.limit}")
            return
        ms.append(eng.transport_ms())
        solve.append(eng.transport_solve_ms())
    if not tr.percolates:
        print(f"  {what} {source:4s}: no spanning component; look {fmt(ms[1:])} ms")
        return
    ms, solve = np.array(ms[1:]), np.array(solve[1:])
    issued = min(-(-tr.iters // 32) * 32, tr.limit)                   # the host issues 32 at a time
    us = 1e3 * np.median(solve) / tr.iters
    floor = BYTES * tr.active / (bw * 1e12) * 1e6
    print(f"  {what} {source:4s}: look {fmt(ms)} ms   solve {fmt(solve)} ms")
    print(f"      ITERS {tr.iters} of {tr.limit} ({issued} issued), CHECKS {tr.checks}, {us:.2f} us an iteration; floor "
          f"{BYTES} B x {tr.active} active / {bw:.2f} TB/s = {floor:.2f} us, {us / floor:.1f} x;  fg {tr.fg}, D_eff/D_0 "
          f"{tr.deff:.6f} +- {tr.deff_bound:.1e}, tortuosity factor {tr.tortuosity_factor:.3f}, conservation {tr.conservation:.1e}")


def main():
    args = sys.argv[1:]
    N, steps = int(args[0]), int(args[1])
    bw = float(args[2]) if len(args) > 2 else 4.0
    qs = [float(a) for a in args[3:]] or [0.5, 0.6]
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde = N, steps + 1, True, 0.0002989112919661156
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} float64 engine={eng.engine}: 1 warm-up, 3 looks: median (min .. max); default limit "
          f"{_lib.transport_iters_default(N)} iterations, tol 1e-6")
    U = eng.get_U()
    for q in qs:
        t = float(np.quantile(U, q))
        for source in ('top', 'left'):
            looks(s, eng, t, source, f"after {steps} steps, below the {q} quantile", bw)
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
