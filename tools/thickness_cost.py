#!/usr/bin/env python3
"""Device time of a look at the local thickness (Solver.thickness, chs_thickness_last_ms: device events around the whole
look, the distance look inside included) beside the distance look on the same handle as the yardstick: 1 warm-up + 5
looks each, on three fields -- the field after 40 steps of the default run thresholded at its median (a two-phase
picture), a random two-level field at density 0.593 and a coarse two-phase picture (eight plane waves of 64 pixels, at
their median: half-widths of about 16 pixels) -- and, at N <= 128 only, on one background pixel in an otherwise full grid
(what the work limit is for: it is not timed above that).  Per field the paint rate, WORK / device time in visits per
second, and the K of chs_thickness_work_default(N) = K N^2 that rate gives: the largest power of two for which K 4096^2
visits take at most about one second, clamped to [1024, 65536].  One size per process; the output of N = 512, 2048 and
4096 in float64 is collected in profiles/thickness.txt.  Nothing asserts a time.
usage: tools/thickness_cost.py N [float64|float32]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chsimpy_amd  # noqa: E402
from chsimpy_amd import _lib  # noqa: E402


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):.4f} ({v.min():.4f} .. {v.max():.4f})"


def k_of(rate):
    """The largest power of two K with K 4096^2 / rate <= 1 s, clamped to [1024, 65536]."""
    k = 1
    while 2 * k * 4096 ** 2 <= rate:
        k *= 2
    return min(max(k, 1024), 65536), k


def looks(s, eng, t, what, max_work=None):
    th_ms, dt_ms = [], []
    for k in range(6):
        try:
            th = s.thickness(t, max_work=max_work)
        except _lib.ThicknessLimitError as e:
            print(f"  {what}: refused, WORK {e.work} ({e.work / eng.N ** 2:.0f} N^2) above the limit {e.limit}")
            return
        th_ms.append(eng.thickness_ms())
        s.distance(t)
        dt_ms.append(eng.distance_ms())
    th_ms, dt_ms = np.array(th_ms[1:]), np.array(dt_ms[1:])
    med = float(np.median(th_ms))
    rate = th.work / (med * 1e-3)
    own = th.work / (max(med - float(np.median(dt_ms)), 1e-6) * 1e-3)
    clamped, raw = k_of(rate)
    print(f"  {what}: thickness {fmt(th_ms)}   distance {fmt(dt_ms)}   thickness / distance {med / np.median(dt_ms):.1f}")
    print(f"    fg {th.fg}, kept {th.kept} ({100.0 * th.kept / max(th.fg, 1):.1f} % of fg), WORK {th.work} = {th.work_per_pixel:.1f} N^2, "
          f"r_max {th.r_max:.2f}, mean_thickness {th.mean_thickness:.3f}, q50 {th.quantile(0.5)}, q90 {th.quantile(0.9)}")
    print(f"    visits / s: {rate:.3e} of the whole look, {own:.3e} without the distance look;  K by the rate: {raw}"
          f" -> {clamped} in [1024, 65536];  the default limit K N^2 = {_lib.thickness_work_default(eng.N)} visits would take "
          f"{1e3 * _lib.thickness_work_default(eng.N) / rate:.1f} ms at that rate")


def main():
    N = int(sys.argv[1])
    dtype = sys.argv[2] if len(sys.argv) > 2 else 'float64'
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.dtype = N, 41, True, 0.0002989112919661156, dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    s.solve_or_resume()
    eng = s._engine
    print(f"N={N} {dtype} engine={eng.engine}: 1 warm-up, 5 looks: median (min .. max), ms")
    looks(s, eng, float(np.median(eng.get_U())), 'after 40 steps, at the median ')
    eng.set_U(np.where(np.random.default_rng(N).random((N, N)) < 0.593, 0.2, 0.8))
    looks(s, eng, 0.5, 'random, density 0.593         ')
    rng = np.random.default_rng(N + 1)            # a coarse two-phase picture: eight plane waves of 64 pixels
    x = np.arange(N, dtype=np.float64)
    W = np.zeros((N, N))
    for a, ph in zip(rng.uniform(0.0, np.pi, 8), rng.uniform(0.0, 2 * np.pi, 8)):
        W += np.cos(2 * np.pi * (np.cos(a) * x[:, None] + np.sin(a) * x[None, :]) / 64.0 + ph)
    eng.set_U(np.where(W < np.median(W), 0.2, 0.8))
    looks(s, eng, 0.5, 'coarse, waves of 64 pixels    ')
    if N <= 128:
        U = np.full((N, N), 0.2)
        U[N // 3, N // 2 + 1] = 0.8
        eng.set_U(U)
        looks(s, eng, 0.5, 'one background pixel (worst)  ', 16 * _lib.thickness_work_default(N))
    s.close(fetch_U=False)


if __name__ == '__main__':
    main()
