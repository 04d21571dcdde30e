#!/usr/bin/env python3
"""Aggregate member-steps/s of the batch (chsimpy_amd.BatchSolver) against one single handle and against
run_ensemble(concurrent=3) at the same N.

Protocol: full_sim, one literal 2000-step call (solve_or_resume(2001) after prepare), 1 warm-up + 3 timed repetitions
(mean and best); members with the A factors of make_rand_values.  Extra rows: 64 x N=2048 (configs[4]'s size) and the
default experiment (N=512, energy stop, ntmax 1e6, 64 members stopping at different steps).

--adaptive: the same members with adaptive_time and delt_max = 4.9e-7/N (the adaptive tests' value: the step grows from
step 502 on, re-evaluated on every second step), so that three quarters of the 2000 steps run under the step-size rule;
rows N in {256, 512, 1024} fp64 and N=512 fp32, no default-experiment row.

--seats S: the seat queue (BatchSolver(seats=S)).  With --only N,dtype,R the R members run as a queue of S seats -- the
price of the queue per step is this row against R/S plain batches of S (--only N,dtype,S).  With --default N the
default experiment (energy stop, ntmax 1e6) of --members M runs at grid size N three ways: groups of S (run_ensemble(
batch=S)), one plain batch of all M, and one queue of S seats (batch=S, queue=True); 1 warm-up + 3 repetitions each,
member-steps/s and end-to-end seconds.

--engine chirp: the chirp batch (grid sizes outside the fast engine's set).  Every configuration runs in a process of
its own (a fresh child per row, one after the other; the first child that fails ends the bench): 200 full_sim steps in
one literal call, 1 warm-up + 3 repetitions, median and spread (max - min) of the member-steps/s.  fp64 at N in {100,
200, 500, 1000, 2000} and fp32 at N=500, B in {1, 4, 16, 64} -- B=64 only where the members' arrays (5 of N^2 elements
each) stay under 4 GiB together.  Baseline of every row: the same B members as single chirp handles stepped one after
the other, which is what --batch did at these N before there was a chirp batch; and run_ensemble(concurrent=3) per N.
With --only N,dtype,B (B a number, or `c3` for the concurrent=3 row) it measures that one row in this process.

usage: tools/batch_bench.py [--quick] [--adaptive] [--only N,dtype,B [--once]] [--seats S] [--default N [--members M]]
                            [--engine chirp [--quick]]
    --engine chirp --quick: N in {100, 1000} fp64, B in {1, 4, 16}, no concurrent=3 row
    --quick: N=512 fp64 only, B in {1, 16}
    --only:  one batched row and nothing else, e.g. --only 512,float64,16; --once: a single call without warm-up or
             repetitions (what a kernel trace should hold)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import chsimpy_amd  # noqa: E402
from chsimpy_amd import experiment as ex  # noqa: E402
from chsimpy_amd.batch import BatchSolver  # noqa: E402

KAPPA = 0.0002989112919661156
STEPS = 2000
REPS = 3
ADAPTIVE = False


def members(N, B, dtype='float64', ntmax=STEPS + 1, full_sim=True, engine=None):
    init = chsimpy_amd.Parameters()
    init.N, init.ntmax, init.full_sim, init.kappa_tilde, init.dtype = N, ntmax, full_sim, KAPPA, dtype
    if engine:
        init.engine = engine
    init.file_id = '/tmp/batch_bench'
    if ADAPTIVE:
        init.adaptive_time, init.delt_max = True, 4.9e-7 / N
    ep = ex.ExperimentParams()
    ep.runs = B
    rv, al, _ = ex.make_rand_values(ep)
    return init, ep, [ex.run_params(init, i, rv, al)[0] for i in range(B)]


def timed(fn, reps=REPS):
    if '--once' in sys.argv:
        t = fn()
        return t, t
    fn()                                  # warm-up
    ts = []
    for _ in range(reps):
        ts.append(fn())
    return float(np.mean(ts)), float(np.min(ts))


def single(N, dtype):
    _, _, ps = members(N, 1, dtype)
    s = chsimpy_amd.Solver(ps[0])
    s.rederive_hat = True

    def run():
        s.prepare()
        t0 = time.perf_counter()
        s.solve_or_resume(STEPS + 1)
        return time.perf_counter() - t0
    mean, best = timed(run)
    s.close(fetch_U=False)
    return STEPS / mean, STEPS / best


def batched(N, B, dtype, seats=None):
    _, _, ps = members(N, B, dtype)
    bs = BatchSolver(ps, seats=seats)

    def run():
        bs.prepare()
        t0 = time.perf_counter()
        bs.solve_or_resume(STEPS + 1)
        return time.perf_counter() - t0
    mean, best = timed(run)
    assert all(s.solution.computed_steps == STEPS + 1 for s in bs.solvers)
    if ADAPTIVE:   # the step did adapt, every member's
        assert all(len(set(s.solution.timedata.data()[:, 8])) > 100 for s in bs.solvers)
    bs.close(fetch_U=False)
    return B * STEPS / mean, B * STEPS / best


def concurrent3(N, dtype, runs=6):
    init, ep, _ = members(N, runs, dtype)

    def run():
        t0 = time.perf_counter()
        ex.run_ensemble(init, ep, concurrent=3,
                        run_fn=lambda i, p, rv, al: ex.run_experiment_gpu(i, p, rv, al, None, postprocess=False))
        return time.perf_counter() - t0
    mean, best = timed(run, reps=2)
    return runs * STEPS / mean, runs * STEPS / best


def default_experiment(B=64, batch=16):
    """N=512, energy stop, ntmax 1e6: the reference's default experiment, members stopping at different steps."""
    init, ep, ps = members(512, B, ntmax=int(1e6), full_sim=False)
    out = {}
    for label, kw in (('concurrent=1', dict(concurrent=1)), (f'batch={batch}', dict(batch=batch))):
        t0 = time.perf_counter()
        recs = ex.run_ensemble(init, ep, run_fn=None if 'batch' in label else
                               (lambda i, p, rv, al: ex.run_experiment_gpu(i, p, rv, al, None, postprocess=False)),
                               batch_fn=(lambda ids, p, rv, al: ex.run_batch_gpu(ids, p, rv, al, None, postprocess=False))
                               if 'batch' in label else None, **kw)
        dt = time.perf_counter() - t0
        steps = sum(int(r[6]) for r in recs)
        out[label] = (dt, steps, sorted(set(int(r[6]) for r in recs)))
    return out


def default_queue(N, M, S):
    """The default experiment of M members at grid size N: groups of S, one plain batch of M, one queue of S seats."""
    init, ep, _ = members(N, M, ntmax=int(1e6), full_sim=False)
    fn = lambda ids, p, rv, al, **kw: ex.run_batch_gpu(ids, p, rv, al, None, postprocess=False, **kw)
    ways = ((f'batch={S}', dict(batch=S, batch_fn=fn)),
            (f'batch={M} (one plain batch)', dict(batch=M, batch_fn=fn)),
            (f'batch={S} queue', dict(batch=S, queue=True, queue_members=M, batch_fn=lambda *a: fn(*a, seats=S))))
    for label, kw in ways:
        steps = []

        def run():
            t0 = time.perf_counter()
            recs = ex.run_ensemble(init, ep, **kw)
            dt = time.perf_counter() - t0
            steps[:] = [int(r[6]) for r in recs]
            return dt
        mean, best = timed(run)
        print(f"default experiment N={N} energy stop, {M} members, {label}: {mean:7.2f} s ({best:7.2f}), "
              f"{sum(steps)} member-steps ({sum(steps) / mean:9.0f}/s), stop steps {min(steps)}..{max(steps)}", flush=True)


# ---------------------------------------------------------------------------
# --engine chirp
# ---------------------------------------------------------------------------
CHIRP_STEPS = 200
CHIRP_ROWS = [(100, 'float64'), (200, 'float64'), (500, 'float64'), (1000, 'float64'), (2000, 'float64'), (500, 'float32')]
CHIRP_BS = (1, 4, 16, 64)
CHIRP_BYTES_MAX = 4 << 30


def chirp_fits(N, dtype, B):
    return 5 * N * N * (8 if dtype == 'float64' else 4) * B <= CHIRP_BYTES_MAX


def _rates(work, fn):
    """1 warm-up + REPS repetitions of fn() -> seconds; (median, spread) of work/seconds"""
    fn()
    r = sorted(work / fn() for _ in range(REPS))
    return float(np.median(r)), float(r[-1] - r[0])


def chirp_row(N, dtype, B):
    """One row, in this process: the batch of B chirp members and the same members one by one."""
    _, _, ps = members(N, B, dtype, ntmax=CHIRP_STEPS + 1, engine='chirp')
    bs = BatchSolver(ps)

    def run_batch():
        bs.prepare()
        t0 = time.perf_counter()
        bs.solve_or_resume(CHIRP_STEPS + 1)
        return time.perf_counter() - t0
    b_med, b_spread = _rates(B * CHIRP_STEPS, run_batch)
    assert all(s.solution.computed_steps == CHIRP_STEPS + 1 for s in bs.solvers)
    bs.close(fetch_U=False)
    singles = [chsimpy_amd.Solver(p) for p in ps]
    for s in singles:
        s.rederive_hat = True

    def run_singles():
        for s in singles:
            s.prepare()
        t0 = time.perf_counter()
        for s in singles:
            s.solve_or_resume(CHIRP_STEPS + 1)
        return time.perf_counter() - t0
    s_med, s_spread = _rates(B * CHIRP_STEPS, run_singles)
    assert singles[0]._engine.engine == 'chirp'
    for s in singles:
        s.close(fetch_U=False)
    print(f"N={N} {dtype} chirp batch B={B:3d}: {b_med:9.0f} (spread {b_spread:8.0f}) member-steps/s   one by one: "
          f"{s_med:9.0f} (spread {s_spread:8.0f})   x{b_med / s_med:5.2f}", flush=True)


def chirp_c3(N, dtype, runs=6):
    init, ep, _ = members(N, runs, dtype, ntmax=CHIRP_STEPS + 1, engine='chirp')

    def run():
        t0 = time.perf_counter()
        ex.run_ensemble(init, ep, concurrent=3,
                        run_fn=lambda i, p, rv, al: ex.run_experiment_gpu(i, p, rv, al, None, postprocess=False))
        return time.perf_counter() - t0
    med, spread = _rates(runs * CHIRP_STEPS, run)
    print(f"N={N} {dtype} chirp run_ensemble(concurrent=3, {runs} runs, end to end): {med:9.0f} (spread {spread:8.0f}) "
          f"member-steps/s", flush=True)


def chirp_bench(quick):
    import subprocess
    print(f"# chirp batch bench: full_sim, one literal {CHIRP_STEPS}-step call, every row in a process of its own, 1 warm-up "
          f"+ {REPS} reps; member-steps/s median (spread = max - min)", flush=True)
    rows = [(100, 'float64'), (1000, 'float64')] if quick else CHIRP_ROWS
    for N, dt in rows:
        todo = ([] if quick else ['c3']) + [str(B) for B in ((1, 4, 16) if quick else CHIRP_BS) if chirp_fits(N, dt, B)]
        for what in todo:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--engine', 'chirp', '--only', f"{N},{dt},{what}"],
                               timeout=300)
            if r.returncode != 0:   # nothing more is started on a device behind a failure
                print(f"N={N} {dt} {what}: the child ended with {r.returncode}; bench stopped", flush=True)
                sys.exit(1)


def main():
    global ADAPTIVE
    if '--engine' in sys.argv:
        if sys.argv[sys.argv.index('--engine') + 1] != 'chirp':
            sys.exit("--engine takes chirp (the fast engine's batch is the default)")
        if '--only' in sys.argv:
            N, dt, B = sys.argv[sys.argv.index('--only') + 1].split(',')
            if B == 'c3':
                chirp_c3(int(N), dt)
            else:
                chirp_row(int(N), dt, int(B))
        else:
            chirp_bench('--quick' in sys.argv)
        return
    quick = '--quick' in sys.argv
    ADAPTIVE = '--adaptive' in sys.argv
    mode = 'adaptive step (delt_max = 4.9e-7/N), ' if ADAPTIVE else ''
    seats = int(sys.argv[sys.argv.index('--seats') + 1]) if '--seats' in sys.argv else None
    if '--default' in sys.argv:
        M = int(sys.argv[sys.argv.index('--members') + 1]) if '--members' in sys.argv else 64
        default_queue(int(sys.argv[sys.argv.index('--default') + 1]), M, seats or 16)
        return
    if '--only' in sys.argv:
        N, dt, B = sys.argv[sys.argv.index('--only') + 1].split(',')
        b_mean, b_best = batched(int(N), int(B), dt, seats)
        what = f"batch B={int(B):3d}" if seats is None else f"queue R={int(B):3d} seats={seats:3d}"
        print(f"N={N} {dt} {mode}{what}: {b_mean:9.0f} ({b_best:9.0f}) member-steps/s", flush=True)
        return
    rows = ([(512, 'float64')] if quick else
            [(256, 'float64'), (512, 'float64'), (1024, 'float64')] + ([] if ADAPTIVE else [(2048, 'float64')])
            + [(512, 'float32')])
    Bs = (1, 16) if quick else (1, 4, 16, 64)
    print(f"# batch bench: full_sim, {mode}one literal {STEPS}-step call, 1 warm-up + {REPS} reps; member-steps/s mean (best)")
    for N, dt in rows:
        s_mean, s_best = single(N, dt)
        print(f"N={N} {dt} single handle: {s_mean:9.0f} ({s_best:9.0f}) steps/s", flush=True)
        c_mean, c_best = concurrent3(N, dt)
        print(f"N={N} {dt} run_ensemble(concurrent=3, 6 runs, end to end): {c_mean:9.0f} ({c_best:9.0f}) member-steps/s",
              flush=True)
        for B in Bs:
            b_mean, b_best = batched(N, B, dt)
            print(f"N={N} {dt} batch B={B:3d}: {b_mean:9.0f} ({b_best:9.0f}) member-steps/s   "
                  f"x{b_mean / s_mean:5.2f} single, x{b_mean / c_mean:5.2f} concurrent=3", flush=True)
    if not quick and not ADAPTIVE:
        r = default_experiment()
        for label, (dt, steps, stops) in r.items():
            print(f"default experiment N=512 energy stop, 64 members, {label}: {dt:7.2f} s, {steps} member-steps "
                  f"({steps / dt:9.0f}/s), stop steps {stops[0]}..{stops[-1]} ({len(stops)} distinct)", flush=True)


if __name__ == '__main__':
    main()
