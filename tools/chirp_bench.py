#!/usr/bin/env python3
"""Steps per second of the chirp engine against the direct engine at grid sizes that are no power of two, the fast
engine at the neighbouring powers of two for scale, and the chirp engine's per-slot times at N=1000.

Protocol: 1 warm-up + 3 repetitions of one full_sim call of `--steps` steps (fewer for the direct engine where a
repetition would take more than a few seconds: its step costs 8 N^3 flops).  Every (size, engine, dtype) runs in a
process of its own under its own time limit; nothing is retried, and after a child that died or ran out of time
nothing more is started.

usage: tools/chirp_bench.py [--out FILE] [--steps 200]
Sets CHS_CHIRP_AUTO_MIN_N (include/chs_hip.h): max(129, the smallest probed N from which chirp is at least 1.1x the
direct engine at every larger probe); the script prints that N.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBES_F64 = (100, 129, 200, 320, 500, 768, 1000, 1500, 2000, 3000, 4000)
PROBES_F32 = (500, 1000)
KAPPA = 0.0002989112919661156


def direct_steps(N, steps):
    """Steps of one repetition of the direct engine: about 2 s at an assumed 3 TFLOP/s of its 8 N^3 flops per step."""
    return int(max(5, min(steps, 2.0 / (8.0 * N ** 3 / 3e12))))


def child(args):
    import chsimpy_amd
    p = chsimpy_amd.Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde, p.engine, p.dtype = args.N, 10 ** 9, True, KAPPA, args.engine, args.dtype
    p.threshold = p.XXX
    s = chsimpy_amd.Solver(p)
    s.prepare()
    eng = s._engine
    assert eng.engine == args.engine, eng.engine
    if args.profile:
        s.solve_or_resume(5)
        ms, calls = eng.profile_steps(args.steps)
        out = dict(kind='profile', N=args.N, engine=args.engine, dtype=args.dtype, steps=args.steps,
                   slots={n: [float(m) / args.steps, int(c)] for n, m, c in zip(eng.kernel_names(), ms, calls) if n and c})
    else:
        s.solve_or_resume(args.steps)           # warm-up
        wall, dev = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            s.solve_or_resume(args.steps)
            wall.append(time.perf_counter() - t0)
            dev.append(eng.last_step_ms() * 1e-3)
        w = sorted(wall)[1]
        out = dict(kind='run', N=args.N, engine=args.engine, dtype=args.dtype, steps=args.steps,
                   steps_per_s=args.steps / w, ms_per_step=w / args.steps * 1e3,
                   ms_per_step_device=sorted(dev)[1] / args.steps * 1e3,
                   spread=(max(wall) - min(wall)) / w)
    s.close(fetch_U=False)
    print('RESULT ' + json.dumps(out), flush=True)


def run_child(N, engine, dtype, steps, limit, profile=False):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '-N', str(N), '--engine', engine, '--dtype', dtype,
           '--steps', str(steps)] + (['--profile'] if profile else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"time limit of {limit} s"
    for line in r.stdout.splitlines():
        if line.startswith('RESULT '):
            return json.loads(line[7:]), None
    return None, f"exit status {r.returncode}: {(r.stderr or r.stdout)[-400:]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('-N', type=int, default=1000)
    ap.add_argument('--engine', default='chirp')
    ap.add_argument('--dtype', default='float64')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    say(f"# chirp vs direct, 1 warm-up + 3 repetitions (median) of one full_sim call; wall time of the call; "
        f"chirp/fast {args.steps} steps, direct fewer at large N (column `steps`)")
    say("# dtype     N  engine  steps   steps/s   ms/step  ms/step(device)  spread")
    jobs = [(N, e, 'float64') for N in PROBES_F64 for e in ('chirp', 'direct')]
    jobs += [(N, e, 'float32') for N in PROBES_F32 for e in ('chirp', 'direct')]
    jobs += [(N, 'fast', 'float64') for N in (128, 256, 512, 1024, 2048, 4096)]
    jobs += [(N, 'fast', 'float32') for N in (512, 1024)]
    res = {}
    for N, engine, dtype in jobs:
        steps = direct_steps(N, args.steps) if engine == 'direct' else args.steps
        out, err = run_child(N, engine, dtype, steps, 150)
        if err:
            say(f"# {dtype} N={N} {engine}: {err} -- nothing more is started")
            return 1
        res[(dtype, N, engine)] = out
        say(f"{dtype:8s} {N:5d}  {engine:6s} {steps:6d} {out['steps_per_s']:9.1f} {out['ms_per_step']:9.4f} "
            f"{out['ms_per_step_device']:12.4f} {out['spread']:11.3f}")
    say("# chirp / direct")
    ratio = {}
    for dtype, probes in (('float64', PROBES_F64), ('float32', PROBES_F32)):
        for N in probes:
            r = res[(dtype, N, 'chirp')]['steps_per_s'] / res[(dtype, N, 'direct')]['steps_per_s']
            say(f"{dtype:8s} {N:5d}  {r:8.2f}x")
            if dtype == 'float64':
                ratio[N] = r
    nstar = None
    for N in sorted(ratio, reverse=True):
        if ratio[N] < 1.1:
            break
        nstar = N
    say(f"# N* (fp64: chirp >= 1.1x direct from here up) = {nstar}; CHS_CHIRP_AUTO_MIN_N = "
        f"{max(129, nstar) if nstar is not None else 'above 4096 (no crossover)'}")
    out, err = run_child(1000, 'chirp', 'float64', 50, 150, profile=True)
    if err:
        say(f"# profile: {err}")
        return 1
    say("# chirp N=1000 float64, per-slot device time (chs_profile_steps, 50 steps): ms per step, launches")
    for name, (ms, calls) in out['slots'].items():
        say(f"  {name:55s} {ms:9.4f}  {calls}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
