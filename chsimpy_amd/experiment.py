#!/usr/bin/env python
"""Monte-Carlo ensemble over (A0, A1) factors: the multi-GPU face of the hot path.

Counterpart of ``chsimpy/experiment.py``.  The reference spreads independent runs over a
``multiprocessing.Pool`` (experiment.py:197-216); here the runs are dealt to the GPUs of a
node -- one process per GPU (``torch.distributed``), ``run_id -> rank = run_id mod world`` --
and every run executes the device-resident timestep loop.  A single N x N grid does not
shard, so there is no data-path collective: the only communication is one gather of the
per-run scalar records (12 numbers per run, experiment.py:114-126) at the end, over RCCL
when the ranks sit on GPUs (backend "nccl") and over gloo in the CPU tests.

The per-run factors depend on ``A_seed`` and ``run_id`` only (experiment.py:148-170), so the
results do not depend on how many ranks share the work.

    python -m torch.distributed.run --nproc-per-node 8 -m chsimpy_amd.experiment -R 64 -N 2048 -n 2000
"""
import argparse
import os
import threading

import numpy as np

from . import utils
from .parameters import Parameters

# sympy/mpmath keep their working precision in a process-global context (nsolve(prec=7) switches it
# temporarily): concurrent members of one rank take turns in the thermodynamic post-processing.  (The
# reference runs its members in separate processes, experiment.py:211.)
_SYMPY_LOCK = threading.Lock()

COLS = ['A0', 'A1', 'ca', 'cb', 'sa', 'sb', 'tau0', 't0', 'tsep', 'id', 'fac_A0', 'fac_A1']  # experiment.py:218


class ExperimentParams:
    """experiment.py:22-30"""

    def __init__(self):
        self.runs = 2
        self.jitter_Arellow = 0.995
        self.jitter_Arelhigh = 1.005
        self.processes = -1
        self.independent = False
        self.A_source = 'uniform'
        self.A_seed = 85972


def _factor_columns(ep):
    """Two rows of per-run factors (for A0, for A1) from the seeded source: experiment.py:148-162."""
    lo, hi = ep.jitter_Arellow, ep.jitter_Arelhigh
    if ep.A_source == 'sobol':
        from scipy.stats import qmc
        # the first `runs` points of the 2^ceil(log2 runs) Sobol points, scaled to [lo, hi]
        pts = qmc.Sobol(d=2, seed=ep.A_seed).random_base2(int(np.ceil(np.log2(ep.runs))))
        return qmc.scale(pts, lo, hi)[:ep.runs].T
    return np.random.Generator(np.random.PCG64(ep.A_seed)).uniform(lo, hi, size=(ep.runs, 2)).T


def _lay_out(col_A0, col_A1, independent):
    """Joint layout: run i scales both coefficients; independent: first only A0 varies, then only A1
    (experiment.py:163-170, 176-186)."""
    n = len(col_A0)
    if not independent:
        return np.column_stack([col_A0, col_A1])
    table = np.ones((2 * n, 2))
    table[:n, 0] = col_A0
    table[n:, 1] = col_A1
    return table


def make_rand_values(ep: ExperimentParams):
    """(rand_values, A_list, number of runs): the factor table of experiment.py:148-190 for the four A sources
    (uniform, sobol, grid, or a CSV file of absolute (A0, A1) pairs)."""
    if ep.A_source in ('uniform', 'sobol'):
        f0, f1 = _factor_columns(ep)
        table = _lay_out(f0, f1, ep.independent)
        limit = 2 * ep.runs if ep.independent else ep.runs
        return table, None, min(limit, table.shape[0])
    if ep.A_source == 'grid':
        side = int(np.floor(np.sqrt(ep.runs)))
        ep.runs = side * side                         # (the reference rounds the run count down to a square)
        axis = np.linspace(ep.jitter_Arellow, ep.jitter_Arelhigh, side)
        if ep.independent:
            table = _lay_out(axis, axis, True)
        else:
            g0, g1 = np.meshgrid(axis, axis, indexing='ij')
            table = np.column_stack([g0.ravel(), g1.ravel()])
        return table, None, min(ep.runs, table.shape[0])
    A_list = utils.csv_import_matrix(ep.A_source)
    return None, A_list, min(ep.runs, A_list.shape[0])


def run_params(init_params: Parameters, run_id, rand_values, A_list):
    """Per-run Parameters with scaled A0/A1 (experiment.py:87-101)."""
    params = init_params.deepcopy()
    params.seed = init_params.seed
    params.file_id = f"{init_params.file_id}-run{run_id}"
    if A_list is None:
        fac_A0 = float(rand_values[run_id, 0])
        fac_A1 = float(rand_values[run_id, 1])
        params.func_A0 = lambda temp, f=fac_A0: utils.A0(temp) * f
        params.func_A1 = lambda temp, f=fac_A1: utils.A1(temp) * f
    else:
        a0, a1 = float(A_list[run_id][0]), float(A_list[run_id][1])
        params.func_A0 = lambda temp, a=a0: a
        params.func_A1 = lambda temp, a=a1: a
        fac_A0 = fac_A1 = None
    return params, fac_A0, fac_A1


def _member_record(run_id, params, solution, fac_A0, fac_A1, postprocess):
    """The 12-tuple of experiment.py:114-126 from a finished run."""
    ca = cb = sa = sb = float('nan')
    if postprocess:
        # experiment.py:110-112 -- a failure here (sympy missing, no common tangent, not exactly two
        # spinodal roots) is an error of the run, as in the reference: a silent NaN would poison
        # -results-agg.csv.  postprocess=False skips the thermodynamic columns explicitly.
        with _SYMPY_LOCK:
            cgap = utils.get_miscibility_gap(params.R, params.temp, params.B, solution.A0, solution.A1)
            ca, cb = float(cgap[0]), float(cgap[1])
            sa, sb = (float(r) for r in utils.get_roots_of_EPP(params.R, params.temp, solution.A0, solution.A1))
    itargmax = int(np.argmax(solution.E2))
    return (solution.A0, solution.A1, ca, cb, sa, sb, solution.tau0, solution.t0, itargmax, run_id,
            np.nan if fac_A0 is None else fac_A0, np.nan if fac_A1 is None else fac_A1)


def _domain_row(sf):
    """(k1, ell, ell_phys) of a member's final field (chsimpy_amd.spectrum.StructureFactor)."""
    return (sf.k1, sf.ell, sf.ell_phys)


def _morphology_row(mo):
    """(threshold, n_A, SA, perimeter, perimeter_inner, euler8, euler4) of a member's final field
    (chsimpy_amd.morphology.Morphology)."""
    return (mo.threshold, mo.n_A, mo.SA, mo.perimeter, mo.perimeter_inner, mo.euler8, mo.euler4)


def _droplets_row(below, above):
    """(threshold, connectivity, count, largest, spanning, mean_area below, the same four above) of a member's final
    field: two chsimpy_amd.components.Components, one per side."""
    return (below.threshold, below.connectivity, below.count, below.largest, below.spanning, below.mean_area,
            above.count, above.largest, above.spanning, above.mean_area)


def _droplets_of(solver, connectivity):
    """The two summary-only looks behind a member's run."""
    return _droplets_row(solver.components(connectivity=connectivity, side='below', table=False),
                         solver.components(connectivity=connectivity, side='above', table=False))


def _widths_side(di):
    """(fg, r_max, r2_mean, r_floor_mean, q50, q90) of one chsimpy_amd.distance.Distance with its histogram; NaN and -1
    where the side has no pixel with a finite distance."""
    if not di.finite:
        return (di.fg, float('nan'), float('nan'), float('nan'), -1, -1)
    return (di.fg, di.r_max, di.r2_mean, di.r_floor_mean, di.quantile(0.5), di.quantile(0.9))


def _widths_of(solver):
    """(threshold, the six values below, the six above) of a member's final field: two looks behind its run, summary and
    histogram alone."""
    below, above = solver.distance(side='below'), solver.distance(side='above')
    return (below.threshold,) + _widths_side(below) + _widths_side(above)


def _chords_of(solver):
    """(threshold, then count, mean, mean_weighted, max, cut for below/above x rows/cols) of a member's final field: one
    look behind its run, the summary words alone; NaN where a phase has no inner chord along a direction."""
    from . import chords as ch
    nan = float('nan')
    co = solver.chords(hist=False)
    row = (co.threshold,)
    for p in ch.PHASES:
        for d in ch.DIRECTIONS:
            k = co.count(p, d)
            row += (k, co.mean(p, d) if k else nan, co.mean_weighted(p, d) if k else nan, co.word('max_inner', p, d), co.cut(p, d))
    return row


def run_experiment_gpu(run_id, init_params, rand_values, A_list, U_init=None, postprocess=True, domains=None,
                       morphology=None, droplets=None, droplets_connectivity=4, widths=None, chords=None):
    """One ensemble member on this rank's GPU; the 12-tuple of experiment.py:114-126.  ``domains`` (a dict): the
    member's domain size, measured on the device behind its run, goes to ``domains[run_id]``; ``morphology`` (a dict):
    likewise the morphology of its final field at ``params.threshold``; ``droplets`` (a dict): likewise its connected
    components on both sides of that threshold (summary-only looks, ``droplets_connectivity`` 4 or 8); ``widths`` (a
    dict): likewise the distance transform on both sides of it (widest point, mean squared radius, radius-bin mean and
    quantiles); ``chords`` (a dict): likewise the chord lengths of both phases along rows and columns (one summary-only
    look)."""
    from .simulator import Simulator
    params, fac_A0, fac_A1 = run_params(init_params, run_id, rand_values, A_list)
    simulator = Simulator(params, U_init)
    try:
        solution = simulator.solve()
        if domains is not None:
            domains[run_id] = _domain_row(simulator.solver.structure_factor())
        if morphology is not None:
            morphology[run_id] = _morphology_row(simulator.solver.morphology())
        if droplets is not None:
            droplets[run_id] = _droplets_of(simulator.solver, droplets_connectivity)
        if widths is not None:
            widths[run_id] = _widths_of(simulator.solver)
        if chords is not None:
            chords[run_id] = _chords_of(simulator.solver)
        simulator.export()
        rec = _member_record(run_id, params, solution, fac_A0, fac_A1, postprocess)
    finally:
        # the record needs scalars only; an exception above must not leak the engine either (it goes back to the pool)
        simulator.solver.close(fetch_U=False)
    return rec


def run_batch_gpu(run_ids, init_params, rand_values, A_list, U_init=None, postprocess=True, seats=None, domains=None,
                  morphology=None, droplets=None, droplets_connectivity=4, widths=None, chords=None):
    """Several ensemble members advanced together as one device workload (chsimpy_amd.batch.BatchSolver): what
    run_experiment_gpu does for each of them -- one solve_or_resume(ntmax), the export, the 12-tuple.  ``seats``: the
    members run as a seat queue, that many at a time (None: all of them from the first step on).  ``domains``,
    ``morphology``: as in run_experiment_gpu, each from one device pass over the group; ``droplets``, ``widths``, ``chords``:
    as there, member by member on the batch's stream."""
    from .batch import BatchSolver
    from .simulator import Simulator
    runs = [run_params(init_params, i, rand_values, A_list) for i in run_ids]
    bs = BatchSolver([r[0] for r in runs], U_init, seats=seats)
    try:
        bs.prepare()
        solutions = bs.solve_or_resume()
        if domains is not None:
            for i, sf in zip(run_ids, bs.structure_factor()):
                domains[i] = _domain_row(sf)
        if morphology is not None:
            for i, mo in zip(run_ids, bs.morphology()):
                morphology[i] = _morphology_row(mo)
        if droplets is not None:
            for i, s in zip(run_ids, bs.solvers):
                droplets[i] = _droplets_of(s, droplets_connectivity)
        if widths is not None:
            for i, s in zip(run_ids, bs.solvers):
                widths[i] = _widths_of(s)
        if chords is not None:
            for i, s in zip(run_ids, bs.solvers):
                chords[i] = _chords_of(s)
        recs = []
        for m, (i, (params, fac_A0, fac_A1)) in enumerate(zip(run_ids, runs)):
            # Simulator.export() of the member (simulator.py:135-156), without a Solver of its own
            sim = Simulator.__new__(Simulator)
            sim.params, sim.solver = params, bs.solvers[m]
            sim.solution_file_id = utils.get_or_create_file_id(params.file_id)
            sim.export()
            recs.append(_member_record(i, params, solutions[m], fac_A0, fac_A1, postprocess))
    finally:
        bs.close(fetch_U=False)
    return recs


def my_run_ids(nr_items, rank, world):
    """run_id -> rank (run_id mod world)."""
    return [i for i in range(nr_items) if i % world == rank]


def gather_records(local, nr_items, rank, world, dist=None, device='cpu'):
    """All per-run records on every rank, ordered by run id.  One all_gather of a
    (ceil(n/world), 12) float64 block per rank -- a few KiB; latency-bound, bandwidth irrelevant."""
    if world == 1 or dist is None:
        return sorted(local, key=lambda r: r[9])
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, len(COLS)), float('nan'), dtype=torch.float64, device=device)
    for i, rec in enumerate(local):
        buf[i] = torch.tensor([float(x) for x in rec], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    recs = []
    for t in out:
        for row in t.cpu().numpy():
            if not np.isnan(row[9]):
                recs.append(tuple(row.tolist()))
    return sorted(recs, key=lambda r: r[9])


def gather_domains(local, nr_items, rank, world, dist=None, device='cpu'):
    """The members' (id, k1, ell, ell_phys) on every rank, ordered by run id: `local` maps this rank's run ids to
    (k1, ell, ell_phys).  One all_gather of a (ceil(n/world), 4) float64 block per rank, as gather_records."""
    rows = [(i,) + tuple(float(x) for x in v) for i, v in sorted(local.items())]
    if world == 1 or dist is None:
        return rows
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, 4), float('nan'), dtype=torch.float64, device=device)
    for k, row in enumerate(rows):
        buf[k] = torch.tensor([float(x) for x in row], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    got = [tuple(r.tolist()) for t in out for r in t.cpu().numpy() if not np.isnan(r[0])]
    return sorted((int(r[0]),) + r[1:] for r in got)


MORPHOLOGY_COLS = ('id', 'threshold', 'n_A', 'SA', 'perimeter', 'perimeter_inner', 'euler8', 'euler4')


def gather_morphology(local, nr_items, rank, world, dist=None, device='cpu'):
    """The members' MORPHOLOGY_COLS on every rank, ordered by run id: `local` maps this rank's run ids to the seven
    values behind the id.  One all_gather of a (ceil(n/world), 8) float64 block per rank, as gather_domains (the counts
    are integers below 2^53: exact in float64)."""
    rows = [(i,) + tuple(v) for i, v in sorted(local.items())]
    if world == 1 or dist is None:
        return rows
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, len(MORPHOLOGY_COLS)), float('nan'), dtype=torch.float64, device=device)
    for k, row in enumerate(rows):
        buf[k] = torch.tensor([float(x) for x in row], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    got = [tuple(r.tolist()) for t in out for r in t.cpu().numpy() if not np.isnan(r[0])]
    return sorted((int(r[0]),) + r[1:] for r in got)


DROPLETS_COLS = ('id', 'threshold', 'connectivity', 'count_below', 'largest_below', 'spanning_below', 'mean_area_below',
                 'count_above', 'largest_above', 'spanning_above', 'mean_area_above')


def gather_droplets(local, nr_items, rank, world, dist=None, device='cpu'):
    """The members' DROPLETS_COLS on every rank, ordered by run id: `local` maps this rank's run ids to the ten values
    behind the id.  One all_gather of a float64 block per rank, as gather_morphology (the counts are integers below
    2^53: exact in float64)."""
    rows = [(i,) + tuple(v) for i, v in sorted(local.items())]
    if world == 1 or dist is None:
        return rows
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, len(DROPLETS_COLS)), float('nan'), dtype=torch.float64, device=device)
    for k, row in enumerate(rows):
        buf[k] = torch.tensor([float(x) for x in row], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    got = [tuple(r.tolist()) for t in out for r in t.cpu().numpy() if not np.isnan(r[0])]
    return sorted((int(r[0]),) + r[1:] for r in got)


def write_droplets(file_id, rows):
    """``<file_id>-droplets.csv``: DROPLETS_COLS per member (--droplets), the counts as integers, the floats written so
    that they read back exactly."""
    name = f"{file_id}-droplets.csv"
    with open(name, 'w') as f:
        f.write(','.join(DROPLETS_COLS) + "\n")
        for i, t, conn, cb, lb, sb, mb, ca, la, sa, ma in rows:
            f.write(f"{int(i)},{float(t)!r},{int(conn)},{int(cb)},{int(lb)},{int(sb)},{float(mb)!r},"
                    f"{int(ca)},{int(la)},{int(sa)},{float(ma)!r}\n")
    return name


WIDTHS_COLS = ('id', 'threshold') + tuple(f"{k}_{side}" for side in ('below', 'above')
                                          for k in ('fg', 'r_max', 'r2_mean', 'r_floor_mean', 'q50', 'q90'))


def gather_widths(local, nr_items, rank, world, dist=None, device='cpu'):
    """The members' WIDTHS_COLS on every rank, ordered by run id: `local` maps this rank's run ids to the thirteen
    values behind the id.  One all_gather of a float64 block per rank, as gather_droplets (the counts are integers below
    2^53: exact in float64; a side without a finite distance has NaN there, which only the id column is tested for)."""
    rows = [(i,) + tuple(v) for i, v in sorted(local.items())]
    if world == 1 or dist is None:
        return rows
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, len(WIDTHS_COLS)), float('nan'), dtype=torch.float64, device=device)
    for k, row in enumerate(rows):
        buf[k] = torch.tensor([float(x) for x in row], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    got = [tuple(r.tolist()) for t in out for r in t.cpu().numpy() if not np.isnan(r[0])]
    return sorted((int(r[0]),) + r[1:] for r in got)


def write_widths(file_id, rows):
    """``<file_id>-widths.csv``: WIDTHS_COLS per member (--widths), the counts and quantiles as integers, the floats
    written so that they read back exactly."""
    name = f"{file_id}-widths.csv"
    with open(name, 'w') as f:
        f.write(','.join(WIDTHS_COLS) + "\n")
        for row in rows:
            i, t, sides = row[0], row[1], (row[2:8], row[8:14])
            f.write(f"{int(i)},{float(t)!r}" + ''.join(
                f",{int(fg)},{float(rm)!r},{float(r2)!r},{float(rf)!r},{int(q50)},{int(q90)}"
                for fg, rm, r2, rf, q50, q90 in sides) + "\n")
    return name


CHORDS_COLS = ('id', 'threshold') + tuple(f"{k}_{phase}_{d}" for phase in ('below', 'above') for d in ('rows', 'cols')
                                          for k in ('count', 'mean', 'mean_weighted', 'max', 'cut'))


def gather_chords(local, nr_items, rank, world, dist=None, device='cpu'):
    """The members' CHORDS_COLS on every rank, ordered by run id: `local` maps this rank's run ids to the twenty-one
    values behind the id.  One all_gather of a float64 block per rank, as gather_widths (the counts are integers below
    2^53: exact in float64; a phase without an inner chord has NaN there, which only the id column is tested for)."""
    rows = [(i,) + tuple(v) for i, v in sorted(local.items())]
    if world == 1 or dist is None:
        return rows
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, len(CHORDS_COLS)), float('nan'), dtype=torch.float64, device=device)
    for k, row in enumerate(rows):
        buf[k] = torch.tensor([float(x) for x in row], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    got = [tuple(r.tolist()) for t in out for r in t.cpu().numpy() if not np.isnan(r[0])]
    return sorted((int(r[0]),) + r[1:] for r in got)


def write_chords(file_id, rows):
    """``<file_id>-chords.csv``: CHORDS_COLS per member (--chords), the counts and the longest chords as integers, the
    floats written so that they read back exactly."""
    name = f"{file_id}-chords.csv"
    with open(name, 'w') as f:
        f.write(','.join(CHORDS_COLS) + "\n")
        for row in rows:
            i, t, groups = row[0], row[1], [row[2 + 5 * k:7 + 5 * k] for k in range(4)]
            f.write(f"{int(i)},{float(t)!r}" + ''.join(
                f",{int(n)},{float(m)!r},{float(mw)!r},{int(mx)},{int(cut)}" for n, m, mw, mx, cut in groups) + "\n")
    return name


def write_morphology(file_id, rows):
    """``<file_id>-morphology.csv``: MORPHOLOGY_COLS per member (--morphology), the counts as integers, the two floats
    written so that they read back exactly."""
    name = f"{file_id}-morphology.csv"
    with open(name, 'w') as f:
        f.write(','.join(MORPHOLOGY_COLS) + "\n")
        for i, t, n_A, SA, per, per_in, e8, e4 in rows:
            f.write(f"{int(i)},{float(t)!r},{int(n_A)},{float(SA)!r},{int(per)},{int(per_in)},{int(e8)},{int(e4)}\n")
    return name


def write_domains(file_id, rows):
    """``<file_id>-domains.csv``: ``id, k1, ell, ell_phys`` per member (--domain-size), the floats written so that
    they read back exactly."""
    name = f"{file_id}-domains.csv"
    with open(name, 'w') as f:
        f.write("id,k1,ell,ell_phys\n")
        for i, k1, ell, ell_phys in rows:
            f.write(f"{int(i)},{float(k1)!r},{float(ell)!r},{float(ell_phys)!r}\n")
    return name


def write_metadata(file_id, ep, extra=()):
    """``<file_id>-metadata.csv`` (experiment.py:193-195): system information followed by the
    experiment parameters, one ``name, value`` per line."""
    lines = list(utils.get_system_info()) + list(extra) + utils.vars_to_list(ep)
    utils.csv_export_list(f"{file_id}-metadata.csv", "\n".join(lines))
    return f"{file_id}-metadata.csv"


def write_results(file_id, records):
    """``<file_id>-results.csv`` and ``-results-agg.csv`` exactly as experiment.py:218-225."""
    import pandas as pd
    df = pd.DataFrame(records, columns=COLS)
    df[['tau0', 'id']] = df[['tau0', 'id']].astype(int)
    # tsep = argmax(E2) is an integer in the reference's tuples (experiment.py:113); after the gather of a float64 block
    # it must read the same, or the file would depend on the number of ranks
    df['tsep'] = df['tsep'].astype(int)
    df.to_csv(f"{file_id}-results.csv")
    agg = df.loc[:, df.columns != 'id'].describe()
    agg.loc['cv'] = agg.loc['std'] / agg.loc['mean']
    agg.T.to_csv(f"{file_id}-results-agg.csv")
    return df, agg


def run_ensemble(init_params, ep, run_fn=None, U_init=None, dist=None, rank=0, world=1, device='cpu',
                 concurrent=1, batch=0, batch_fn=None, queue=False, queue_members=256, domains=None, morphology=None,
                 droplets=None, droplets_connectivity=4, widths=None, chords=None):
    """Deal the runs to the ranks, execute, gather.  ``run_fn(run_id, init_params, rand_values,
    A_list)`` defaults to the GPU run; the CPU tests inject a stand-in.

    ``concurrent`` members of a rank run at the same time (one engine handle = one HIP stream each;
    the C ABI calls release the GIL): at ensemble sizes such as N=2048 a single run leaves the GPU
    partly idle between its latency-bound kernels, two or three concurrent runs fill the gaps.

    ``batch`` > 0: the rank's members run ``batch`` at a time as one device workload, every step kernel launched
    once for the whole group (``batch_fn(run_ids, init_params, rand_values, A_list)`` -> their 12-tuples; default
    run_batch_gpu).  An ensemble with ``adaptive_time`` is taken too: its members all adapt their step.  A configuration
    outside the batch's scope (chsimpy_amd.batch.scope_error: N, engine, jitter) runs member by member instead, with a
    note.  An N of the chirp engine (engine='chirp', or 'auto' from N=129 where N is no power of two) is a chirp batch.

    ``queue`` (with ``batch`` > 0): the rank's members form one seat queue with ``batch`` seats instead of groups of
    ``batch`` -- a member that stops hands its seat to the next one on the device, so the device does not run the tail
    of every group nearly empty.  Every member of a queue owns its device arrays from the start, so the runs are cut
    into queues of at most ``queue_members``; ``batch_fn`` is called once per queue.  A chirp batch has no queue:
    ``queue`` at such an N runs member by member, with the note.

    ``domains`` (a dict, with the default run functions): every member's domain size -- first moment k1 of the radially
    averaged structure factor of its final field, the characteristic length 2N/k1 and that length in the solver's unit
    -- is measured on the device behind its run and left in ``domains[run_id]`` for this rank's runs (gather_domains).

    ``morphology`` (a dict, with the default run functions): likewise the morphology of every member's final field at
    its ``params.threshold`` -- area, interface length, Euler numbers (chsimpy_amd/morphology.py) -- in
    ``morphology[run_id]`` (gather_morphology).

    ``droplets`` (a dict, with the default run functions): likewise the connected components of every member's final
    field on both sides of its ``params.threshold`` -- count, largest, spanning, mean area (chsimpy_amd/components.py),
    at ``droplets_connectivity`` -- in ``droplets[run_id]`` (gather_droplets).

    ``widths`` (a dict, with the default run functions): likewise the distance transform of every member's final field
    on both sides of its ``params.threshold`` -- foreground, widest point, mean squared radius, radius-bin mean and
    quantiles (chsimpy_amd/distance.py) -- in ``widths[run_id]`` (gather_widths).

    ``chords`` (a dict, with the default run functions): likewise the chord lengths of both phases of every member's
    final field along rows and columns -- count, mean, weighted mean, longest inner chord and the chords at a wall
    (chsimpy_amd/chords.py) -- in ``chords[run_id]`` (gather_chords)."""
    rand_values, A_list, nr_items = make_rand_values(ep)
    dom = {} if domains is None else {'domains': domains}   # (the run functions are called as ever without it)
    if morphology is not None:
        dom['morphology'] = morphology
    if droplets is not None:
        dom['droplets'], dom['droplets_connectivity'] = droplets, int(droplets_connectivity)
    if widths is not None:
        dom['widths'] = widths
    if chords is not None:
        dom['chords'] = chords
    if run_fn is None:
        def run_fn(run_id, p, rv, al):
            return run_experiment_gpu(run_id, p, rv, al, U_init, **dom)
    ids = my_run_ids(nr_items, rank, world)
    if batch > 0 and batch_fn is None:
        from .batch import scope_error
        why = scope_error(init_params, seats=batch if queue else None)
        if why:
            print(f"chsimpy_amd.experiment: --batch {batch} not taken ({why}); members run one by one")
            batch = 0
        else:
            def batch_fn(run_ids, p, rv, al):
                if queue:
                    return run_batch_gpu(run_ids, p, rv, al, U_init, seats=batch, **dom)
                return run_batch_gpu(run_ids, p, rv, al, U_init, **dom)
    if batch > 0:
        local = []
        group = max(int(queue_members), 1) if queue else batch
        for k in range(0, len(ids), group):
            local.extend(batch_fn(ids[k:k + group], init_params, rand_values, A_list))
    elif concurrent > 1 and len(ids) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=concurrent) as pool:
            local = list(pool.map(lambda i: run_fn(i, init_params, rand_values, A_list), ids))
    else:
        local = [run_fn(i, init_params, rand_values, A_list) for i in ids]
    return gather_records(local, nr_items, rank, world, dist, device)


def _dry_member(run_id, init_params, rand_values, A_list):
    """`--dry-run`: a member without device work (launcher / partition / collective rehearsal on CPUs) -- a
    deterministic function of the run's coefficients, so that the result files can be compared across world sizes."""
    params, f0, f1 = run_params(init_params, run_id, rand_values, A_list)
    a0, a1 = params.func_A0(params.temp), params.func_A1(params.temp)
    return (a0, a1, 0.1, 0.9, 0.2, 0.8, 100 + run_id, 1.5 * run_id, 7 * run_id, run_id,
            np.nan if f0 is None else f0, np.nan if f1 is None else f1)


def _dry_batch(run_ids, init_params, rand_values, A_list):
    """`--dry-run --batch B`: a group of members without device work (see _dry_member)."""
    return [_dry_member(i, init_params, rand_values, A_list) for i in run_ids]


def _launch_own_ranks(a, argv):
    """`--gpus G` without a launcher around it: this process -- which has not touched the GPU -- starts the G ranks as
    ordinary child processes, one per GPU, as the reference starts its own pool (experiment.py:197-216), and forwards
    rank 0's output."""
    import sys
    from . import launch
    if not a.dry_run:
        import importlib.util
        entry = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), '__graft_entry__.py')
        if os.path.exists(entry):   # build once, before the ranks start (hipcc only; no device needed)
            spec = importlib.util.spec_from_file_location('__graft_entry__', entry)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mod.build_hip()
    args = list(sys.argv[1:] if argv is None else argv)
    failed, codes, texts = launch.spawn_ranks([sys.executable, '-m', 'chsimpy_amd.experiment'] + args, a.gpus,
                                              timeout_s=float(os.environ.get('CHS_LAUNCH_TIMEOUT', '86400')))
    if failed is not None:
        launch.report_failure('chsimpy_amd.experiment', failed, codes, texts)
        raise SystemExit(1)
    sys.stdout.write(texts[0])
    sys.stdout.flush()


def main(argv=None):
    ap = argparse.ArgumentParser(description='chsimpy_amd ensemble (cf. chsimpy-experiment)')
    ap.add_argument('-N', type=int, default=512)
    ap.add_argument('-n', '--ntmax', type=int, default=int(1e6))
    ap.add_argument('-R', '--runs', type=int, default=3)
    ap.add_argument('--independent', action='store_true')
    ap.add_argument('--A-source', default='uniform')
    ap.add_argument('--A-seed', type=int, default=85972)
    ap.add_argument('-K', '--kappa-tilde', type=float, default=None)
    ap.add_argument('--full-sim', action='store_true')
    ap.add_argument('-a', '--adaptive-time', action='store_true', help='adaptive time stepping (the reference\'s -a)')
    ap.add_argument('--delt-max', type=float, default=None, help='upper bound of the adaptive step (parameters.py: 9e-8)')
    ap.add_argument('--file-id', default='auto')
    ap.add_argument('--export-csv', default=None)
    ap.add_argument('--Uinit-file', default=None)
    ap.add_argument('--concurrent', type=int, default=2, help='ensemble members running at once per GPU')
    ap.add_argument('--batch', type=int, default=0, help='advance a rank\'s members this many at a time as one device '
                    'workload (0: one member per engine handle, see --concurrent)')
    ap.add_argument('--queue', action='store_true', help='with --batch B: the rank\'s members form one seat queue of B seats; '
                    'a member that stops hands its seat to the next one on the device')
    ap.add_argument('--queue-members', type=int, default=256, help='members of one queue at the most (each owns its device '
                    'arrays from the start)')
    ap.add_argument('--domain-size', action='store_true', help='measure every member\'s domain size on the device behind its '
                    'run (radially averaged structure factor of the final field): <id>-domains.csv with id, k1, ell, ell_phys')
    ap.add_argument('--morphology', action='store_true', help='measure the morphology of every member\'s final field on the '
                    'device behind its run (bit-quad counts of the field below the threshold): <id>-morphology.csv with id, '
                    'threshold, n_A, SA, perimeter, perimeter_inner, euler8, euler4')
    ap.add_argument('--droplets', action='store_true', help='label the connected components of every member\'s final field on '
                    'the device behind its run, on both sides of the threshold: <id>-droplets.csv with id, threshold, '
                    'connectivity, and count, largest, spanning, mean_area below and above')
    ap.add_argument('--widths', action='store_true', help='measure the exact Euclidean distance transform of every member\'s '
                    'final field on the device behind its run, on both sides of the threshold: <id>-widths.csv with id, '
                    'threshold, and fg, r_max, r2_mean, r_floor_mean, q50, q90 (radius-bin quantiles) below and above')
    ap.add_argument('--chords', action='store_true', help='measure the chord lengths (linear intercepts) of both phases of '
                    'every member\'s final field on the device behind its run, along rows and columns: <id>-chords.csv with '
                    'id, threshold, and count, mean, mean_weighted, max (inner chords), cut (chords at a wall) for '
                    'below/above x rows/cols')
    ap.add_argument('--droplets-connectivity', type=int, choices=(4, 8), default=4, help='the connectivity of --droplets')
    ap.add_argument('--gpus', type=int, default=1, help='start this many ranks (one per GPU) from here when no launcher '
                    'such as torch.distributed.run has set RANK/WORLD_SIZE')
    ap.add_argument('--backend', default=os.environ.get('CHS_DIST_BACKEND', 'nccl'),
                    help='torch.distributed backend: nccl (= RCCL, ranks on GPUs) or gloo (CPU rehearsal)')
    ap.add_argument('--dry-run', action='store_true', help='members without device work: rehearses launcher, partition, '
                    'core placement and the gather on CPUs; the result files are not results')
    a = ap.parse_args(argv)

    if a.gpus > 1 and 'RANK' not in os.environ:
        return _launch_own_ranks(a, argv)

    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    # Placement first, before anything touches the GPU: this rank's share of the host cores (the reference sizes its
    # pool to the physical cores, experiment.py:197-202; here the cores are dealt to the ranks), one torch intra-op thread
    from . import launch
    pinned = launch.pin_rank_to_cores(local_rank, world)
    dist = None
    device = 'cpu'
    if world > 1:
        import torch
        import torch.distributed as dist
        launch.quiet_host_threads()
        if a.backend == 'nccl':
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend='nccl', device_id=torch.device('cuda', local_rank))
            device = f'cuda:{local_rank}'
        else:
            dist.init_process_group(backend=a.backend)

    p = Parameters()
    p.N, p.ntmax, p.full_sim, p.kappa_tilde = a.N, a.ntmax, a.full_sim, a.kappa_tilde
    p.no_gui, p.export_csv, p.Uinit_file = True, a.export_csv, a.Uinit_file
    p.adaptive_time = a.adaptive_time
    if a.delt_max is not None:
        p.delt_max = a.delt_max
    # (CHS_SAME_GPU=1: every rank on device 0 -- rehearsing the multi-rank path with real device work on a one-GPU box)
    p.device = 0 if os.environ.get('CHS_SAME_GPU') == '1' else local_rank
    p.file_id = utils.get_or_create_file_id(a.file_id)
    ep = ExperimentParams()
    ep.runs, ep.independent, ep.A_source, ep.A_seed = a.runs, a.independent, a.A_source, a.A_seed
    U_init = utils.csv_import_matrix(p.Uinit_file) if p.Uinit_file else None

    if rank == 0:
        write_metadata(p.file_id, ep, extra=[f"ranks, {world}", f"concurrent_per_rank, {a.concurrent}",
                                             f"host_cores_per_rank, {'all' if pinned is None else len(pinned)}"]
                       + ([f"batch_per_rank, {a.batch}"] if a.batch > 0 else [])
                       + ([f"queue_members, {a.queue_members}"] if (a.batch > 0 and a.queue) else [])
                       + (["dry_run, True"] if a.dry_run else []))
    domains = {} if a.domain_size else None
    morph = {} if a.morphology else None
    drops = {} if a.droplets else None
    wid = {} if a.widths else None
    cho = {} if a.chords else None
    records = run_ensemble(p, ep, run_fn=_dry_member if a.dry_run else None, U_init=U_init, dist=dist, rank=rank,
                           world=world, device=device, concurrent=a.concurrent, batch=max(a.batch, 0),
                           batch_fn=_dry_batch if (a.dry_run and a.batch > 0) else None,
                           queue=bool(a.queue and a.batch > 0), queue_members=a.queue_members, domains=domains,
                           **({} if morph is None else {'morphology': morph}),
                           **({} if drops is None else {'droplets': drops, 'droplets_connectivity': a.droplets_connectivity}),
                           **({} if wid is None else {'widths': wid}),
                           **({} if cho is None else {'chords': cho}))
    if domains is not None:
        if a.dry_run:   # (members without device work: a function of the run id, as their records are)
            nr = make_rand_values(ep)[2]
            domains = {i: (1.0 + i, 2.0 * p.N / (1.0 + i), 2.0 * p.N / (1.0 + i) * p.L / (p.N - 1)) for i in my_run_ids(nr, rank, world)}
        domain_rows = gather_domains(domains, make_rand_values(ep)[2], rank, world, dist, device)
    if morph is not None:
        nr = make_rand_values(ep)[2]
        if a.dry_run:   # (made up from the run id, as above: a full field with i single-pixel holes)
            morph = {i: (float(p.threshold), p.N * p.N - i, (p.N * p.N - i) / (p.N * p.N), 4 * p.N + 4 * i, 4 * i, 1 - i, 1 - i)
                     for i in my_run_ids(nr, rank, world)}
        morphology_rows = gather_morphology(morph, nr, rank, world, dist, device)
    if drops is not None:
        nr = make_rand_values(ep)[2]
        if a.dry_run:   # (made up from the run id, as above: i + 1 droplets of 3 pixels in a spanning matrix with i holes)
            drops = {i: (float(p.threshold), a.droplets_connectivity, i + 1, 3, 0, 3.0, 1, p.N * p.N - 3 * (i + 1), 1,
                         float(p.N * p.N - 3 * (i + 1))) for i in my_run_ids(nr, rank, world)}
        droplets_rows = gather_droplets(drops, nr, rank, world, dist, device)
    if wid is not None:
        nr = make_rand_values(ep)[2]
        if a.dry_run:   # (made up from the run id, as above: i + 1 pixels below, each its own distance 1; a matrix i + 2 wide)
            wid = {i: (float(p.threshold), i + 1, 1.0, 1.0, 1.0, 1, 1,
                       p.N * p.N - (i + 1), float(i + 2), 0.5 * (i + 2) ** 2, 0.5 * (i + 2), (i + 2) // 2, i + 2)
                   for i in my_run_ids(nr, rank, world)}
        widths_rows = gather_widths(wid, nr, rank, world, dist, device)
    if cho is not None:
        nr = make_rand_values(ep)[2]
        if a.dry_run:   # (made up from the run id, as above: i + 1 inner chords of 2 and 4 pixels below along the rows, ...)
            cho = {i: (float(p.threshold), i + 1, 3.0, 10.0 / 3.0, 4, 1, i + 2, 1.5, 1.75, 2, 0,
                       i + 3, float(i + 2), i + 2.5, 2 * i + 4, p.N, i + 4, 0.1 * (i + 1), 1.0 / (i + 3), i + 5, p.N + 1)
                   for i in my_run_ids(nr, rank, world)}
        chords_rows = gather_chords(cho, nr, rank, world, dist, device)
    if rank == 0:
        df, agg = write_results(p.file_id, records)
        print(agg.T)
        print('Output files:')
        print(f"  {p.file_id}-metadata.csv")
        print(f"  {p.file_id}-results-agg.csv")
        print(f"  {p.file_id}-results.csv")
        if domains is not None:
            print(f"  {write_domains(p.file_id, domain_rows)}")
        if morph is not None:
            print(f"  {write_morphology(p.file_id, morphology_rows)}")
        if drops is not None:
            print(f"  {write_droplets(p.file_id, droplets_rows)}")
        if wid is not None:
            print(f"  {write_widths(p.file_id, widths_rows)}")
        if cho is not None:
            print(f"  {write_chords(p.file_id, chords_rows)}")
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
