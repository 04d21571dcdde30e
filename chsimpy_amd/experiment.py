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
from typing import Callable, NamedTuple, Optional

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
    return (float(sf.k1), float(sf.ell), float(sf.ell_phys))


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


def _composition_of(solver):
    """(threshold, n_nan, min, max, mean, var, SA, mean_below, mean_above, q05, q50, q95) of a member's final field: one
    look behind its run and one select, without the histogram; NaN where a value does not exist."""
    nan = float('nan')
    co = solver.composition(bins=1, quantiles=(0.05, 0.5, 0.95), hist=False)
    val = lambda v: nan if v is None else v
    return (co.threshold, co.n_nan, co.min, co.max, val(co.mean), val(co.var), co.SA, val(co.mean_below), val(co.mean_above),
            co.quantiles.get(0.05, nan), co.quantiles.get(0.5, nan), co.quantiles.get(0.95, nan))


DOMAINS_COLS = ('id', 'k1', 'ell', 'ell_phys')
MORPHOLOGY_COLS = ('id', 'threshold', 'n_A', 'SA', 'perimeter', 'perimeter_inner', 'euler8', 'euler4')
DROPLETS_COLS = ('id', 'threshold', 'connectivity', 'count_below', 'largest_below', 'spanning_below', 'mean_area_below',
                 'count_above', 'largest_above', 'spanning_above', 'mean_area_above')
WIDTHS_COLS = ('id', 'threshold') + tuple(f"{k}_{side}" for side in ('below', 'above')
                                          for k in ('fg', 'r_max', 'r2_mean', 'r_floor_mean', 'q50', 'q90'))
CHORDS_COLS = ('id', 'threshold') + tuple(f"{k}_{phase}_{d}" for phase in ('below', 'above') for d in ('rows', 'cols')
                                          for k in ('count', 'mean', 'mean_weighted', 'max', 'cut'))
COMPOSITION_COLS = ('id', 'threshold', 'n_nan', 'min', 'max', 'mean', 'var', 'SA', 'mean_below', 'mean_above', 'q05', 'q50',
                    'q95')


# `--dry-run`: rows made up from the run id, as the members' records are (_dry_member) -- members without device work
def _dry_domains(i, p, opts):
    return (1.0 + i, 2.0 * p.N / (1.0 + i), 2.0 * p.N / (1.0 + i) * p.L / (p.N - 1))


def _dry_morphology(i, p, opts):
    """A full field with i single-pixel holes."""
    return (float(p.threshold), p.N * p.N - i, (p.N * p.N - i) / (p.N * p.N), 4 * p.N + 4 * i, 4 * i, 1 - i, 1 - i)


def _dry_droplets(i, p, opts):
    """i + 1 droplets of 3 pixels in a spanning matrix with i holes."""
    return (float(p.threshold), opts['droplets_connectivity'], i + 1, 3, 0, 3.0, 1, p.N * p.N - 3 * (i + 1), 1,
            float(p.N * p.N - 3 * (i + 1)))


def _dry_widths(i, p, opts):
    """i + 1 pixels below, each its own distance 1; a matrix i + 2 wide."""
    return (float(p.threshold), i + 1, 1.0, 1.0, 1.0, 1, 1,
            p.N * p.N - (i + 1), float(i + 2), 0.5 * (i + 2) ** 2, 0.5 * (i + 2), (i + 2) // 2, i + 2)


def _dry_chords(i, p, opts):
    """i + 1 inner chords of 2 and 4 pixels below along the rows, ..."""
    return (float(p.threshold), i + 1, 3.0, 10.0 / 3.0, 4, 1, i + 2, 1.5, 1.75, 2, 0,
            i + 3, float(i + 2), i + 2.5, 2 * i + 4, p.N, i + 4, 0.1 * (i + 1), 1.0 / (i + 3), i + 5, p.N + 1)


def _dry_composition(i, p, opts):
    """i NaN pixels in a field of two compositions."""
    return (float(p.threshold), i, 0.125, 0.875 + 0.001 * i, 0.5, 0.1 / (i + 1), 0.5, 0.25, 0.75, 0.126, 0.5, 0.874)


class Measurement(NamedTuple):
    """One look at a member's final field, measured on the device behind its run: the keyword of the run functions under
    which its rows are collected (a dict, run id -> the values behind the id), the command-line flag, the file
    ``<file_id>-<suffix>.csv`` with its columns (``int_cols`` of them written as integers), and where a row comes from:
    ``row_of(solver, opts)`` of one member, ``rows_of_batch(bs)`` where one device pass serves a whole BatchSolver, and
    ``dry_row(i, p, opts)`` of a `--dry-run`.  ``opts``: {'droplets_connectivity': 4 or 8}."""
    key: str
    flag: str
    help: str
    suffix: str
    cols: tuple
    int_cols: frozenset
    row_of: Callable
    dry_row: Callable
    rows_of_batch: Optional[Callable] = None


# In the order in which the files are written and printed.
MEASUREMENTS = (
    Measurement('domains', '--domain-size', 'measure every member\'s domain size on the device behind its run (radially '
                'averaged structure factor of the final field): <id>-domains.csv with id, k1, ell, ell_phys',
                'domains', DOMAINS_COLS, frozenset({'id'}),
                lambda s, opts: _domain_row(s.structure_factor()), _dry_domains,
                lambda bs: [_domain_row(sf) for sf in bs.structure_factor()]),
    Measurement('morphology', '--morphology', 'measure the morphology of every member\'s final field on the device behind '
                'its run (bit-quad counts of the field below the threshold): <id>-morphology.csv with id, threshold, n_A, '
                'SA, perimeter, perimeter_inner, euler8, euler4',
                'morphology', MORPHOLOGY_COLS,
                frozenset({'id', 'n_A', 'perimeter', 'perimeter_inner', 'euler8', 'euler4'}),
                lambda s, opts: _morphology_row(s.morphology()), _dry_morphology,
                lambda bs: [_morphology_row(mo) for mo in bs.morphology()]),
    Measurement('droplets', '--droplets', 'label the connected components of every member\'s final field on the device '
                'behind its run, on both sides of the threshold: <id>-droplets.csv with id, threshold, connectivity, and '
                'count, largest, spanning, mean_area below and above',
                'droplets', DROPLETS_COLS,
                frozenset({'id', 'connectivity', 'count_below', 'largest_below', 'spanning_below', 'count_above', 'largest_above',
                           'spanning_above'}),
                lambda s, opts: _droplets_of(s, opts['droplets_connectivity']), _dry_droplets),
    Measurement('widths', '--widths', 'measure the exact Euclidean distance transform of every member\'s final field on the '
                'device behind its run, on both sides of the threshold: <id>-widths.csv with id, threshold, and fg, r_max, '
                'r2_mean, r_floor_mean, q50, q90 (radius-bin quantiles) below and above',
                'widths', WIDTHS_COLS,
                frozenset({'id', 'fg_below', 'q50_below', 'q90_below', 'fg_above', 'q50_above', 'q90_above'}),
                lambda s, opts: _widths_of(s), _dry_widths),
    Measurement('chords', '--chords', 'measure the chord lengths (linear intercepts) of both phases of every member\'s final '
                'field on the device behind its run, along rows and columns: <id>-chords.csv with id, threshold, and count, '
                'mean, mean_weighted, max (inner chords), cut (chords at a wall) for below/above x rows/cols',
                'chords', CHORDS_COLS,
                frozenset(c for c in CHORDS_COLS if c == 'id' or c.split('_')[0] in ('count', 'max', 'cut')),
                lambda s, opts: _chords_of(s), _dry_chords),
)

# The looks at the values of the field rather than at its thresholded image: entries of the same kind, walked behind
# MEASUREMENTS everywhere (ALL_MEASUREMENTS).  A tuple of its own only because tests/test_measurements_host.py pins
# MEASUREMENTS to its five keys.
FIELD_MEASUREMENTS = (
    Measurement('composition', '--composition', 'measure the composition of every member\'s final field on the device '
                'behind its run (range, moments, the means on either side of the threshold, exact quantiles): '
                '<id>-composition.csv with id, threshold, n_nan, min, max, mean, var, SA, mean_below, mean_above, q05, q50, '
                'q95',
                'composition', COMPOSITION_COLS, frozenset({'id', 'n_nan'}),
                lambda s, opts: _composition_of(s), _dry_composition),
)
ALL_MEASUREMENTS = MEASUREMENTS + FIELD_MEASUREMENTS


def _asked(domains, morphology, droplets, widths, chords, composition=None):
    """The measurements a caller asked for, keyed like ALL_MEASUREMENTS: the dicts its rows go to."""
    given = dict(domains=domains, morphology=morphology, droplets=droplets, widths=widths, chords=chords,
                 composition=composition)
    return {k: v for k, v in given.items() if v is not None}


def run_experiment_gpu(run_id, init_params, rand_values, A_list, U_init=None, postprocess=True, domains=None,
                       morphology=None, droplets=None, droplets_connectivity=4, widths=None, chords=None, composition=None):
    """One ensemble member on this rank's GPU; the 12-tuple of experiment.py:114-126.  ``domains``, ``morphology``,
    ``droplets``, ``widths``, ``chords``, ``composition`` (a dict each): the member's row of that entry of ALL_MEASUREMENTS, measured on the
    device behind its run at ``params.threshold``, goes to ``<dict>[run_id]`` (``droplets_connectivity`` 4 or 8: that of
    the droplets)."""
    from .simulator import Simulator
    asked = _asked(domains, morphology, droplets, widths, chords, composition)
    opts = {'droplets_connectivity': droplets_connectivity}
    params, fac_A0, fac_A1 = run_params(init_params, run_id, rand_values, A_list)
    simulator = Simulator(params, U_init)
    try:
        solution = simulator.solve()
        for m in ALL_MEASUREMENTS:
            if m.key in asked:
                asked[m.key][run_id] = m.row_of(simulator.solver, opts)
        simulator.export()
        rec = _member_record(run_id, params, solution, fac_A0, fac_A1, postprocess)
    finally:
        # the record needs scalars only; an exception above must not leak the engine either (it goes back to the pool)
        simulator.solver.close(fetch_U=False)
    return rec


def run_batch_gpu(run_ids, init_params, rand_values, A_list, U_init=None, postprocess=True, seats=None, domains=None,
                  morphology=None, droplets=None, droplets_connectivity=4, widths=None, chords=None, composition=None):
    """Several ensemble members advanced together as one device workload (chsimpy_amd.batch.BatchSolver): what
    run_experiment_gpu does for each of them -- one solve_or_resume(ntmax), the export, the 12-tuple.  ``seats``: the
    members run as a seat queue, that many at a time (None: all of them from the first step on).  The measurements: as
    in run_experiment_gpu, from one device pass over the group where the entry has ``rows_of_batch``, else member by
    member on the batch's stream."""
    from .batch import BatchSolver
    from .simulator import Simulator
    asked = _asked(domains, morphology, droplets, widths, chords, composition)
    opts = {'droplets_connectivity': droplets_connectivity}
    runs = [run_params(init_params, i, rand_values, A_list) for i in run_ids]
    bs = BatchSolver([r[0] for r in runs], U_init, seats=seats)
    try:
        bs.prepare()
        solutions = bs.solve_or_resume()
        for m in ALL_MEASUREMENTS:
            if m.key in asked:
                rows = m.rows_of_batch(bs) if m.rows_of_batch else (m.row_of(s, opts) for s in bs.solvers)
                asked[m.key].update(zip(run_ids, rows))
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


def _all_gather_rows(rows, ncols, id_col, nr_items, world, dist, device):
    """Every rank's rows, as tuples of floats: one all_gather of a (ceil(n/world), ncols) float64 block per rank -- a few
    KiB; latency-bound, bandwidth irrelevant.  A block is padded with NaN rows, recognised by their id column alone
    (other columns may hold NaN in a member's row)."""
    import torch
    per = (nr_items + world - 1) // world
    buf = torch.full((per, ncols), float('nan'), dtype=torch.float64, device=device)
    for k, row in enumerate(rows):
        buf[k] = torch.tensor([float(x) for x in row], dtype=torch.float64, device=device)
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    return [tuple(r.tolist()) for t in out for r in t.cpu().numpy() if not np.isnan(r[id_col])]


def gather_records(local, nr_items, rank, world, dist=None, device='cpu'):
    """All per-run records on every rank, ordered by run id."""
    if world > 1 and dist is not None:
        local = _all_gather_rows(local, len(COLS), 9, nr_items, world, dist, device)
    return sorted(local, key=lambda r: r[9])


def gather_rows(local, ncols, nr_items, rank, world, dist=None, device='cpu'):
    """The members' rows of one measurement on every rank, ordered by run id: `local` maps this rank's run ids to the
    ``ncols - 1`` values behind the id (the counts are integers below 2^53: exact in the float64 block)."""
    rows = [(i,) + tuple(v) for i, v in sorted(local.items())]
    if world == 1 or dist is None:
        return rows
    got = _all_gather_rows(rows, ncols, 0, nr_items, world, dist, device)
    return sorted((int(r[0]),) + r[1:] for r in got)


def write_rows(file_id, measurement, rows):
    """``<file_id>-<suffix>.csv``: the measurement's columns per member, its integer columns as integers, the floats
    written so that they read back exactly."""
    name = f"{file_id}-{measurement.suffix}.csv"
    with open(name, 'w') as f:
        f.write(','.join(measurement.cols) + "\n")
        for row in rows:
            f.write(','.join(str(int(x)) if c in measurement.int_cols else repr(float(x))
                             for c, x in zip(measurement.cols, row)) + "\n")
    return name


def _writer(measurement):
    return lambda file_id, rows: write_rows(file_id, measurement, rows)


# the writers by the names callers know: write_widths(file_id, rows) is write_rows with the widths entry
write_domains, write_morphology, write_droplets, write_widths, write_chords = (_writer(m) for m in MEASUREMENTS)
write_composition, = (_writer(m) for m in FIELD_MEASUREMENTS)


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
                 droplets=None, droplets_connectivity=4, widths=None, chords=None, composition=None):
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

    ``domains``, ``morphology``, ``droplets``, ``widths``, ``chords``, ``composition`` (a dict each, with the default run
    functions): that entry of ALL_MEASUREMENTS -- the domain size from the radially averaged structure factor (chsimpy_amd/spectrum.py), the
    morphology (morphology.py), the connected components on both sides of the threshold at ``droplets_connectivity``
    (components.py), the distance transform on both sides (distance.py), the chord lengths of both phases along rows
    and columns (chords.py), the composition (composition.py) -- is measured on every member's final field, on the device behind its run at its
    ``params.threshold``, and left in ``<dict>[run_id]`` for this rank's runs (gather_rows)."""
    rand_values, A_list, nr_items = make_rand_values(ep)
    dom = _asked(domains, morphology, droplets, widths, chords, composition)   # (the run functions are called as ever without them)
    if droplets is not None:
        dom['droplets_connectivity'] = int(droplets_connectivity)
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


def arg_parser():
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
    for m in ALL_MEASUREMENTS:
        ap.add_argument(m.flag, dest=m.key, action='store_true', help=m.help)
    ap.add_argument('--droplets-connectivity', type=int, choices=(4, 8), default=4, help='the connectivity of --droplets')
    ap.add_argument('--gpus', type=int, default=1, help='start this many ranks (one per GPU) from here when no launcher '
                    'such as torch.distributed.run has set RANK/WORLD_SIZE')
    ap.add_argument('--backend', default=os.environ.get('CHS_DIST_BACKEND', 'nccl'),
                    help='torch.distributed backend: nccl (= RCCL, ranks on GPUs) or gloo (CPU rehearsal)')
    ap.add_argument('--dry-run', action='store_true', help='members without device work: rehearses launcher, partition, '
                    'core placement and the gather on CPUs; the result files are not results')
    return ap


def main(argv=None):
    a = arg_parser().parse_args(argv)

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
    asked = [m for m in ALL_MEASUREMENTS if getattr(a, m.key)]
    local = {m.key: {} for m in asked}
    opts = {'droplets_connectivity': a.droplets_connectivity}
    records = run_ensemble(p, ep, run_fn=_dry_member if a.dry_run else None, U_init=U_init, dist=dist, rank=rank,
                           world=world, device=device, concurrent=a.concurrent, batch=max(a.batch, 0),
                           batch_fn=_dry_batch if (a.dry_run and a.batch > 0) else None,
                           queue=bool(a.queue and a.batch > 0), queue_members=a.queue_members,
                           **local, **(opts if a.droplets else {}))
    nr = make_rand_values(ep)[2] if asked else 0
    rows = {}
    for m in asked:
        if a.dry_run:   # (members without device work: a function of the run id, as their records are)
            local[m.key] = {i: m.dry_row(i, p, opts) for i in my_run_ids(nr, rank, world)}
        rows[m.key] = gather_rows(local[m.key], len(m.cols), nr, rank, world, dist, device)
    if rank == 0:
        df, agg = write_results(p.file_id, records)
        print(agg.T)
        print('Output files:')
        print(f"  {p.file_id}-metadata.csv")
        print(f"  {p.file_id}-results-agg.csv")
        print(f"  {p.file_id}-results.csv")
        for m in asked:
            print(f"  {write_rows(p.file_id, m, rows[m.key])}")
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
