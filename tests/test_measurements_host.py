"""CPU tests of the measurement table of chsimpy_amd.experiment: one record per look, one gather, one writer."""
import os
import subprocess
import sys

import pytest

import chsimpy_amd
from chsimpy_amd import experiment as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [m.flag for m in ex.MEASUREMENTS]


def test_the_table_is_consistent():
    assert [m.key for m in ex.MEASUREMENTS] == ['domains', 'morphology', 'droplets', 'widths', 'chords']
    by_key = {m.key: m for m in ex.MEASUREMENTS}
    assert by_key['domains'].cols == ('id', 'k1', 'ell', 'ell_phys')
    assert by_key['morphology'].cols is ex.MORPHOLOGY_COLS and by_key['droplets'].cols is ex.DROPLETS_COLS
    assert by_key['widths'].cols is ex.WIDTHS_COLS and by_key['chords'].cols is ex.CHORDS_COLS
    # the integer columns, written out: what the five writers printed with int()
    assert by_key['domains'].int_cols == {'id'}
    assert by_key['morphology'].int_cols == {'id', 'n_A', 'perimeter', 'perimeter_inner', 'euler8', 'euler4'}
    assert by_key['droplets'].int_cols == {'id', 'connectivity'} | {
        f"{k}_{s}" for k in ('count', 'largest', 'spanning') for s in ('below', 'above')}
    assert by_key['widths'].int_cols == {'id'} | {f"{k}_{s}" for k in ('fg', 'q50', 'q90') for s in ('below', 'above')}
    assert by_key['chords'].int_cols == {'id'} | {
        f"{k}_{p}_{d}" for k in ('count', 'max', 'cut') for p in ('below', 'above') for d in ('rows', 'cols')}
    p = chsimpy_amd.Parameters()
    p.N = 16
    known = ex.arg_parser()._option_string_actions
    for m in ex.MEASUREMENTS:
        assert m.cols[0] == 'id' and len(set(m.cols)) == len(m.cols)
        assert m.int_cols <= set(m.cols)
        assert len(m.dry_row(2, p, {'droplets_connectivity': 8})) == len(m.cols) - 1
        assert m.flag in known and known[m.flag].dest == m.key
        assert (m.rows_of_batch is not None) == (m.key in ('domains', 'morphology'))
    assert len({m.key for m in ex.MEASUREMENTS}) == len({m.flag for m in ex.MEASUREMENTS}) == 5
    assert len({m.suffix for m in ex.MEASUREMENTS}) == 5


@pytest.mark.parametrize('batch', [[], ['--batch', '2']], ids=['one_by_one', 'batch2'])
def test_all_flags_together_write_what_each_flag_alone_writes(tmp_path, batch):
    """No cross-talk in the table: every file of a dry run with the five flags has the bytes of the run with its flag
    alone, and the result files are those of a run without any."""
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        base = ['-N', '16', '-R', '3', '--dry-run'] + batch
        ex.main(base + ['--file-id', 'bare'])
        ex.main(base + ['--file-id', 'all'] + FLAGS)
        for m in ex.MEASUREMENTS:
            ex.main(base + ['--file-id', m.key, m.flag])
    finally:
        os.chdir(cwd)
    for m in ex.MEASUREMENTS:
        assert (tmp_path / f'all-{m.suffix}.csv').read_bytes() == (tmp_path / f'{m.key}-{m.suffix}.csv').read_bytes()
        assert (tmp_path / f'all-{m.suffix}.csv').read_text().splitlines()[0] == ','.join(m.cols)
        assert len((tmp_path / f'all-{m.suffix}.csv').read_text().splitlines()) == 4
        for other in ex.MEASUREMENTS:
            assert (other is m) == (tmp_path / f'{m.key}-{other.suffix}.csv').exists()
        assert not (tmp_path / f'bare-{m.suffix}.csv').exists()
    for kind in ('results.csv', 'results-agg.csv'):
        assert (tmp_path / f'all-{kind}').read_bytes() == (tmp_path / f'bare-{kind}').read_bytes()


def test_gather_rows_under_gloo_with_a_rank_that_holds_no_rows(tmp_path):
    """`--gpus 2 --backend gloo --dry-run -R 1`: rank 1 has no member and sends a block of NaN rows alone; rank 0 writes
    the files a single rank writes.  (The rows of a dry run hold no NaN: that a row is told by its id alone is the test
    below.)"""
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    base = ['-N', '16', '-K', '3e-4', '-R', '1', '--dry-run', '--backend', 'gloo'] + FLAGS
    r2 = subprocess.run([sys.executable, '-m', 'chsimpy_amd.experiment', '--gpus', '2', '--file-id', str(tmp_path / 'g2')] + base,
                        env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-3000:]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        ex.main(base + ['--file-id', 'g1'])
    finally:
        os.chdir(cwd)
    for m in ex.MEASUREMENTS:
        text = (tmp_path / f'g2-{m.suffix}.csv').read_text()
        assert text == (tmp_path / f'g1-{m.suffix}.csv').read_text()
        assert len(text.splitlines()) == 2 and text.splitlines()[1].startswith('0,')
    assert 'ranks, 2' in (tmp_path / 'g2-metadata.csv').read_text()


def test_gather_rows_keeps_rows_with_nan_behind_the_id():
    """What the gather does to a block, without the ranks: a fake all_gather that hands back this rank's block and an
    all-NaN one.  Rows come back with an int id, in order, NaN kept where a side or phase has none."""
    import math

    class _Dist:
        @staticmethod
        def all_gather(out, buf):
            out[0].fill_(float('nan'))
            out[1].copy_(buf)
    nan = float('nan')
    local = {3: (0.5, 0, nan, nan, nan, -1, -1), 1: (0.5, 4, 1.0, 1.0, 1.0, 1, 1)}
    rows = ex.gather_rows(local, 8, 4, 1, 2, _Dist)
    assert [r[0] for r in rows] == [1, 3] and all(type(r[0]) is int and len(r) == 8 for r in rows)
    assert rows[0][1:] == local[1] and rows[1][1:3] == (0.5, 0.0) and all(math.isnan(x) for x in rows[1][3:6])
    assert ex.gather_rows(local, 8, 4, 0, 1) == [(1,) + local[1], (3,) + local[3]]
