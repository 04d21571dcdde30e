"""`bench.py --gpus 1` on the device: a plain run carries the headline only, `--full` adds the figures measured beside
it, and `--dump-outputs` writes what the timed call computed -- the same arrays whether or not `--full` follows it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--grid', '128', '--steps', '20',
                        '--warmup', '5'] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_timed_call(gpu, tmp_path):
    plain = _bench(['--dump-outputs', str(tmp_path / 'plain')])
    assert plain['steps'] == 20 and plain['ms_per_step'] > 0 and plain['value'] > 0 and plain['dtype'] == 'f64'
    assert 'roofline' not in plain and 'cpu_baseline' not in plain and 'other_protocol_ms_per_step' not in plain['config']
    td = np.load(tmp_path / 'plain' / 'timedata.npy')
    U = np.load(tmp_path / 'plain' / 'U.npy')
    assert td.dtype == np.float64 and td.shape == (20, 9) and U.dtype == np.float64 and U.shape == (128 * 128,)
    assert np.all(np.diff(td[:, 0]) == 1) and np.isfinite(td).all() and np.isfinite(U).all()
    assert [td[-1, 1], td[-1, 2]] == plain['energies_last_step'][0]

    full = _bench(['--full', '--dump-outputs', str(tmp_path / 'full')])
    assert full['roofline']['kernel_ms'] and full['cpu_baseline']['value'] > 0
    assert full['config']['other_protocol_ms_per_step'] > 0
    # the same arguments start from the same field: the timed call computes the same arrays
    assert np.allclose(np.load(tmp_path / 'full' / 'timedata.npy'), td, rtol=1e-12, atol=0)
    assert np.allclose(np.load(tmp_path / 'full' / 'U.npy'), U, rtol=1e-12, atol=0)
