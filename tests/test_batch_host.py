"""CPU tests of the batch (include/chs_hip.h chs_batch_*, chsimpy_amd.batch, run_ensemble(batch=B)): bindings,
host-side validation and the grouping of an ensemble into batches."""
import os
import re

import numpy as np
import pytest
import torch.multiprocessing as mp

import chsimpy_amd
from chsimpy_amd import _lib, batch as bt, experiment as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_batch_prototype_has_a_binding():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    declared = set(re.findall(r'\b(chs_batch_\w+)\s*\(', hdr))
    assert {'chs_batch_create', 'chs_batch_destroy', 'chs_batch_set_U', 'chs_batch_init_U_pcg64', 'chs_batch_get_U',
            'chs_batch_prepare', 'chs_batch_step_n', 'chs_batch_get_state', 'chs_batch_set_state'} <= declared
    src = open(os.path.join(ROOT, 'chsimpy_amd', '_lib.py')).read()
    for name in declared:
        assert f"'{name}'" in src, f"{name} not in SYMBOLS"
        assert f"lib.{name}.argtypes" in src, f"{name} has no argtypes"
    assert declared <= set(_lib.SYMBOLS)


def _p(N=256, **kw):
    p = chsimpy_amd.Parameters()
    p.N, p.kappa_tilde = N, 3e-4
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize('members, what', [
    ([_p(256), _p(512)], 'differs'),
    ([_p(256), _p(256, dtype='float32')], 'differs'),
    ([_p(256), _p(256, device=1)], 'differs'),
    ([_p(256), _p(256, adaptive_time=True)], 'adaptive'),
    ([_p(256, jitter=0.01)], 'jitter'),
    ([_p(4096)], 'N=4096'),
    ([_p(100)], 'N=100'),
    ([_p(256, engine='direct')], 'fast engine'),
    ([], 'at least one'),
])
def test_rejected_configurations_raise_before_the_device(members, what, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device handle was created")
    monkeypatch.setattr(_lib, 'Batch', no_device)
    monkeypatch.setattr(_lib, 'load', no_device)
    with pytest.raises(ValueError, match=what):
        bt.BatchSolver(members)


def test_scope_of_the_default_experiment():
    assert bt.scope_error(_p(512)) is None
    assert bt.scope_error(_p(2048, dtype='float32')) is None
    assert 'N=8192' in bt.scope_error(_p(8192))


def _calls_recorder(log):
    def batch_fn(run_ids, p, rv, al):
        log.append(list(run_ids))
        return ex._dry_batch(run_ids, p, rv, al)
    return batch_fn


def _ens(runs=61):
    p = chsimpy_amd.Parameters()
    p.N, p.kappa_tilde, p.file_id = 512, 3e-4, 'ens'
    ep = ex.ExperimentParams()
    ep.runs = runs
    return p, ep


def test_batch_grouping_world1_equals_member_path(tmp_path):
    p, ep = _ens()
    ref = ex.run_ensemble(p, ep, run_fn=ex._dry_member)
    log = []
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, batch_fn=_calls_recorder(log))
    assert np.array_equal(np.array(got, dtype=np.float64), np.array(ref, dtype=np.float64), equal_nan=True)
    assert log == [list(range(k, min(k + 4, 61))) for k in range(0, 61, 4)]
    for name, recs in (('a', ref), ('b', got)):
        ex.write_results(str(tmp_path / name), recs)
    for suffix in ('-results.csv', '-results-agg.csv'):
        assert open(tmp_path / ('a' + suffix), 'rb').read() == open(tmp_path / ('b' + suffix), 'rb').read()


def _worker(rank, world, port, out, batch):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group(backend='gloo', rank=rank, world_size=world)
    p, ep = _ens()
    recs = ex.run_ensemble(p, ep, run_fn=ex._dry_member, dist=dist, rank=rank, world=world, batch=batch,
                           batch_fn=ex._dry_batch if batch else None)
    if rank == 0:
        ex.write_results(out, recs)
        np.save(out + '.npy', np.array(recs, dtype=np.float64))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_batch_grouping_gloo_world2_equals_member_path(tmp_path):
    outs = {}
    for batch in (0, 4):
        out = str(tmp_path / f'w2b{batch}')
        mp.spawn(_worker, args=(2, _free_port(), out, batch), nprocs=2, join=True)
        outs[batch] = out
    p, ep = _ens()
    single = np.array(ex.run_ensemble(p, ep, run_fn=ex._dry_member), dtype=np.float64)
    for batch, out in outs.items():
        assert np.array_equal(np.load(out + '.npy'), single, equal_nan=True), batch
    for suffix in ('-results.csv', '-results-agg.csv'):
        assert open(outs[0] + suffix, 'rb').read() == open(outs[4] + suffix, 'rb').read()


def test_out_of_scope_batch_falls_back_with_a_note(capsys):
    p, ep = _ens(runs=5)
    p.N = 4096
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4)
    assert 'not taken' in capsys.readouterr().out
    assert np.array_equal(np.array(got, dtype=np.float64),
                          np.array(ex.run_ensemble(p, ep, run_fn=ex._dry_member), dtype=np.float64), equal_nan=True)
