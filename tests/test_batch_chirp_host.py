"""CPU tests of the chirp batch (include/chs_hip.h chs_batch_*, chsimpy_amd.batch, run_ensemble(batch=B)): which
configurations a batch takes now that it runs the engine a single handle of its members would run -- the fast engine at
its five sizes, the chirp engine at every other N it supports -- decided on the host before any device handle exists."""
import os
import re

import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, batch as bt, experiment as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(N=256, **kw):
    p = chsimpy_amd.Parameters()
    p.N, p.kappa_tilde = N, 3e-4
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture
def no_device(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("a device handle was created")
    monkeypatch.setattr(_lib, 'Batch', fail)
    monkeypatch.setattr(_lib, 'load', fail)


def test_auto_at_a_chirp_size_is_a_batch():
    """The test that fails without the feature: N=1000 under 'auto' runs the chirp engine, and a batch takes it."""
    assert bt.scope_error(_p(1000)) is None
    assert bt.batch_engine(_p(1000)) == 'chirp'


@pytest.mark.parametrize('params, engine', [
    (_p(1000), 'chirp'),
    (_p(100, engine='chirp'), 'chirp'),
    (_p(129), 'chirp'),
    (_p(8, engine='chirp'), 'chirp'),
    (_p(4095), 'chirp'),
    (_p(4096, engine='chirp'), 'chirp'),
    (_p(1000, dtype='float32'), 'chirp'),
    (_p(512), 'fast'),
    (_p(2048, engine='fast'), 'fast'),
])
def test_accepted_configurations(params, engine, no_device):
    assert bt.scope_error(params) is None
    assert bt.batch_engine(params) == engine
    bt.validate([params, params])
    bs = bt.BatchSolver([params, params])      # host side only: the device batch is created at prepare()
    assert len(bs) == 2


@pytest.mark.parametrize('params, what', [
    (_p(100), 'N=100'),                        # 'auto' below CHS_CHIRP_AUTO_MIN_N is the direct engine
    (_p(128 + 0, engine='chirp'), 'fast engine only'),
    (_p(4096), 'N=4096'),                      # 'auto' at a power of two is the fast engine, which has no batch there
    (_p(8192), 'N=8192'),
    (_p(4097, engine='chirp'), 'N=4097'),
    (_p(7, engine='chirp'), 'N=7'),
    (_p(1000, engine='fast'), 'N=1000'),
    (_p(256, engine='direct'), 'fast engine'),
    (_p(1000, engine='direct'), 'fast engine'),
    (_p(256, engine='chirp'), 'fast engine only'),
    (_p(1000, jitter=0.01), 'jitter'),
    (_p(1000, adaptive_time=True), 'adaptive'),
    (_p(100, engine='chirp', adaptive_time=True), 'adaptive'),
])
def test_refused_configurations(params, what, no_device):
    assert what in bt.scope_error(params)
    with pytest.raises(ValueError, match=what):
        bt.BatchSolver([params])


def test_mixed_members_are_refused(no_device):
    with pytest.raises(ValueError, match='adaptive'):
        bt.BatchSolver([_p(256), _p(256, adaptive_time=True)])          # a fast batch: all members or none
    with pytest.raises(ValueError, match='adaptive') as e:
        bt.BatchSolver([_p(1000), _p(1000, adaptive_time=True)])        # a chirp batch: none
    assert 'member 1' in str(e.value)
    # members that spell the same engine differently are one batch: both resolve to chirp (chs_batch_create agrees)
    assert len(bt.BatchSolver([_p(1000), _p(1000, engine='chirp')])) == 2
    with pytest.raises(ValueError, match='differs'):
        bt.BatchSolver([_p(1000), _p(1001)])
    with pytest.raises(ValueError, match='differs'):
        bt.BatchSolver([_p(1000), _p(1000, dtype='float32')])


def test_a_chirp_batch_has_no_seat_queue(no_device):
    with pytest.raises(ValueError, match='queue'):
        bt.BatchSolver([_p(1000), _p(1000)], seats=2)
    with pytest.raises(ValueError, match='queue'):
        bt.BatchSolver([_p(100, engine='chirp')] * 3, seats=1)
    assert len(bt.BatchSolver([_p(512), _p(512)], seats=2)) == 2       # the fast batch keeps its queue


def _ens(N, runs=5):
    p = chsimpy_amd.Parameters()
    p.N, p.kappa_tilde, p.file_id = N, 3e-4, 'ens'
    ep = ex.ExperimentParams()
    ep.runs = runs
    return p, ep


def _dry_device_path(monkeypatch, log):
    """run_ensemble's default batch function goes to the device: a stand-in that notes the call."""
    def fake(run_ids, p, rv, al, U_init=None, postprocess=True, seats=None):
        log.append((list(run_ids), seats))
        return ex._dry_batch(run_ids, p, rv, al)
    monkeypatch.setattr(ex, 'run_batch_gpu', fake)


def test_run_ensemble_takes_a_chirp_size_as_batches(monkeypatch, capsys):
    p, ep = _ens(1000)
    log = []
    _dry_device_path(monkeypatch, log)
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4)
    assert 'not taken' not in capsys.readouterr().out
    assert log == [([0, 1, 2, 3], None), ([4], None)]
    want = ex.run_ensemble(p, ep, run_fn=ex._dry_member)
    assert np.array_equal(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64), equal_nan=True)


def test_run_ensemble_at_n100_auto_still_falls_back(monkeypatch, capsys):
    p, ep = _ens(100)
    log = []
    _dry_device_path(monkeypatch, log)
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4)
    out = capsys.readouterr().out
    assert 'not taken' in out and 'N=100' in out
    assert log == []
    want = ex.run_ensemble(p, ep, run_fn=ex._dry_member)
    assert np.array_equal(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64), equal_nan=True)


def test_run_ensemble_queue_at_a_chirp_size_falls_back(monkeypatch, capsys):
    p, ep = _ens(1000)
    log = []
    _dry_device_path(monkeypatch, log)
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, queue=True)
    out = capsys.readouterr().out
    assert 'not taken' in out and 'queue' in out
    assert log == []
    want = ex.run_ensemble(p, ep, run_fn=ex._dry_member)
    assert np.array_equal(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64), equal_nan=True)


def test_header_and_binding_agree_on_the_scope():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    defs = dict(re.findall(r'#define\s+(CHS_\w+)\s+(-?\d+)\b', hdr))
    assert int(defs['CHS_BATCH_CHIRP_MIN_N']) == _lib.BATCH_CHIRP_MIN_N
    assert int(defs['CHS_BATCH_CHIRP_MAX_N']) == _lib.BATCH_CHIRP_MAX_N
    assert int(defs['CHS_CHIRP_AUTO_MIN_N']) == _lib.CHS_CHIRP_AUTO_MIN_N
    # the chirp engine's own range (its header is not part of the C ABI)
    host = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_chirp_host.h')).read()
    own = dict(re.findall(r'#define\s+(CHS_CHIRP_M\w+_N)\s+(\d+)', host))
    assert (int(own['CHS_CHIRP_MIN_N']), int(own['CHS_CHIRP_MAX_N'])) == (_lib.BATCH_CHIRP_MIN_N, _lib.BATCH_CHIRP_MAX_N)
    # the batch comment block names both engines' sets and what stays outside
    at = hdr.index('---- Batches')
    block = hdr[at:hdr.index('typedef struct chs_batch_s', at)]
    for n in _lib.BATCH_SIZES:
        assert str(n) in block
    for word in ('CHS_BATCH_CHIRP_MIN_N', 'CHS_BATCH_CHIRP_MAX_N', 'CHS_CHIRP_AUTO_MIN_N', 'CHS_ENGINE_CHIRP',
                 'CHS_ENGINE_DIRECT', 'adaptive_time', 'seat queue'):
        assert word in block, word
    # every size of the fast batch is one of the fast engine's, and 'auto' never gives those to the chirp engine
    assert set(_lib.BATCH_SIZES) <= set(_lib.FAST_SIZES)
    assert all(bt.batch_engine(_p(n)) == 'fast' for n in _lib.BATCH_SIZES)
