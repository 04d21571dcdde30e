"""CPU tests of the adaptive batch's host side: a batch takes ``adaptive_time`` when every member has it, a mixed
list is rejected before the device is touched, and an adaptive ensemble with ``--batch B`` goes through the batch."""
import numpy as np
import pytest

import chsimpy_amd
from chsimpy_amd import _lib, batch as bt, experiment as ex


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


def test_all_adaptive_members_validate(no_device):
    bt.validate([_p(256, adaptive_time=True, delt_max=4.9e-7 / 256) for _ in range(3)])
    bs = bt.BatchSolver([_p(512, adaptive_time=True), _p(512, adaptive_time=True, delt_max=2e-7)])
    assert len(bs) == 2 and all(s.params.adaptive_time for s in bs.solvers)


@pytest.mark.parametrize('flags, first', [
    ((True, False), 1),
    ((False, False, True, True), 2),
    ((True, True, True, False), 3),
])
def test_mixed_members_are_rejected_naming_the_first_that_differs(flags, first, no_device):
    members = [_p(256, adaptive_time=f) for f in flags]
    with pytest.raises(ValueError, match='adaptive') as e:
        bt.validate(members)
    assert f"member {first}:" in str(e.value)
    with pytest.raises(ValueError, match='adaptive'):
        bt.BatchSolver(members)


def test_adaptive_time_is_in_scope(no_device):
    assert bt.scope_error(_p(512, adaptive_time=True)) is None
    # what is still outside: jitter, the direct engine, other sizes -- adaptive or not
    assert 'jitter' in bt.scope_error(_p(512, adaptive_time=True, jitter=0.01))
    assert 'fast engine' in bt.scope_error(_p(512, adaptive_time=True, engine='direct'))
    assert 'N=4096' in bt.scope_error(_p(4096, adaptive_time=True))


def test_adaptive_ensemble_takes_the_batch(capsys, monkeypatch):
    p = _p(512, adaptive_time=True, delt_max=4.9e-7 / 512)
    p.file_id = 'ens'
    ep = ex.ExperimentParams()
    ep.runs = 10
    log = []

    def recorder(run_ids, q, rv, al):
        assert q.adaptive_time
        log.append(list(run_ids))
        return ex._dry_batch(run_ids, q, rv, al)
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, batch_fn=recorder)
    assert 'not taken' not in capsys.readouterr().out
    assert log == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    ref = ex.run_ensemble(p, ep, run_fn=ex._dry_member)
    assert np.array_equal(np.array(got, dtype=np.float64), np.array(ref, dtype=np.float64), equal_nan=True)
    # ... and without an injected batch function the scope check lets it through to the device path
    taken = []
    monkeypatch.setattr(ex, 'run_batch_gpu', lambda ids, q, rv, al, U=None: taken.append(list(ids)) or ex._dry_batch(ids, q, rv, al))
    ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4)
    assert 'not taken' not in capsys.readouterr().out
    assert taken == log


def test_experiment_cli_has_the_adaptive_switch(tmp_path, capsys):
    fid = str(tmp_path / 'cli')
    ex.main(['-N', '512', '-R', '5', '-a', '--delt-max', '9.5e-10', '--batch', '4', '--dry-run', '--file-id', fid,
             '-K', '3e-4'])
    out = capsys.readouterr().out
    assert 'not taken' not in out
    assert (tmp_path / 'cli-results.csv').exists()
