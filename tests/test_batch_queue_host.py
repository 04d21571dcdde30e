"""CPU tests of the seat queue (include/chs_hip.h chs_batch_step_n_queued / chs_batch_member_rows,
``BatchSolver(seats=S)``, ``run_ensemble(batch=B, queue=True)``): bindings, host-side validation and how an ensemble's
runs are dealt to queues, and the queue's host decisions (chsimpy_amd/csrc/chs_batch_host.h) against a model of the seat kernel.
Nothing here touches a device."""
import os
import re
import subprocess

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


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device handle was created")
    monkeypatch.setattr(_lib, 'Batch', no_device)
    monkeypatch.setattr(_lib, 'load', no_device)


def test_the_queued_prototypes_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'chs_hip.h')).read()
    declared = set(re.findall(r'\b(chs_batch_\w+)\s*\(', hdr))
    assert {'chs_batch_step_n_queued', 'chs_batch_member_rows'} <= declared
    assert {'chs_batch_step_n_queued', 'chs_batch_member_rows'} <= set(_lib.SYMBOLS)
    assert callable(getattr(_lib.Batch, 'step_n_queued'))


def test_host_decisions_against_a_model_of_the_seat_kernel(tmp_path):
    """tests/batch_queue_model.cpp: the step bound and the last-step bookkeeping of chs_batch_step_n_queued, driven
    step by step with polls two batches late -- every member gets its last-step pair on its last step, nobody is left
    with steps to do, the bound is the finishing step.  Host C++ only, compiled with the build's compiler."""
    from chsimpy_amd import _build
    exe = str(tmp_path / 'batch_queue_model')
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-I' + _build.CSRC,
                    os.path.join(ROOT, 'tests', 'batch_queue_model.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and ' 0 failures' in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    # the header is host code: nothing of HIP in it
    hdr = open(os.path.join(_build.CSRC, 'chs_batch_host.h')).read()
    assert not re.search(r'#include\s*[<"](hip/|chs_common|chs_fast)', hdr)


@pytest.mark.parametrize('seats', [0, -1, 1.5, True])
def test_bad_seats_raise_before_the_device(seats, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match='seats'):
        bt.BatchSolver([_p(), _p()], seats=seats)
    with pytest.raises(ValueError, match='seats'):
        bt.validate([_p(), _p()], seats)


@pytest.mark.parametrize('seats', [None, 1, 2, 16])
def test_good_seats_are_kept_and_no_device_is_touched_at_construction(seats, monkeypatch):
    _no_device(monkeypatch)
    bs = bt.BatchSolver([_p(), _p()], seats=seats)     # (more seats than members is legal)
    assert bs.seats == seats and len(bs) == 2
    bt.validate([_p(), _p()])                          # the plain batch's signature still stands


def test_a_queue_takes_what_a_batch_takes(monkeypatch):
    _no_device(monkeypatch)
    for members, what in (([_p(256), _p(512)], 'differs'), ([_p(256), _p(256, adaptive_time=True)], 'adaptive'),
                          ([_p(256, jitter=0.01)], 'jitter'), ([_p(4096)], 'N=4096'), ([], 'at least one')):
        with pytest.raises(ValueError, match=what):
            bt.BatchSolver(members, seats=2)


def test_solve_or_resume_goes_through_the_queued_call_only_with_seats():
    class FakeBatch:
        def __init__(self):
            self.calls = []

        def step_n(self, counts):
            self.calls.append(('step_n', list(counts)))
            return [np.zeros((0, 9))] * len(counts), [0] * len(counts)

        def step_n_queued(self, counts, seats):
            self.calls.append(('step_n_queued', list(counts), seats))
            return [np.zeros((0, 9))] * len(counts), [0] * len(counts)

    for seats, want in ((None, ('step_n', [0, 0])), (3, ('step_n_queued', [0, 0], 3))):
        bs = bt.BatchSolver([_p(), _p()], seats=seats)
        fake = FakeBatch()
        bs._batch, bs._prepared = fake, True
        for m, s in enumerate(bs.solvers):
            s._engine = bt._Member(fake, m)
            s._absorb = lambda rows, status, n: None
            s.solution._bind_device_U = lambda *a, **k: None
            s.solution.computed_steps = 5
        bs.solve_or_resume(0)
        assert fake.calls == [want]
        bs._batch = None
        for s in bs.solvers:
            s._engine = None


def _recorder(log):
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


@pytest.mark.parametrize('queue_members, want', [
    (None, [list(range(61))]),                                                  # default 256: one queue of all runs
    (25, [list(range(0, 25)), list(range(25, 50)), list(range(50, 61))]),
    (61, [list(range(61))]),
    (1, [[i] for i in range(61)]),
])
def test_queue_deals_every_id_once_and_respects_queue_members(queue_members, want, tmp_path):
    p, ep = _ens()
    ref = ex.run_ensemble(p, ep, run_fn=ex._dry_member)
    log = []
    kw = {} if queue_members is None else dict(queue_members=queue_members)
    got = ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, queue=True, batch_fn=_recorder(log), **kw)
    assert log == want
    assert sorted(i for g in log for i in g) == list(range(61))
    assert np.array_equal(np.array(got, dtype=np.float64), np.array(ref, dtype=np.float64), equal_nan=True)
    for name, recs in (('a', ref), ('b', got)):
        ex.write_results(str(tmp_path / name), recs)
    assert open(tmp_path / 'a-results.csv', 'rb').read() == open(tmp_path / 'b-results.csv', 'rb').read()


def test_queue_of_a_rank_holds_that_ranks_ids_only():
    p, ep = _ens()
    log = []
    ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, queue=True, queue_members=8, batch_fn=_recorder(log),
                    rank=1, world=3)
    mine = ex.my_run_ids(61, 1, 3)
    assert len(mine) == 20 and log == [mine[:8], mine[8:16], mine[16:]]


def test_without_queue_the_calls_are_todays(monkeypatch):
    p, ep = _ens()
    log = []
    ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, batch_fn=_recorder(log))
    assert log == [list(range(k, min(k + 4, 61))) for k in range(0, 61, 4)]
    log2 = []
    ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, queue=False, queue_members=7, batch_fn=_recorder(log2))
    assert log2 == log
    # the device path is called as before: no `seats` argument without a queue, seats = batch with one
    seen = []
    monkeypatch.setattr(ex, 'run_batch_gpu', lambda ids, q, rv, al, U=None, **kw: seen.append((list(ids), kw))
                        or ex._dry_batch(ids, q, rv, al))
    ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4)
    assert seen == [(g, {}) for g in log]
    del seen[:]
    ex.run_ensemble(p, ep, run_fn=ex._dry_member, batch=4, queue=True)
    assert seen == [(list(range(61)), {'seats': 4})]


def test_experiment_cli_has_the_queue_switches(tmp_path, capsys):
    base = ['-N', '512', '-R', '9', '--batch', '4', '--dry-run', '-K', '3e-4']
    ex.main(base + ['--file-id', str(tmp_path / 'plain')])
    ex.main(base + ['--queue', '--queue-members', '5', '--file-id', str(tmp_path / 'queued')])
    assert 'not taken' not in capsys.readouterr().out
    assert open(tmp_path / 'plain-results.csv', 'rb').read() == open(tmp_path / 'queued-results.csv', 'rb').read()
    meta = open(tmp_path / 'queued-metadata.csv').read()
    assert 'queue_members, 5' in meta and 'queue_members' not in open(tmp_path / 'plain-metadata.csv').read()
