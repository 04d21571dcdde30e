"""``BatchSolver``: several ``Solver`` runs of one grid size advanced together on one device.

An ensemble over (A0, A1) at the reference's default grid (N=512) leaves an MI355X mostly idle with one run at a
time: a step is two short dependent chains of kernels.  A batch launches every step kernel once for all of its
members (``chs_batch_*`` of ``include/chs_hip.h``), so that the members' chains overlap on the device.

Member by member a ``BatchSolver`` is a ``Solver`` with ``rederive_hat=True``: same constants, start field, records,
stop rules and quirks (the first ``solve_or_resume`` after ``prepare`` runs ``nsteps-1`` iterations; ``prepare`` does
not reset ``delt`` / ``time_delta_sum`` / ``skip_check``), every call a literal ``solve_or_resume`` of the reference.
A batch runs the engine a single ``Solver`` of its members would run.  Its scope: one N, dtype and device for all
members, no jitter, and

- the fast engine at N in {128, 256, 512, 1024, 2048} (``engine`` 'auto' or 'fast'): ``adaptive_time`` set in all
  members or in none (an adaptive batch: every member adapts its step by its own rule, step counter and ``delt_max``);
- the chirp engine at every other N in [8, 4096], where ``engine='chirp'`` asks for it or 'auto' resolves to it
  (N >= 129 and not a power of two): one launch set of the chirp step's 13 kernels for all members, bit for bit the
  members' single chirp ``Solver``s.  Fixed time step only, and no seat queue.

Anything else -- the direct engine, 'auto' below N=129, ``engine='chirp'`` at one of the fast engine's five sizes, an
adaptive chirp batch, ``seats`` with chirp members -- raises ``ValueError`` before the device is touched.

    bs = BatchSolver([params_0, params_1, ...])
    bs.prepare()
    solutions = bs.solve_or_resume()      # one Solution per member
    bs.close()

``BatchSolver(params_list, seats=S)`` runs the members as a seat queue: S seats are launched every step, and when a
member stops or has done its call the next one in member order takes its seat on the device
(``chs_batch_step_n_queued``).  A default ensemble's members stop at their own steps, so a plain batch thins out
towards the end of every call; a queue of all the runs keeps S of them going.  The results are bit for bit the plain
batch's.
"""
import functools

import numpy as np

from . import _lib, contour, two_point
from .solver import Solver


def _auto_is_chirp(N):
    """Does engine='auto' resolve to the chirp engine at this N (chs_api.hip: resolve_auto)?"""
    fast = N in _lib.FAST_SIZES
    return not fast and _lib.CHS_CHIRP_AUTO_MIN_N <= N <= _lib.BATCH_CHIRP_MAX_N


def batch_engine(params):
    """The engine a batch of such members runs, 'fast' or 'chirp' (the rule of chs_batch_create), or None."""
    N, engine = int(params.N), str(getattr(params, 'engine', 'auto'))
    if N in _lib.BATCH_SIZES:
        return 'fast' if engine in ('auto', 'fast') else None
    if _lib.BATCH_CHIRP_MIN_N <= N <= _lib.BATCH_CHIRP_MAX_N and (engine == 'chirp' or (engine == 'auto' and _auto_is_chirp(N))):
        return 'chirp'
    return None


def scope_error(params, seats=None):
    """Why one member's parameters are outside what a batch runs (a string), or None.  ``seats``: the seats of a
    queue (None: a plain batch)."""
    N = int(params.N)
    engine = str(getattr(params, 'engine', 'auto'))
    if engine == 'direct':
        return f"engine={engine!r}: a batch runs the fast engine or the chirp engine"
    which = batch_engine(params)
    if which is None:
        if N in _lib.BATCH_SIZES:
            return f"engine={engine!r} at N={N}: a batch of the fast engine only"
        return (f"N={N}: a batch takes N in {{{', '.join(str(n) for n in _lib.BATCH_SIZES)}}} (fast engine), or the chirp "
                f"engine's N in [{_lib.BATCH_CHIRP_MIN_N}, {_lib.BATCH_CHIRP_MAX_N}] (engine='chirp', or 'auto' from "
                f"N={_lib.CHS_CHIRP_AUTO_MIN_N} where it is no power of two)")
    if which == 'chirp' and params.adaptive_time:
        return "adaptive_time: a chirp batch has no adaptive time step"
    if which == 'chirp' and seats is not None:
        return "seats: a chirp batch has no seat queue"
    if str(getattr(params, 'dtype', 'float64')) not in _lib.DTYPES:
        return f"dtype={params.dtype!r} is not supported"
    if params.jitter is not None and 0.0 < params.jitter < 0.1:
        return "jitter: a batch has no per-step noise"
    return None


def _key(params):
    return (int(params.N), _lib.DTYPES[str(getattr(params, 'dtype', 'float64'))], int(getattr(params, 'device', 0) or 0))


def validate(params_list, seats=None):
    """Raise ValueError unless the members can share one batch (host-side checks only).  ``seats``: the seats of a
    queue (None: a plain batch)."""
    if len(params_list) < 1:
        raise ValueError("a batch needs at least one member")
    if seats is not None and (isinstance(seats, bool) or int(seats) != seats or int(seats) < 1):
        raise ValueError(f"seats={seats!r}: a queue needs seats >= 1")
    for i, p in enumerate(params_list):
        why = scope_error(p, seats)
        if why:
            raise ValueError(f"member {i}: {why}")
    a0 = bool(params_list[0].adaptive_time)
    for i, p in enumerate(params_list):
        if bool(p.adaptive_time) != a0:
            raise ValueError(f"member {i}: adaptive_time={bool(p.adaptive_time)} differs from member 0's "
                             f"(a batch adapts the step of all its members or of none)")
    k0 = _key(params_list[0])
    for i, p in enumerate(params_list):
        if _key(p) != k0:
            raise ValueError(f"member {i}: (N, dtype, device) = {_key(p)} differs from member 0's {k0}")


class _Member:
    """What a member's ``Solver`` calls on its engine, answered by the batch."""

    def __init__(self, batch, m):
        self._b, self._m = batch, m

    def get_state(self):
        return self._b.get_state(self._m)

    def set_state(self, s):
        self._b.set_state(self._m, s)

    def get_U(self):
        return self._b.get_U(self._m)

    def set_U(self, U):
        self._b.set_U(self._m, U)

    def morphology(self, threshold):
        return self._b.morphology(threshold, self._m)

    _LOOKS = ('components', 'components_look', 'distance', 'distance_look', 'chords', 'chords_look', 'composition',
              'composition_look', 'composition_select', 'two_point', 'two_point_look', 'contour', 'contour_look', 'shapes',
              'shapes_look', 'track', 'track_look', 'track_reset', 'thickness', 'thickness_look',
              'geodesic', 'geodesic_look', 'skeleton', 'skeleton_look',
              'transport', 'transport_look')

    def __getattr__(self, name):
        """A look of the member by the signature of `Engine`: the batch's, with the member in front."""
        if name in self._LOOKS:
            return functools.partial(getattr(self._b, name), self._m)
        raise AttributeError(name)

    def close(self):
        pass  # (the batch owns the device state)


class BatchSolver:
    def __init__(self, params_list, U_init=None, seats=None):
        params_list = list(params_list)
        validate(params_list, seats)
        self.seats = None if seats is None else int(seats)
        B = len(params_list)
        if U_init is None or (isinstance(U_init, np.ndarray) and U_init.ndim == 2):
            inits = [U_init] * B
        else:
            inits = list(U_init)
            if len(inits) != B:
                raise ValueError(f"U_init: {len(inits)} fields for {B} members")
        self.solvers = [Solver(p, u) for p, u in zip(params_list, inits)]
        lam0 = self.solvers[0].solution.lam
        for i, s in enumerate(self.solvers):
            if not np.array_equal(s.solution.lam, lam0):
                raise ValueError(f"member {i}: eigenvalue table differs from member 0's")
        self._batch = None
        self._prepared = False
        self.member_errors = {}

    @property
    def solutions(self):
        return [s.solution for s in self.solvers]

    def __len__(self):
        return len(self.solvers)

    def _get_batch(self):
        if self._batch is None:
            self._batch = _lib.Batch([s._consts() for s in self.solvers], self.solvers[0].solution.lam)
            for m, s in enumerate(self.solvers):
                s._engine = _Member(self._batch, m)
        return self._batch

    # -- solver.py:84-135, member by member -------------------------------------------------------------------
    def prepare(self):
        b = self._get_batch()
        on_device = []
        for m, s in enumerate(self.solvers):
            s._push_state()
            dev = s._U_init is None and s._pcg_state0 is not None and s.device_rng
            on_device.append(dev)
            if dev:
                st = s._pcg_state0['state']
                p = s.params
                b.init_U_pcg64(m, p.XXX, p.XXX * 0.01, st['state'], st['inc'])
            else:
                U = s.U_init.copy()
                assert U.shape == (s.params.N, s.params.N)
                b.set_U(m, U)
        rows0 = b.prepare()
        from .timedata import TimeData
        for m, s in enumerate(self.solvers):
            row = rows0[m]
            data = TimeData()
            data.insert(it=0, delt=row[8], E=row[1], E2=row[2], SA=0, domtime=0, Ra=row[5], L2=0, PS=row[7])
            sol = s.solution
            sol._bind_device_U(None if on_device[m] else s.U_init.copy(), s._engine.get_U if on_device[m] else None)
            sol.timedata = data
            sol.tau0 = 0.0
            sol.t0 = 0.0
            sol.stop_reason = 'None'
            sol.computed_steps = 1
            s._prepared = True
        self._prepared = True

    # -- solver.py:137-252, member by member; one device call for all ----------------------------------------
    def solve_or_resume(self, nsteps=None):
        """One literal solve_or_resume call of every member (``nsteps``: one count for all, a list of one per
        member, or None = each member's ntmax).  Returns the members' Solutions.  A member whose record turns NaN
        raises AssertionError as ``Solver`` does -- after every member's result has been taken in
        (``member_errors`` maps the member to its error)."""
        assert self._prepared is True
        b = self._batch
        B = len(self.solvers)
        if nsteps is None or np.isscalar(nsteps):
            per = [nsteps] * B
        else:
            per = list(nsteps)
            if len(per) != B:
                raise ValueError(f"nsteps: {len(per)} counts for {B} members")
        counts = []
        for m, s in enumerate(self.solvers):
            n = per[m]
            if n is None:
                n = max(s.params.ntmax, 0)
            sol = s.solution
            if sol.__dict__.get('_U_dirty') or sol._host_edited():
                b.set_U(m, sol.__dict__['_U'])   # solver.py:158: the field the caller assigned
                sol.__dict__['_U_dirty'] = False
                sol.__dict__['_U_print'] = None
            itbegin = 1 if sol.computed_steps == 1 else 0
            counts.append(max(int(n) - itbegin, 0))
        rows, status = b.step_n(counts) if self.seats is None else b.step_n_queued(counts, self.seats)
        self.member_errors = {}
        for m, s in enumerate(self.solvers):
            try:
                s._absorb(rows[m], status[m], counts[m])
            except AssertionError as e:
                self.member_errors[m] = e
                continue
            s.solution._bind_device_U(None, s._engine.get_U)   # downloaded when somebody looks at solution.U
        if self.member_errors:
            m, e = next(iter(self.member_errors.items()))
            raise AssertionError(f"member {m}: {e}")
        return self.solutions

    def structure_factor(self, member=None):
        """The members' radially averaged structure factors (`Solver.structure_factor`): a list of one
        `spectrum.StructureFactor` per member from one device pass over the batch, or the one of ``member``.  Bit for
        bit what the members' single Solvers return; the members' runs do not notice the look."""
        from . import spectrum
        b = self._get_batch()   # (EngineError without a device, like every compute call; no field yet: AssertionError)
        for s in self.solvers:
            s._push_edited_U()
        if member is not None:
            s = self.solvers[member]
            return spectrum.StructureFactor(b.structure_factor(member), s.params.N, s.solution.delx)
        ssum = b.structure_factor()
        return [spectrum.StructureFactor(ssum[m], s.params.N, s.solution.delx) for m, s in enumerate(self.solvers)]

    def morphology(self, member=None, threshold=None):
        """The members' morphology (`Solver.morphology`): a list of one `morphology.Morphology` per member from one
        device pass over the batch, or the one of ``member``.  ``threshold``: one value for all, one per member, or None
        for every member's own ``params.threshold``.  The members' runs do not notice the look."""
        from . import morphology
        b = self._get_batch()
        for s in self.solvers:
            s._push_edited_U()
        ts = [float(s.params.threshold) if t is None else t for s, t in zip(self.solvers, self._member_thresholds(threshold))]
        if member is not None:
            s = self.solvers[member]
            return morphology.Morphology(b.morphology(ts[member], member), s.params.N, ts[member], s.solution.delx)
        words = b.morphology(ts)
        return [morphology.Morphology(words[m], s.params.N, ts[m], s.solution.delx) for m, s in enumerate(self.solvers)]

    def _member_thresholds(self, threshold):
        """One threshold per member of a look that goes member by member: None (the member's own ``params.threshold``)
        for None, the one value for all, or the given list."""
        if threshold is None:
            return [None] * len(self.solvers)
        if np.ndim(threshold) == 0:
            return [float(threshold)] * len(self.solvers)
        ts = [float(t) for t in threshold]
        if len(ts) != len(self.solvers):
            raise ValueError(f"{len(self.solvers)} thresholds are needed, got {len(ts)}")
        return ts

    def _member_by_member(self, look, member, threshold, *args):
        """`Solver.<look>(threshold, *args)` of every member, one after the other on the batch's stream with the batch's
        one set of buffers, as a list -- or that of ``member`` alone.  ``threshold``: one value for all, one per member,
        or None for every member's own ``params.threshold``.  The members' runs do not notice the looks."""
        self._get_batch()
        ts = self._member_thresholds(threshold)
        if member is not None:
            return getattr(self.solvers[member], look)(ts[member], *args)
        return [getattr(s, look)(t, *args) for s, t in zip(self.solvers, ts)]

    def components(self, member=None, threshold=None, connectivity=4, side='below', table=True, labels=False):
        """The members' connected components (`Solver.components`), a `components.Components` each: _member_by_member."""
        return self._member_by_member('components', member, threshold, connectivity, side, table, labels)

    def distance(self, member=None, threshold=None, side='below', hist=True, map=False):
        """The members' distance transforms (`Solver.distance`), a `distance.Distance` each: _member_by_member."""
        return self._member_by_member('distance', member, threshold, side, hist, map)

    def thickness(self, member=None, threshold=None, side='below', hist=True, map=False, max_work=None):
        """The members' local thickness (`Solver.thickness`), a `thickness.Thickness` each: _member_by_member."""
        return self._member_by_member('thickness', member, threshold, side, hist, map, max_work)

    def geodesic(self, member=None, threshold=None, connectivity=8, side='below', source='top', hist=True, profile=True, map=False,
                 max_rounds=None):
        """The members' geodesic looks (`Solver.geodesic`), a `geodesic.Geodesic` each: _member_by_member."""
        return self._member_by_member('geodesic', member, threshold, connectivity, side, source, hist, profile, map, max_rounds)

    def skeleton(self, member=None, threshold=None, side='below', hist=True, map=False, max_subiters=None):
        """The members' skeleton looks (`Solver.skeleton`), a `skeleton.Skeleton` each: _member_by_member."""
        return self._member_by_member('skeleton', member, threshold, side, hist, map, max_subiters)

    def transport(self, member=None, threshold=None, side='below', source='top', tol=1e-6, profile=True, map=False, max_iters=None):
        """The members' transport looks (`Solver.transport`), a `transport.Transport` each: _member_by_member."""
        return self._member_by_member('transport', member, threshold, side, source, tol, profile, map, max_iters)

    def chords(self, member=None, threshold=None, hist=True):
        """The members' chord lengths (`Solver.chords`), a `chords.Chords` each: _member_by_member."""
        return self._member_by_member('chords', member, threshold, hist)

    def composition(self, member=None, threshold=None, bins=15, range=None, quantiles=(0.05, 0.5, 0.95), hist=True):
        """The members' compositions (`Solver.composition`), a `composition.Composition` each: _member_by_member."""
        return self._member_by_member('composition', member, threshold, bins, range, quantiles, hist)

    def two_point(self, member=None, threshold=None, rmax=two_point.DEFAULT_RMAX, counts=True):
        """The members' two-point correlations (`Solver.two_point`), a `two_point.TwoPoint` each: _member_by_member."""
        return self._member_by_member('two_point', member, threshold, rmax, counts)

    def contour(self, member=None, threshold=None, bins=contour.DEFAULT_BINS, kmax=contour.DEFAULT_KMAX, hist=True, map=False):
        """The members' sub-pixel interfaces (`Solver.contour`), a `contour.Contour` each: _member_by_member."""
        return self._member_by_member('contour', member, threshold, bins, kmax, hist, map)

    def shapes(self, member=None, threshold=None, connectivity=4, side='below', labels=False):
        """The members' droplet shapes (`Solver.shapes`), a `shapes.Shapes` each: _member_by_member."""
        return self._member_by_member('shapes', member, threshold, connectivity, side, labels)

    def track(self, member=None, threshold=None, connectivity=4, side='below', keep=True, reset=False):
        """The members' droplet tracking (`Solver.track`), a `tracking.Track` each: _member_by_member.  Every member keeps
        its own frame on the device."""
        return self._member_by_member('track', member, threshold, connectivity, side, keep, reset)

    def close(self, fetch_U=True):
        """Free the device batch; the members' fields are downloaded first unless the caller needs scalars only."""
        if self._batch is not None:
            for s in self.solvers:
                sol = s.solution
                if fetch_U:
                    _ = sol.U
                else:
                    sol._bind_device_U(sol.__dict__.get('_U'), track=False)
                s._engine = None
            self._batch.close()
            self._batch = None

    def __del__(self):
        try:
            self.close(fetch_U=False)
        except Exception:
            pass
