"""``Solver``: the Cahn-Hilliard integrator of ``chsimpy/solver.py`` with the
timestep loop running on an MI355X through the C ABI of ``include/chs_hip.h``.

Same constructor, methods and result object as the reference class
(``Solver(params, U_init)``, ``prepare()``, ``solve_or_resume(nsteps)`` ->
``Solution``), same quirks: the first ``solve_or_resume`` after ``prepare`` runs
``nsteps-1`` iterations (solver.py:160-165), ``hat_U`` is re-derived from ``U`` on
every call (solver.py:159), every call starts with the coefficient grids of
``params.delt`` while ``self.delt`` keeps its adapted value until the adaptive
step fires again (solver.py:154-155 against 185-193), ``prepare`` does not reset
``delt``/``time_delta_sum``/``skip_check`` (solver.py:50-54 are only set in
``__init__``), and a field assigned to ``solution.U`` between two calls is what the
next call continues from (solver.py:158).
"""
import numpy as np

from . import (_lib, chords, components, composition, contour, distance, geodesic, morphology, mport, shapes, skeleton, spectrum,
               thickness, tracking, transport, two_point)
from .solution import Solution, _fingerprint
from .timedata import TimeData


class Solver:
    def __init__(self, params=None, U_init=None):
        self.params = params
        self.solution = Solution(self.params)
        N = params.N
        self.skip_check = False
        self.time_delta_sum = 0.0
        self.time_passed = 0.0
        self._prepared = False
        self.delt = self.params.delt
        self._engine = None

        self.create_rand = None
        self._pcg = None
        self._pcg_state0 = None  # the default generator's state before the start field was drawn
        self.device_rng = True   # draw start field and jitter noise on the device when the generator is numpy's PCG64
        # A call that follows a completed call (fixed time step, nothing assigned in between) continues the device
        # loop where it stopped, hat_U included; True recomputes hat_U = dctn(U) at every call as solver.py:159
        # does (the same array up to rounding, one transform more per call)
        self.rederive_hat = False
        # with rederive_hat: take the first step's operand (row transform of EnergieEut(U)) over from the previous call's
        # last step instead of computing it again (CHS_STEP_KEEP_T1; the same run bit for bit, no faster at N=4096)
        self.rederive_keeps_t1 = False
        self._U_init = None
        # initial concentration field, solver.py:59-82
        if U_init is not None:
            if U_init.shape == (N, N):
                self.U_init = U_init
            else:
                print("U_init has wrong shape, must match parameters.N")
                raise SystemExit(1)
        elif params.generator == 'lcg':
            # no "-0.5" here, as in the reference (solver.py:66)
            self.U_init = params.XXX + (params.XXX * 0.01 * mport.matlab_lcg_sample(N, N, params.seed))
        elif params.generator == 'sobol':
            from scipy.stats import qmc
            qrng = qmc.Sobol(d=N, seed=params.seed)
            self.create_rand = lambda n: qrng.random(n)
        elif params.generator == 'simplex':
            try:
                import opensimplex
            except ImportError as e:  # pragma: no cover - depends on the image
                raise ImportError("generator='simplex' needs the `opensimplex` package") from e
            self.create_rand = lambda n: opensimplex.noise2array(np.linspace(0, 48, n), np.linspace(0, 48, n))
        else:
            rng = np.random.Generator(np.random.PCG64(params.seed))
            self.create_rand = lambda n: rng.random((n, n))
            self._pcg = rng   # the device can continue this stream itself (jitter, solve_or_resume)
            # The start field XXX + XXX*0.01*(rng.random((N,N)) - 0.5) (solver.py:78-82) is not drawn
            # here: prepare() lets the device draw it from the same stream (no N*N*8-byte upload), the
            # attribute U_init computes it on the host when somebody looks at it.  The generator moves
            # on by the N*N draws either way.
            self._pcg_state0 = rng.bit_generator.state
            rng.bit_generator.advance(N * N)
        if self._U_init is None and self._pcg_state0 is None:
            self._U_init = params.XXX + (params.XXX * 0.01 * (self.create_rand(N) - 0.5))

    @property
    def U_init(self):
        if self._U_init is None and self._pcg_state0 is not None:
            g = np.random.Generator(np.random.PCG64())
            g.bit_generator.state = self._pcg_state0
            p = self.params
            self._U_init = p.XXX + (p.XXX * 0.01 * (g.random((p.N, p.N)) - 0.5))
        return self._U_init

    @U_init.setter
    def U_init(self, value):
        self._U_init = value

    # -- engine ----------------------------------------------------------------
    def _consts(self):
        p, s = self.params, self.solution
        c = _lib.chs_consts()
        c.N = int(p.N)
        c.dtype = _lib.DTYPES[str(getattr(p, 'dtype', 'float64'))]
        c.device = int(getattr(p, 'device', 0) or 0)
        c.engine = _lib.ENGINES[str(getattr(p, 'engine', 'auto'))]
        c.adaptive_time = 1 if p.adaptive_time else 0
        c.full_sim = 1 if p.full_sim else 0
        c.RT, c.BRT, c.B = float(s.RT), float(s.BRT), float(p.B)
        c.A0, c.A1, c.Amr = float(s.A0), float(s.A1), float(s.Amr)
        c.kappa_tilde, c.L, c.delx = float(s.kappa_tilde), float(p.L), float(s.delx)
        c.delt, c.delt_max, c.M_tilde = float(p.delt), float(p.delt_max), float(p.M_tilde)
        c.threshold = float(p.threshold)
        c.time_limit_s = float(p.time_max * 60) if (p.time_max is not None and p.time_max > 0) else 0.0
        return c

    def _get_engine(self):
        if self._engine is None:
            self._engine = _lib.Engine(self._consts(), self.solution.lam)
            self._push_state()
        return self._engine

    def _push_state(self):
        st = self._engine.get_state()
        st.delt = float(self.delt)
        st.time_delta_sum = float(self.time_delta_sum)
        st.time_passed = float(self.time_passed)
        st.skip_check = 1 if self.skip_check else 0
        self._engine.set_state(st)

    def _pull_state(self):
        st = self._engine.get_state()
        sol = self.solution
        self.delt = st.delt
        self.time_delta_sum = st.time_delta_sum
        self.time_passed = st.time_passed
        self.skip_check = bool(st.skip_check)
        sol.computed_steps = int(st.computed_steps)
        sol.tau0 = int(st.tau0) if float(st.tau0).is_integer() else st.tau0
        sol.t0 = st.t0
        sol.stop_reason = _lib.STOP_NAMES[st.stop_reason]
        return st

    def close(self, fetch_U=True):
        """Free the device engine.  A download of the field that is still pending (Solution.U is
        fetched on first access) happens now unless the caller does not need it."""
        if self._engine is not None:
            if fetch_U:
                _ = self.solution.U
            else:
                # the caller needs scalars only: solution.U stays what the host already has (None when
                # the field was never downloaded)
                self.solution._bind_device_U(self.solution.__dict__.get('_U'), track=False)
            self._engine.close()
            self._engine = None

    def _push_edited_U(self):
        """The caller replaced the field since the last call -- by assignment, or by editing the array `solution.U`
        handed out in place: `U = self.solution.U` (solver.py:158) is where the reference starts."""
        sol = self.solution
        if sol.__dict__.get('_U_dirty') or sol._host_edited():
            u = sol.__dict__['_U']
            self._engine.set_U(u)
            sol.__dict__['_U_dirty'] = False
            sol.__dict__['_U_print'] = _fingerprint(u)   # (the array mirrors the device field again: a later edit is noticed)

    def _look_engine(self):
        """The opening of a look: the engine, with a field the host edited pushed to the device."""
        eng = self._get_engine()
        self._push_edited_U()
        return eng

    def structure_factor(self):
        """The radially averaged structure factor of the field the device holds, a `spectrum.StructureFactor`
        (Ssum, n, S, k1, ell, ell_phys).  Computed on the device between two calls without changing the run; a field
        the host edited is pushed first, as solve_or_resume does.  Needs a field: prepare() first."""
        return spectrum.StructureFactor(self._look_engine().structure_factor(), self.params.N, self.solution.delx)

    def morphology(self, threshold=None):
        """Area, interface length and Euler number of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``, the one of the recorded ``SA``): a `morphology.Morphology` from one sweep on the device
        between two calls, which the run does not notice.  A field the host edited is pushed first, as solve_or_resume
        does.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        eng = self._look_engine()
        return morphology.Morphology(eng.morphology(t), self.params.N, t, self.solution.delx)

    def components(self, threshold=None, connectivity=4, side='below', table=True, labels=False):
        """The connected components of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): droplet count, sizes, bounding boxes, spanning -- a self-contained
        `components.Components` from one look on the device between two calls, which the run does not notice.
        ``side='below'`` is the foreground of `morphology`, ``'above'`` its complement; ``connectivity`` 4 or 8; the
        table (one row per component) and the label image are fetched in this call when asked for.  A field the host
        edited is pushed first, as solve_or_resume does.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        conn, code = components.check_connectivity(connectivity), components.side_code(side)
        eng = self._look_engine()
        words, tab, lab = eng.components_look(t, conn, code, table, labels)
        return components.Components(words, self.params.N, t, conn, code, table=tab, labels=lab, delx=self.solution.delx)

    def distance(self, threshold=None, side='below', hist=True, map=False):
        """The exact Euclidean distance transform of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): how wide the domains are in real space -- the widest point, the mean squared half-width,
        the histogram of local radii -- a self-contained `distance.Distance` from one look on the device between two
        calls, which the run does not notice.  ``side='below'`` is the foreground of `morphology`, ``'above'`` its
        complement; the histogram and the N x N map of squared distances are fetched in this call when asked for (without
        ``map=True`` nothing N x N leaves the device).  A field the host edited is pushed first, as solve_or_resume
        does.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        code = distance.side_code(side)
        eng = self._look_engine()
        words, hi, d2 = eng.distance_look(t, code, hist, map)
        return distance.Distance(words, self.params.N, t, code, hist=hi, d2=d2, delx=self.solution.delx)

    def thickness(self, threshold=None, side='below', hist=True, map=False, max_work=None):
        """The local thickness of a phase of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): for every pixel the radius of the largest disc that fits inside the phase and covers it --
        the area-weighted histogram of those radii is the pore-size distribution, twice its mean the mean domain width --
        a self-contained `thickness.Thickness` (with the `distance.Distance` of the same field in ``.distance``) from
        looks on the device between two calls, which the run does not notice.  ``side`` as for `distance`; histogram and
        N x N map are fetched in this call when asked for (without ``map=True`` nothing N x N leaves the device).
        ``max_work`` (None: ``_lib.thickness_work_default(N)``) bounds the disc pixels the look may paint: a field that
        needs more raises `_lib.ThicknessLimitError` with ``work`` and ``limit``, and nothing is painted.  Needs a field:
        prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        code = thickness.side_code(side)
        eng = self._look_engine()
        (words, hi, t2), (dwords, dhi, d2) = eng.thickness_look(t, code, hist, map, max_work)
        di = distance.Distance(dwords, self.params.N, t, code, hist=dhi, d2=d2, delx=self.solution.delx)
        return thickness.Thickness(words, self.params.N, t, code, hist=hi, t2=t2, distance=di, delx=self.solution.delx)

    def geodesic(self, threshold=None, connectivity=8, side='below', source='top', hist=True, profile=True, map=False,
                 max_rounds=None):
        """The geodesic look at a phase of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): the length of the shortest path through the phase alone from the wall ``source`` ('top',
        'bottom', 'left', 'right') to every pixel of the phase -- the geodesic tortuosity of the way across, the fraction
        of the phase that can be reached from that face and how much of it within a given depth -- a self-contained
        `geodesic.Geodesic` from a look on the device between two calls, which the run does not notice.  ``connectivity``
        and ``side`` as for `components`; histogram, profile and N x N map are fetched in this call when asked for
        (without ``map=True`` nothing N x N leaves the device).  ``max_rounds`` (None:
        ``_lib.geodesic_rounds_default(N)``) bounds the relaxation rounds: a field that needs more raises
        `_lib.GeodesicLimitError` with ``rounds`` and ``limit``.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        conn = components.check_connectivity(connectivity)
        code, src = components.side_code(side), geodesic.source_code(source)
        eng = self._look_engine()
        words, hi, pr, g = eng.geodesic_look(t, conn, code, src, hist, profile, map, max_rounds)
        return geodesic.Geodesic(words, self.params.N, t, conn, code, src, hist=hi, profile=pr, g=g, delx=self.solution.delx)

    def skeleton(self, threshold=None, side='below', hist=True, map=False, max_subiters=None):
        """The skeleton look at a phase of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): the medial network of the phase by a topology-preserving parallel thinning on the device --
        its dead ends, links, branch points and crossings, the length of network per area, its coordination and the
        half-widths along it, the narrowest neck among them -- a self-contained `skeleton.Skeleton` from a look on the
        device between two calls, which the run does not notice.  ``side`` as for `distance`; the histogram of the widths
        and the packed plane (``map=True``; N*N/8 bytes, `Skeleton.mask()` unpacks it) are fetched in this call when asked
        for.  ``max_subiters`` (None: ``_lib.skeleton_subiters_default(N)``) bounds the sub-iterations, a kernel launch
        each: a field that needs more raises `_lib.SkeletonLimitError` with ``subiters`` and ``limit``.  Needs a field:
        prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        code = skeleton.side_code(side)
        eng = self._look_engine()
        words, hi, plane = eng.skeleton_look(t, code, hist, map, max_subiters)
        return skeleton.Skeleton(words, self.params.N, t, code, hist=hi, plane=plane, delx=self.solution.delx)

    def transport(self, threshold=None, side='below', source='top', tol=1e-6, profile=True, map=False, max_iters=None):
        """The transport look at a phase of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): steady diffusion through the phase alone from the wall ``source`` ('top', 'bottom', 'left',
        'right'), held at c = 1, to the opposite wall, held at c = 0, solved on the device by conjugate gradients in fp64
        -- the effective diffusivity ``deff`` = D_eff / D_0 with its certified error bound, the formation factor and the
        tortuosity factor eps / deff -- a self-contained `transport.Transport` from a look on the device between two
        calls, which the run does not notice.  ``side`` as for `components` (the connectivity is 4); ``tol`` in [1e-12,
        1e-2] is the relative accuracy of ``deff`` the look has to certify; the profile by depth and the N x N map of c
        are fetched in this call when asked for (without ``map=True`` nothing N x N leaves the device).  ``max_iters``
        (None: ``_lib.transport_iters_default(N)``) bounds the iterations: a solve that is not accepted by then raises
        `_lib.TransportLimitError` with ``iters`` and ``limit``.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        code, src = components.side_code(side), transport.source_code(source)
        eng = self._look_engine()
        words, vals, pr, cm = eng.transport_look(t, code, src, tol, profile, map, max_iters)
        return transport.Transport(words, vals, self.params.N, t, code, src, profile=pr, c=cm, delx=self.solution.delx)

    def chords(self, threshold=None, hist=True):
        """The chord lengths (linear intercepts) of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): the segments the rows and the columns cut out of each phase -- count, mean, weighted
        mean and longest chord per phase and direction, the anisotropy, and with the histograms the quantiles and the
        lineal-path function -- a self-contained `chords.Chords` from one look on the device between two calls, which
        the run does not notice.  One look gives both phases and both directions; the histograms (8 (N + 1) integers)
        are fetched in this call unless ``hist=False``; nothing N x N leaves the device.  A field the host edited is
        pushed first, as solve_or_resume does.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        eng = self._look_engine()
        words, hi = eng.chords_look(t, hist)
        return chords.Chords(words, self.params.N, t, hist=hi, delx=self.solution.delx)

    def composition(self, threshold=None, bins=15, range=None, quantiles=(0.05, 0.5, 0.95), hist=True):
        """The values of the field the device holds: how far the two phases have moved towards their compositions, how
        much material sits between them, and whether the field has left [0, 1] or gone NaN -- minimum, maximum, mean,
        variance, skewness and kurtosis, the mean on either side of `threshold` (None: ``params.threshold``), a
        histogram of ``bins`` bins over ``range`` (None: the field's own minimum and maximum; ``bins=15, range=None`` is
        the reference's ``Uhist``) and the exact ``quantiles`` -- a self-contained `composition.Composition` from two
        sweeps on the device between two calls, and one radix select for up to eight quantiles, which the run does not
        notice; nothing N x N leaves the device.  A quantile q is the pixel of rank ``floor(q (n - n_nan - 1))`` among
        those that are not NaN (``numpy.quantile(..., method='lower')``).  The histogram is fetched in this call unless
        ``hist=False``.  A field the host edited is pushed first, as solve_or_resume does.  Needs a field: prepare()
        first."""
        t = float(self.params.threshold if threshold is None else threshold)
        nbins = composition.check_bins(bins)
        lo, hi = composition.check_range(range)
        qs = [float(q) for q in (quantiles or ())]
        eng = self._look_engine()
        iw, fw, counts = eng.composition_look(t, nbins, lo, hi, hist)
        sortable = int(iw[composition.CHS_CMP_N_TOTAL] - iw[composition.CHS_CMP_N_NAN])
        found = {}
        if sortable > 0:
            ranks = [composition.quantile_rank(q, sortable) for q in qs]
            for k in np.arange(0, len(ranks), composition.CHS_CMP_MAX_RANKS):   # (`range` is the argument)
                part = slice(int(k), int(k) + composition.CHS_CMP_MAX_RANKS)
                found.update(zip(qs[part], (float(v) for v in eng.composition_select(ranks[part]))))
        return composition.Composition(iw, fw, self.params.N, t, hist=counts, quantiles=found, delx=self.solution.delx)

    def two_point(self, threshold=None, rmax=two_point.DEFAULT_RMAX, counts=True):
        """The two-point correlation of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): for either phase the number of pixel pairs of that phase at every displacement (dy, dx)
        with ``0 <= dy <= rmax, |dx| <= rmax`` -- the two-point probability function S2 as a full map, its radial
        average, the autocovariance and its first zero (the real-space domain size), the cross-phase correlation -- a
        self-contained `two_point.TwoPoint` from one look on the device between two calls, which the run does not
        notice.  ``rmax`` left at its default is clipped to ``two_point.max_r(N) = min(N - 1, 256)``; a value given
        outside ``[1, max_r(N)]`` raises.  The count table (2 (rmax + 1)(2 rmax + 1) integers) is fetched in this call
        unless ``counts=False``; nothing N x N leaves the device.  A field the host edited is pushed first, as
        solve_or_resume does.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        N = self.params.N
        r = min(int(rmax), two_point.max_r(N)) if rmax is two_point.DEFAULT_RMAX else rmax
        r = two_point.check_rmax(N, r)
        eng = self._look_engine()
        words, c = eng.two_point_look(t, r, counts)
        return two_point.TwoPoint(words, N, t, r, counts=c, delx=self.solution.delx)

    def contour(self, threshold=None, bins=contour.DEFAULT_BINS, kmax=contour.DEFAULT_KMAX, hist=True, map=False):
        """The interface of the field the device holds below the pixel: the marching-squares contour of ``U =
        threshold`` (None: ``params.threshold``) -- its true length per area ``S_V`` (the pixel perimeter of
        `morphology` overestimates an isotropic interface by 4 / pi), its orientation tensor, and the curvature of the
        level set at every crossed cell from the field's own derivatives: mean, mean absolute and rms curvature, the
        integral of kappa^2 and a histogram of ``bins`` bins over ``[-kmax, kmax]`` (1 / pixel) by cells and by length --
        a self-contained `contour.Contour` from one sweep on the device between two calls, which the run does not
        notice.  The histograms are fetched in this call unless ``hist=False``; the two (N-1) x (N-1) maps of ell and
        kappa only with ``map=True`` (without it nothing N x N leaves the device).  A field the host edited is pushed
        first, as solve_or_resume does.  Needs a field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        nb, km = contour.check_bins(bins), contour.check_kmax(kmax)
        eng = self._look_engine()
        words, sums, hi, mp = eng.contour_look(t, nb, km, hist, map)
        return contour.Contour(words, sums, self.params.N, t, nb, km, hist=hi, map=mp, delx=self.solution.delx)

    def shapes(self, threshold=None, connectivity=4, side='below', labels=False):
        """The shape of every droplet of the field the device holds, thresholded at `threshold` (None:
        ``params.threshold``): centroid, second moments and the ellipse of equal moments, perimeter, circularity, holes,
        wall contact, mean composition and its variance per connected component -- a self-contained `shapes.Shapes`
        from one components look and one more sweep on the device between two calls, which the run does not notice.
        Foreground, ``connectivity`` and ``side`` are those of `components`; the `components.Components` of the same
        look is its ``.components`` (with the label image when ``labels=True``).  Only the two tables leave the
        device, 152 bytes per droplet.  A field the host edited is pushed first, as solve_or_resume does.  Needs a
        field: prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        conn, code = components.check_connectivity(connectivity), components.side_code(side)
        eng = self._look_engine()
        words, tab, cctab, lab = eng.shapes_look(t, conn, code, labels)
        co = components.Components(words[:components.CHS_CC_WORDS], self.params.N, t, conn, code, table=cctab, labels=lab,
                                   delx=self.solution.delx)
        return shapes.Shapes(words, tab, co)

    def track(self, threshold=None, connectivity=4, side='below', keep=True, reset=False):
        """The droplets of the field the device holds against those of the last track look that was kept: which droplet
        of then is which droplet of now, what merged, split, vanished or was born, and how the continued ones grew -- a
        self-contained `tracking.Track` from one shapes look and the overlap passes on the device between two calls,
        which the run does not notice.  The device keeps the number image of the kept look (the frame) and overlaps it
        with the labelling of now; only the pair table and the two tables of `shapes` leave the device.  ``keep=True``
        makes this look the frame of the next one; ``keep=False`` leaves the frame, which compares many later times
        against one reference; ``reset=True`` drops the frame first.  The first look (and one after a reset) finds no
        frame: its `Track` has ``have_prev`` False and nothing to link.  Foreground, ``connectivity`` and ``side`` are
        those of `components` and need not be the frame's.  Overlap tracking assumes looks close enough in time that a
        droplet overlaps itself.  A field the host edited is pushed first, as solve_or_resume does.  Needs a field:
        prepare() first."""
        t = float(self.params.threshold if threshold is None else threshold)
        conn, code = components.check_connectivity(connectivity), components.side_code(side)
        eng = self._look_engine()
        held = self.__dict__.get('_track_prev')
        if held is not None and held[0] is not eng:          # (the frame went with the engine that held it)
            held = self._track_prev = None
        if reset:
            eng.track_reset()
            held = self._track_prev = None
        words, pairs, tab, cctab = eng.track_look(t, conn, code, keep)
        co = components.Components(words[:components.CHS_CC_WORDS], self.params.N, t, conn, code, table=cctab,
                                   delx=self.solution.delx)
        now = shapes.Shapes(words[:shapes.CHS_SH_WORDS], tab, co)
        steps = self.solution.computed_steps
        at = (None if steps is None else int(steps), float(self.time_passed))
        if words[tracking.CHS_TR_HAVE_PREV] and held is None:
            raise ValueError("the device holds a frame that this Solver did not take: track(reset=True) starts anew")
        prev, was = (held[1], held[2]) if words[tracking.CHS_TR_HAVE_PREV] else (None, (None, None))
        out = tracking.Track(words, pairs, prev, now, steps=(was[0], at[0]), times=(was[1], at[1]))
        if keep:
            self._track_prev = (eng, now, at)
        return out

    # -- solver.py:84-135 ----------------------------------------------------------
    def prepare(self):
        N = self.params.N
        eng = self._get_engine()
        self._push_state()
        on_device = self._U_init is None and self._pcg_state0 is not None and self.device_rng
        if on_device:
            st = self._pcg_state0['state']
            p = self.params
            eng.init_U_pcg64(p.XXX, p.XXX * 0.01, st['state'], st['inc'])
            U = None
        else:
            U = self.U_init.copy()
            assert (U.shape == (N, N))
            eng.set_U(U)
        row = eng.prepare()
        data = TimeData()
        data.insert(it=0, delt=row[8], E=row[1], E2=row[2], SA=0, domtime=0, Ra=row[5], L2=0, PS=row[7])
        # on_device: downloaded when somebody looks at solution.U
        self.solution._bind_device_U(U, eng.get_U if on_device else None)
        self.solution.timedata = data
        self.solution.tau0 = 0.0
        self.solution.t0 = 0.0
        self.solution.stop_reason = 'None'
        self.solution.computed_steps = 1
        self._prepared = True

    # -- solver.py:137-252 ---------------------------------------------------------
    def solve_or_resume(self, nsteps=None):
        """Run the timestep loop on the device and return the solution object."""
        assert (self._prepared is True)
        p = self.params
        if nsteps is None:
            nsteps = max(p.ntmax, 0)
        eng = self._engine
        if self.solution.__dict__.get('_U_dirty') or self.solution._host_edited():
            # the caller replaced the field since the last call -- by assignment, or by editing the array
            # `solution.U` handed out in place: `U = self.solution.U` (solver.py:158) is where the reference starts
            eng.set_U(self.solution.__dict__['_U'])
            self.solution.__dict__['_U_dirty'] = False
            self.solution.__dict__['_U_print'] = None
        itbegin = 1 if self.solution.computed_steps == 1 else 0
        count = max(int(nsteps) - itbegin, 0)

        jitter_on = p.jitter is not None and 0.0 < p.jitter < 0.1
        if not jitter_on:
            eng.set_jitter_noise(0.0, None)
            # (a call that reaches ntmax ends the run: its last step need not prepare a continuation)
            rows, rc = eng.step_n(count, rederive_hat=self.rederive_hat, keep_t1=self.rederive_hat and self.rederive_keeps_t1,
                                  last_call=self.solution.computed_steps + count >= p.ntmax)
            self._absorb(rows, rc, count)
        elif self._pcg is not None and self.device_rng:
            # The reference's default generator (numpy PCG64, solver.py:78-82): the device continues
            # its stream from the generator's current state -- N*N draws per step in C order, exactly
            # what `create_rand(N)` would have returned (solver.py:211) -- and the whole chunk runs as
            # one device loop; afterwards the host generator is moved on by what the device consumed.
            st = self._pcg.bit_generator.state['state']
            eng.set_jitter_pcg64(p.jitter, st['state'], st['inc'])
            rows, rc = eng.step_n(count)
            try:
                self._absorb(rows, rc, count)
            finally:
                self._pcg.bit_generator.advance(int(rows.shape[0]) * p.N * p.N)
        else:
            # Other generators: the noise comes from the host generator so that its stream stays the
            # reference's (solver.py:211); hat_U is carried between the one-step
            # calls exactly as inside the reference's loop.
            first = True
            for _ in range(count):
                eng.set_jitter_noise(p.jitter, self.create_rand(p.N))
                rows, rc = eng.step_n(1, carry_hat=not first)
                first = False
                if self._absorb(rows, rc, 1):
                    break
            if count == 0:
                self._pull_state()
        self.solution._bind_device_U(None, eng.get_U)   # downloaded when somebody looks at solution.U
        return self.solution

    def _absorb(self, rows, rc, requested):
        """Append the rows of one device call; True when the device loop broke early."""
        sol = self.solution
        if rc == _lib.CHS_ENAN:
            if rows.shape[0] > 1:
                sol.timedata.extend(rows[:-1])
            self._pull_state()
            sol._bind_device_U(self._engine.get_U(), track=False)
            # the reference fails the same way: assert in TimeData.insert (timedata.py:10)
            raise AssertionError("NaN in a recorded scalar (U left (0,1)) at step %d" % sol.computed_steps)
        if rows.shape[0]:
            sol.timedata.extend(rows)
        st = self._pull_state()
        if rows.shape[0] < requested:
            return True
        return (st.stop_reason == _lib.CHS_STOP_ENERGY and not self.params.full_sim
                and st.tau0 == st.computed_steps)
