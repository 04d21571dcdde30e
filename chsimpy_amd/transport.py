"""Transport look at a phase of the thresholded field -- steady diffusion through the phase alone between two opposite walls:
effective diffusivity, formation factor, tortuosity factor: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_transport).

Foreground and walls.  ``threshold``, ``side`` ('below' / 'above') and the NaN convention are those of `components` at
connectivity 4, with no wrap-around.  ``source`` is 0 'top' (row 0), 1 'bottom' (row N-1), 2 'left' (column 0) or 3 'right'
(column N-1), as in `geodesic`; the target is the opposite wall; the depth k of a pixel is its distance from the source wall
along that axis.

Active set.  The active pixels are those of the components whose bounding box touches both the source wall and the target
wall.  Every other pixel carries no flux and takes no part in the solve; this also keeps the system non-singular.

System.  One unknown c_p per active pixel.  Two 4-adjacent active pixels share a bond of conductance 1.  An active pixel on
the source wall has a bond of conductance 2 to the wall face, which is held at c = 1 (the face is half a pixel away); an
active pixel on the target wall has a bond of conductance 2 to the wall face, which is held at c = 0.  No flux passes
through the other two walls or into pixels that are not active.  ``A c = b`` is the balance of every pixel: b_p = 2 on the
source wall and 0 elsewhere; A is symmetric positive definite.

Results.  ``F_in`` = sum over the source wall of 2 (1 - c_p); ``F_out`` = sum over the target wall of 2 c_p; ``cut[k]``, k = 0
.. N, is the flux through the face between depth k-1 and depth k, so cut[0] = F_in and cut[N] = F_out.  For the exact
solution all cuts equal F*, and D_eff / D_0 = F*.  The formation factor is 1 / F*; with the porosity eps = FG / N^2 the
tortuosity factor is eps / F*.

Certificate.  With r = b - A c evaluated from the returned c: |F_out - F*| <= |r|_1, |F_in - F*| <= |r|_1 and |cut[k] -
F_out| = |sum over depth >= k of r_p| <= |r|_1 (maximum principle: the adjoint potentials lie in [0, 1]).

Acceptance.  A look succeeds only if ``RES1 <= tol min(F_in, F_out)``, RES1 being the 1-norm of the true residual recomputed
from the final c; the recurrence residual of the iteration does not count.  ``tol`` lies in [1e-12, 1e-2].

Words (`WORDS`, int64): ``fg, active, cc_count, cc_spanning, src_pixels, tgt_pixels, bonds, iters, checks, limit``.  Values
(`VALS`, float64): ``f_in, f_out, res1, resinf, cut_min, cut_max, csum, tol``.  Profile: float64 [N+1][3], one row per face
or depth k: cut[k], the sum of c at depth k, the active pixels at depth k; row N holds zeros in the last two columns.  Map:
float64 [N][N]: c on the active pixels, -1.0 on the background, -2.0 on foreground that is not active.  Without a spanning
component ``active`` == 0, no iteration runs and every value is 0.

The model runs the conjugate-gradient iteration of the device -- no preconditioner, no restart, the same stopping logic --
in numpy's summation order: its map agrees with the device's to the certificate, not bit for bit.
"""
import numpy as np

from . import components, geodesic

WORDS = ('fg', 'active', 'cc_count', 'cc_spanning', 'src_pixels', 'tgt_pixels', 'bonds', 'iters', 'checks', 'limit')
VALS = ('f_in', 'f_out', 'res1', 'resinf', 'cut_min', 'cut_max', 'csum', 'tol')
CHS_TRN_WORDS, CHS_TRN_VALS = len(WORDS), len(VALS)
(CHS_TRN_FG, CHS_TRN_ACTIVE, CHS_TRN_CC_COUNT, CHS_TRN_CC_SPANNING, CHS_TRN_SRC_PIXELS, CHS_TRN_TGT_PIXELS, CHS_TRN_BONDS,
 CHS_TRN_ITERS, CHS_TRN_CHECKS, CHS_TRN_LIMIT) = range(CHS_TRN_WORDS)
(CHS_TRN_F_IN, CHS_TRN_F_OUT, CHS_TRN_RES1, CHS_TRN_RESINF, CHS_TRN_CUT_MIN, CHS_TRN_CUT_MAX, CHS_TRN_CSUM,
 CHS_TRN_TOL) = range(CHS_TRN_VALS)
UNIQUE = [k for k in range(CHS_TRN_WORDS) if k not in (CHS_TRN_ITERS, CHS_TRN_CHECKS)]   # the words a field determines
UP, DOWN, LEFT, RIGHT, SRC, TGT, ACT = 1, 2, 4, 8, 16, 32, 64                            # the byte of a pixel
BACKGROUND, EXCLUDED = -1.0, -2.0
TOL_DEFAULT, TOL_MIN, TOL_MAX = 1e-6, 1e-12, 1e-2
ITERS_FACTOR, ITERS_SLACK, MAX_FACTOR = 48, 64, 16
SOURCES, SOURCE_NAMES = geodesic.SOURCES, geodesic.SOURCE_NAMES
source_code = geodesic.source_code
depth_of = geodesic.depth_of
EPS = float(np.finfo(np.float64).eps)


def iters_default(N):
    """The default iteration limit at grid size N (chs_transport_iters_default): 48 N + 64."""
    return ITERS_FACTOR * int(N) + ITERS_SLACK


def check_tol(tol):
    tol = float(tol)
    if not TOL_MIN <= tol <= TOL_MAX:
        raise ValueError(f"tol is in [{TOL_MIN}, {TOL_MAX}], got {tol!r}")
    return tol


class IterationLimit(ValueError):
    """The model's solve was not accepted within ``limit`` iterations (the device: CHS_ELIMIT)."""

    def __init__(self, iters, limit):
        super().__init__(f"the solve is not accepted after {iters} iterations, max_iters = {limit}")
        self.iters, self.limit = int(iters), int(limit)


# ---------------------------------------------------------------------------
# the system
# ---------------------------------------------------------------------------
class System:
    """The linear system of a mask and a source wall: ``codes`` (uint8 [N][N], the byte of every pixel: bond bits `UP`,
    `DOWN`, `LEFT`, `RIGHT`, wall bits `SRC`, `TGT`, the active bit `ACT`), ``degree`` (the diagonal of A) and ``b``, all
    zero off the active set; ``mask``, ``active``, ``cc_count``, ``cc_spanning``.  Unpacks as (codes, degree, b)."""

    def __init__(self, mask, source='top'):
        X = np.asarray(mask, dtype=bool)
        if X.ndim != 2 or X.shape[0] != X.shape[1]:
            raise ValueError(f"a square mask is needed, got shape {X.shape}")
        N = X.shape[0]
        self.N, self.source, self.mask = N, source_code(source), X
        labels, table = components.label(np.where(X, 0.0, 1.0), 0.5, 4)
        lo, hi = (table[:, 2], table[:, 3]) if self.source < 2 else (table[:, 4], table[:, 5])
        span = (lo == 0) & (hi == N - 1)
        self.cc_count, self.cc_spanning = int(table.shape[0]), int(span.sum())
        act = X & np.append(span, False)[labels]            # (label -1: background)
        P = np.zeros((N + 2, N + 2), dtype=bool)
        P[1:-1, 1:-1] = act
        self.active = act
        self._nb = [(UP, act & P[:-2, 1:-1], (slice(0, N), slice(1, N + 1))), (DOWN, act & P[2:, 1:-1], (slice(2, N + 2), slice(1, N + 1))),
                    (LEFT, act & P[1:-1, :-2], (slice(1, N + 1), slice(0, N))), (RIGHT, act & P[1:-1, 2:], (slice(1, N + 1), slice(2, N + 2)))]
        self.depth = depth_of(N, self.source)
        self.src, self.tgt = act & (self.depth == 0), act & (self.depth == N - 1)
        codes = act * ACT + self.src * SRC + self.tgt * TGT
        degree = 2.0 * self.src + 2.0 * self.tgt
        for bit, has, _ in self._nb:
            codes = codes + has * bit
            degree = degree + has
        self.codes, self.degree, self.b = codes.astype(np.uint8), degree, 2.0 * self.src
        self.bonds = int(self._nb[1][1].sum() + self._nb[3][1].sum())
        self._pad = np.zeros((N + 2, N + 2))

    def __iter__(self):
        return iter((self.codes, self.degree, self.b))

    def apply(self, c):
        """A c for c [N][N]; what c holds off the active set is not read."""
        c = np.where(self.active, c, 0.0)
        self._pad[1:-1, 1:-1] = c
        out = self.degree * c
        for _, has, at in self._nb:
            out -= np.where(has, self._pad[at], 0.0)
        return out

    def residual_of(self, c):
        """b - A c."""
        return self.b - self.apply(c)

    def fluxes(self, c):
        """(F_in, F_out) of c."""
        return float((2.0 * (1.0 - c[self.src])).sum()), float((2.0 * c[self.tgt]).sum())

    def map_of(self, c):
        """c on the active pixels, -1 on the background, -2 on foreground that is not active."""
        return np.where(self.active, c, np.where(self.mask, EXCLUDED, BACKGROUND))

    def matrix(self):
        """(A as a scipy.sparse CSR matrix over the active pixels in row-major order, b over them): for references."""
        import scipy.sparse as sp
        N = self.N
        idx = np.full((N + 2, N + 2), -1, dtype=np.int64)
        n = int(self.active.sum())
        inner = idx[1:-1, 1:-1]
        inner[self.active] = np.arange(n)
        rows, cols, vals = [np.arange(n)], [np.arange(n)], [self.degree[self.active]]
        for _, has, at in self._nb:
            rows.append(inner[has]); cols.append(idx[at][has]); vals.append(-np.ones(int(has.sum())))
        A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
        return A, self.b[self.active]


def system_of(mask, source='top'):
    """The `System` of a boolean mask and a source wall; unpacks as (codes, degree, b)."""
    return System(mask, source)


def apply(system, c):
    """A c of a `System`."""
    return system.apply(c)


def residual_of(system, c):
    """b - A c of a `System`."""
    return system.residual_of(c)


def reference(mask, source='top'):
    """(map, F) of the exact solution by scipy's sparse direct solver; F = 0 and no active pixel without a spanning
    component.  For tests and tables, not for the package: scipy is imported here alone."""
    from scipy.sparse.linalg import spsolve
    S = System(mask, source)
    c = np.zeros((S.N, S.N))
    if S.active.any():
        A, b = S.matrix()
        c[S.active] = spsolve(A.tocsc(), b)
    fin, fout = S.fluxes(c) if S.active.any() else (0.0, 0.0)
    return S.map_of(c), 0.5 * (fin + fout)


# ---------------------------------------------------------------------------
# the solve and the statistics
# ---------------------------------------------------------------------------
def solve(mask, source='top', tol=TOL_DEFAULT, max_iters=None, system=None):
    """(map, words, vals, profile) of the mask: the conjugate-gradient iteration of the device from c = 0 -- p <- r + beta p,
    q = A p, alpha = r.r / p.q, c += alpha p, r -= alpha q, beta = r.r / (the r.r before), a zero denominator giving a zero
    step -- until the recurrence residual meets the acceptance rule; then the true residual decides, and where it fails
    it takes the place of r, p stays and the iteration goes on.  Raises `IterationLimit` past ``max_iters`` (None: the
    default)."""
    tol = check_tol(tol)
    S = System(mask, source) if system is None else system
    N = S.N
    default = iters_default(N)
    limit = default if max_iters is None else int(max_iters)
    if not 0 <= limit <= MAX_FACTOR * default:
        raise ValueError(f"max_iters = {limit} is outside [0, {MAX_FACTOR * default}]")
    limit = limit or default
    x = np.zeros((N, N))
    iters = checks = 0
    accepted = not S.active.any()
    if not accepted:
        r = S.b.copy()
        p = np.zeros((N, N))
        beta, rr = 0.0, float((r * r).sum())
        while iters < limit:
            p = r + beta * p
            q = S.apply(p)
            pq = float((p * q).sum())
            alpha = rr / pq if pq != 0.0 else 0.0
            x += alpha * p
            r -= alpha * q
            new = float((r * r).sum())
            beta = new / rr if rr != 0.0 else 0.0
            rr = new
            iters += 1
            if float(np.abs(r).sum()) <= tol * min(S.fluxes(x)):
                true = S.residual_of(x)
                checks += 1
                if float(np.abs(true).sum()) <= tol * min(S.fluxes(x)):
                    accepted = True
                    break
                r, rr = true, float((true * true).sum())
    if not accepted:
        raise IterationLimit(iters, limit)
    words, vals, profile = stats_of(S.map_of(x), source, iters=iters, checks=checks, limit=limit, tol=tol, system=S)
    return S.map_of(x), words, vals, profile


def stats_of(cmap, source='top', iters=0, checks=0, limit=None, tol=TOL_DEFAULT, system=None):
    """(words int64 [10], vals float64 [8], profile float64 [N+1][3]) of a map in the convention of the look (c, -1, -2):
    the mask is ``cmap != -1``, the system is built from it anew and the residual evaluated from the map's c."""
    cmap = np.asarray(cmap, dtype=np.float64)
    N = cmap.shape[0]
    S = System(cmap != BACKGROUND, source) if system is None else system
    if not np.array_equal(S.active, (cmap != BACKGROUND) & (cmap != EXCLUDED)):
        raise ValueError("the map's -2 pixels are not the foreground outside the spanning components")
    c = np.where(S.active, cmap, 0.0)
    w = np.zeros(CHS_TRN_WORDS, dtype=np.int64)
    v = np.zeros(CHS_TRN_VALS)
    profile = np.zeros((N + 1, 3))
    w[CHS_TRN_FG], w[CHS_TRN_ACTIVE] = S.mask.sum(), S.active.sum()
    w[CHS_TRN_CC_COUNT], w[CHS_TRN_CC_SPANNING] = S.cc_count, S.cc_spanning
    w[CHS_TRN_SRC_PIXELS], w[CHS_TRN_TGT_PIXELS], w[CHS_TRN_BONDS] = S.src.sum(), S.tgt.sum(), S.bonds
    w[CHS_TRN_ITERS], w[CHS_TRN_CHECKS] = iters, checks
    w[CHS_TRN_LIMIT] = iters_default(N) if limit is None else limit
    if not S.active.any():
        return w, v, profile
    r = S.residual_of(c)
    # the flux into every pixel from its neighbour towards the source wall, by depth
    toward = {0: 0, 1: 1, 2: 2, 3: 3}[S.source]
    _, has, at = S._nb[toward]
    S._pad[1:-1, 1:-1] = c
    into = np.where(has, S._pad[at] - c, 0.0) + np.where(S.src, 2.0 * (1.0 - c), 0.0)
    k = S.depth.ravel()
    profile[:N, 0] = np.bincount(k, weights=into.ravel(), minlength=N)
    profile[N, 0] = (2.0 * c[S.tgt]).sum()
    profile[:N, 1] = np.bincount(k, weights=c.ravel(), minlength=N)
    profile[:N, 2] = np.bincount(k, weights=S.active.ravel(), minlength=N)
    v[CHS_TRN_F_IN], v[CHS_TRN_F_OUT] = profile[0, 0], profile[N, 0]
    v[CHS_TRN_RES1], v[CHS_TRN_RESINF] = np.abs(r).sum(), np.abs(r).max()
    v[CHS_TRN_CUT_MIN], v[CHS_TRN_CUT_MAX] = profile[:, 0].min(), profile[:, 0].max()
    v[CHS_TRN_CSUM], v[CHS_TRN_TOL] = c.sum(), tol
    return w, v, profile


def model_look(U, t, side='below', source='top', tol=TOL_DEFAULT, max_iters=None):
    """The `Transport` of the field U thresholded at t: the numpy model of chs_transport."""
    X = components.foreground(U, t, side)
    cmap, words, vals, profile = solve(X, source, tol, max_iters)
    return Transport(words, vals, X.shape[0], t, side, source, profile=profile, c=cmap)


# ---------------------------------------------------------------------------
# the result
# ---------------------------------------------------------------------------
class Transport:
    """One transport look: the ten words as Python integers (`WORDS`) and the eight values as floats (`VALS`), ``profile``
    ([N+1][3], None unless fetched), ``C`` (the float64 map, None unless fetched), and ``N``, ``threshold``, ``side``,
    ``source``, ``delx``.  D_eff is relative to the free diffusivity and has no unit; the ``_phys`` values are the depths
    scaled with ``delx``.  Refuses words and values that no solve has."""

    def __init__(self, words, vals, N, threshold, side='below', source='top', profile=None, c=None, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.side = 'above' if components.side_code(side) == components.CHS_CC_ABOVE else 'below'
        self.source = SOURCE_NAMES[source_code(source)]
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        self.vals = np.array(vals, dtype=np.float64)
        if self.words.shape != (CHS_TRN_WORDS,) or self.vals.shape != (CHS_TRN_VALS,):
            raise ValueError(f"{CHS_TRN_WORDS} words and {CHS_TRN_VALS} values are needed, got shapes {self.words.shape}, {self.vals.shape}")
        for name, x in zip(WORDS, self.words):
            setattr(self, name, int(x))
        for name, x in zip(VALS, self.vals):
            setattr(self, name, float(x))
        N = self.N
        none = self.active == 0
        ok = (0 <= self.active <= self.fg <= N * N and 0 <= self.cc_spanning <= self.cc_count <= self.fg
              and none == (self.cc_spanning == 0) == (self.src_pixels == 0) == (self.tgt_pixels == 0) == (self.iters == 0)
              == (self.checks == 0)
              and self.cc_spanning <= self.src_pixels <= N and self.cc_spanning <= self.tgt_pixels <= N
              and self.active >= N * self.cc_spanning
              and self.active - self.cc_spanning <= self.bonds <= 2 * self.active
              and self.checks <= self.iters <= self.limit and bool(np.isfinite(self.vals).all()))
        if ok and none:
            ok = not self.vals.any()
        elif ok:
            ok = (TOL_MIN <= self.tol <= TOL_MAX and 0.0 <= self.resinf <= self.res1
                  and self.f_in > 0.0 and self.f_out > 0.0 and self.res1 <= self.tol * min(self.f_in, self.f_out)
                  and self.cut_min <= min(self.f_in, self.f_out) and max(self.f_in, self.f_out) <= self.cut_max
                  and max(self.cut_max - self.f_out, self.f_out - self.cut_min) <= self.res1 + 64.0 * EPS * (self.active + N + 1)
                  and self.f_out <= 2.0 * self.tgt_pixels + self.res1 and self.f_in <= 2.0 * self.src_pixels + self.res1
                  and -self.res1 <= self.csum <= self.active + self.res1)
        if not ok:
            raise ValueError(f"not the words of a transport look: {dict(zip(WORDS, self.words.tolist()))}, "
                             f"{dict(zip(VALS, self.vals.tolist()))}")
        self.profile = None
        if profile is not None:
            self.profile = np.array(profile, dtype=np.float64)
            if self.profile.shape != (N + 1, 3):
                raise ValueError(f"a profile of shape {(N + 1, 3)} is needed, got {self.profile.shape}")
            pr = self.profile
            if (pr[0, 0] != self.f_in or pr[N, 0] != self.f_out or pr[:, 0].min() != self.cut_min or pr[:, 0].max() != self.cut_max
                    or pr[N, 1:].any() or pr[:, 2].sum() != self.active or pr[0, 2] != self.src_pixels
                    or pr[N - 1, 2] != self.tgt_pixels or (pr[:, 2] != np.rint(pr[:, 2])).any()
                    or abs(pr[:, 1].sum() - self.csum) > 64.0 * EPS * (self.active + N + 1)):
                raise ValueError("the profile does not fit the words and values")
        self.C = None
        if c is not None:
            self.C = np.asarray(c, dtype=np.float64)
            if self.C.shape != (N, N):
                raise ValueError(f"a map of shape {(N, N)} is needed, got {self.C.shape}")

    def _scale(self, v):
        if self.delx is None:
            raise ValueError("physical lengths need delx")
        return v * self.delx

    @property
    def percolates(self):
        """Whether a component spans from the source wall to the target wall."""
        return self.active > 0

    @property
    def deff(self):
        """D_eff / D_0: the mean of F_in and F_out (0 when not percolating)."""
        return 0.5 * (self.f_in + self.f_out)

    @property
    def deff_bound(self):
        """RES1: the certified bound of |F_in - F*| and |F_out - F*|, hence of ``deff``."""
        return self.res1

    @property
    def formation_factor(self):
        """1 / deff (inf when not percolating)."""
        return 1.0 / self.deff if self.percolates else float('inf')

    @property
    def porosity(self):
        """FG / N^2."""
        return self.fg / (self.N * self.N)

    @property
    def tortuosity_factor(self):
        """porosity / deff: at least 1 (inf when not percolating)."""
        return self.porosity / self.deff if self.percolates else float('inf')

    @property
    def active_fraction(self):
        """ACTIVE / FG: the part of the phase that belongs to a spanning component (0 without foreground)."""
        return self.active / self.fg if self.fg else 0.0

    @property
    def conservation(self):
        """CUT_MAX - CUT_MIN: how far the flux through the N + 1 faces is from constant; at most 2 RES1."""
        return self.cut_max - self.cut_min

    def flux_profile(self):
        """float [N+1]: cut[k], the flux through the face between depth k-1 and depth k."""
        if self.profile is None:
            raise ValueError("the flux profile needs the profile")
        return self.profile[:, 0].copy()

    def mean_c_profile(self):
        """float [N]: the mean of c over the active pixels of depth k; nan where there is none."""
        if self.profile is None:
            raise ValueError("the concentration profile needs the profile")
        with np.errstate(divide='ignore', invalid='ignore'):
            out = self.profile[:self.N, 1] / self.profile[:self.N, 2]
        out[self.profile[:self.N, 2] == 0] = np.nan
        return out

    def depth_phys(self):
        """float [N]: the depths of the pixel centres, (k + 1/2) delx, in the solver's unit."""
        return self._scale(np.arange(self.N, dtype=np.float64) + 0.5)

    def face_phys(self):
        """float [N+1]: the depths of the faces of `flux_profile`, k delx, in the solver's unit."""
        return self._scale(np.arange(self.N + 1, dtype=np.float64))

    def __repr__(self):
        return (f"Transport(N={self.N}, threshold={self.threshold!r}, side={self.side!r}, source={self.source!r}, fg={self.fg}, "
                f"active={self.active}, percolates={self.percolates}, deff={self.deff:.6g} +- {self.deff_bound:.2g}, "
                f"tortuosity_factor={self.tortuosity_factor:.4f}, iters={self.iters})")
