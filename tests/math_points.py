"""Point sets, literal references and derived error bounds shared by tests/test_math_model_host.py (the exact-fma model,
no GPU) and tests/test_gpu_math.py (the device functions of chsimpy_amd/csrc/chs_math.h).

Error bounds of the pure arithmetic chains.  A chain of +, -, * and fma in round-to-nearest returns the exact value of
its expression with every input perturbed by at most (1 + u)^k, k the number of ROUNDED operations on the longest path
from an input to the result (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 ff.; an fma is one
rounding, so a contraction only lowers k).  Hence

    |got - exact| <= (k + L) * u * S,    u = 2^-53 (fp64) or 2^-24 (fp32),

where S -- "the sum of absolute terms" -- is the same expression with every operand and every operation replaced by its
absolute value (Uinv - U becomes Uinv + U), evaluated in numpy.longdouble from the same inputs, and L * u * S' accounts
for a logarithm that is not an input: L its relative error in units of u and S' its term in S.  The bound is relative
to S, not to the result: mu and E cross zero inside the point sets.  `slack` = 1 + 2^-8 covers the second-order terms
of (1 + u)^k and the roundings of the longdouble reference itself (u_longdouble = 2^-64 = 2^-11 u, a dozen of them).
An operation whose result is denormal errs by up to half a step of the denormal grid instead: `bound` adds those.
"""
import functools

import numpy as np

from oracle import chs_oracle as orc

LD = np.longdouble
U64, U32 = 2.0 ** -53, 2.0 ** -24
SLACK = 1 + 2.0 ** -8


@functools.lru_cache(maxsize=None)
def oracle():
    return orc.OracleSolver(orc.make_params(64, 2))


def physics_consts(sE0=0.0):
    """consts of the hook's physics codes: RT, B, BRT, A0, A1, sE0"""
    o = oracle()
    return (o.RT, o.params.B, o.BRT, o.A0, o.A1, sE0)


@functools.lru_cache(maxsize=None)
def reference_table():
    """The log table by its definition (chs_math.h, tools/log_table.py), without reading chs_log_table.h:
    {rc_i, lc_i} = {fl(256/i), fl(-log rc_i)}, i = 128..256, the log in longdouble (its 11 spare bits leave no entry
    near enough to a tie of the double grid to round differently: tests/test_math_model_host.py)."""
    rc = 256.0 / np.arange(128, 257)
    lc = (-np.log(rc.astype(LD))).astype(np.float64) + 0.0     # (+ 0.0: the last entry is +0, as the header has it)
    return tuple(zip(rc.tolist(), lc.tolist()))


def _specials():
    grid = np.arange(128, 257) / 256.0
    mid = (np.arange(128, 256) + 0.5) / 256.0
    p2 = 2.0 ** -np.arange(1.0, 1075.0, 7.0)      # down through the denormals
    return np.concatenate([
        grid, np.nextafter(grid, 0), np.nextafter(grid, 2), mid, np.nextafter(mid, 0), np.nextafter(mid, 2),
        grid / 2, mid / 2, np.nextafter(mid / 2, 0), np.nextafter(mid / 2, 2),   # the same nodes one binade down (U < 1/2)
        p2, np.nextafter(p2, 0), np.nextafter(p2, 2),
        [2.2250738585072014e-308, 5e-324, 1e-310, 1e-320, 2.2250738585072009e-308]])


@functools.lru_cache(maxsize=None)
def unit_points(n, seed=11):
    """Arguments in (0, 1] of the logs, `n` random points per family: uniform, 1 - 1e-3 r, 1 - 1e-9 r, 1e-6 r,
    exp(uniform(-700, 0)), the ramp 1e-6 .. 1-1e-6, the band 0.875 +- 0.01, 0.5 +- 1e-3, then the table nodes i/256,
    the midpoints and their neighbours, powers of two and their neighbours, the smallest normal and denormals."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([
        rng.random(n), 1 - rng.random(n) * 1e-3, 1 - rng.random(n) * 1e-9, rng.random(n) * 1e-6,
        np.exp(rng.uniform(-700, 0, n)), np.linspace(1e-6, 1 - 1e-6, n) + rng.uniform(-5e-7, 5e-7, n),
        0.875 + rng.uniform(-0.01, 0.01, n), 0.5 + rng.uniform(-1e-3, 1e-3, n), _specials()])
    x = np.unique(x[(x > 0) & (x <= 1)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def field_points(n, seed=11):
    """Field values U with 0 < U < 1 and fl(1 - U) > 0 (it is 1 for U < 2^-54): unit_points and their mirror images"""
    x = unit_points(n, seed)
    U = np.unique(np.concatenate([x, 1 - x]))
    U = U[(U > 0) & (U < 1) & (1 - U > 0)]
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def field_points_f32(n, seed=11):
    """The same values rounded to float; duplicates and what rounds to 0 or 1 (or whose 1 - U does) dropped"""
    with np.errstate(under='ignore'):
        U = np.unique(field_points(n, seed).astype(np.float32))
    V = np.float32(1) - U
    U = U[(U > 0) & (U < 1) & (V > 0) & (V < 1) & (U >= np.finfo(np.float32).tiny)]
    U.setflags(write=False)
    return U


def log_unit_table_points():
    """The point set of test_log_unit_table_accuracy (tests/test_gpu_math.py builds its own there, as it always has:
    the two are the same seeded recipe)"""
    k = int
    rng = np.random.default_rng(5)
    grid = np.arange(128, 257) / 256.0
    x = np.concatenate([rng.random(k(400000)), 1 - rng.random(k(100000)) * 1e-3, 1 - rng.random(k(50000)) * 1e-9,
                        np.exp(rng.uniform(-700, 0, k(100000))), np.linspace(0.70, 0.72, k(50000) + 1),
                        np.linspace(0.49, 0.51, k(50000) + 1), np.linspace(0.99, 1.0, k(200000) + 1), grid,
                        (grid[:-1] + 0.5 / 256.0), np.nextafter(grid[:-1] + 0.5 / 256.0, 0),
                        2.0 ** -np.arange(1, 1000, 7.0), np.nextafter(2.0 ** -np.arange(1, 1000, 7.0), 0)])
    return x[(x > 0) & (x <= 1)]


def ulp_err(got, ref, dtype=np.float64):
    """|got - ref| in units of the spacing of `dtype` at ref; `ref` may be longdouble (it is not rounded first)"""
    ref = np.asarray(ref, dtype=LD)
    unit = np.spacing(np.abs(ref.astype(dtype))).astype(LD)
    return (np.abs(np.asarray(got, dtype=LD) - ref) / unit).astype(np.float64)


# ---------------------------------------------------------------------------
# literal reference expressions (solver.py:166-175, 218-221) in longdouble, and their sums of absolute terms
# ---------------------------------------------------------------------------
def energy_literal(U, Uinv, lU, lV, k):
    """RT*(U*(lU - B) + Uinv*lV) + (A0 + A1*(Uinv - U))*U*Uinv and its S"""
    RT, B, _, A0, A1 = (LD(v) for v in k[:5])
    U, Uinv, lU, lV = (np.asarray(v, dtype=LD) for v in (U, Uinv, lU, lV))
    val = RT * (U * (lU - B) + Uinv * lV) + (A0 + A1 * (Uinv - U)) * U * Uinv
    S = abs(RT) * (U * (np.abs(lU) + abs(B)) + Uinv * np.abs(lV)) + (abs(A0) + abs(A1) * (Uinv + U)) * U * Uinv
    return val, S


def mu_literal(U, Uinv, lU, lV, k):
    """RT*(lU - lV) - BRT + (A0 + A1*(Uinv - U))*(Uinv - U) - 2*A1*U*Uinv and its S"""
    RT, _, BRT, A0, A1 = (LD(v) for v in k[:5])
    U, Uinv, lU, lV = (np.asarray(v, dtype=LD) for v in (U, Uinv, lU, lV))
    V2 = Uinv - U
    val = RT * (lU - lV) - BRT + (A0 + A1 * V2) * V2 - 2 * A1 * U * Uinv
    S = abs(RT) * (np.abs(lU) + np.abs(lV)) + abs(BRT) + (abs(A0) + abs(A1) * (Uinv + U)) * (Uinv + U) + 2 * abs(A1) * U * Uinv
    return val, S


# k of the literal chains (chs_energy_from_logs, chs_mu_from_logs and their _fast forms; a contraction lowers it):
#   energy: Uinv-U, A1*, A0+, *U, *Uinv, the last + : 6      mu: U2inv, A1*, A0+, *U2inv, (..)+t2, -t3 : 6
K_ENERGY_LITERAL = 6
K_MU_LITERAL = 6

# chs_energy_mu_from_logs forms   sE0 + RT*(lV + U*d) + U*((A0 + A1*V2)*Uinv - RT*B)   and
#                                 V2*(A0 + A1h*V2) + (RT*d + c0),  A1h = fl(3/2 A1), c0 = -fl(BRT + A1/2):
#   energy: d, s, the fma onto sE, the second fma (or V2, g, t, the second fma): 4
#   mu:     V2 (or A1h), h, the last fma (or d, m, the last fma): 3
# Both are the literal expressions only where U + Uinv = 1 exactly; Uinv = fl(1 - U) misses that by at most u/2 (and by
# nothing for U >= 1/2), which moves E by RT*|lV|*u/2 and mu by |A1|*u/2 (1 + u): one more unit of k each.
K_ENERGY_SHARED = 4 + 1
K_MU_SHARED = 3 + 1


def energy_shared_S(U, Uinv, lU, lV, k, sE0=0.0):
    RT, B, _, A0, A1 = (LD(v) for v in k[:5])
    U, Uinv, lU, lV = (np.asarray(v, dtype=LD) for v in (U, Uinv, lU, lV))
    return abs(LD(sE0)) + abs(RT) * (np.abs(lV) + U * (np.abs(lU) + np.abs(lV))) + U * ((abs(A0) + abs(A1) * (Uinv + U)) * Uinv + abs(RT * B))


def mu_shared_S(U, Uinv, lU, lV, k):
    RT, _, BRT, A0, A1 = (LD(v) for v in k[:5])
    U, Uinv, lU, lV = (np.asarray(v, dtype=LD) for v in (U, Uinv, lU, lV))
    return (Uinv + U) * (abs(A0) + 1.5 * abs(A1) * (Uinv + U)) + abs(RT) * (np.abs(lU) + np.abs(lV)) + abs(BRT) + abs(A1) / 2


def bound(k, S, u=U64):
    """k u S, plus 8 k half-steps of the denormal grid: where an operation underflows its error is absolute, and what
    follows it multiplies by RT < 8 at the most (every other later factor is U, Uinv <= 1)"""
    eta = LD(2.0) ** (-1075 if u == U64 else -150)
    return (k * u * SLACK) * np.asarray(S, dtype=LD) + 8 * k * eta
