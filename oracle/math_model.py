"""Executable model of the explicit-fma fp64 chains of chsimpy_amd/csrc/chs_math.h, operation by operation as the
header writes them, with an exact fused multiply-add (the exact value of a*b + c, rounded once).  No GPU needed.

Modelled: chs_log_unit_tab_f64, chs_log_poly, the fma tails of chs_div_pos / chs_div_pos1 (the hardware reciprocal is an
input), chs_pw_consts, the three forms of chs_energy_mu_from_logs, and the chain of the fused row kernel
(u -> 1 - u -> two table logs -> chs_energy_mu_from_logs).  tools/row_arith_model.py prints its margins against the
oracle's expressions; tests/test_math_model_host.py and tests/test_gpu_math.py hold the model and the device to it."""
import math
import os
import re
import struct
from fractions import Fraction

LN2 = 0.6931471805599453
DOM_MAX = 0x100FFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TWO53 = 9007199254740992.0
_MIN_NORMAL = 2.2250738585072014e-308


def fma_rational(a, b, c):
    """The definition: rational arithmetic, rounded once (finite operands)."""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    try:
        return float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf


def _split(x):
    """x = n * 2**e exactly, n an integer"""
    m, e = math.frexp(x)
    return int(m * _TWO53), e - 53


def fma(a, b, c):
    """a*b + c rounded once.  Integer arithmetic on the significands (int -> float rounds to nearest even); a result
    that is zero, subnormal or out of range takes the rational definition, where a second rounding could slip in."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    na, ea = _split(a)
    nb, eb = _split(b)
    nc, ec = _split(c)
    n, e = na * nb, ea + eb
    if nc:
        if e >= ec:
            n, e = (n << (e - ec)) + nc, ec
        else:
            n += nc << (ec - e)
    if n == 0:
        return a * b + c   # an exact zero: a*b is then exactly -c (or both are zero), so the plain sum has IEEE's sign
    try:
        r = math.ldexp(float(n), e)
    except OverflowError:
        return fma_rational(a, b, c)
    if abs(r) < _MIN_NORMAL or math.isinf(r):
        return fma_rational(a, b, c)
    return r


def table():
    txt = open(os.path.join(ROOT, 'chsimpy_amd', 'csrc', 'chs_log_table.h')).read()
    rows = re.findall(r'\{(-?0x[0-9a-f.]+p[+-]\d+), (-?0x[0-9a-f.]+p[+-]\d+)\}', txt)
    assert len(rows) == 129
    return [(float.fromhex(a), float.fromhex(b)) for a, b in rows]


TAB = table()


def log_unit_tab(x, tab=None):
    """chs_log_unit_tab_f64 for finite x > 0; `tab`: the table to read instead of the header's (the tests pass one
    computed from the table's definition, so that the device is held to more than its own copy)"""
    m, e = math.frexp(x)
    hi = struct.unpack('<II', struct.pack('<d', m))[1]
    w = (hi - (0x3FE00000 - 0x1000)) & 0xFFFFFFFF
    assert w <= DOM_MAX
    rc, lc = (tab or TAB)[min(w, DOM_MAX) >> 13]
    r = fma(m, rc, -1.0)
    p = fma(r, -1.0 / 6.0, 1.0 / 5.0)
    p = fma(r, p, -1.0 / 4.0)
    p = fma(r, p, 1.0 / 3.0)
    p = fma(r, p, -0.5)
    q = fma(r, p, 1.0)
    return fma(r, q, fma(float(e), LN2, lc))


def log_poly(s):
    """chs_log_poly: s -> 2 atanh(s)"""
    z = s * s
    p = 0.1467141530063111
    p = fma(p, z, 0.15327184863231447)
    p = fma(p, z, 0.18183028385247743)
    p = fma(p, z, 0.22222209184316374)
    p = fma(p, z, 0.2857142863817006)
    p = fma(p, z, 0.3999999999987206)
    p = fma(p, z, 0.6666666666666671)
    return fma(s * z, p, s + s)


def div_pos_tail(d, sig, r):
    """chs_div_pos behind its reciprocal seed r = rcp(sig): two Newton steps and the residual correction"""
    e = fma(-sig, r, 1.0)
    r = fma(r, e, r)
    e = fma(-sig, r, 1.0)
    r = fma(r, e, r)
    q = d * r
    rho = fma(-sig, q, d)
    return fma(rho, r, q)


def div_pos1_tail(d, sig, r):
    """chs_div_pos1 behind its reciprocal seed: one Newton step and the residual correction"""
    e = fma(-sig, r, 1.0)
    r = fma(r, e, r)
    q = d * r
    rho = fma(-sig, q, d)
    return fma(rho, r, q)


class PwConsts:
    """chs_pw_consts"""

    def __init__(self, RT, B, BRT, A0, A1):
        self.RT, self.A0, self.A1 = RT, A0, A1
        self.A1h = 1.5 * A1
        self.nRTB = -(RT * B)
        self.c0 = -(BRT + 0.5 * A1)


def pw_consts(o):
    """the constants of an OracleSolver"""
    return PwConsts(o.RT, o.params.B, o.BRT, o.A0, o.A1)


def energy_mu_from_logs(U, Uinv, lU, lV, k, sE=0.0, mu=0.0, energy=True, want_mu=True):
    """chs_energy_mu_from_logs<energy, want_mu>: (sE, mu) after the call; what a form does not compute stays"""
    V2 = Uinv - U
    d = lU - lV
    if energy:
        g = fma(k.A1, V2, k.A0)
        t = fma(g, Uinv, k.nRTB)
        s = fma(U, d, lV)
        sE = fma(k.RT, s, sE)
        sE = fma(U, t, sE)
    if want_mu:
        h = fma(k.A1h, V2, k.A0)
        m = fma(k.RT, d, k.c0)
        mu = fma(V2, h, m)
    return sE, mu


def kernel_chain(u, k, sE=0.0, tab=None):
    """One grid point of the fused fp64 row kernel: u -> uinv = 1 - u -> two table logs -> chs_energy_mu_from_logs"""
    uinv = 1.0 - u
    return energy_mu_from_logs(u, uinv, log_unit_tab(u, tab), log_unit_tab(uinv, tab), k, sE)


def energy_mu(U, o):
    """(E, mu) of one point as chs_energy_mu_from_logs<true, true> forms them (E: the two fmas onto a zero sum)."""
    return kernel_chain(U, pw_consts(o))
