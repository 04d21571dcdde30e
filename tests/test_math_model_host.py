"""The exact-fma model of the fp64 pointwise chains (oracle/math_model.py) held to numpy.longdouble; no GPU.
tests/test_gpu_math.py then holds the device to the model bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import math_points as mp
from oracle import math_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_table_has_129_rows():
    assert len(mm.TAB) == 129 == len(mm.table())
    assert mm.TAB[0] == (2.0, float.fromhex('-0x1.62e42fefa39efp-1')) and mm.TAB[128] == (1.0, 0.0)
    for i, (rc, lc) in enumerate(mm.TAB, start=128):
        assert rc == 256.0 / i


def test_table_entries_are_their_definition():
    """Every entry of chs_log_table.h, bit for bit, is {fl(256/i), fl(-log fl(256/i))} with the log taken in longdouble:
    an lc off in its last digit fails here (the model and the device read the same header, so their agreement says
    nothing about it; tests/test_gpu_math.py runs the model on this reference table for the same reason).  The
    longdouble log is far enough from every tie of the double grid for the rounding to be the exact value's."""
    ref = mp.reference_table()
    assert len(ref) == 129
    for i, (have, want) in enumerate(zip(mm.TAB, ref), start=128):
        assert have[0].hex() == want[0].hex() and have[1].hex() == want[1].hex(), (i, have, want)
    rc = np.array([r for r, _ in ref], dtype=LD)
    exact = -np.log(rc[:-1])
    lc = np.array([l for _, l in ref[:-1]])
    frac = np.abs(np.abs(exact - lc.astype(LD)) / np.spacing(lc).astype(LD) - 0.5)   # distance from a tie, in ulp
    assert frac.min() > 2.0 ** -9, frac.min()   # longdouble's own error is 2^-11 ulp of the double


def test_fma_is_the_rational_definition():
    """The integer fma of the model against rational arithmetic rounded once: random operands of every magnitude,
    products that cancel against the addend, ties, zeros of both signs, results that are subnormal or overflow."""
    rng = np.random.default_rng(3)
    n = 4000
    a = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    b = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    c = np.where(rng.random(n) < 0.5, -a * b * (1 + rng.integers(-4, 5, n) * 2.0 ** -52),
                 rng.standard_normal(n) * 2.0 ** rng.integers(-80, 80, n))
    cases = list(zip(a.tolist(), b.tolist(), c.tolist()))
    cases += [(1 + 2.0 ** -52, 1 + 2.0 ** -52, -1.0), (1 + 2.0 ** -30, 1 - 2.0 ** -30, -1.0), (3.0, 2.0 ** -1074, 0.0),
              (2.0 ** -600, 2.0 ** -500, 2.0 ** -1074), (0.5, 2.0 ** -1074, 2.0 ** -1074), (1.5, 2.0 ** -1073, 5e-324),
              (2.0 ** 600, 2.0 ** 500, -2.0 ** 1023), (1e300, 1e300, -1e300), (2.0 ** 1023, 2.0, -2.0 ** 1023),
              (1.0, 2.0 ** 53 + 2, 1.0), (1.0, 2.0 ** 53, 1.0), (1.0, 2.0 ** 53 + 2, -1.0), (0.1, 10.0, -1.0)]
    for x, y, z in cases:
        got, want = mm.fma(x, y, z), mm.fma_rational(x, y, z)
        assert got == want, (x, y, z, got, want)
    assert mm.fma(2.0 ** 600, 2.0 ** 500, -2.0 ** 1023) == math.inf and mm.fma(0.5, 2.0 ** -1074, 2.0 ** -1074) == 2.0 ** -1073
    # exact zeros carry IEEE's sign; non-finite operands follow IEEE
    assert math.copysign(1, mm.fma(1.0, -0.0, -0.0)) == -1 and math.copysign(1, mm.fma(2.0, 3.0, -6.0)) == 1
    assert math.isnan(mm.fma(math.nan, 1.0, 1.0)) and mm.fma(math.inf, 1.0, 1.0) == math.inf


def test_model_log_within_2_ulp():
    """"2.0 ulp in the CPU model", measured like test_log_unit_table_accuracy measures the device (the
    longdouble log rounded to double; the error in its ulp): held on that test's whole point set, 9.5e5 points."""
    x = mp.log_unit_table_points()
    got = np.array([mm.log_unit_tab(v) for v in x.tolist()])
    ref = np.log(np.asarray(x, dtype=LD)).astype(np.float64)
    ok = ref != 0
    e = np.abs(got[ok] - ref[ok]) / np.spacing(np.abs(ref[ok]))
    assert e.max() <= 2.0, (e.max(), x[ok][np.argmax(e)])
    assert np.all(got[x == 1.0] == 0.0)
    # against the unrounded longdouble value the same points stay inside the device test's 2.5 ulp
    assert mp.ulp_err(got[ok], np.log(np.asarray(x, dtype=LD))[ok]).max() <= 2.5


def test_model_log_poly_and_division_tails():
    """chs_log_poly is 2 atanh(s) to the 6e-18 the header states plus its rounding, and both division tails turn a
    reciprocal seed of 2^-20 relative error (the hardware's is better) into a quotient under 1 ulp."""
    rng = np.random.default_rng(8)
    s = rng.uniform(-0.1716, 0.1716, 3000)
    got = np.array([mm.log_poly(float(v)) for v in s])
    ref = 2 * np.arctanh(np.asarray(s, dtype=LD))
    assert mp.ulp_err(got, ref).max() < 1.5
    sig = np.concatenate([rng.uniform(0.5, 4, 1500), 1 + 10.0 ** rng.uniform(-6, 9, 1500)])
    d = rng.standard_normal(3000) * 2.0 ** rng.integers(-60, 60, 3000)
    seed = (1 / sig) * (1 + rng.uniform(-1, 1, 3000) * 2.0 ** -20)
    for tail in (mm.div_pos_tail, mm.div_pos1_tail):
        q = np.array([tail(float(a), float(b), float(r)) for a, b, r in zip(d, sig, seed)])
        assert mp.ulp_err(q, np.asarray(d, dtype=LD) / np.asarray(sig, dtype=LD)).max() < 1.0


@pytest.mark.parametrize("sE0", [0.0, -1234.5678])
def test_model_energy_mu_against_literal(sE0):
    """E and mu as chs_energy_mu_from_logs forms them, against the literal reference expressions (solver.py:166-175,
    218-221) in longdouble from the SAME U, Uinv, lU, lV: |got - exact| <= k u S with k and S of math_points.py."""
    U = mp.field_points(600)
    Uinv = 1 - U
    kc = mp.physics_consts(sE0)
    k = mm.pw_consts(mp.oracle())
    lU = np.array([mm.log_unit_tab(float(v)) for v in U])
    lV = np.array([mm.log_unit_tab(float(v)) for v in Uinv])
    got = np.array([mm.energy_mu_from_logs(float(u), float(v), float(a), float(b), k, sE0)
                    for u, v, a, b in zip(U, Uinv, lU, lV)])
    E, _ = mp.energy_literal(U, Uinv, lU, lV, kc)
    M, _ = mp.mu_literal(U, Uinv, lU, lV, kc)
    eE = np.abs(got[:, 0].astype(LD) - (E + LD(sE0)))
    eM = np.abs(got[:, 1].astype(LD) - M)
    bE = mp.bound(mp.K_ENERGY_SHARED, mp.energy_shared_S(U, Uinv, lU, lV, kc, sE0))
    bM = mp.bound(mp.K_MU_SHARED, mp.mu_shared_S(U, Uinv, lU, lV, kc))
    assert np.all(eE <= bE), (float((eE / bE).max()), U[np.argmax(eE / bE)])
    assert np.all(eM <= bM), (float((eM / bM).max()), U[np.argmax(eM / bM)])
    assert (eE / bE).max() > 0.02 and (eM / bM).max() > 0.02   # the bound is of the error's size, not a blanket


def test_model_forms_agree_bitwise():
    """<true,false> and <false,true> give the bits of <true,true> for the output they compute, and leave the other"""
    U = mp.field_points(300)
    k = mm.pw_consts(mp.oracle())
    for u in U.tolist():
        v = 1.0 - u
        lU, lV = mm.log_unit_tab(u), mm.log_unit_tab(v)
        both = mm.energy_mu_from_logs(u, v, lU, lV, k, 7.25)
        e = mm.energy_mu_from_logs(u, v, lU, lV, k, 7.25, want_mu=False)
        m = mm.energy_mu_from_logs(u, v, lU, lV, k, 7.25, energy=False)
        assert e == (both[0], 0.0) and m == (7.25, both[1])
        assert mm.kernel_chain(u, k, 7.25) == both


def test_tool_prints_the_recorded_margins():
    """tools/row_arith_model.py on the shared model prints, to the character, what profiles/row_arith_parity_margins.txt
    records of it (the run with 4096 points)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'row_arith_model.py'), '4096'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    recorded = open(os.path.join(ROOT, 'profiles', 'row_arith_parity_margins.txt')).read().splitlines()
    at = next(i for i, line in enumerate(recorded) if line.startswith('CPU model, tools/row_arith_model.py 4096'))
    assert r.stdout.splitlines() == recorded[at + 1:at + 4]
