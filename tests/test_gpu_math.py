"""GPU tests of the device math primitives (chsimpy_amd/csrc/chs_math.h) against numpy."""
import functools
import os

import numpy as np
import pytest

import math_points as mp
from chsimpy_amd import _lib
from gpu_helpers import GOLD, log_line
from oracle import chs_oracle as orc
from oracle import math_model as mm

pytestmark = pytest.mark.gpu


def ulp_err(got, ref):
    return np.abs(got - ref) / np.spacing(np.abs(ref))


def test_log_accuracy(gpu):
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.random(200000), 1 - rng.random(200000) * 1e-3, rng.random(50000) * 1e-6,
                        np.exp(rng.uniform(-700, 700, 100000)), np.linspace(0.70, 0.72, 50001),
                        np.linspace(0.999, 1.001, 50001), [0.5, 1.0, 2.0, 0.875, 0.125]])
    got = _lib.test_math(0, x)
    ref = np.log(np.asarray(x, dtype=np.longdouble)).astype(np.float64)
    ok = ref != 0
    e = ulp_err(got[ok], ref[ok])
    assert e.max() <= 2.5, e.max()
    assert got[x == 1.0].tolist() == [0.0] * int((x == 1.0).sum())
    # domain: numpy semantics
    sp = _lib.test_math(0, np.array([0.0, -1.0, np.inf, np.nan]))
    assert sp[0] == -np.inf and np.isnan(sp[1]) and sp[2] == np.inf and np.isnan(sp[3])


def test_log_pos_accuracy(gpu):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.random(300000), 1 - rng.random(100000) * 1e-3, np.exp(rng.uniform(-700, 700, 100000)),
                        np.linspace(0.70, 0.72, 50001), np.linspace(0.999, 1.001, 50001)])
    x = x[x > 0]
    got = _lib.test_math(4, x)
    ref = np.log(np.asarray(x, dtype=np.longdouble)).astype(np.float64)
    ok = ref != 0
    assert ulp_err(got[ok], ref[ok]).max() <= 2.5


def test_log_unit_table_accuracy(gpu):
    """The table-driven log (no division, no selects) of the fused row kernel's pointwise part,
    chs_log_unit_tab_f64: the kernel only ever asks for log U and log(1-U) with U in (0,1)."""
    rng = np.random.default_rng(5)
    grid = np.arange(128, 257) / 256.0
    # (tests/math_points.py: log_unit_table_points builds the same set for the CPU model)
    x = np.concatenate([rng.random(400000), 1 - rng.random(100000) * 1e-3, 1 - rng.random(50000) * 1e-9,
                        np.exp(rng.uniform(-700, 0, 100000)), np.linspace(0.70, 0.72, 50001),
                        np.linspace(0.49, 0.51, 50001), np.linspace(0.99, 1.0, 200001), grid,
                        (grid[:-1] + 0.5 / 256.0), np.nextafter(grid[:-1] + 0.5 / 256.0, 0),
                        2.0 ** -np.arange(1, 1000, 7.0), np.nextafter(2.0 ** -np.arange(1, 1000, 7.0), 0)])
    x = x[(x > 0) & (x <= 1)]
    got = _lib.test_math(5, x)
    ref = np.log(np.asarray(x, dtype=np.longdouble)).astype(np.float64)
    ok = ref != 0
    e = ulp_err(got[ok], ref[ok])
    assert e.max() <= 2.5, (e.max(), x[ok][np.argmax(e)])
    assert np.all(got[x == 1.0] == 0.0)
    # x > 1 (never asked for by the timestep): e ln2 and the table term cancel, the absolute error stays small
    y = np.concatenate([1 + rng.random(100000), np.exp(rng.uniform(0, 700, 100000))])
    goty = _lib.test_math(5, y)
    refy = np.log(np.asarray(y, dtype=np.longdouble)).astype(np.float64)
    assert np.max(np.abs(goty - refy) / np.maximum(1.0, np.abs(refy))) < 4e-16
    # domain: the table index flags x <= 0 (the row kernel poisons its sums then); NaN and inf propagate
    sp = _lib.test_math(5, np.array([0.0, -0.0, -1.0, -1e-300, -np.inf, np.nan, np.inf]))
    assert np.all(np.isnan(sp[:6])) and not np.isfinite(sp[6])
    assert np.all(np.isfinite(_lib.test_math(5, np.array([5e-324, 1e-310, 2.2250738585072014e-308]))))  # denormals are fine


def test_log_ratio_accuracy(gpu):
    rng = np.random.default_rng(1)
    U = np.concatenate([rng.uniform(0.5, 1 - 1e-9, 300000), rng.uniform(1e-9, 0.5, 300000),
                        rng.uniform(0.86, 0.89, 100000), rng.uniform(0.499, 0.501, 100000)])
    Uinv = 1 - U
    got = _lib.test_math(1, U, Uinv)
    # log(U/Uinv) = log1p((U-Uinv)/Uinv): the difference is exact in extended precision, so the
    # reference stays accurate where the quotient is close to 1
    Ul, Il = np.asarray(U, dtype=np.longdouble), np.asarray(Uinv, dtype=np.longdouble)
    near1 = np.abs(np.asarray(U) - 0.5) < 0.1
    ref = np.where(near1, np.log1p((Ul - Il) / Il), np.log(Ul / Il)).astype(np.float64)
    ok = np.abs(ref) > 1e-300
    e = ulp_err(got[ok], ref[ok])
    assert e.max() <= 2.5, e.max()
    # numpy's own log(U/Uinv) (what the reference evaluates) agrees to a few ulp
    # (its own error is ~1 ulp of max(1, |log|) because the quotient is rounded first)
    npv = np.log(U / Uinv)
    assert np.all(np.abs(got - npv) <= 4 * np.spacing(np.maximum(np.abs(npv), 1.0)))
    sp = _lib.test_math(1, np.array([1.5, 0.0, 1.0, np.nan]), np.array([-0.5, 1.0, 0.0, 1.0]))
    assert np.all(~np.isfinite(sp))


def test_mu_and_energy_density(gpu):
    o = orc.OracleSolver(orc.make_params(64, 2))
    rng = np.random.default_rng(2)
    U = rng.uniform(0.6, 0.99, 500000)
    mu = _lib.test_math(2, U, np.array([o.RT, o.BRT, o.A0, o.A1]))
    ref = o.mu(U)
    assert np.max(np.abs(mu - ref)) < 4e-14  # |mu| ~ 100, absolute error of a few ulp of RT*log
    e = _lib.test_math(3, U, np.array([o.RT, o.params.B, o.A0, o.A1]))
    Uinv = 1 - U
    eref = o.RT * (U * (np.log(U) - o.params.B) + Uinv * np.log(Uinv)) + (o.A0 + o.A1 * (Uinv - U)) * U * Uinv
    assert np.allclose(e, eref, rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------
# Every inline function of chs_math.h through chs_test_math_cols (chsimpy_amd/_lib.py: test_math_cols), pointwise.
#   kind A: explicit-fma fp64 chains without a hardware seed    == the exact-fma model (oracle/math_model.py), bit for bit
#   kind B: contraction-off chains                               == numpy's elementwise chain in the same type, bit for bit
#   kind C: hardware seeds / contraction allowed                 error against numpy.longdouble from the same inputs:
#           a figure the source states, a running-error bound derived in tests/math_points.py, or -- where the source
#           says only "~2 ulp" / "1 ulp" of a hardware instruction -- the maximum measured on the MI355X against that
#           reference (profiles/math_pointwise.txt), rounded up to the next half ulp, plus one ulp for the seeds of
#           the points not sampled.
# ---------------------------------------------------------------------------
LD = np.longdouble
F32 = np.float32
N_MODEL = 1000      # random points per family where the Python model is the reference (~2e4 points in all)
N_WIDE = 40000      # ... where numpy is (~7e5 points, one launch)
SE0 = -1234.5678    # the running energy sum the point is added to

# Measured on the MI355X (profiles/math_pointwise.txt: `python -m pytest -m gpu tests/test_gpu_math.py`, the lines
# "math pointwise: ... max" of the parity log); asserted: the measured maximum rounded up to the next half ulp + 1 ulp.
MEASURED_ULP = {
    'chs_dt_integrand_fast(double)': 2.5913,   # asserted: 4.0
    'chs_dt_integrand_fast(float)': 2.0542,    # asserted: 3.5
    'chs_logf': 1.9166,                        # asserted: 3.0
    'chs_log_ratio<float>': 2.2600,            # asserted: 3.5  (ulp of max(|log|, 1))
}


def measured_bound(name):
    m = MEASURED_ULP[name]
    return np.ceil(m * 2) / 2 + 1.0


def check_measured(name, err, where):
    i = int(np.argmax(err))
    log_line(f"math pointwise: {name}: {err.size} points, max {err[i]:.4f} ulp at {where[i]!r}")
    print(f"math pointwise: {name}: {err.size} points, max {err[i]:.4f} ulp at {where[i]!r}")
    assert err[i] <= measured_bound(name), (name, err[i], where[i])


def assert_bits(got, want, what, *inputs):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        first = [(tuple(float(c[i]).hex() for c in inputs), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]
        raise AssertionError(f"{what}: {bad.size} of {got.size} points differ; (inputs, device, reference): {first}")


def f32cols(*cols):
    return [np.asarray(c, dtype=F32) for c in cols]


@functools.lru_cache(maxsize=None)
def model_points():
    """U, Uinv and the model's lU, lV, (sE, mu) of the kernel's chain onto SE0: computed once, shared, read-only.
    The model reads the table by its definition (math_points.reference_table), not the header the device compiles."""
    U = mp.field_points(N_MODEL)
    Uinv = 1 - U
    k = mm.pw_consts(mp.oracle())
    tab = mp.reference_table()
    lU = np.array([mm.log_unit_tab(v, tab) for v in U.tolist()])
    lV = np.array([mm.log_unit_tab(v, tab) for v in Uinv.tolist()])
    em = np.array([mm.energy_mu_from_logs(u, v, a, b, k, SE0) for u, v, a, b in zip(U.tolist(), Uinv.tolist(), lU.tolist(), lV.tolist())])
    out = (U, Uinv, lU, lV, em[:, 0].copy(), em[:, 1].copy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wide_points():
    """U, Uinv = fl(1 - U) and numpy's logs of both (inputs of the from-logs functions), fp64 and fp32"""
    U = mp.field_points(N_WIDE)
    Uinv = 1 - U
    Uf = mp.field_points_f32(N_WIDE)
    Vf = F32(1) - Uf
    out = (U, Uinv, np.log(U), np.log(Uinv), Uf, Vf, np.log(Uf), np.log(Vf))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mu_points():
    """Arguments of the adaptive-step integrand: 0, +-1e-8, +-1, +-1e4, +-1e8, the band of |mu| the oracle's first 600
    adaptive steps at N = 64 show (tests/golden/n64_adaptive_600.npz: pointwise over its final field, and the root mean
    square N * L2 of every recorded step), log-uniform over that band and over 1e-8 .. 1e8, both signs."""
    g = np.load(os.path.join(GOLD, 'n64_adaptive_600.npz'))
    pw = np.abs(mp.oracle().mu(g['U_final']))
    rms = g['timedata'][1:, 6] * 64
    lo, hi = min(pw[pw > 0].min(), rms[rms > 0].min()), max(pw.max(), rms.max())
    rng = np.random.default_rng(21)
    band = np.exp(rng.uniform(np.log(lo), np.log(hi), 100000))
    sweep = 10.0 ** rng.uniform(-8, 8, 100000)
    m = np.concatenate([[0.0, 1e-8, 1.0, 1e4, 1e8, lo, hi], band, sweep, pw.ravel()])
    m = np.concatenate([m, -m])
    m.setflags(write=False)
    return m


DELT_MAX = 9e-8   # OracleParams.delt_max


def dt_exact(mu, dmax):
    mu = np.asarray(mu, dtype=LD)
    return LD(dmax) / np.sqrt(1 + LD(62.5) * mu * mu)


@functools.lru_cache(maxsize=None)
def spectral_points():
    """(li, lj, lam1, lam2) of every kind of coefficient the spectral update meets at N = 4096, 8192, 16384: the four
    corners and 10^4 random (i, j) per N and per time step -- the default delt and the largest the adaptive rule can
    reach, N * delt_max (np.linalg.norm(.., ord=-1) is a column sum of N integrands <= delt_max) -- with lam, lam1,
    lam2 by the oracle's formulas (chs_oracle.eigenvalues, get_coefficients)."""
    o = mp.oracle()
    rng = np.random.default_rng(31)
    cols = []
    for N in (4096, 8192, 16384):
        lam = 2 * np.cos(np.pi * np.arange(0, N) / (N - 1)) - 2
        delx2 = (o.params.L / (N - 1)) ** 2
        i = np.concatenate([[0, 0, N - 1, N - 1], rng.integers(0, N, 10000)])
        j = np.concatenate([[0, N - 1, 0, N - 1], rng.integers(0, N, 10000)])
        for delt in (o.params.delt, N * o.params.delt_max):
            lam1 = delt / delx2
            lam2 = o.kappa_tilde * lam1 / delx2
            cols.append(np.stack([lam[i], lam[j], np.full(i.size, lam1), np.full(i.size, lam2)]))
    out = np.concatenate(cols, axis=1)
    out.setflags(write=False)
    return out


def cheig_of(sp):
    leig = sp[0] + sp[1]
    return 1.0 + (sp[3] * leig) * leig


# ------------------------------------------------------------------ kind A
def test_table_log_bits_of_the_model(gpu):
    """chs_log_unit_tab_f64 == the exact-fma model on every point (today's test of code 5 bounds it by 2.5 ulp only);
    the domain word flags none of them.  The model reads {fl(256/i), fl(-log fl(256/i))} computed here from the
    definition, not chs_log_table.h: a table entry off in its last digit shows at its node and around it."""
    x = mp.unit_points(2 * N_MODEL)
    got, dom = _lib.test_math_cols(_lib.MATH_LOG_TAB, [x])
    tab = mp.reference_table()
    want = np.array([mm.log_unit_tab(v, tab) for v in x.tolist()])
    assert_bits(got, want, 'chs_log_unit_tab_f64', x)
    assert not dom.any()
    assert_bits(_lib.test_math(5, x), want, 'chs_test_math code 5', x)


@pytest.mark.parametrize("code,energy,want_mu", [(_lib.MATH_EMU_BOTH, True, True), (_lib.MATH_EMU_ENERGY, True, False),
                                                (_lib.MATH_EMU_MU, False, True)])
def test_energy_mu_from_logs_bits_of_the_model(gpu, code, energy, want_mu):
    """chs_energy_mu_from_logs<ENERGY, MU>, fed the model's lU, lV and a nonzero running sum: every fma as the header
    writes it (a wrong 3/2 A1, a swapped operand or a contraction shows here)."""
    U, Uinv, lU, lV, sE, mu = model_points()
    gE, gM = _lib.test_math_cols(code, [U, Uinv, lU, lV], mp.physics_consts(SE0))
    assert_bits(gE, sE if energy else np.full(U.size, SE0), f'sE of form {code}', U, lU, lV)
    assert_bits(gM, mu if want_mu else np.zeros(U.size), f'mu of form {code}', U, lU, lV)


def test_kernel_chain_bits_of_the_model(gpu):
    """One grid point as the fused fp64 row kernel forms it: u -> 1 - u -> two table logs -> chs_energy_mu_from_logs"""
    U, _, _, _, sE, mu = model_points()
    gE, gM = _lib.test_math_cols(_lib.MATH_CHAIN, [U], mp.physics_consts(SE0))
    assert_bits(gE, sE, 'sE of the chain', U)
    assert_bits(gM, mu, 'mu of the chain', U)
    gM2, dom = _lib.test_math_cols(_lib.MATH_CHAIN_DOM, [U], mp.physics_consts(SE0))
    assert_bits(gM2, mu, 'mu of the chain (domain form)', U)
    assert not dom.any()


@functools.lru_cache(maxsize=None)
def division_points():
    """d in +-[2^-60, 2^60]; sig in [0.5, 4) (what the logs ask for) and every kind of CHeig of spectral_points()"""
    rng = np.random.default_rng(41)
    ch = cheig_of(spectral_points())
    sig = np.concatenate([rng.uniform(0.5, 4.0, 200000), [0.5, np.nextafter(4.0, 0), 1.0, np.nextafter(1.0, 2)], ch])
    d = np.where(rng.random(sig.size) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-60, 60, sig.size)
    return d, sig


@pytest.mark.parametrize("code,tail", [(_lib.MATH_DIV_POS, mm.div_pos_tail), (_lib.MATH_DIV_POS1, mm.div_pos1_tail)])
def test_division(gpu, code, tail):
    """chs_div_pos / chs_div_pos1.  Kind C: |got - d/sig| < 1 ulp of the exact quotient (the header's claim; the
    longdouble quotient is exact to 2^-11 ulp) over both ranges of sig.  Kind A: the fma tail behind the hardware
    reciprocal, which the hook returns beside the quotient, is the model's bit for bit (2e4 points of the set)."""
    d, sig = division_points()
    q, seed = _lib.test_math_cols(code, [d, sig])
    e = mp.ulp_err(q, np.asarray(d, dtype=LD) / np.asarray(sig, dtype=LD))
    i = int(np.argmax(e))
    log_line(f"math pointwise: division code {code}: {e.size} points, max {e[i]:.4f} ulp at d={d[i]!r} sig={sig[i]!r}; "
             f"seed max rel err {np.max(np.abs(seed * sig - 1)):.3e}")
    assert e[i] < 1.0, (e[i], d[i], sig[i])
    pick = np.random.default_rng(42).choice(d.size, 20000, replace=False)
    pick[:8] = np.arange(200000, 200008)   # the edges of [0.5, 4) and the first corners of CHeig
    want = np.array([tail(a, b, r) for a, b, r in zip(d[pick].tolist(), sig[pick].tolist(), seed[pick].tolist())])
    assert_bits(q[pick], want, f'fma tail of code {code}', d[pick], sig[pick], seed[pick])


# ------------------------------------------------------------------ kind B
def np_energy_from_logs(U, Uinv, lU, lV, RT, B, A0, A1):
    a = U * (lU - B)
    b = Uinv * lV
    c = ((A0 + A1 * (Uinv - U)) * U) * Uinv
    return RT * (a + b) + c


def np_mu_from_logs(U, Uinv, lU, lV, RT, BRT, A0, A1):
    U2inv = Uinv - U
    t1 = RT * (lU - lV)
    t2 = (A0 + A1 * U2inv) * U2inv
    t3 = ((2 * A1) * U) * Uinv
    return ((t1 - BRT) + t2) - t3


@pytest.mark.parametrize("dtype", ['float64', 'float32'])
def test_from_logs_bits_of_numpy(gpu, dtype):
    """chs_energy_from_logs<T> and chs_mu_from_logs<T> (contraction off): the bits of numpy's elementwise chain in T"""
    w = wide_points()
    T = np.dtype(dtype).type
    U, Uinv, lU, lV = w[:4] if dtype == 'float64' else w[4:]
    RT, B, BRT, A0, A1 = (T(v) for v in mp.physics_consts()[:5])
    codes = (_lib.MATH_E_LOGS, _lib.MATH_MU_LOGS) if dtype == 'float64' else (_lib.MATH_E_LOGS_F32, _lib.MATH_MU_LOGS_F32)
    with np.errstate(under='ignore'):
        wantE = np_energy_from_logs(U, Uinv, lU, lV, RT, B, A0, A1)
        wantM = np_mu_from_logs(U, Uinv, lU, lV, RT, BRT, A0, A1)
    assert wantE.dtype == T and wantM.dtype == T
    gE, _ = _lib.test_math_cols(codes[0], [U, Uinv, lU, lV], mp.physics_consts())
    gM, _ = _lib.test_math_cols(codes[1], [U, Uinv, lU, lV], mp.physics_consts())
    assert_bits(gE, wantE.astype(np.float64), f'chs_energy_from_logs<{dtype}>', U, lU, lV)
    assert_bits(gM, wantM.astype(np.float64), f'chs_mu_from_logs<{dtype}>', U, lU, lV)


def test_dt_integrand_bits_of_numpy(gpu):
    """chs_dt_integrand: fp64 sqrt and / are correctly rounded, so numpy's delt_max / sqrt(1 + 62.5 (mu mu)) to the bit"""
    mu = mu_points()
    got, _ = _lib.test_math_cols(_lib.MATH_DT, [mu], [DELT_MAX])
    assert_bits(got, DELT_MAX / np.sqrt(1.0 + 62.5 * (mu * mu)), 'chs_dt_integrand', mu)


@functools.lru_cache(maxsize=None)
def spectral_operands():
    sp = spectral_points()
    rng = np.random.default_rng(51)
    hatU = rng.standard_normal(sp.shape[1]) * 10.0 ** rng.uniform(-6, 3, sp.shape[1])
    hatMu = rng.standard_normal(sp.shape[1]) * 10.0 ** rng.uniform(-6, 3, sp.shape[1])
    return hatU, hatMu


def spectral_launch(code):
    """one launch per (lam1, lam2) pair: they are uniform constants of the hook, as they are of the kernels"""
    sp = spectral_points()
    hatU, hatMu = spectral_operands()
    out = np.empty(sp.shape[1])
    for lam1, lam2 in sorted(set(zip(sp[2].tolist(), sp[3].tolist()))):
        m = (sp[2] == lam1) & (sp[3] == lam2)
        out[m] = _lib.test_math_cols(code, [hatU[m], hatMu[m], sp[0][m], sp[1][m]], [lam1, lam2])[0]
    return out


def test_spectral_f64_within_1ulp_of_numpy(gpu):
    """chs_spectral<double>: numerator and denominator are numpy's separate operations (contraction off), the quotient
    is chs_div_pos1: within 1 ulp of numpy's (hatU + Seig*hatMu) / CHeig, the comment's claim."""
    sp = spectral_points()
    hatU, hatMu = spectral_operands()
    leig = sp[0] + sp[1]
    want = (hatU + (sp[2] * leig) * hatMu) / (1.0 + (sp[3] * leig) * leig)
    got = spectral_launch(_lib.MATH_SPECTRAL)
    diff = np.abs(got - want) / np.spacing(np.abs(want))
    log_line(f"math pointwise: chs_spectral<double>: {got.size} points, {100.0 * np.mean(got != want):.3f} % differ from "
             f"numpy's quotient, max {diff.max():.1f} ulp; CHeig up to {cheig_of(sp).max():.4e}")
    assert diff.max() <= 1.0, (diff.max(), int(np.argmax(diff)))
    # the operands themselves: the same quotient by the hook's division from numpy's numerator and denominator
    q, _ = _lib.test_math_cols(_lib.MATH_DIV_POS1, [hatU + (sp[2] * leig) * hatMu, 1.0 + (sp[3] * leig) * leig])
    assert_bits(got, q, 'numerator / denominator of chs_spectral<double>', hatU, hatMu, sp[0], sp[1])


# ------------------------------------------------------------------ kind C
def test_dt_integrand_fast_f64(gpu):
    """chs_dt_integrand_fast(double), "~2 ulp" of a v_rsq seed: measured against the exact integrand (longdouble)"""
    mu = mu_points()
    got, _ = _lib.test_math_cols(_lib.MATH_DT_FAST, [mu], [DELT_MAX])
    check_measured('chs_dt_integrand_fast(double)', mp.ulp_err(got, dt_exact(mu, DELT_MAX)), mu)
    assert _lib.test_math_cols(_lib.MATH_DT_FAST, [[0.0, -0.0]], [DELT_MAX])[0].tolist() == [DELT_MAX, DELT_MAX]


def test_dt_integrand_fast_f32(gpu):
    """chs_dt_integrand_fast(float), "1 ulp" of v_rsq_f32: measured against the exact integrand of the float operands"""
    mu = np.unique(mu_points().astype(F32))
    dmax = F32(DELT_MAX)
    got, _ = _lib.test_math_cols(_lib.MATH_DT_FAST_F32, [mu], [dmax])
    assert np.array_equal(got, got.astype(F32))   # a float came back
    check_measured('chs_dt_integrand_fast(float)', mp.ulp_err(got, dt_exact(mu, dmax), F32), mu)
    assert _lib.test_math_cols(_lib.MATH_DT_FAST_F32, [[0.0, -0.0]], [dmax])[0].tolist() == [float(dmax)] * 2


def test_logf(gpu):
    """chs_logf = v_log_f32 * ln 2 over the float point set (0, 1): measured against log in longdouble"""
    x = np.unique(np.concatenate([mp.field_points_f32(N_WIDE), F32(1) - mp.field_points_f32(N_WIDE)]))
    got, _ = _lib.test_math_cols(_lib.MATH_LOGF, [x])
    check_measured('chs_logf', mp.ulp_err(got, np.log(x.astype(LD)), F32), x)
    assert _lib.test_math_cols(_lib.MATH_LOGF, [[1.0]])[0][0] == 0.0
    # chs_log_unit_tab<float> is the same function beside its domain word, which flags none of these
    tab, dom = _lib.test_math_cols(_lib.MATH_LOG_TAB_F32, [x])
    assert_bits(tab, got, 'chs_log_unit_tab<float>', x)
    assert not dom.any()


def log_ratio_exact(U, Uinv):
    """log(U / Uinv) in longdouble, by log1p where the quotient is near 1 (test_log_ratio_accuracy)"""
    Ul, Il = np.asarray(U, dtype=LD), np.asarray(Uinv, dtype=LD)
    near1 = np.abs(Ul - 0.5) < 0.1
    with np.errstate(divide='ignore'):   # (the branch not taken: log1p(-1) at a denormal U)
        return np.where(near1, np.log1p((Ul - Il) / Il), np.log(Ul / Il))


def test_log_ratio_f32(gpu):
    """chs_log_ratio<float> = chs_logf(a / b): the quotient is rounded first, so the error is absolute where the log
    crosses zero (U = 1/2 is inside the set) -- measured in ulp(float) of max(|log|, 1), the unit test_log_ratio_accuracy
    uses for numpy's own log(U / Uinv)."""
    U = mp.field_points_f32(N_WIDE)
    V = F32(1) - U
    got, _ = _lib.test_math_cols(_lib.MATH_LOG_RATIO_F32, [U, V])
    ref = log_ratio_exact(U, V)
    err = np.abs(got.astype(LD) - ref) / np.spacing(np.maximum(np.abs(ref), 1).astype(F32)).astype(LD)
    check_measured('chs_log_ratio<float>', err.astype(np.float64), U)


def test_spectral_f32_within_1ulp_of_the_quotient(gpu):
    """chs_spectral_f32: rhs and CHeig are formed by float fmas (modelled in longdouble: the products of floats are
    exact there), and the result is within 1 ulp of the fp32 quotient rhs / CHeig, the header's claim."""
    sp = spectral_points()
    hatU, hatMu = f32cols(*spectral_operands())
    got = spectral_launch(_lib.MATH_SPECTRAL_F32)
    assert np.array_equal(got, got.astype(F32))
    leig = (sp[0].astype(F32) + sp[1].astype(F32))
    lam1, lam2 = sp[2].astype(F32), sp[3].astype(F32)
    ch = ((lam2 * leig).astype(LD) * leig.astype(LD) + 1).astype(F32)
    rhs = ((lam1 * leig).astype(LD) * hatMu.astype(LD) + hatU.astype(LD)).astype(F32)
    q = rhs.astype(LD) / ch.astype(LD)
    qf = q.astype(F32)
    d = np.abs(got - qf.astype(np.float64)) / np.spacing(np.abs(qf)).astype(np.float64)
    e = mp.ulp_err(got, q, F32)
    log_line(f"math pointwise: chs_spectral_f32: {got.size} points, {100.0 * np.mean(got != qf):.3f} % differ from the fp32 "
             f"quotient, max {d.max():.1f} ulp of it, {e.max():.4f} ulp from the exact quotient")
    assert d.max() <= 1.0, (d.max(), int(np.argmax(d)))


def test_spectral_f32io_is_the_rounded_f64_update(gpu):
    """chs_spectral<float, false>: the fp64 update of float operands, rounded to float on the way out.  Derived: the
    double quotient is within 1 ulp(double) = 2^-29 ulp(float) of numpy's, and the conversion adds half an ulp(float)."""
    sp = spectral_points()
    hatU, hatMu = f32cols(*spectral_operands())
    got = spectral_launch(_lib.MATH_SPECTRAL_F32IO)
    assert np.array_equal(got, got.astype(F32))
    leig = sp[0] + sp[1]
    want = (hatU.astype(np.float64) + (sp[2] * leig) * hatMu.astype(np.float64)) / (1.0 + (sp[3] * leig) * leig)
    e = mp.ulp_err(got, want, F32)
    assert e.max() <= 0.5 + 2.0 ** -28, e.max()


@pytest.mark.parametrize("dtype", ['float64', 'float32'])
def test_from_logs_fast_within_the_running_error_bound(gpu, dtype):
    """chs_energy_from_logs_fast<T>, chs_mu_from_logs_fast<T> (the compiler may contract): against the literal
    expressions in longdouble from the same inputs, |got - exact| <= k u S (tests/math_points.py: k = 6 for both, a
    contraction only lowers it; S the sum of absolute terms)."""
    w = wide_points()
    U, Uinv, lU, lV = w[:4] if dtype == 'float64' else w[4:]
    u = mp.U64 if dtype == 'float64' else mp.U32
    kc = mp.physics_consts() if dtype == 'float64' else tuple(float(F32(v)) for v in mp.physics_consts())
    codes = ((_lib.MATH_E_LOGS_FAST, _lib.MATH_MU_LOGS_FAST) if dtype == 'float64'
             else (_lib.MATH_E_LOGS_FAST_F32, _lib.MATH_MU_LOGS_FAST_F32))
    for code, lit, k, name in ((codes[0], mp.energy_literal, mp.K_ENERGY_LITERAL, 'energy'), (codes[1], mp.mu_literal, mp.K_MU_LITERAL, 'mu')):
        got, _ = _lib.test_math_cols(code, [U, Uinv, lU, lV], kc)
        val, S = lit(U, Uinv, lU, lV, kc)
        r = np.abs(got.astype(LD) - val) / mp.bound(k, S, u)
        log_line(f"math pointwise: chs_{name}_from_logs_fast<{dtype}>: {got.size} points, worst error / bound {float(r.max()):.3f}")
        assert r.max() <= 1, (name, float(r.max()), U[int(np.argmax(r))])


def mu_exact(U, kc):
    """EnergieEut of U and its sum of absolute terms as chs_mu forms it from U alone (1 - U has the absolute form 1 + U,
    Uinv - U the form 1 + 2U), with the exact log(U / (1 - U))"""
    RT, _, BRT, A0, A1 = (LD(v) for v in kc[:5])
    Ul = np.asarray(U, dtype=LD)
    Il = 1 - Ul
    lr = log_ratio_exact(Ul, Il)
    val = RT * lr - BRT + (A0 + A1 * (Il - Ul)) * (Il - Ul) - 2 * A1 * Ul * Il
    S = abs(RT) * np.abs(lr) + abs(BRT) + (abs(A0) + abs(A1) * (1 + 2 * Ul)) * (1 + 2 * Ul) + 2 * abs(A1) * Ul * (1 + Ul)
    return val, S, lr


def energy_exact(U, kc):
    """the bulk energy density of U, its sum of absolute terms in the same form, and the two logs"""
    RT, B, _, A0, A1 = (LD(v) for v in kc[:5])
    Ul = np.asarray(U, dtype=LD)
    Il = 1 - Ul
    lU, lV = np.log(Ul), np.log1p(-Ul)
    val = RT * (Ul * (lU - B) + Il * lV) + (A0 + A1 * (Il - Ul)) * Ul * Il
    S = abs(RT) * (Ul * (np.abs(lU) + abs(B)) + (1 + Ul) * np.abs(lV)) + (abs(A0) + abs(A1) * (1 + 2 * Ul)) * Ul * (1 + Ul)
    return val, S, lU, lV


@pytest.mark.parametrize("dtype", ['float64', 'float32'])
def test_mu_and_energy_density_over_the_whole_set(gpu, dtype):
    """chs_mu<T> and chs_energy_density<T> from U alone, over the whole point set (test_mu_and_energy_density samples
    (0.6, 0.99) only), against the exact expressions of the same U in longdouble.  Running-error bound
    (tests/math_points.py), k = 7 rounded operations on the longest path of either (1 - U, Uinv - U, A1*, A0 +, two
    products, the last sum), plus the logs, which are not inputs here:
      fp64  chs_log_f64, chs_log_ratio_f64: 2.5 ulp (the header) <= 5 u |log|, and the rounding of 1 - U moves
            log(1 - U) by up to u more:  RT u (5 |log| + 1) for mu,  RT u (5 U |log U| + (1 + U)(5 |log(1 - U)| + 1)) for E;
      fp32  the measured figures M of chs_logf (ulp of the log) and chs_log_ratio<float> (ulp of max(|log|, 1)) in
            place of 2.5: 2 M u |log| resp. 2 M u max(|log|, 1)."""
    if dtype == 'float64':
        U, u, kc = mp.field_points(N_WIDE), mp.U64, mp.physics_consts()
        gM = _lib.test_math(2, U, np.array([kc[0], kc[2], kc[3], kc[4]]))
        gE = _lib.test_math(3, U, np.array([kc[0], kc[1], kc[3], kc[4]]))
        Lr = Ll = 5.0
        floor = 0.0
    else:
        U, u = mp.field_points_f32(N_WIDE), mp.U32
        kc = tuple(float(F32(v)) for v in mp.physics_consts())
        gM, _ = _lib.test_math_cols(_lib.MATH_MU_F32, [U], kc)
        gE, _ = _lib.test_math_cols(_lib.MATH_ENERGY_F32, [U], kc)
        Lr, Ll = 2 * measured_bound('chs_log_ratio<float>'), 2 * measured_bound('chs_logf')
        floor = 1.0
    RT = abs(LD(kc[0]))
    Ul = np.asarray(U, dtype=LD)
    val, S, lr = mu_exact(U, kc)
    bM = mp.bound(7, S, u) + mp.SLACK * u * RT * (Lr * np.maximum(np.abs(lr), floor) + 1)
    rM = np.abs(gM.astype(LD) - val) / bM
    val, S, lU, lV = energy_exact(U, kc)
    bE = mp.bound(7, S, u) + mp.SLACK * u * RT * (Ul * Ll * np.abs(lU) + (1 + Ul) * (Ll * np.abs(lV) + 1))
    rE = np.abs(gE.astype(LD) - val) / bE
    log_line(f"math pointwise: chs_mu<{dtype}>, chs_energy_density<{dtype}>: {U.size} points, worst error / bound "
             f"{float(rM.max()):.3f}, {float(rE.max()):.3f}")
    assert rM.max() <= 1, (float(rM.max()), U[int(np.argmax(rM))])
    assert rE.max() <= 1, (float(rE.max()), U[int(np.argmax(rE))])


# ------------------------------------------------------------------ special values
BAD_U = np.array([0.0, 1.0, -0.25, np.nan, np.inf])


def test_special_values_of_the_domain_word(gpu):
    """U in {0, 1, -0.25, NaN, inf}: the fp32 domain word of chs_log_unit_tab<float> flags every argument that is not
    positive (0, -0.25, NaN; a float 1 or inf is a legal argument of the log itself: log 1 = 0, log inf = inf), and
    through the fp64 kernel chain -- where both U and 1 - U go through the table log -- every one of the five is
    flagged.  Good points beside them are not."""
    with np.errstate(all='ignore'):
        v, dom = _lib.test_math_cols(_lib.MATH_LOG_TAB_F32, [BAD_U])
        v1, dom1 = _lib.test_math_cols(_lib.MATH_LOG_TAB_F32, [1 - BAD_U])
    assert dom.tolist() == [1, 0, 1, 1, 0] and dom1.tolist() == [0, 1, 0, 1, 1]
    assert np.all((dom + dom1) >= 1)      # as the row kernel uses it, on U and on 1 - U: every one of them is flagged
    assert v[0] == -np.inf and v[1] == 0.0 and np.isnan(v[2]) and np.isnan(v[3]) and v[4] == np.inf
    _, dom = _lib.test_math_cols(_lib.MATH_CHAIN_DOM, [np.concatenate([BAD_U, [-0.0, -np.inf, 2.0, -5e-324]])], mp.physics_consts())
    assert dom.tolist() == [1] * 9
    _, dom = _lib.test_math_cols(_lib.MATH_LOG_TAB, [[0.0, -0.25, np.nan, np.inf, 1.0, 0.875, 5e-324]])
    assert dom.tolist() == [1, 1, 1, 1, 0, 0, 0]
    _, dom = _lib.test_math_cols(_lib.MATH_LOG_TAB_F32, [[0.875, 1e-30, 0.5]])
    assert dom.tolist() == [0, 0, 0]


def test_special_values_of_the_integrands(gpu):
    """mu in {+-inf, NaN}: the literal form gives 0 for an infinite mu (delt_max / sqrt(inf)); the fast fp64 form gives
    NaN (rsq(inf) = 0 times h = inf in its Newton step), the fast fp32 form 0 (delt_max * rsq(inf)); NaN stays NaN in
    all three.  An infinite mu only arises from a field that has already tripped the NaN record."""
    mu = np.array([np.inf, -np.inf, np.nan])
    lit, _ = _lib.test_math_cols(_lib.MATH_DT, [mu], [DELT_MAX])
    f64, _ = _lib.test_math_cols(_lib.MATH_DT_FAST, [mu], [DELT_MAX])
    f32, _ = _lib.test_math_cols(_lib.MATH_DT_FAST_F32, [mu], [DELT_MAX])
    assert lit[:2].tolist() == [0.0, 0.0] and np.isnan(lit[2])
    assert np.all(np.isnan(f64))
    assert f32[:2].tolist() == [0.0, 0.0] and np.isnan(f32[2])


def test_hook_rejects_bad_arguments(gpu):
    for which in (9, 37, -1, 0):
        with pytest.raises(_lib.EngineError, match='bad argument'):
            _lib.test_math_cols(which, [[0.5]])
    with pytest.raises(ValueError):
        _lib.test_math_cols(_lib.MATH_LOGF, [[0.5], [0.5, 0.25]])
