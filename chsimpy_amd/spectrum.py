"""Radially averaged structure factor: the host side (numpy only, no device).

The definition the device and every test share (include/chs_hip.h: chs_structure_factor).  For an N x N field U,
``C = dctn(U - mean(U), norm='ortho')``; the power of mode (i, j) is ``C[i, j]**2``, that of mode (0, 0) counts as 0.
The mode's bin is the integer nearest to ``sqrt(i*i + j*j)``, decided in integer arithmetic: with ``s = i*i + j*j`` the
one ``b`` with ``b*b - b < s <= b*b + b`` (``b = 0`` for ``s = 0``).  No tie exists -- ``(b + 1/2)**2`` is no integer --
so no floating-point square root decides a bin.  Bins run ``0 .. nb-1``, ``nb = bin_of(N-1, N-1) + 1``; every mode is
counted, the corners included.

The device returns ``Ssum[b]``, the sum of the power over the modes of bin b (float64).  `StructureFactor` derives the
rest: ``S = Ssum / n`` with ``n = bin_sizes(N)``, the first moment ``k1 = sum(b * Ssum[b]) / sum(Ssum[b])`` over
``1 <= b <= N-1`` and the characteristic length ``ell = 2N / k1`` in grid points (a cosine mode of index i has the
wavelength 2N/i), ``ell_phys = ell * delx`` in the solver's length unit.
"""
import numpy as np


def bin_of(i, j):
    """The bin of mode (i, j); arrays broadcast.  The float square root is a first guess, two integer comparisons
    decide."""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    s = i * i + j * j
    b = np.rint(np.sqrt(s.astype(np.float64))).astype(np.int64)
    b = b - (b * b - b >= s)          # b*b - b < s ...
    b = b + (s > b * b + b)           # ... <= b*b + b
    b = np.where(s == 0, 0, b)
    assert np.all((s == 0) | ((b * b - b < s) & (s <= b * b + b)))
    return b if b.ndim else int(b)


def bin_count(N):
    """nb(N): the number of bins of an N x N grid (chs_structure_factor_bins)."""
    return int(bin_of(N - 1, N - 1)) + 1


def bin_map(N):
    """The N x N array of bins, mode (i, j) at [i, j]."""
    k = np.arange(N, dtype=np.int64)
    return bin_of(k[:, None], k[None, :])


def bin_sizes(N):
    """n_b: how many modes each bin has (mode (0, 0) included in bin 0), an int64 array of bin_count(N) entries."""
    return np.bincount(bin_map(N).ravel(), minlength=bin_count(N)).astype(np.int64)


def bin_power(C):
    """Ssum of an N x N array of coefficients C: the host's route, and the tests' reference."""
    C = np.asarray(C, dtype=np.float64)
    N = C.shape[0]
    P = C * C
    P[0, 0] = 0.0
    return np.bincount(bin_map(N).ravel(), weights=P.ravel(), minlength=bin_count(N))


class StructureFactor:
    """``Ssum`` of one field with what follows from it: ``n``, ``S``, ``k1``, ``ell``, ``ell_phys`` (None without
    ``delx``) and ``N``."""

    def __init__(self, Ssum, N, delx=None):
        self.N = int(N)
        self.Ssum = np.asarray(Ssum, dtype=np.float64)
        if self.Ssum.shape != (bin_count(self.N),):
            raise ValueError(f"Ssum needs {bin_count(self.N)} bins for N={self.N}, got shape {self.Ssum.shape}")
        self.delx = None if delx is None else float(delx)

    @property
    def n(self):
        return bin_sizes(self.N)

    @property
    def S(self):
        return self.Ssum / self.n

    @property
    def k1(self):
        """First moment of Ssum over the bins 1 .. N-1 (NaN for a field without fluctuations)."""
        b = np.arange(1, self.N, dtype=np.float64)
        w = self.Ssum[1:self.N]
        tot = float(w.sum())
        return float((b * w).sum() / tot) if tot > 0.0 else float('nan')

    @property
    def ell(self):
        """Characteristic length 2N / k1 in grid points."""
        return 2.0 * self.N / self.k1

    @property
    def ell_phys(self):
        return None if self.delx is None else self.ell * self.delx

    def __repr__(self):
        return f"StructureFactor(N={self.N}, k1={self.k1:.6g}, ell={self.ell:.6g})"
