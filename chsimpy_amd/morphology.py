"""Morphology of the thresholded field -- area, interface length, Euler number: the host side (numpy only, no device).

The definition the device, this model and every test share (include/chs_hip.h: chs_morphology).

Foreground.  For an N x N field U and a threshold t (a finite double) the foreground is ``X[i][j] = ((double)U[i][j] < t)``:
the comparison is strict and done in double on the stored element (for an fp32 handle that element is the fp32 value
widened); a NaN pixel is background; a pixel equal to t is background.

Windows.  X is padded with one ring of background.  There are ``(N+1)**2`` windows; window (i, j), for i, j in [0, N],
holds the four pixels ``X[i-1][j-1], X[i-1][j], X[i][j-1], X[i][j]``, pixels outside the grid being 0.

Classes.  Every window is classified by its number of foreground pixels, n = 0 .. 4; among the n = 2 windows the two
diagonal patterns (QD) are separated from the four adjacent ones (Q2).

Border count.  ``border`` is the number of foreground pixels in row 0, plus row N-1, plus column 0, plus column N-1 (a
corner pixel counts twice): the foreground pixel edges that lie on the box.

Result.  Seven int64 words ``Q0, Q1, Q2, QD, Q3, Q4, border`` (`WORDS`; CHS_MORPH_WORDS and the CHS_MORPH_* indices of
the header).  `Morphology` derives the rest, all exact integers:

    n_A             = (Q1 + 2 Q2 + 2 QD + 3 Q3 + 4 Q4) / 4     foreground pixels
    SA              = n_A / N**2                               the area fraction the run records (solver.py:228)
    perimeter       = Q1 + Q2 + 2 QD + Q3                      unit edges between foreground and background, the
                                                               padding ring included
    perimeter_inner = perimeter - border                       4-adjacent unlike pixel pairs inside the grid
    euler8          = (Q1 - Q3 - 2 QD) / 4                     8-connected foreground components minus 4-connected holes
    euler4          = (Q1 - Q3 + 2 QD) / 4                     4-connected foreground components minus 8-connected holes
    interface_phys  = perimeter_inner * delx
"""
import numpy as np

WORDS = ('Q0', 'Q1', 'Q2', 'QD', 'Q3', 'Q4', 'border')
CHS_MORPH_WORDS = len(WORDS)
CHS_MORPH_Q0, CHS_MORPH_Q1, CHS_MORPH_Q2, CHS_MORPH_QD, CHS_MORPH_Q3, CHS_MORPH_Q4, CHS_MORPH_BORDER = range(7)


def foreground(U, threshold):
    """X of the definition, a boolean N x N array."""
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1]:
        raise ValueError(f"an N x N field is needed, got shape {U.shape}")
    t = float(threshold)
    if not np.isfinite(t):
        raise ValueError("the threshold must be finite")
    return U.astype(np.float64) < t      # (NaN < t is False)


def quad_counts(U, threshold):
    """The seven words of the field U at `threshold`, an int64 array: the numpy model of chs_morphology."""
    X = foreground(U, threshold)
    N = X.shape[0]
    P = np.zeros((N + 2, N + 2), dtype=np.int64)
    P[1:-1, 1:-1] = X
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]     # the four pixels of window (i, j), each (N+1, N+1)
    n = a + b + c + d
    q = np.bincount(n.ravel(), minlength=5).astype(np.int64)
    qd = int(np.count_nonzero((n == 2) & (a == d)))                 # (a == d and n == 2: b == c != a)
    border = int(X[0].sum()) + int(X[-1].sum()) + int(X[:, 0].sum()) + int(X[:, -1].sum())
    return np.array([q[0], q[1], q[2] - qd, qd, q[3], q[4], border], dtype=np.int64)


class Morphology:
    """The seven words of one field with what follows from them: ``Q0 .. Q4, QD, border, n_A, SA, perimeter,
    perimeter_inner, euler8, euler4, interface_phys`` (None without ``delx``), ``N`` and ``threshold``.  The counts are
    Python integers."""

    def __init__(self, words, N, threshold, delx=None):
        self.N = int(N)
        self.threshold = float(threshold)
        self.delx = None if delx is None else float(delx)
        self.words = np.array(words, dtype=np.int64)
        if self.words.shape != (CHS_MORPH_WORDS,):
            raise ValueError(f"{CHS_MORPH_WORDS} words are needed, got shape {self.words.shape}")
        self.Q0, self.Q1, self.Q2, self.QD, self.Q3, self.Q4, self.border = (int(w) for w in self.words)
        if self.Q0 + self.Q1 + self.Q2 + self.QD + self.Q3 + self.Q4 != (self.N + 1) ** 2:
            raise ValueError(f"the six classes do not add up to (N+1)^2 = {(self.N + 1) ** 2}: {self.words}")
        area4 = self.Q1 + 2 * self.Q2 + 2 * self.QD + 3 * self.Q3 + 4 * self.Q4
        e8, e4 = self.Q1 - self.Q3 - 2 * self.QD, self.Q1 - self.Q3 + 2 * self.QD
        if area4 % 4 or e8 % 4 or e4 % 4:
            raise ValueError(f"not the counts of a binary image: {self.words}")
        self.n_A = area4 // 4
        self.SA = self.n_A / (self.N * self.N)
        self.perimeter = self.Q1 + self.Q2 + 2 * self.QD + self.Q3
        self.perimeter_inner = self.perimeter - self.border
        self.euler8 = e8 // 4
        self.euler4 = e4 // 4
        self.interface_phys = None if self.delx is None else self.perimeter_inner * self.delx

    def __repr__(self):
        return (f"Morphology(N={self.N}, threshold={self.threshold!r}, n_A={self.n_A}, perimeter_inner={self.perimeter_inner}, "
                f"euler8={self.euler8}, euler4={self.euler4})")
