"""Executable model of the chirp engine's 1-D dataflow (chsimpy_amd/csrc/chs_chirp.hip, chs_chirp_host.h): a design
aid and the test oracle of its index maps; nothing here runs in the product.

A line of ANY length N is transformed by Bluestein's chirp-z algorithm on a power-of-two FFT of length P >= 2N-1:
   Makhoul reorder -> chirp -> zero padding -> forward FFT (decimation in frequency, radix 8, the last pass radix
   8, 4 or 2 on the 8 neighbouring positions a lane owns) -> pointwise product with Bhat, stored at the forward FFT's
   digit-reversed output positions -> inverse FFT (decimation in time: the same network backwards) -> output factors.
`positions(plan, ls)` is the LDS position of register q of lane t in a pass of stride 2^ls, exactly the kernel's
address arithmetic; the passes themselves work on the equivalent reshaped view of the line (`_view`).  The inverse
(DCT-III) forms the spectrum from the pairs (X[n], X[N-n]) and runs the same core.  The constant part of a line (forward: its first value, inverse: X[0]) is taken out in front of the
convolution and put back behind it: see chs_chirp.hip.
"""
import numpy as np

LD = np.longdouble
PI = LD('3.14159265358979323846264338327950288419716939937510')


def plan(N):
    P, logP = 16, 4
    while P < 2 * N - 1:
        P, logP = P * 2, logP + 1
    rl = logP % 3
    nt = logP // 3 if rl else logP // 3 - 1
    return dict(N=N, P=P, logP=logP, nt=nt, rl=rl)


def pos_of_point(N, i):
    i = np.asarray(i)
    return np.where(i & 1, N - 1 - (i - 1) // 2, i // 2)


def freq_of_pos(pl, pos):
    pos = np.array(pos, dtype=np.int64)
    L, f, mul = pl['P'], np.zeros_like(pos), 1
    for _ in range(pl['nt']):
        s = L // 8
        f += mul * (pos // s)
        pos %= s
        mul *= 8
        L = s
    return f + mul * pos


def _expm(num, den):
    a = PI * np.asarray(num, dtype=LD) / LD(den)
    return np.cos(a) - 1j * np.sin(a)


def tables(N, ctype=np.complex128):
    """The tables of chs_chirp_host.h, evaluated in extended precision and rounded once to `ctype`."""
    pl = plan(N)
    P = pl['P']
    n = np.arange(N, dtype=np.int64)
    w = _expm((n * n) % (2 * N), N)
    g = _expm((n + 2 * n * n) % (4 * N), 2 * N)
    f = np.full(N, np.sqrt(LD(1) / (2 * N)), dtype=LD)
    f[0] = np.sqrt(LD(1) / (4 * N))
    b = np.zeros(P, dtype=w.dtype)
    b[:N] = np.conj(w)
    b[P - n[1:]] = np.conj(w[1:])
    # (the model takes numpy's double FFT of b; the header's long double FFT is checked by tests/chirp_tables.cpp)
    B = np.fft.fft(b.astype(np.complex128)) / P
    return dict(plan=pl, tw=_expm(2 * np.arange(P), P).astype(ctype), bhat=B[freq_of_pos(pl, np.arange(P))].astype(ctype),
                fin=w.astype(ctype), fout=(2 * f * g).astype(ctype), iin=(g / (2 * f)).astype(ctype),
                iout=(w / N).astype(ctype))


def positions(pl, ls):
    """[P/8, 8] LDS positions of the registers of every lane in a pass of stride 2^ls (ls = 0: the 8 neighbours)."""
    t = np.arange(pl['P'] // 8)[:, None]
    q = np.arange(8)[None, :]
    return ((t >> ls) << (ls + 3)) + (t & ((1 << ls) - 1)) + (q << ls)


def _view(lds, ls):
    """The registers of a pass of stride 2^ls as a view of the LDS image: [line, t >> ls, q, t & (2^ls - 1)], the same
    positions as `positions(plan, ls)` (tests/test_chirp_host.py compares the two)."""
    n, P = lds.shape
    return lds.reshape(n, P >> (ls + 3), 8, 1 << ls)


def _dft(v, r, inv):
    """DFTs of size r along axis 2 of [line, hi, 8, j]: 8/r of them side by side (r = 8: one)."""
    k = np.arange(r)
    M = np.exp((2j if inv else -2j) * np.pi * np.outer(k, k) / r).astype(v.dtype, copy=False)
    sh = v.shape
    if sh[3] == 1:
        return (v.reshape(-1, r) @ M.T).reshape(sh)
    if sh[3] < 64:      # (many small products: one large one on a transposed copy instead)
        return (v.transpose(0, 1, 3, 2).reshape(-1, 8) @ M.T).reshape(sh[0], sh[1], sh[3], 8).transpose(0, 1, 3, 2)
    return np.matmul(M, v)


def core(a, tb):
    """a: [lines, P] in natural position order (the LDS image behind the input stage) -> P * circular convolution
    with b, natural order.  Follows the kernel pass by pass; every pass works in place on the positions it reads."""
    pl = tb['plan']
    logP, nt, rl = pl['logP'], pl['nt'], pl['rl']
    lds = np.array(a, dtype=tb['tw'].dtype)
    k = np.arange(8)[:, None]

    def twiddles(ls):
        j = np.arange(1 << ls)[None, :]
        return tb['tw'][(j * k) << (logP - ls - 3)]          # [k, j]
    strides = [logP - 3 - 3 * i for i in range(nt)]
    for ls in strides:                                        # forward, decimation in frequency
        v = _view(lds, ls)
        v[...] = _dft(v, 8, False) * twiddles(ls)
    v = _view(lds, 0)                                         # the 8 neighbours of a lane, never leaving its registers
    r = (8, 2, 4)[rl]
    z = _dft(v, r, False) * tb['bhat'].reshape(1, -1, 8, 1)
    v[...] = _dft(z.astype(lds.dtype, copy=False), r, True)
    for ls in reversed(strides):                              # inverse, decimation in time
        v = _view(lds, ls)
        v[...] = _dft((v * np.conj(twiddles(ls))).astype(lds.dtype, copy=False), 8, True)
    return lds


def lines(x, tb, inverse=False):
    """Orthonormal DCT-II (DCT-III with inverse=True) of every row of x."""
    pl = tb['plan']
    N, P = pl['N'], pl['P']
    x = np.asarray(x)
    rdtype = tb['tw'].real.dtype
    a = np.zeros((x.shape[0], P), dtype=tb['tw'].dtype)
    pos = pos_of_point(N, np.arange(N))
    x = x.astype(rdtype)
    ref = x[:, :1]           # forward: the line's first value, inverse: X[0] -- the constant part goes round the FFTs
    if not inverse:
        a[:, pos] = (x - ref) * tb['fin'][pos]
        c = core(a, tb)[:, :N]
        X = (tb['fout'].real * c.real - tb['fout'].imag * c.imag).astype(rdtype)
        X[:, :1] += ref * rdtype.type(np.sqrt(LD(N)))
        return X
    x = np.concatenate([x[:, :1] * 0, x[:, 1:]], axis=1)
    xr = np.concatenate([x[:, :1] * 0, x[:, :0:-1]], axis=1)      # X[N-n], X[N] := 0
    a[:, :N] = tb['iin'] * (x + 1j * xr)
    c = core(a, tb)[:, :N]
    v = (tb['iout'].real * c.real - tb['iout'].imag * c.imag).astype(rdtype) + ref * rdtype.type(1 / np.sqrt(LD(N)))
    return v[:, pos]


def dct2d(x, tb, inverse=False, chunk=256):
    """rows, transpose, rows, transpose: what chs_chirp_dct2d launches."""
    def rows(y):
        return np.concatenate([lines(y[i:i + chunk], tb, inverse) for i in range(0, y.shape[0], chunk)])
    return rows(rows(np.asarray(x)).T.copy()).T.copy()


if __name__ == '__main__':
    from scipy import fftpack
    rng = np.random.default_rng(0)
    for N in (8, 9, 24, 100, 127, 129, 250, 1000):
        tb = tables(N)
        x = rng.standard_normal((N, N))
        y = fftpack.dctn(x, norm='ortho')
        ef = np.max(np.abs(dct2d(x, tb) - y)) / np.max(np.abs(y))
        ei = np.max(np.abs(dct2d(y, tb, True) - x)) / np.max(np.abs(x))
        print(f"N={N} P={tb['plan']['P']} forward {ef:.2e} inverse {ei:.2e}")
