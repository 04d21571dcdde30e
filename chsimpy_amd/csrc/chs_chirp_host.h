// chs_chirp_host.h -- plan and tables of the chirp engine (chs_chirp.hip): the orthonormal DCT-II/III of a line of ANY
// length N through Bluestein's chirp-z algorithm on a power-of-two FFT of length P >= 2N-1.  Everything is evaluated
// in long double with the arguments reduced in integers and rounded once to the element type.  Plain C++, nothing of
// HIP: chs_chirp.hip uploads these tables, tests/chirp_tables.cpp checks them on a CPU, tools/chirp_model.py restates
// the index maps in numpy.
//
// One line, forward (DCT-II):
//   a[pos(i)] = x[i] * w[pos(i)]           pos(i) = i/2 (i even), N-1-(i-1)/2 (i odd)   (Makhoul), zero up to P
//   A = FFT_P(a)  (decimation in frequency: digit-reversed positions, chirp_freq_of_pos)
//   A *= Bhat     (Bhat = FFT_P(b)/P at the same positions, b[+-n] = conj(w[n]), |n| < N)
//   c = P * IFFT_P(A)  (decimation in time: natural order again)
//   X[k] = Re(fout[k] * c[k])              fout[k] = 2 f_k exp(-i pi k/2N) w[k]
// inverse (DCT-III):
//   a[n] = iin[n] * (X[n] + i X[N-n])      iin[n] = exp(-i pi n/2N) w[n] / (2 f_n),   X[N] := 0
//   the same convolution;  v[k] = Re(iout[k] * c[k]),  iout[k] = w[k]/N;  x[i] = v[pos(i)]
// with w[n] = exp(-i pi n^2/N), f_0 = sqrt(1/4N), f_k = sqrt(1/2N).  (The kernel sends the constant part of a line round
// this: x - x[0] goes in and x[0] sqrt(N) is added to X[0]; X[0] is left out of a[] and X[0]/sqrt(N) added to every x.)
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

#define CHS_CHIRP_MIN_N 8
#define CHS_CHIRP_MAX_N 4096

struct ChirpPlan {
  int N = 0;
  int P = 0;      // FFT length: the smallest power of two >= 2N-1 (16 .. 8192)
  int logP = 0;
  int nt = 0;     // radix-8 passes that exchange through LDS (strides P/8, P/64, ...), each followed by twiddles
  int rl = 0;     // the last pass, on 8 neighbouring positions of a lane: 0 = one radix 8, 1 = four radix 2, 2 = two radix 4
};

inline ChirpPlan chirp_plan(int N) {
  ChirpPlan p;
  p.N = N;
  p.P = 16;
  p.logP = 4;
  while (p.P < 2 * N - 1) { p.P <<= 1; ++p.logP; }
  p.rl = p.logP % 3;
  p.nt = p.rl ? p.logP / 3 : p.logP / 3 - 1;
  return p;
}

// Where the Makhoul reorder puts grid point i of a line.
inline int chirp_pos_of_point(int N, int i) { return (i & 1) ? N - 1 - (i - 1) / 2 : i / 2; }

// The frequency that position `pos` of the forward FFT's output holds.
inline int chirp_freq_of_pos(const ChirpPlan& p, int pos) {
  int L = p.P, f = 0, mul = 1;
  for (int i = 0; i < p.nt; ++i) {
    const int s = L / 8;
    f += mul * (pos / s);
    pos %= s;
    mul *= 8;
    L = s;
  }
  // the last pass: blocks of r = L neighbouring positions (r = 8, 4 or 2), natural order inside
  return f + mul * pos;
}

typedef long double chirp_ld;
struct ChirpCx { chirp_ld re, im; };

inline chirp_ld chirp_pi() { return 3.14159265358979323846264338327950288419716939937510L; }
// exp(-i pi num/den) for an integer num that the caller has reduced mod 2 den
inline ChirpCx chirp_expm(long long num, long long den) {
  const chirp_ld a = chirp_pi() * (chirp_ld)num / (chirp_ld)den;
  return ChirpCx{cosl(a), -sinl(a)};
}
// w[n] = exp(-i pi n^2/N), n^2 reduced mod 2N in integers
inline ChirpCx chirp_w(int N, long long n) { return chirp_expm((n * n) % (2LL * N), N); }
inline chirp_ld chirp_f(int N, int k) { return k == 0 ? sqrtl(1.0L / (4.0L * N)) : sqrtl(1.0L / (2.0L * N)); }

// plain recursive radix-2 FFT (forward), n a power of two; root(m) = exp(-2 pi i m/n0) of the full length n0
inline void chirp_fft_rec(ChirpCx* x, int n, int stride_in_n0, int n0, ChirpCx* tmp) {
  if (n == 1) return;
  const int h = n / 2;
  for (int i = 0; i < h; ++i) { tmp[i] = x[2 * i]; tmp[h + i] = x[2 * i + 1]; }
  for (int i = 0; i < n; ++i) x[i] = tmp[i];
  chirp_fft_rec(x, h, stride_in_n0 * 2, n0, tmp);
  chirp_fft_rec(x + h, h, stride_in_n0 * 2, n0, tmp);
  for (int k = 0; k < h; ++k) {
    const ChirpCx w = chirp_expm(2LL * k * stride_in_n0, n0);
    const ChirpCx e = x[k], o = x[h + k];
    const ChirpCx t{o.re * w.re - o.im * w.im, o.re * w.im + o.im * w.re};
    x[k] = ChirpCx{e.re + t.re, e.im + t.im};
    x[h + k] = ChirpCx{e.re - t.re, e.im - t.im};
  }
}

// The tables of one N in long double (re, im interleaved is left to chirp_round).
struct ChirpTablesLd {
  ChirpPlan plan;
  std::vector<ChirpCx> tw;    // [P]  exp(-2 pi i m/P)
  std::vector<ChirpCx> bhat;  // [P]  FFT_P(b)/P at the forward FFT's output positions
  std::vector<ChirpCx> fin;   // [N]  w[n]
  std::vector<ChirpCx> fout;  // [N]  2 f_k exp(-i pi k/2N) w[k]
  std::vector<ChirpCx> iin;   // [N]  exp(-i pi n/2N) w[n] / (2 f_n)
  std::vector<ChirpCx> iout;  // [N]  w[k]/N
};

inline ChirpTablesLd chirp_tables_ld(int N) {
  ChirpTablesLd t;
  t.plan = chirp_plan(N);
  const int P = t.plan.P;
  t.tw.resize((size_t)P);
  for (int m = 0; m < P; ++m) t.tw[(size_t)m] = chirp_expm(2LL * m, P);
  std::vector<ChirpCx> b((size_t)P, ChirpCx{0, 0}), tmp((size_t)P);
  for (int n = 0; n < N; ++n) {
    const ChirpCx w = chirp_w(N, n);
    b[(size_t)n] = ChirpCx{w.re, -w.im};
    if (n) b[(size_t)(P - n)] = ChirpCx{w.re, -w.im};
  }
  chirp_fft_rec(b.data(), P, 1, P, tmp.data());
  t.bhat.resize((size_t)P);
  for (int pos = 0; pos < P; ++pos) {
    const ChirpCx v = b[(size_t)chirp_freq_of_pos(t.plan, pos)];
    t.bhat[(size_t)pos] = ChirpCx{v.re / P, v.im / P};
  }
  t.fin.resize((size_t)N); t.fout.resize((size_t)N); t.iin.resize((size_t)N); t.iout.resize((size_t)N);
  for (int k = 0; k < N; ++k) {
    const ChirpCx w = chirp_w(N, k);
    // exp(-i pi k/2N) w[k] = exp(-i pi (k + 2k^2)/(2N)), the numerator reduced mod 4N
    const ChirpCx g = chirp_expm(((long long)k + 2LL * k * k) % (4LL * N), 2LL * N);
    const chirp_ld f = chirp_f(N, k);
    t.fin[(size_t)k] = w;
    t.fout[(size_t)k] = ChirpCx{2 * f * g.re, 2 * f * g.im};
    t.iin[(size_t)k] = ChirpCx{g.re / (2 * f), g.im / (2 * f)};
    t.iout[(size_t)k] = ChirpCx{w.re / N, w.im / N};
  }
  return t;
}

// rounded once to the element type, (re, im) interleaved
template <typename T>
inline std::vector<T> chirp_round(const std::vector<ChirpCx>& v) {
  std::vector<T> r(2 * v.size());
  for (size_t i = 0; i < v.size(); ++i) { r[2 * i] = (T)v[i].re; r[2 * i + 1] = (T)v[i].im; }
  return r;
}

// LDS: a line keeps P complex values; position i sits at item i + i/32 (8-byte items), so that the strided
// exchanges of the passes spread over the banks.  fp64: a plane of real parts and one of imaginary parts per
// line; fp32: one plane of (re, im) pairs.
inline int chirp_lds_items(int P) { return P + P / 32; }
inline int chirp_line_lanes(int P) { return P / 8; }
inline int chirp_block_threads(int P) { return P / 8 > 256 ? P / 8 : 256; }
inline int chirp_lines_per_block(int P) { return chirp_block_threads(P) / chirp_line_lanes(P); }
inline size_t chirp_lds_bytes(int P, int elem_bytes) {
  return (size_t)chirp_lines_per_block(P) * chirp_lds_items(P) * (elem_bytes == 8 ? 16 : 8);
}
