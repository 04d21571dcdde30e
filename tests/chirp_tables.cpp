// The tables of the chirp engine (chsimpy_amd/csrc/chs_chirp_host.h) against their definitions evaluated directly in
// long double, on a CPU (tests/test_chirp_host.py compiles and runs this): the chirp, the four factor tables, the FFT
// twiddles, and Bhat -- the header takes it from a recursive radix-2 FFT and stores it at the device FFT's
// digit-reversed output positions; here it is the O(P^2) sum, frequency by frequency.  Also: the position map is a
// permutation and agrees with a decimation-in-frequency FFT written down naively, and the rounding to the element
// types is the nearest value.  `chirp_tables --dump N` prints the tables rounded to double instead, one "name index
// re im" line per entry: tests/test_chirp_host.py compares them with the tables of tools/chirp_model.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chs_chirp_host.h"

namespace {
int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL N=%d: ", N); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

const long double PI = 3.14159265358979323846264338327950288419716939937510L;
const long double TOL = 64 * 1.0842021724855044e-19L;  // 64 ulp of long double at 1: the tables are O(1) or smaller

long double dist(ChirpCx a, long double re, long double im) { return hypotl(a.re - re, a.im - im); }

// exp(-i pi num/den) without the header's reduction helpers: fmodl of the exact product
void expm(long double num, long double den, long double* re, long double* im) {
  const long double r = fmodl(num, 2 * den);
  *re = cosl(PI * r / den);
  *im = -sinl(PI * r / den);
}

// a decimation-in-frequency FFT with the plan's radices, written down pass by pass on an array: X[freq_of_pos(p)]
// must be what position p holds
void dif_naive(const ChirpPlan& pl, std::vector<ChirpCx>& x) {
  int L = pl.P;
  std::vector<int> radices((size_t)pl.nt, 8);
  radices.push_back(pl.rl == 0 ? 8 : (pl.rl == 1 ? 2 : 4));
  for (int r : radices) {
    const int s = L / r;
    std::vector<ChirpCx> y(x.size());
    for (int b = 0; b < pl.P; b += L)
      for (int j = 0; j < s; ++j)
        for (int k = 0; k < r; ++k) {
          long double sr = 0, si = 0;
          for (int q = 0; q < r; ++q) {
            long double cr, ci;
            expm(2.0L * ((long long)q * k % r) * s + 2.0L * ((long long)j * k), L, &cr, &ci);  // w_r^(qk) w_L^(jk)
            const ChirpCx v = x[(size_t)(b + j + s * q)];
            sr += v.re * cr - v.im * ci;
            si += v.re * ci + v.im * cr;
          }
          y[(size_t)(b + j + s * k)] = ChirpCx{sr, si};
        }
    x.swap(y);
    L = s;
  }
}

void check_N(int N) {
  const ChirpTablesLd t = chirp_tables_ld(N);
  const ChirpPlan pl = t.plan;
  const int P = pl.P;
  CHECK(P >= 2 * N - 1 && (P == 16 || P / 2 < 2 * N - 1) && (P & (P - 1)) == 0 && (1 << pl.logP) == P, "P = %d", P);
  CHECK(3 * pl.nt + (pl.rl ? pl.rl : 3) == pl.logP, "passes nt=%d rl=%d logP=%d", pl.nt, pl.rl, pl.logP);
  CHECK((int)t.tw.size() == P && (int)t.bhat.size() == P && (int)t.fin.size() == N && (int)t.fout.size() == N &&
        (int)t.iin.size() == N && (int)t.iout.size() == N, "table sizes");
  // the position map is a permutation of the frequencies
  std::vector<int> seen((size_t)P, 0);
  for (int p = 0; p < P; ++p) {
    const int f = chirp_freq_of_pos(pl, p);
    CHECK(f >= 0 && f < P, "freq_of_pos(%d) = %d", p, f);
    if (f >= 0 && f < P) seen[(size_t)f]++;
  }
  for (int f = 0; f < P; ++f) CHECK(seen[(size_t)f] == 1, "frequency %d held by %d positions", f, seen[(size_t)f]);
  // ... the one of the decimation-in-frequency network: an impulse response is one row of the DFT matrix
  for (int src : {1, P / 2 + 3 < P ? P / 2 + 3 : 1}) {
    std::vector<ChirpCx> x((size_t)P, ChirpCx{0, 0});
    x[(size_t)src] = ChirpCx{1, 0};
    dif_naive(pl, x);
    long double worst = 0;
    for (int p = 0; p < P; ++p) {
      long double cr, ci;
      expm(2.0L * (((long long)chirp_freq_of_pos(pl, p) * src) % P), P, &cr, &ci);
      worst = fmaxl(worst, dist(x[(size_t)p], cr, ci));
    }
    CHECK(worst < 1e-15L, "DIF network vs position map, impulse at %d: %Lg", src, worst);
  }
  // the Makhoul positions are a permutation of 0..N-1, evens ascending from 0, odds descending from N-1
  std::vector<int> hit((size_t)N, 0);
  for (int i = 0; i < N; ++i) {
    const int p = chirp_pos_of_point(N, i);
    CHECK(p >= 0 && p < N, "pos_of_point(%d) = %d", i, p);
    if (p >= 0 && p < N) hit[(size_t)p]++;
    CHECK(p == ((i % 2 == 0) ? i / 2 : N - 1 - i / 2), "pos_of_point(%d) = %d", i, p);
  }
  for (int p = 0; p < N; ++p) CHECK(hit[(size_t)p] == 1, "position %d taken %d times", p, hit[(size_t)p]);
  // twiddles
  for (int m = 0; m < P; ++m) {
    long double cr, ci;
    expm(2.0L * m, P, &cr, &ci);
    CHECK(dist(t.tw[(size_t)m], cr, ci) < TOL, "tw[%d]", m);
  }
  // chirp and factor tables
  std::vector<long double> wr((size_t)N), wi((size_t)N);
  for (int k = 0; k < N; ++k) {
    expm((long double)k * k, N, &wr[(size_t)k], &wi[(size_t)k]);
    const long double f = (k == 0) ? sqrtl(0.25L / N) : sqrtl(0.5L / N);
    long double hr, hi;
    expm((long double)k, 2.0L * N, &hr, &hi);   // exp(-i pi k/2N)
    const long double gr = hr * wr[(size_t)k] - hi * wi[(size_t)k], gi = hr * wi[(size_t)k] + hi * wr[(size_t)k];
    CHECK(dist(t.fin[(size_t)k], wr[(size_t)k], wi[(size_t)k]) < TOL, "fin[%d]", k);
    CHECK(dist(t.fout[(size_t)k], 2 * f * gr, 2 * f * gi) < TOL, "fout[%d]", k);
    CHECK(dist(t.iin[(size_t)k], gr / (2 * f), gi / (2 * f)) < TOL * (1 + 1 / (2 * f)), "iin[%d]", k);
    CHECK(dist(t.iout[(size_t)k], wr[(size_t)k] / N, wi[(size_t)k] / N) < TOL, "iout[%d]", k);
  }
  // Bhat[pos] = (1/P) sum_m b[m] exp(-2 pi i m f/P), f = freq_of_pos(pos), b[+-n] = conj(w[n])
  long double worst = 0;
  for (int p = 0; p < P; ++p) {
    const long long f = chirp_freq_of_pos(pl, p);
    long double sr = 0, si = 0;
    for (int n = 0; n < N; ++n) {
      for (int sgn = 0; sgn < (n ? 2 : 1); ++sgn) {
        const long long m = sgn ? P - n : n;
        long double cr, ci;
        expm(2.0L * ((m * f) % P), P, &cr, &ci);
        // conj(w) * c
        sr += wr[(size_t)n] * cr + wi[(size_t)n] * ci;
        si += wr[(size_t)n] * ci - wi[(size_t)n] * cr;
      }
    }
    worst = fmaxl(worst, dist(t.bhat[(size_t)p], sr / P, si / P));
  }
  // a sum of 2N-1 unit terms over P: rounding of the O(P^2) sum itself is ~ sqrt(2N) ulp
  CHECK(worst < TOL * 8, "Bhat: %Lg", worst);
  // rounding once to the element type
  const std::vector<double> d = chirp_round<double>(t.bhat);
  const std::vector<float> s = chirp_round<float>(t.fout);
  CHECK(d.size() == 2 * (size_t)P && s.size() == 2 * (size_t)N, "rounded sizes");
  for (int p = 0; p < P; ++p)
    CHECK(d[2 * (size_t)p] == (double)t.bhat[(size_t)p].re && d[2 * (size_t)p + 1] == (double)t.bhat[(size_t)p].im, "round f64 %d", p);
  for (int k = 0; k < N; ++k)
    CHECK(s[2 * (size_t)k] == (float)t.fout[(size_t)k].re && s[2 * (size_t)k + 1] == (float)t.fout[(size_t)k].im, "round f32 %d", k);
  // LDS budget: inside the 160 KiB of a CU, every padded position inside its plane
  CHECK(chirp_lds_bytes(P, 8) <= 160 * 1024 && chirp_lds_bytes(P, 4) <= 160 * 1024, "LDS bytes %zu", chirp_lds_bytes(P, 8));
  CHECK((P - 1) + (P - 1) / 32 < chirp_lds_items(P), "padded position outside the plane");
  CHECK(chirp_line_lanes(P) * chirp_lines_per_block(P) == chirp_block_threads(P) && chirp_block_threads(P) <= 1024, "block shape");
  std::printf("N=%d P=%d nt=%d rl=%d: Bhat max error %Lg\n", N, P, pl.nt, pl.rl, worst);
}

void dump(int N) {
  const ChirpTablesLd t = chirp_tables_ld(N);
  std::printf("plan %d %d %d %d\n", t.plan.P, t.plan.logP, t.plan.nt, t.plan.rl);
  const struct { const char* name; const std::vector<ChirpCx>* tab; } all[] = {
      {"tw", &t.tw}, {"bhat", &t.bhat}, {"fin", &t.fin}, {"fout", &t.fout}, {"iin", &t.iin}, {"iout", &t.iout}};
  for (const auto& a : all) {
    const std::vector<double> d = chirp_round<double>(*a.tab);
    for (size_t i = 0; i < a.tab->size(); ++i) std::printf("%s %zu %.17g %.17g\n", a.name, i, d[2 * i], d[2 * i + 1]);
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) {
    dump(std::atoi(argv[2]));
    return 0;
  }
  for (int N : {9, 100, 129, 250}) check_N(N);
  // the plan alone at the edges of the range
  for (int N : {8, 4096}) {
    const ChirpPlan pl = chirp_plan(N);
    CHECK(pl.P >= 2 * N - 1 && chirp_lds_bytes(pl.P, 8) <= 160 * 1024, "plan at the edge: P = %d", pl.P);
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
