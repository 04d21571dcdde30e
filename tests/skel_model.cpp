// skel_model.cpp -- host model of the skeleton look's per-word functions (chsimpy_amd/csrc/chs_skeleton.hip, DESIGN.md
// section 3o), through the header the kernels compile (chs_skel_host.h): chs_sk::deletes of every word of a packed plane
// against a per-pixel loop over the definition -- the neighbour in the direction is background, Y == 1, B >= 2 -- and
// chs_sk::kinds_of against per-pixel counts of B, Y, the adjacent pairs and the 2 x 2 windows, over random planes at
// N = 1 .. 200 with partial last words and one-word rows, and whole thinnings to the fixed point with ping-pong planes as
// the host of the look runs them (the full grids against the sub-iteration counts of the definition's table).
// Prints "<n> checks" and "<n> failures"; exit status 1 on a failure.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "chs_skel_host.h"

namespace {
typedef chs_sk::u64 u64;
long checks = 0, failures = 0;
std::mt19937_64 rng(20261021);

void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    if (failures < 20) printf("FAILED: %s\n", what.c_str());
  }
}

struct Image {
  int N;
  std::vector<char> X;
  int at(int i, int j) const { return (i < 0 || j < 0 || i >= N || j >= N) ? 0 : X[(size_t)i * N + j]; }
};

// x0 .. x7 clockwise from north
const int DI[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
const int DJ[8] = {0, 1, 1, 1, 0, -1, -1, -1};

void by_pixel(const Image& im, int i, int j, int* B, int* Y, int x[8]) {
  *B = 0; *Y = 0;
  for (int k = 0; k < 8; ++k) { x[k] = im.at(i + DI[k], j + DJ[k]); *B += x[k]; }
  for (int k = 0; k < 8; k += 2) *Y += (!x[k] && (x[k + 1] || x[(k + 2) & 7])) ? 1 : 0;
}

std::vector<u64> pack(const Image& im) {
  const int W = chs_sk::words_of(im.N);
  std::vector<u64> P((size_t)im.N * W, 0);
  for (int i = 0; i < im.N; ++i)
    for (int j = 0; j < im.N; ++j)
      if (im.X[(size_t)i * im.N + j]) P[(size_t)i * W + j / 64] |= 1ull << (j % 64);
  return P;
}

// what sk_load9 of the kernels does: a word outside the plane is 0
chs_sk::Nine load9(const std::vector<u64>& P, int N, int W, int i, int w) {
  chs_sk::Nine n;
  for (int r = 0; r < 3; ++r) {
    const int ii = i + r - 1;
    const bool row = ii >= 0 && ii < N;
    n.c[r] = row ? P[(size_t)ii * W + w] : 0;
    n.l[r] = (row && w > 0) ? P[(size_t)ii * W + w - 1] : 0;
    n.r[r] = (row && w + 1 < W) ? P[(size_t)ii * W + w + 1] : 0;
  }
  return n;
}

Image random_image(int N, double density) {
  Image im{N, std::vector<char>((size_t)N * N)};
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (auto& v : im.X) v = u(rng) < density;
  return im;
}

int bit(u64 v, int j) { return (int)((v >> j) & 1ull); }

void check_plane(const Image& im, const std::string& what) {
  const int N = im.N, W = chs_sk::words_of(N);
  const std::vector<u64> P = pack(im);
  long bad_del = 0, bad_kind = 0, beyond = 0;
  for (int i = 0; i < N; ++i)
    for (int w = 0; w < W; ++w) {
      const chs_sk::Nine n = load9(P, N, W, i, w);
      u64 del[4];
      for (int d = 0; d < 4; ++d) del[d] = chs_sk::deletes(n, d);
      const chs_sk::Kinds k = chs_sk::kinds_of(n);
      for (int b = 0; b < 64; ++b) {
        const int j = w * 64 + b;
        if (j >= N) {
          for (int d = 0; d < 4; ++d) beyond += bit(del[d], b);
          beyond += bit(k.isolated | k.ends | k.b2 | k.y[0] | k.y[1] | k.y[2] | k.y[3] | k.y[4] | k.axial_e | k.axial_s | k.diag_se |
                        k.diag_sw | k.tri | k.full, b);
          continue;
        }
        int B, Y, x[8];
        by_pixel(im, i, j, &B, &Y, x);
        const int c = im.at(i, j);
        const int toward[4] = {x[0], x[4], x[2], x[6]};   // N, S, E, W
        for (int d = 0; d < 4; ++d) bad_del += bit(del[d], b) != (c && !toward[d] && Y == 1 && B >= 2);
        bad_kind += bit(k.isolated, b) != (c && B == 0);
        bad_kind += bit(k.ends, b) != (c && B == 1);
        bad_kind += bit(k.b2, b) != (c && B >= 2);
        for (int y = 0; y <= 4; ++y) bad_kind += bit(k.y[y], b) != (c && Y == y);
        bad_kind += bit(k.axial_e, b) != (c && x[2]);
        bad_kind += bit(k.axial_s, b) != (c && x[4]);
        bad_kind += bit(k.diag_se, b) != (c && x[3]);
        bad_kind += bit(k.diag_sw, b) != (c && x[5]);
        const int win = c + x[2] + x[4] + x[3];
        bad_kind += bit(k.tri, b) != (win == 3);
        bad_kind += bit(k.full, b) != (win == 4);
      }
    }
  expect(bad_del == 0, what + ": deletes");
  expect(bad_kind == 0, what + ": kinds_of");
  expect(beyond == 0, what + ": a bit at or beyond N");
}

// sub-iterations with two planes until four in a row delete nothing; returns the index of the last one that deleted
long thin(const Image& im, std::vector<u64>* out) {
  const int N = im.N, W = chs_sk::words_of(N);
  std::vector<u64> plane[2] = {pack(im), std::vector<u64>((size_t)N * W)};
  long last = 0;
  for (long it = 1; it <= last + 4; ++it) {
    const std::vector<u64>& src = plane[(it - 1) & 1];
    std::vector<u64>& dst = plane[it & 1];
    for (int i = 0; i < N; ++i)
      for (int w = 0; w < W; ++w) {
        const chs_sk::Nine n = load9(src, N, W, i, w);
        const u64 del = chs_sk::deletes(n, chs_sk::dir_of(it));
        dst[(size_t)i * W + w] = n.c[1] & ~del;
        if (del) last = it;
      }
  }
  expect(plane[0] == plane[1], "both planes are equal behind the fixed point");
  *out = plane[0];
  return last;
}

// the same by pixels
long thin_by_pixel(Image im, Image* out) {
  long last = 0;
  for (long it = 1; it <= last + 4; ++it) {
    const int d = (int)((it - 1) % 4);
    std::vector<char> next = im.X;
    for (int i = 0; i < im.N; ++i)
      for (int j = 0; j < im.N; ++j) {
        if (!im.at(i, j)) continue;
        int B, Y, x[8];
        by_pixel(im, i, j, &B, &Y, x);
        const int toward[4] = {x[0], x[4], x[2], x[6]};
        if (!toward[d] && Y == 1 && B >= 2) { next[(size_t)i * im.N + j] = 0; last = it; }
      }
    im.X = next;
  }
  *out = im;
  return last;
}

long euler_of(const std::vector<u64>& P, int N) {
  const int W = chs_sk::words_of(N);
  long e = 0;
  for (int i = 0; i < N; ++i)
    for (int w = 0; w < W; ++w) {
      const chs_sk::Kinds k = chs_sk::kinds_of(load9(P, N, W, i, w));
      e += chs_sk::euler8_of(chs_sk::popc(P[(size_t)i * W + w]), chs_sk::popc(k.axial_e) + chs_sk::popc(k.axial_s),
                             chs_sk::popc(k.diag_se) + chs_sk::popc(k.diag_sw), chs_sk::popc(k.tri), chs_sk::popc(k.full));
    }
  return e;
}
}  // namespace

int main() {
  const int sizes[] = {1, 2, 3, 8, 63, 64, 65, 127, 128, 129, 200};
  const double densities[] = {0.3, 0.5, 0.8, 0.95};
  for (int N : sizes)
    for (double p : densities) check_plane(random_image(N, p), "random N=" + std::to_string(N) + " p=" + std::to_string(p));
  const int full_counts[][2] = {{1, 4}, {8, 17}, {64, 129}, {65, 130}};   // (the four quiet sub-iterations included)
  for (const auto& fc : full_counts) {
    const int N = fc[0];
    Image full{N, std::vector<char>((size_t)N * N, 1)};
    check_plane(full, "full N=" + std::to_string(N));
    std::vector<u64> S;
    const long last = thin(full, &S);
    expect(last + 4 == fc[1], "full grid N=" + std::to_string(N) + ": " + std::to_string(last + 4) + " sub-iterations");
    expect(euler_of(S, N) == 1, "full grid N=" + std::to_string(N) + ": Euler number 1");
  }
  for (int N : {7, 64, 65, 130})
    for (double p : {0.5, 0.7, 0.9}) {
      const Image im = random_image(N, p);
      std::vector<u64> S;
      Image Q;
      const long a = thin(im, &S), b = thin_by_pixel(im, &Q);
      const std::string what = "thinning N=" + std::to_string(N) + " p=" + std::to_string(p);
      expect(a == b, what + ": SUBITERS " + std::to_string(a) + " / " + std::to_string(b));
      expect(S == pack(Q), what + ": the plane");
      expect(euler_of(S, N) == euler_of(pack(im), N), what + ": the Euler number is kept");
    }
  printf("%ld checks\n%ld failures\n", checks, failures);
  return failures ? 1 : 0;
}
