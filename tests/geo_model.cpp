// geo_model.cpp -- host model of the relaxation rounds of the geodesic look (chsimpy_amd/csrc/chs_geodesic.hip, DESIGN.md
// section 3n), through the functions the kernel uses (chs_geo_host.h): the in-tile relaxation chs_geo::relax_segment of
// the 256 threads of a tile in the two phases of the kernel's sweep (all read, then all store), the sweep cap, and the
// flagging rule chs_geo::wakes.  The rounds run the active tiles in a scrambled order, and every halo word a tile loads
// is, at random, the word as it was when the round began or as it is now -- the two values a load can return between two
// launches.  The fixed point is held to a heap Dijkstra on every pattern, both connectivities and all four sources, at
// N = 8, 63, 65 and 130, and the rounds to the default limit 32 nt^2 + 64.
// Prints "<n> checks" and "<n> failures"; exit status 1 on a failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <random>
#include <string>
#include <vector>

#include "chs_geo_host.h"

namespace {
const int INF = CHS_GEO_UNREACHED;
long checks = 0, failures = 0;
std::mt19937 rng(20261021);

void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    if (failures < 20) printf("FAILED: %s\n", what.c_str());
  }
}

int depth_of(int source, int N, int i, int j) { return source == 0 ? i : source == 1 ? N - 1 - i : source == 2 ? j : N - 1 - j; }

std::vector<int> dijkstra(const std::vector<char>& X, int N, int conn, int source) {
  std::vector<int> G((size_t)N * N);
  typedef std::pair<int, int> E;
  std::priority_queue<E, std::vector<E>, std::greater<E>> heap;
  for (int p = 0; p < N * N; ++p) {
    G[p] = X[p] ? INF : -1;
    if (X[p] && depth_of(source, N, p / N, p % N) == 0) { G[p] = 0; heap.push(E(0, p)); }
  }
  const int a = chs_geo::unit_of(conn), d = chs_geo::diag_of(conn);
  while (!heap.empty()) {
    const E e = heap.top();
    heap.pop();
    if (e.first > G[e.second]) continue;
    const int i = e.second / N, j = e.second % N;
    for (int di = -1; di <= 1; ++di)
      for (int dj = -1; dj <= 1; ++dj) {
        if (!di && !dj) continue;
        const int w = (di && dj) ? d : a;
        const int y = i + di, x = j + dj;
        if (!w || y < 0 || y >= N || x < 0 || x >= N || !X[(size_t)y * N + x]) continue;
        if (e.first + w < G[(size_t)y * N + x]) { G[(size_t)y * N + x] = e.first + w; heap.push(E(e.first + w, y * N + x)); }
      }
  }
  return G;
}

// One active tile of one round, as k_geo_relax runs it.  Returns the neighbours to wake; *capped where the loop ends at
// its cap.
unsigned run_tile(std::vector<int>& G, const std::vector<int>& begin, int N, int conn, int ti, int tj, bool* capped) {
  const int P = CHS_GEO_P, T = CHS_GEO_T;
  std::vector<int> S((size_t)P * P);
  const int i0 = ti * T, j0 = tj * T;
  for (int q = 0; q < P * P; ++q) {
    const int lr = q / P, lc = q % P, gi = i0 + lr - 1, gj = j0 + lc - 1;
    const bool halo = lr == 0 || lr == P - 1 || lc == 0 || lc == P - 1;
    if (gi < 0 || gi >= N || gj < 0 || gj >= N) { S[q] = -1; continue; }
    const size_t p = (size_t)gi * N + gj;
    S[q] = (halo && (rng() & 1)) ? begin[p] : G[p];
  }
  const int per_row = T / CHS_GEO_SEG;
  std::vector<int> v((size_t)CHS_GEO_THREADS * CHS_GEO_SEG);
  std::vector<unsigned> fell(CHS_GEO_THREADS), ever(CHS_GEO_THREADS, 0u);
  for (int t = 0; t < CHS_GEO_THREADS; ++t)
    for (int k = 0; k < CHS_GEO_SEG; ++k) v[(size_t)t * CHS_GEO_SEG + k] = S[(t / per_row + 1) * P + (t % per_row) * CHS_GEO_SEG + 1 + k];
  bool done = false;
  for (int n = 0; n < CHS_GEO_SWEEP_CAP; ++n) {
    unsigned any = 0;
    for (int t = 0; t < CHS_GEO_THREADS; ++t) {   // every thread reads ...
      fell[t] = chs_geo::relax_segment(S.data(), conn, t / per_row, (t % per_row) * CHS_GEO_SEG, &v[(size_t)t * CHS_GEO_SEG]);
      any |= fell[t];
    }
    for (int t = 0; t < CHS_GEO_THREADS; ++t)     // ... then every thread stores
      for (int k = 0; k < CHS_GEO_SEG; ++k)
        if (fell[t] >> k & 1u) S[(t / per_row + 1) * P + (t % per_row) * CHS_GEO_SEG + 1 + k] = v[(size_t)t * CHS_GEO_SEG + k];
    for (int t = 0; t < CHS_GEO_THREADS; ++t) ever[t] |= fell[t];
    if (!any) { done = true; break; }
  }
  if (!done) *capped = true;
  unsigned wake = 0;
  for (int t = 0; t < CHS_GEO_THREADS; ++t)
    for (int k = 0; k < CHS_GEO_SEG; ++k) {
      if (!(ever[t] >> k & 1u)) continue;
      const int r = t / per_row, c = (t % per_row) * CHS_GEO_SEG + k;
      G[(size_t)(i0 + r) * N + j0 + c] = v[(size_t)t * CHS_GEO_SEG + k];
      wake |= chs_geo::wakes(conn, r, c);
    }
  return wake;
}

void wake_tiles(std::vector<char>& flags, int nt, int ti, int tj, unsigned wake) {
  for (int k = 0; k < CHS_GEO_NB; ++k) {
    int di, dj;
    chs_geo::nb_of(k, &di, &dj);
    const int ni = ti + di, nj = tj + dj;
    if ((wake >> k & 1u) && ni >= 0 && ni < nt && nj >= 0 && nj < nt) flags[(size_t)ni * nt + nj] = 1;
  }
}

void run_case(const std::vector<char>& X, int N, int conn, int source, const std::string& what) {
  const int nt = chs_geo::tiles_of(N), T = CHS_GEO_T;
  std::vector<int> G((size_t)N * N);
  std::vector<char> flags[2] = {std::vector<char>((size_t)nt * nt, 0), std::vector<char>((size_t)nt * nt, 0)};
  for (int p = 0; p < N * N; ++p) {   // k_geo_init
    const int i = p / N, j = p % N;
    const bool src = X[p] && depth_of(source, N, i, j) == 0;
    G[p] = !X[p] ? -1 : (src ? 0 : INF);
    if (src) {
      flags[1][(size_t)(i / T) * nt + j / T] = 1;
      wake_tiles(flags[1], nt, i / T, j / T, chs_geo::wakes(conn, i % T, j % T));
    }
  }
  const long limit = 32l * nt * nt + 64;
  long rounds = 0;
  bool capped = false;
  for (long round = 1; round <= limit + 1; ++round) {
    std::vector<char>& now = flags[round & 1];
    std::vector<int> act;
    for (int t = 0; t < nt * nt; ++t)
      if (now[t]) { act.push_back(t); now[t] = 0; }
    if (act.empty()) break;
    rounds = round;
    std::shuffle(act.begin(), act.end(), rng);
    const std::vector<int> begin = G;
    for (int t : act) wake_tiles(flags[(round + 1) & 1], nt, t / nt, t % nt, run_tile(G, begin, N, conn, t / nt, t % nt, &capped));
  }
  expect(!capped, what + ": a sweep loop reached its cap");
  expect(rounds <= limit, what + ": " + std::to_string(rounds) + " rounds, the default limit is " + std::to_string(limit));
  expect(G == dijkstra(X, N, conn, source), what + ": the fixed point is not Dijkstra's map");
}

std::vector<char> serpentine(int N, bool transpose) {
  std::vector<char> X((size_t)N * N, 0);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      const bool on = i % 2 == 0 || j == ((i / 2) % 2 == 0 ? N - 1 : 0);
      X[transpose ? (size_t)j * N + i : (size_t)i * N + j] = on;
    }
  return X;
}
}  // namespace

int main() {
  const int sizes[] = {8, 63, 65, 130};
  for (int N : sizes) {
    std::vector<std::pair<std::string, std::vector<char>>> pats;
    pats.push_back({"full", std::vector<char>((size_t)N * N, 1)});
    pats.push_back({"empty", std::vector<char>((size_t)N * N, 0)});
    pats.push_back({"serpentine", serpentine(N, false)});
    pats.push_back({"serpentine^T", serpentine(N, true)});
    std::vector<char> diag((size_t)N * N, 0), anti((size_t)N * N, 0), stair((size_t)N * N, 0);
    for (int i = 0; i < N; ++i) { diag[(size_t)i * N + i] = 1; anti[(size_t)i * N + N - 1 - i] = 1; }
    pats.push_back({"diagonal", diag});
    pats.push_back({"antidiagonal", anti});
    if (N > 70) {   // the only link of two tiles is a diagonal step through the tile corner: (63,63)-(64,64), (63,64)-(64,63)
      std::vector<char> back((size_t)N * N, 0);
      for (int i = 0; i < N; ++i) {
        stair[(size_t)i * N + (i < 64 ? 63 : 64)] = 1;
        back[(size_t)i * N + (i < 64 ? 64 : 63)] = 1;
      }
      pats.push_back({"staircase", stair});
      pats.push_back({"staircase back", back});
    }
    for (double dens : {0.45, 0.62, 0.9}) {
      std::vector<char> X((size_t)N * N);
      std::uniform_real_distribution<double> u(0.0, 1.0);
      for (auto& x : X) x = u(rng) < dens;
      pats.push_back({"random " + std::to_string(dens), X});
    }
    for (auto& pat : pats)
      for (int conn : {4, 8})
        for (int source = 0; source < 4; ++source)
          run_case(pat.second, N, conn, source, pat.first + " N=" + std::to_string(N) + " conn=" + std::to_string(conn) + " source=" + std::to_string(source));
  }
  // the flagging rule: the tiles that see a pixel through their halo, by brute force
  for (int conn : {4, 8})
    for (int r = 0; r < CHS_GEO_T; ++r)
      for (int c = 0; c < CHS_GEO_T; ++c) {
        unsigned want = 0;
        for (int k = 0; k < CHS_GEO_NB; ++k) {
          int di, dj;
          chs_geo::nb_of(k, &di, &dj);
          bool sees = false;   // a pixel of tile (di, dj) one step from (r, c)
          for (int y = -1; y <= 1; ++y)
            for (int x = -1; x <= 1; ++x) {
              if ((!y && !x) || (conn == 4 && y && x)) continue;
              const int rr = r + y, cc = c + x;
              const int tdi = rr < 0 ? -1 : rr >= CHS_GEO_T ? 1 : 0, tdj = cc < 0 ? -1 : cc >= CHS_GEO_T ? 1 : 0;
              if (tdi == di && tdj == dj) sees = true;
            }
          if (sees) want |= 1u << k;
        }
        expect(chs_geo::wakes(conn, r, c) == want, "wakes(" + std::to_string(conn) + ", " + std::to_string(r) + ", " + std::to_string(c) + ")");
      }
  printf("%ld checks\n%ld failures\n", checks, failures);
  return failures ? 1 : 0;
}
