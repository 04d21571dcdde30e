// cc_model.cpp -- phases 1 to 4 of the connected-component labelling (chsimpy_amd/csrc/chs_components.hip) run on the
// host through the functions the kernels share with it (chs_cc_host.h): the index maps, find and unite, with a plain
// sequential stand-in for the atomic minimum.  Inside every phase the work items are processed in scrambled orders (a
// fixed-seed shuffle), and in half of the runs every load of a label word returns, at random, an EARLIER value of the
// word -- what a stale cache line does on the device.  Every pattern of the device tests, both connectivities, both
// sides, N in {8, T-1, T, T+1, 2T+1}: labels, numbering, table and summary against a breadth-first flood fill written
// here.  Host C++ only; built with the address and undefined-behaviour sanitizers (tests/test_components_host.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <queue>
#include <string>
#include <vector>

#include "chs_cc_host.h"

namespace {
int failures = 0;
long checks = 0;

struct Rng {   // xorshift64*: the same orders at every run
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 2685821657736338717ull + 1442695040888963407ull) {}
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 2685821657736338717ull; }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

template <class T> void shuffle(std::vector<T>& v, Rng& r) {
  for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[(size_t)r.below((int)i)]);
}

// The words of a phase with every value each of them has held: load() returns the present value or, when `stale`, any
// earlier one; amin() is the atomic minimum, sequentially.
struct Words {
  std::vector<int> start;               // the value a word began with ...
  std::vector<std::vector<int>> more;   // ... and every value it took since, in order
  Rng* rng;
  bool stale;
  Words(const std::vector<int>& st, Rng* r, bool stale_) : start(st), more(st.size()), rng(r), stale(stale_) {}
  int now(int i) const { return more[(size_t)i].empty() ? start[(size_t)i] : more[(size_t)i].back(); }
  int load(int i) {
    const std::vector<int>& h = more[(size_t)i];
    if (!stale || h.empty()) return now(i);
    const int k = rng->below((int)h.size() + 1);
    return k == 0 ? start[(size_t)i] : h[(size_t)k - 1];
  }
  int amin(int i, int v) {
    const int old = now(i);
    if (v < old) more[(size_t)i].push_back(v);
    return old;
  }
  void store(int i, int v) { more[(size_t)i].push_back(v); }
};

struct Pair { int p, q; };

struct Result {
  std::vector<int> labels;               // [N * N] the component's number, -1
  std::vector<int32_t> table;            // [C][6]
};

void table_of(const std::vector<int>& labels, int N, int C, std::vector<int32_t>& table) {
  table.assign((size_t)C * 6, 0);
  std::vector<char> seen((size_t)C, 0);
  for (int p = 0; p < N * N; ++p) {
    const int k = labels[(size_t)p];
    if (k < 0) continue;
    int32_t* r = &table[(size_t)k * 6];
    const int i = p / N, j = p % N;
    if (!seen[(size_t)k]) { seen[(size_t)k] = 1; r[0] = p; r[1] = 0; r[2] = r[3] = i; r[4] = r[5] = j; }
    r[1] += 1;
    r[2] = std::min(r[2], i); r[3] = std::max(r[3], i); r[4] = std::min(r[4], j); r[5] = std::max(r[5], j);
  }
}

// the reference: a breadth-first flood fill from every unlabelled foreground pixel in ascending order, which numbers the
// components by ascending `first`
Result flood(const std::vector<char>& X, int N, int conn) {
  Result R;
  R.labels.assign((size_t)N * N, -1);
  int C = 0;
  const int di[8] = {0, 0, 1, -1, 1, 1, -1, -1}, dj[8] = {1, -1, 0, 0, 1, -1, 1, -1};
  for (int s = 0; s < N * N; ++s) {
    if (!X[(size_t)s] || R.labels[(size_t)s] >= 0) continue;
    std::queue<int> todo;
    todo.push(s);
    R.labels[(size_t)s] = C;
    while (!todo.empty()) {
      const int p = todo.front();
      todo.pop();
      for (int d = 0; d < conn; ++d) {
        const int i = p / N + di[d], j = p % N + dj[d];
        if (i < 0 || j < 0 || i >= N || j >= N) continue;
        const int q = i * N + j;
        if (X[(size_t)q] && R.labels[(size_t)q] < 0) { R.labels[(size_t)q] = C; todo.push(q); }
      }
    }
    ++C;
  }
  table_of(R.labels, N, C, R.table);
  return R;
}

// phases 1 to 4 as the kernels run them; returns false when a loop reached its cap
bool model(const std::vector<char>& X, int N, int conn, Rng& rng, bool stale, Result& R) {
  const int ty = chs_cc::tiles_of(N, CHS_CC_TR), tx = chs_cc::tiles_of(N, CHS_CC_TC), n2 = N * N;
  std::vector<int> L((size_t)n2, -1);
  int err = 0;
  // phase 1, tile by tile (in a scrambled order of the tiles, and of the pairs inside one)
  std::vector<int> tiles((size_t)tx * ty);
  for (size_t t = 0; t < tiles.size(); ++t) tiles[t] = (int)t;
  shuffle(tiles, rng);
  for (int t : tiles) {
    const int ti = t / tx, tj = t % tx;
    std::vector<int> par(CHS_CC_TILE, -1);
    for (int k = 0; k < CHS_CC_TILE; ++k) {
      const int i = ti * CHS_CC_TR + k / CHS_CC_TC, j = tj * CHS_CC_TC + k % CHS_CC_TC;
      if (i < N && j < N && X[(size_t)i * N + j]) par[(size_t)k] = k;
      int a, b, local;
      if (i < N && j < N) {
        chs_cc::tile_of(i, j, &a, &b, &local);
        if (a != ti || b != tj || local != k || chs_cc::global_of(N, ti, tj, k) != i * N + j) { ++failures; std::printf("FAIL tile_of / global_of at (%d, %d)\n", i, j); }
      }
    }
    std::vector<Pair> pairs;
    for (int k = 0; k < CHS_CC_TILE; ++k) {
      if (par[(size_t)k] < 0) continue;
      int q[4];
      const int n = chs_cc::tile_pairs(conn, k / CHS_CC_TC, k % CHS_CC_TC, q);
      for (int s = 0; s < n; ++s)
        if (par[(size_t)q[s]] >= 0) pairs.push_back(Pair{k, q[s]});
    }
    shuffle(pairs, rng);
    Words w(par, &rng, stale);
    for (const Pair& pr : pairs) chs_cc::unite(w, pr.p, pr.q, CHS_CC_TILE, &err, CHS_CC_ERR_TILE_FIND, CHS_CC_ERR_TILE_UNITE);
    std::vector<int> joined(CHS_CC_TILE);
    for (int k = 0; k < CHS_CC_TILE; ++k) joined[(size_t)k] = w.now(k);
    Words flat(joined, &rng, false);
    for (int k = 0; k < CHS_CC_TILE; ++k) {
      const int i = ti * CHS_CC_TR + k / CHS_CC_TC, j = tj * CHS_CC_TC + k % CHS_CC_TC;
      if (i >= N || j >= N || par[(size_t)k] < 0) continue;
      const int r = chs_cc::find(flat, k, CHS_CC_TILE, &err, CHS_CC_ERR_TILE_FIND);
      L[(size_t)i * N + j] = chs_cc::global_of(N, ti, tj, r);
    }
  }
  // phase 2: every border position of every tile, scrambled; the only write is amin
  {
    std::vector<Pair> pairs;
    for (int t = 0; t < tx * ty; ++t)
      for (int k = 0; k < CHS_CC_BORDER; ++k) {
        int p = 0, q[3];
        const int n = chs_cc::border_pairs(N, conn, t / tx, t % tx, k, &p, q);
        if (n == 0 || L[(size_t)p] < 0) continue;
        for (int s = 0; s < n; ++s)
          if (L[(size_t)q[s]] >= 0) pairs.push_back(Pair{p, q[s]});
      }
    shuffle(pairs, rng);
    Words w(L, &rng, stale);
    for (const Pair& pr : pairs) chs_cc::unite(w, pr.p, pr.q, n2, &err, CHS_CC_ERR_MERGE_FIND, CHS_CC_ERR_MERGE_UNITE);
    for (int p = 0; p < n2; ++p) L[(size_t)p] = w.now(p);
  }
  // phase 3: flatten, pixels in a scrambled order, every one storing its root at once (what a later pixel reads is
  // then an old word or a root, as on the device)
  {
    std::vector<int> order((size_t)n2);
    for (int p = 0; p < n2; ++p) order[(size_t)p] = p;
    shuffle(order, rng);
    Words w(L, &rng, false);
    for (int p : order) {
      const int l = w.now(p);
      if (l < 0 || l == p) continue;
      const int r = chs_cc::find(w, l, n2, &err, CHS_CC_ERR_FLATTEN);
      if (r != l) w.store(p, r);
    }
    for (int p = 0; p < n2; ++p) L[(size_t)p] = w.now(p);
  }
  if (err) { std::printf("FAIL a loop reached its cap: error word %d\n", err); return false; }
  // phase 4: counts per block, the scan, the scatter
  const int nblk = chs_cc::num_blocks(N);
  std::vector<int> cnt((size_t)nblk, 0), id((size_t)n2, -1);
  for (int p = 0; p < n2; ++p)
    if (L[(size_t)p] == p) cnt[(size_t)chs_cc::num_block_of(p)] += 1;
  int C = 0;
  for (int b = 0; b < nblk; ++b) { const int c = cnt[(size_t)b]; cnt[(size_t)b] = C; C += c; }
  std::vector<int> blocks((size_t)nblk);
  for (int b = 0; b < nblk; ++b) blocks[(size_t)b] = b;
  shuffle(blocks, rng);
  for (int b : blocks) {
    int rank = cnt[(size_t)b];
    for (int p = b * CHS_CC_NUM_BLOCK; p < std::min(n2, (b + 1) * CHS_CC_NUM_BLOCK); ++p)
      if (L[(size_t)p] == p) id[(size_t)p] = rank++;
  }
  R.labels.assign((size_t)n2, -1);
  for (int p = 0; p < n2; ++p) {
    const int l = L[(size_t)p];
    if (l < 0) continue;
    if (l > p || L[(size_t)l] != l) { ++failures; std::printf("FAIL L[%d] = %d is no root at or below its pixel\n", p, l); return false; }
    R.labels[(size_t)p] = id[(size_t)l];
  }
  table_of(R.labels, N, C, R.table);
  return true;
}

bool same_summary(const chs_cc::Summary& a, const chs_cc::Summary& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check_summary(const std::vector<int32_t>& table, int N, Rng& rng, const std::string& what) {
  const int C = (int)(table.size() / 6);
  chs_cc::Summary want = chs_cc::summary_zero();   // computed directly
  for (int r = 0; r < C; ++r) {
    const int32_t* row = &table[(size_t)r * 6];
    want.count += 1; want.area += row[1]; want.sumsq += (long long)row[1] * row[1];
    if (row[2] > 0 && row[3] < N - 1 && row[4] > 0 && row[5] < N - 1) want.inner += 1;
    if ((row[2] == 0 && row[3] == N - 1) || (row[4] == 0 && row[5] == N - 1)) want.spanning += 1;
    if (row[1] > want.largest) { want.largest = row[1]; want.largest_first = row[0]; }   // (ascending first: the first of the largest)
  }
  std::vector<chs_cc::Summary> parts;
  for (int r = 0; r < C; ++r) parts.push_back(chs_cc::summary_of_row(&table[(size_t)r * 6], N));
  shuffle(parts, rng);
  while (parts.size() > 1) {   // a scrambled tree
    const size_t a = (size_t)rng.below((int)parts.size());
    chs_cc::Summary x = parts[a];
    parts.erase(parts.begin() + (long)a);
    const size_t b = (size_t)rng.below((int)parts.size());
    parts[b] = rng.below(2) ? chs_cc::summary_add(x, parts[b]) : chs_cc::summary_add(parts[b], x);
  }
  chs_cc::Summary got = parts.empty() ? chs_cc::summary_zero() : parts[0];
  got = chs_cc::summary_add(got, chs_cc::summary_zero());
  ++checks;
  if (!same_summary(got, want)) { ++failures; std::printf("FAIL summary of %s\n", what.c_str()); }
}

struct Pattern { std::string name; std::vector<double> U; double t; };

const double FG = 0.2, BG = 0.8, T = 0.5;

std::vector<Pattern> patterns(int N) {
  std::vector<Pattern> out;
  auto blank = [&]() { return std::vector<char>((size_t)N * N, 0); };
  auto add = [&](const std::string& name, const std::vector<char>& X) {
    Pattern p{name, std::vector<double>((size_t)N * N), T};
    for (size_t k = 0; k < X.size(); ++k) p.U[k] = X[k] ? FG : BG;
    out.push_back(p);
  };
  auto at = [&](std::vector<char>& X, int i, int j) -> char& { return X[(size_t)i * N + j]; };
  const int TT = std::max(CHS_CC_TR, CHS_CC_TC), B = N > TT ? TT : N / 2;   // a tile border where the grid has one
  std::vector<char> X = blank();
  add("empty", X);
  add("full", std::vector<char>((size_t)N * N, 1));
  const int corner[4][2] = {{0, 0}, {0, N - 1}, {N - 1, 0}, {N - 1, N - 1}};
  for (auto& c : corner) { X = blank(); at(X, c[0], c[1]) = 1; add("corner", X); }
  X = blank(); for (int i = 0; i < N; ++i) at(X, i, i) = 1; add("diagonal", X);
  X = blank(); for (int i = 0; i < N; ++i) at(X, i, N - 1 - i) = 1; add("anti-diagonal", X);
  X = blank(); for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) at(X, i, j) = (i + j) % 2 == 0; add("checkerboard", X);
  X = blank(); for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) at(X, i, j) = (i == N - 1) || (j % 2 == 0); add("comb", X);
  X = blank();
  for (int i = 0; i < N; ++i) {
    if (i % 2 == 0) for (int j = 0; j < N; ++j) at(X, i, j) = 1;
    else at(X, i, ((i / 2) % 2 == 0) ? N - 1 : 0) = 1;
  }
  add("serpentine", X);
  // rings two apart, and the spiral made of them: ring k (offset o = 2k) is opened one pixel below its upper left corner
  // and joined to ring k + 1 by the pixel (o+2, o+1)
  std::vector<char> rings = blank();
  for (int o = 0; o <= N - 1 - o; o += 2)
    for (int i = o; i <= N - 1 - o; ++i)
      for (int j = o; j <= N - 1 - o; ++j)
        if (i == o || j == o || i == N - 1 - o || j == N - 1 - o) at(rings, i, j) = 1;
  add("rings", rings);
  X = rings;
  for (int o = 0; o <= N - 1 - o; o += 2) {
    const int side = N - 2 * o;
    if (side >= 3) at(X, o + 1, o) = 0;
    if (side >= 5) at(X, o + 2, o + 1) = 1;
  }
  add("spiral", X);
  X = blank(); for (int i = 0; i < N; ++i) for (int j = 0; j < N; j += 2) at(X, i, j) = 1; add("stripes", X);
  X = blank(); at(X, 5, B - 1) = at(X, 5, B) = 1; add("pair-h", X);
  X = blank(); at(X, B - 1, 6) = at(X, B, 6) = 1; add("pair-v", X);
  X = blank(); at(X, B - 1, B - 1) = at(X, B, B) = 1; add("pair-d", X);
  X = blank(); at(X, B - 1, B) = at(X, B, B - 1) = 1; add("pair-a", X);
  {   // the threshold, NaN and one-ulp pixels
    Pattern p{"threshold-nan-ulp", std::vector<double>((size_t)N * N, FG), T};
    p.U[(size_t)3 * N + 3] = T;
    p.U[(size_t)0 * N + 5] = T;
    p.U[(size_t)3 * N + 4] = std::numeric_limits<double>::quiet_NaN();
    p.U[(size_t)(N - 1) * N + 2] = std::nextafter(T, 0.0);
    p.U[(size_t)(N - 1) * N + 3] = std::nextafter(T, 1.0);
    out.push_back(p);
    Pattern e{"all-at-the-threshold", std::vector<double>((size_t)N * N, T), T};
    out.push_back(e);
  }
  {   // random fields at the site-percolation threshold and around it
    Rng r((uint64_t)N);
    const double dens[3] = {0.3, 0.593, 0.8};
    for (double d : dens) {
      X = blank();
      for (auto& x : X) x = (double)(r.next() >> 11) / 9007199254740992.0 < d;
      add("random", X);
    }
  }
  return out;
}

void run(int N) {
  Rng rng(1000003u * (uint64_t)N);
  for (const Pattern& pat : patterns(N))
    for (int above = 0; above < 2; ++above) {
      std::vector<char> X((size_t)N * N);
      for (size_t k = 0; k < X.size(); ++k) X[k] = chs_cc::fg_of(pat.U[k], pat.t, above) ? 1 : 0;
      if (pat.name == "threshold-nan-ulp") {   // the definition, spelled out: T and NaN are background below, foreground above
        const bool ok = X[(size_t)3 * N + 3] == above && X[(size_t)3 * N + 4] == above && X[(size_t)(N - 1) * N + 2] == !above &&
                        X[(size_t)(N - 1) * N + 3] == above;
        ++checks;
        if (!ok) { ++failures; std::printf("FAIL the foreground of the threshold / NaN / one-ulp pixels, side %d\n", above); }
      }
      for (int conn = 4; conn <= 8; conn += 4) {
        const Result want = flood(X, N, conn);
        for (int order = 0; order < 4; ++order) {
          Result got;
          const bool stale = order % 2 == 1;
          const std::string what = pat.name + " N=" + std::to_string(N) + " connectivity " + std::to_string(conn) + " side " +
                                   std::to_string(above) + " order " + std::to_string(order) + (stale ? " (stale loads)" : "");
          ++checks;
          if (!model(X, N, conn, rng, stale, got)) { ++failures; std::printf("FAIL %s\n", what.c_str()); continue; }
          if (got.labels != want.labels) { ++failures; std::printf("FAIL labels / numbering of %s\n", what.c_str()); }
          if (got.table != want.table) { ++failures; std::printf("FAIL table of %s\n", what.c_str()); }
          check_summary(got.table, N, rng, what);
        }
      }
    }
}
}  // namespace

int main() {
  const int TT = std::max(CHS_CC_TR, CHS_CC_TC), Tm = std::min(CHS_CC_TR, CHS_CC_TC);
  const int sizes[5] = {8, Tm - 1, TT, TT + 1, 2 * TT + 1};
  for (int N : sizes) run(N);
  std::printf("%ld checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
