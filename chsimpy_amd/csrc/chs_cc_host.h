// chs_cc_host.h -- connected components of the thresholded field: what the kernels of
// chs_components.hip and the host model tests/cc_model.cpp share.  No HIP in here: the index maps (tile of a pixel, the
// border pairs of the merge, the blocks of the numbering) and the find / unite logic, templated on how a label word is
// read and min-updated -- device atomics in the kernels, a plain sequential stand-in on the host.
//
// The forest.  Every foreground pixel p has a label word W[p] (the tile's words in LDS in phase 1, L[] in global memory
// from phase 2 on); W[p] is the index of a pixel of p's component and W[p] <= p.  A word starts as p itself (phase 1)
// or as p's tile root (phase 2) and is only ever changed by an atomic minimum, so it only ever decreases.  p is a root
// while W[p] == p.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define CHS_CC_HD __attribute__((host)) __attribute__((device)) inline
#else
#define CHS_CC_HD inline
#endif

#define CHS_CC_TR 64                       // pixel rows of a tile
#define CHS_CC_TC 64                       // pixel columns of a tile
#define CHS_CC_TILE (CHS_CC_TR * CHS_CC_TC)
#define CHS_CC_BORDER (CHS_CC_TR + CHS_CC_TC)   // border positions of a tile: its first row, then its first column
#define CHS_CC_NUM_BLOCK 4096              // pixels of one block of the numbering (consecutive linear indices)
#define CHS_CC_MAX_N 16384                 // N * N and every linear index stay below 2^31

// the bits of the error word: which loop reached its cap
#define CHS_CC_ERR_TILE_FIND 1
#define CHS_CC_ERR_TILE_UNITE 2
#define CHS_CC_ERR_MERGE_FIND 4
#define CHS_CC_ERR_MERGE_UNITE 8
#define CHS_CC_ERR_FLATTEN 16

namespace chs_cc {

// The foreground of the definition: side below (above == 0) is u < t in double, a NaN and u == t being background; side
// above is its complement.
CHS_CC_HD bool fg_of(double u, double t, int above) { return (u < t) != (above != 0); }

CHS_CC_HD int tiles_of(int N, int T) { return (N + T - 1) / T; }

// The tile of pixel (i, j) and the pixel's position inside it.
CHS_CC_HD void tile_of(int i, int j, int* ti, int* tj, int* local) {
  *ti = i / CHS_CC_TR;
  *tj = j / CHS_CC_TC;
  *local = (i % CHS_CC_TR) * CHS_CC_TC + (j % CHS_CC_TC);
}

// The global linear index of the tile-local position `local` of tile (ti, tj).
CHS_CC_HD int global_of(int N, int ti, int tj, int local) {
  return (ti * CHS_CC_TR + local / CHS_CC_TC) * N + tj * CHS_CC_TC + local % CHS_CC_TC;
}

// Phase 1: the earlier neighbours, inside the tile, that the pixel at tile-local (r, c) is united with -- left, upper,
// and for connectivity 8 BOTH upper diagonals.  q[] receives their tile-local positions; returns how many.  (Rows and
// columns of the tile beyond the grid hold background, so the tile's own extent bounds them.)
CHS_CC_HD int tile_pairs(int conn, int r, int c, int q[4]) {
  int n = 0;
  if (c > 0) q[n++] = r * CHS_CC_TC + c - 1;
  if (r > 0) q[n++] = (r - 1) * CHS_CC_TC + c;
  if (conn == 8 && r > 0) {
    if (c > 0) q[n++] = (r - 1) * CHS_CC_TC + c - 1;
    if (c + 1 < CHS_CC_TC) q[n++] = (r - 1) * CHS_CC_TC + c + 1;
  }
  return n;
}

// Phase 2: border position k of tile (ti, tj) -- k < CHS_CC_TC: pixel (i0, j0 + k) of the tile's first row, else pixel
// (i0 + k - CHS_CC_TC, j0) of its first column -- and the neighbours in OTHER tiles it is united with.  *p receives the
// pixel's linear index, q[] the neighbours'; returns how many (0 also where the pixel is outside the grid or the tile
// has no neighbour on that side).
//   first row, ti > 0:     (i-1, j); connectivity 8: (i-1, j-1) and (i-1, j+1) -- at the tile's ends these lie in the
//                          diagonal tiles: the corner pairs
//   first column, tj > 0:  (i, j-1); connectivity 8: (i-1, j-1) and (i+1, j-1) -- the first of them, for the corner
//                          pixel, is the corner pair once more (harmless)
// Every pair of 4- or 8-neighbours in different tiles is among these: a pair across a horizontal tile border has its
// lower pixel in a first row; any other pair crosses a vertical border only, and its right pixel is in a first column.
CHS_CC_HD int border_pairs(int N, int conn, int ti, int tj, int k, int* p, int q[3]) {
  const int i0 = ti * CHS_CC_TR, j0 = tj * CHS_CC_TC;
  int n = 0;
  if (k < CHS_CC_TC) {
    const int i = i0, j = j0 + k;
    if (ti == 0 || j >= N || i >= N) return 0;
    *p = i * N + j;
    q[n++] = (i - 1) * N + j;
    if (conn == 8) {
      if (j > 0) q[n++] = (i - 1) * N + j - 1;
      if (j + 1 < N) q[n++] = (i - 1) * N + j + 1;
    }
  } else {
    const int i = i0 + k - CHS_CC_TC, j = j0;
    if (tj == 0 || i >= N || j >= N) return 0;
    *p = i * N + j;
    q[n++] = i * N + j - 1;
    if (conn == 8) {
      if (i > 0) q[n++] = (i - 1) * N + j - 1;
      if (i + 1 < N) q[n++] = (i + 1) * N + j - 1;
    }
  }
  return n;
}

// Phase 4: the block of the numbering that holds pixel p, and the number of blocks.
CHS_CC_HD int num_block_of(int p) { return p / CHS_CC_NUM_BLOCK; }
CHS_CC_HD int num_blocks(int N) { return (N * N + CHS_CC_NUM_BLOCK - 1) / CHS_CC_NUM_BLOCK; }

// find: follow the words from p to a pixel that reads as its own label.
// Termination: a word holds a smaller index of the same component or the pixel itself, so the walk visits strictly
// decreasing indices and ends after at most p steps; `cap` (the number of words: the tile's pixel count in LDS, N * N
// in global memory) is a count it cannot reach.  Reaching it all the same sets `bit` in *err and leaves: no spinning.
// A.load(p) may return ANY EARLIER value of the word (a stale cache line): every value a word ever held is a pixel of
// the same component that is no larger, so the walk still descends inside the component; what it returns is then a
// pixel that WAS a root, and unite() finds out from its atomic whether it still is.
template <class A>
CHS_CC_HD int find(A& a, int p, int cap, int* err, int bit) {
  for (int n = 0; n < cap; ++n) {
    const int q = a.load(p);
    if (q == p) return p;
    p = q;
  }
  *err |= bit;
  return p;
}

// unite: join the trees of p and q.  A.amin(i, v) is W[i] = min(W[i], v) as ONE atomic operation that returns the value
// before; it is the only write there is.
//   find both roots; hi = the larger, lo = the smaller; old = amin(hi, lo).
//   old == hi: hi was a root and now hangs below lo: done.
//   old != hi: hi had a parent `old` < hi already (another unite was faster, or the find read a stale word).  The
//     atomic has left W[hi] = min(old, lo): hi stays linked to one of the two, and the other one must still be joined
//     with it -- go on with the pair (old, lo).
// Termination: both members of the next pair are below hi (old < hi, lo < hi) and a find never returns more than it was
// given, so the larger root strictly decreases from retry to retry: fewer than max(p, q) retries, which is below `cap`,
// the number of words.  Reaching the cap all the same sets `unite_bit` and leaves.
// Stale reads: the decision "was a root" is taken from the value the atomic returns, never from a load; a stale load
// only makes find stop early (at a pixel that was a root once) or walk a few more steps, and lo need not be a root at
// all: hanging hi below any smaller pixel of the component lo belongs to keeps the forest a forest of decreasing links.
// Completeness: a word changes from y to z < y only in the atomic of a unite that then goes on with the pair (y, z), so
// when all unites of a launch have ended every pixel is in one tree with every value its word ever held, and p with q.
template <class A>
CHS_CC_HD void unite(A& a, int p, int q, int cap, int* err, int find_bit, int unite_bit) {
  for (int n = 0; n < cap; ++n) {
    p = find(a, p, cap, err, find_bit);
    q = find(a, q, cap, err, find_bit);
    if (p == q || (*err & find_bit)) return;
    const int hi = p > q ? p : q, lo = p > q ? q : p;
    const int old = a.amin(hi, lo);
    if (old == hi || old == lo) return;   // (old == lo: already hanging there)
    p = old;
    q = lo;
  }
  *err |= unite_bit;
}

// The summary of the table (phase 6): how one row counts, and how two partial summaries combine.  The largest component
// is the maximum of (area, -first), a total order, so every combination order gives the same words.
struct Summary {
  long long count, area, largest, sumsq, inner, spanning, largest_first;
};
CHS_CC_HD Summary summary_zero() { return Summary{0, 0, 0, 0, 0, 0, -1}; }
CHS_CC_HD Summary summary_of_row(const int32_t* row, int N) {
  const long long a = row[1];
  const int imin = row[2], imax = row[3], jmin = row[4], jmax = row[5];
  Summary s;
  s.count = 1; s.area = a; s.largest = a; s.sumsq = a * a;
  s.inner = (imin > 0 && imax < N - 1 && jmin > 0 && jmax < N - 1) ? 1 : 0;
  s.spanning = ((imin == 0 && imax == N - 1) || (jmin == 0 && jmax == N - 1)) ? 1 : 0;
  s.largest_first = row[0];
  return s;
}
CHS_CC_HD Summary summary_add(const Summary& x, const Summary& y) {
  Summary s;
  s.count = x.count + y.count; s.area = x.area + y.area; s.sumsq = x.sumsq + y.sumsq;
  s.inner = x.inner + y.inner; s.spanning = x.spanning + y.spanning;
  const bool xw = x.largest > y.largest ||
                  (x.largest == y.largest && (y.largest_first < 0 || (x.largest_first >= 0 && x.largest_first < y.largest_first)));
  s.largest = xw ? x.largest : y.largest;
  s.largest_first = xw ? x.largest_first : y.largest_first;
  return s;
}

}  // namespace chs_cc
