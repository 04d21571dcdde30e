// chs_geo_host.h -- geodesic look: what k_geo_relax of chs_geodesic.hip and the host model
// tests/geo_model.cpp share.  No HIP in here: the step costs, the relaxation of a thread's row segment against the tile
// in LDS (a plain array on the host), the sweep count that cannot be reached and the flagging rule.
//
// The tile.  A workgroup holds its 64 x 64 pixels and a one-pixel halo as S[66][66] int32, the pixel at tile-local (r, c)
// at S[(r + 1) * 66 + c + 1].  A word is -1 (background, also everything outside the grid), CHS_GEO_INF (foreground that
// no path has reached) or the cost of a real path from the source wall.  Values only ever decrease.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define CHS_GEO_HD __attribute__((host)) __attribute__((device)) inline
#else
#define CHS_GEO_HD inline
#endif

#define CHS_GEO_T 64                        // pixel rows and columns of a tile
#define CHS_GEO_P (CHS_GEO_T + 2)           // pitch of the tile with its halo
#define CHS_GEO_SEG 16                      // consecutive pixels of a row that one thread relaxes
#define CHS_GEO_THREADS (CHS_GEO_T * CHS_GEO_T / CHS_GEO_SEG)
#define CHS_GEO_UNREACHED 0x7fffffff        // CHS_GEO_INF of include/chs_hip.h
// A sweep settles every pixel whose best path from the halo or from the tile's settled pixels has one more segment; a
// path visits a pixel once, so the pixels of tile and halo bound the sweeps.  The loop is counted up to this and never
// gets there.
#define CHS_GEO_SWEEP_CAP (CHS_GEO_T * CHS_GEO_T + 4 * CHS_GEO_T + 4)

// the neighbour tiles a changed border pixel wakes: bit k is the tile at (di, dj) of chs_geo::nb_of(k)
#define CHS_GEO_NB 8

namespace chs_geo {

CHS_GEO_HD int tiles_of(int N) { return (N + CHS_GEO_T - 1) / CHS_GEO_T; }
CHS_GEO_HD int unit_of(int conn) { return conn == 8 ? 3 : 1; }
CHS_GEO_HD int diag_of(int conn) { return conn == 8 ? 4 : 0; }   // 0: no diagonal step

// (di, dj) of neighbour tile k: the four sides, then the four corners
CHS_GEO_HD void nb_of(int k, int* di, int* dj) {
  *di = k < 4 ? (k == 0 ? -1 : k == 1 ? 1 : 0) : (k < 6 ? -1 : 1);
  *dj = k < 4 ? (k == 2 ? -1 : k == 3 ? 1 : 0) : ((k & 1) ? 1 : -1);
}

// The flagging rule: the neighbour tiles that can read the pixel at tile-local (r, c) through their halo.  A corner
// pixel is in the halo of the diagonal neighbour too -- at connectivity 8, where a diagonal step exists.
CHS_GEO_HD unsigned wakes(int conn, int r, int c) {
  const bool n = r == 0, s = r == CHS_GEO_T - 1, w = c == 0, e = c == CHS_GEO_T - 1;
  unsigned m = (n ? 1u : 0u) | (s ? 2u : 0u) | (w ? 4u : 0u) | (e ? 8u : 0u);
  if (conn == 8) m |= ((n && w) ? 16u : 0u) | ((n && e) ? 32u : 0u) | ((s && w) ? 64u : 0u) | ((s && e) ? 128u : 0u);
  return m;
}

// g + w where g is the cost of a path, CHS_GEO_UNREACHED otherwise (background -1 is above it as an unsigned word)
CHS_GEO_HD int via(int g, int w) { return (unsigned)g >= (unsigned)CHS_GEO_UNREACHED ? CHS_GEO_UNREACHED : g + w; }
CHS_GEO_HD int lower(int a, int b) { return a < b ? a : b; }

// One sweep of the thread that owns the pixels (r, c0 .. c0 + CHS_GEO_SEG) of the tile: v[] holds their present words.
// It reads the rows above and below and the two pixels beside the segment from S, takes the best step down, up or
// diagonally into every foreground pixel, and then runs the axial step along the segment in both directions, so a
// value crosses the whole segment in one sweep.  v[] receives the new words; returns the bits of the pixels that fell.
// S is only read: the caller stores what changed after every thread of the tile has read.
CHS_GEO_HD unsigned relax_segment(const int* S, int conn, int r, int c0, int v[CHS_GEO_SEG]) {
  const int a = unit_of(conn), d = diag_of(conn);
  const int* up = S + r * CHS_GEO_P + c0 + 1;            // row r - 1, column c0
  const int* dn = S + (r + 2) * CHS_GEO_P + c0 + 1;      // row r + 1
  const int* me = S + (r + 1) * CHS_GEO_P + c0 + 1;
  int nv[CHS_GEO_SEG];
#pragma unroll
  for (int k = 0; k < CHS_GEO_SEG; ++k) {
    int best = lower(via(up[k], a), via(dn[k], a));
    if (d) {
      best = lower(best, lower(via(up[k - 1], d), via(up[k + 1], d)));
      best = lower(best, lower(via(dn[k - 1], d), via(dn[k + 1], d)));
    }
    nv[k] = v[k] < 0 ? v[k] : lower(v[k], best);
  }
  int run = via(me[-1], a);                                // left to right; a background pixel breaks the run
#pragma unroll
  for (int k = 0; k < CHS_GEO_SEG; ++k) {
    if (nv[k] >= 0) nv[k] = lower(nv[k], run);
    run = via(nv[k], a);
  }
  run = via(me[CHS_GEO_SEG], a);                           // right to left
#pragma unroll
  for (int k = CHS_GEO_SEG - 1; k >= 0; --k) {
    if (nv[k] >= 0) nv[k] = lower(nv[k], run);
    run = via(nv[k], a);
  }
  unsigned fell = 0;
#pragma unroll
  for (int k = 0; k < CHS_GEO_SEG; ++k) {
    if (nv[k] != v[k]) fell |= 1u << k;
    v[k] = nv[k];
  }
  return fell;
}

}  // namespace chs_geo
