// chs_contour.hip -- the level set U = t of the field below the pixel on the device: the length of the marching-squares
// contour, its orientation tensor and the curvature of the level set at every crossed cell (the
// definition: include/chs_hip.h, chs_contour).
//
// Phases that depend on each other are separate launches: no workgroup ever waits for another one, nothing is polled.
//   1  k_ct_cells  a workgroup owns a tile of CT_TW x CT_TH cells and stages the pixels of the tile and of the halo the
//                  4 x 4 stencil needs (rows -1 .. CT_TH + 1, columns -1 .. CT_TW + 1) into LDS, widened to double:
//                  element loads, or 16-byte loads where N is a multiple of the vector (the tile's first column is one,
//                  the staged columns begin CT_PAD before it), every load issued before the first is looked at and none
//                  guarded by a branch.
//                  Classify: a wavefront owns a row of the tile's cells at a time, a lane one cell.  The cell's code and
//                  what is counted in integers (codes, vertices, ends, pixels below, pixels not finite) go into 16-bit
//                  counters packed in two registers, summed over the wavefront by shuffles.  A cell of the last row or
//                  column counts its far edge and its far pixels as well, so that every edge and every pixel is counted
//                  by exactly one cell.
//                  Compact: the ballot of the crossed cells of a row gives the row's count and a lane's place within
//                  it; the rows' counts are scanned by one wavefront; the crossed cells then stand in the LDS queue in
//                  row-major order of the tile -- a FIXED order, no racing counter.
//                  Work off: thread q takes the queue's entries q, q + CT_THREADS, ...: the vertices (a division each),
//                  the segments (a square root and three divisions each), the 16 stencil values and the curvature (a
//                  division and a square root) -- the fp64 work runs on full wavefronts whatever share of the cells is
//                  crossed.  fix(ell) and the histograms are integer sums (order-free): packed counters and the
//                  workgroup's LDS histograms, flushed by integer atomicAdd as k_cmp_hist does -- into one of
//                  CT_HCOPIES copies of the global words and histograms, since every workgroup adding to one cache
//                  line of words and to the few bins of a smooth field queues up.  The six doubles are added by the
//                  thread in queue order, joined over the workgroup by a fixed tree and stored into the workgroup's
//                  slot.  No float atomics.  A tile without a crossed cell stores a zero slot and leaves after the
//                  classification.
//   2  k_ct_fin    one workgroup joins the slots -- a thread every CT_FIN_THREADS-th slot in order, then a fixed tree --
//                  and the copies of the words and of the histograms, and adds up the histograms for the look's check.
// Nothing of the handle is written and nothing the step loop owns is read: its field alone.
#include <cmath>
#include <cstring>

#include "chs_look.h"

#define CT_TW 64                            // cells of a tile along a row: a wavefront's lanes
#define CT_TH 16                            // cells of a tile along a column
#define CT_THREADS 256
#define CT_PAD 4                            // staged columns in front of the tile's first: the halo of 1, a whole vector of either type
#define CT_FIN_THREADS 1024                 // k_ct_fin: one workgroup
#define CT_MAX_N 16384                      // N of chs_create at most: the tiles are two grid dimensions, L_FIX stays below 2^61
#define CT_HCOPIES 64                       // copies of the global words and histograms, a workgroup adds to copy (its number mod this)
#define CT_NX 2                             // the words k_ct_fin leaves beside the sums: the histograms added up

#define CT_LW (CT_TW + 2 * CT_PAD)          // doubles of a staged row
#define CT_LH (CT_TH + 3)                   // staged rows: -1 .. CT_TH + 1
#define CT_NW (CT_THREADS / CHS_WAVE)
#define CT_CPT (CT_TW * CT_TH / CT_THREADS) // cells of a thread

static_assert(CT_TW == CHS_WAVE, "a lane owns a cell of a row: the ballot is the row");
static_assert(CT_THREADS % CHS_WAVE == 0 && CT_TH % CT_NW == 0, "whole wavefronts, whole rounds of rows");
static_assert(CT_TH <= CHS_WAVE, "one wavefront scans the rows' counts");
static_assert(CT_TW * CT_TH <= 1024, "a queue entry: 10 bits of cell, 4 bits of code");
static_assert(CT_PAD % 4 == 0 && CT_PAD >= 1 && CT_TW % 4 == 0, "the staged columns begin on a 16-byte vector of either type");
static_assert(CHS_WAVE * 4 * CT_CPT < (1 << 16), "a wavefront's count fits a 16-bit counter (a cell adds 4 at most)");
static_assert(CT_THREADS == 1 << 8 && CT_FIN_THREADS == 1 << 10, "the trees above a thread's sum are 8 and 10 deep (ct_run)");
static_assert(CHS_CT_WORDS == 16 && CHS_CT_SUMS == 6, "the words and sums of include/chs_hip.h");
static_assert(CHS_CT_MAX_BINS * (sizeof(unsigned) + sizeof(unsigned long long)) <= 16384, "both histograms fit LDS beside the tile");

typedef long long ct_i64;
typedef unsigned long long ct_u64;
static_assert(sizeof(ct_i64) == sizeof(int64_t), "the result words are int64");

// the segments of a code: a nibble (P << 2) | Q per code, P and Q the edges T = 0, B = 1, L = 2, R = 3; the second segment
// of the saddles 6 (L-B) and 9 (B-R) beside it
#define CT_SEG0 0x083B91877319B380ull
#define CT_EDGE_T 0
#define CT_EDGE_B 1
#define CT_EDGE_L 2
#define CT_EDGE_R 3

// ---- the arithmetic of a cell: every operation rounded on its own ------------------------------------------------------
__device__ __forceinline__ bool ct_finite(double x) { return fabs(x) < __builtin_inf(); }

// the vertex of the edge (p, q), p the pixel with the lower index: its fraction from p
__device__ __forceinline__ double ct_frac(double p, double q, double t) {
#pragma clang fp contract(off)
  const bool pb = p < t;
  const double lo = pb ? p : q, hi = pb ? q : p;
  double s = (t - lo) / (hi - lo);
  if (!ct_finite(p) || !ct_finite(q)) s = 0.5;
  return pb ? s : 1.0 - s;
}

__device__ __forceinline__ void ct_vertex(int e, double a, double b, double c, double d, double t, double& x, double& y) {
  const double p = (e == CT_EDGE_T || e == CT_EDGE_L) ? a : (e == CT_EDGE_B ? c : b);
  const double q = e == CT_EDGE_T ? b : (e == CT_EDGE_L ? c : d);
  const double f = ct_frac(p, q, t);
  x = e < CT_EDGE_L ? f : (e == CT_EDGE_L ? 0.0 : 1.0);
  y = e < CT_EDGE_L ? (e == CT_EDGE_T ? 0.0 : 1.0) : f;
}

struct CtSeg {
  double l, txx, txy, tyy;
};

__device__ __forceinline__ CtSeg ct_segment(int pq, double a, double b, double c, double d, double t) {
#pragma clang fp contract(off)
  double px, py, qx, qy;
  ct_vertex(pq >> 2, a, b, c, d, t, px, py);
  ct_vertex(pq & 3, a, b, c, d, t, qx, qy);
  const double dx = qx - px, dy = qy - py;
  const double xx = dx * dx, yy = dy * dy, xy = dx * dy;
  CtSeg s;
  s.l = sqrt(xx + yy);
  const bool z = s.l == 0.0;
  s.txx = z ? 0.0 : xx / s.l;
  s.txy = z ? 0.0 : xy / s.l;
  s.tyy = z ? 0.0 : yy / s.l;
  return s;
}

// p: A(0, 0) of the staged tile, rows CT_LW apart.  false: one of the 16 values is not finite.
__device__ __forceinline__ bool ct_curvature(const double* p, double& kappa) {
#pragma clang fp contract(off)
  double A[4][4];
  bool fin = true;
#pragma unroll
  for (int di = 0; di < 4; ++di) {
#pragma unroll
    for (int dj = 0; dj < 4; ++dj) {
      A[di][dj] = p[(di - 1) * CT_LW + (dj - 1)];
      fin = fin && ct_finite(A[di][dj]);
    }
  }
#define CT_A(di, dj) A[(di) + 1][(dj) + 1]
  const double ux = ((CT_A(0, 1) + CT_A(1, 1)) - (CT_A(0, 0) + CT_A(1, 0))) * 0.5;
  const double uy = ((CT_A(1, 0) + CT_A(1, 1)) - (CT_A(0, 0) + CT_A(0, 1))) * 0.5;
  const double uxy = (CT_A(1, 1) - CT_A(1, 0)) - (CT_A(0, 1) - CT_A(0, 0));
  const double uxx = (((CT_A(0, 2) - CT_A(0, 1)) - (CT_A(0, 0) - CT_A(0, -1))) + ((CT_A(1, 2) - CT_A(1, 1)) - (CT_A(1, 0) - CT_A(1, -1)))) * 0.25;
  const double uyy = (((CT_A(2, 0) - CT_A(1, 0)) - (CT_A(0, 0) - CT_A(-1, 0))) + ((CT_A(2, 1) - CT_A(1, 1)) - (CT_A(0, 1) - CT_A(-1, 1)))) * 0.25;
#undef CT_A
  const double g2 = ux * ux + uy * uy;
  kappa = ((uxx * (uy * uy) - (2.0 * (ux * uy)) * uxy) + uyy * (ux * ux)) / (g2 * sqrt(g2));
  return fin;
}

// ---- what the kernels share -------------------------------------------------------------------------------------------
__device__ __forceinline__ ct_u64 ct_wave_sum(ct_u64 v) {
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The workgroup's v joined by a fixed tree, log2(64 NW) deep: shuffles inside the wavefront, the NW wavefronts' results
// through red[NW], shuffles over those in the first wavefront.  Thread 0 has the result.
template <int NW>
__device__ __forceinline__ double ct_block_sum(double v, double* red) {
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int lane = threadIdx.x % CHS_WAVE, w = threadIdx.x / CHS_WAVE;
  __syncthreads();   // (red is free again)
  if (lane == 0) red[w] = v;
  __syncthreads();
  if (w == 0) {
    v = red[lane < NW ? lane : 0];
#pragma unroll
    for (int off = NW / 2; off > 0; off >>= 1) v += __shfl_down(v, off);   // (lane 0 reaches lanes < NW only)
  }
  return v;
}

// ct_block_sum of CHS_CT_SUMS values at once: the same trees, one pair of barriers.  red: [NW][CHS_CT_SUMS].
template <int NW>
__device__ __forceinline__ void ct_block_sums(double (&v)[CHS_CT_SUMS], double* red) {
  const int lane = threadIdx.x % CHS_WAVE, w = threadIdx.x / CHS_WAVE;
#pragma unroll
  for (int k = 0; k < CHS_CT_SUMS; ++k) {
#pragma unroll
    for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
  }
  __syncthreads();   // (red is free again)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < CHS_CT_SUMS; ++k) red[w * CHS_CT_SUMS + k] = v[k];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int k = 0; k < CHS_CT_SUMS; ++k) {
      v[k] = red[(lane < NW ? lane : 0) * CHS_CT_SUMS + k];
#pragma unroll
      for (int off = NW / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);   // (lane 0 reaches lanes < NW only)
    }
  }
}

// ---- phase 1 ---------------------------------------------------------------------------------------------------------
// grid (tiles along a row, tiles along a column).  hist: [CT_HCOPIES][2][bins], the cells per bin and their fix(ell);
// iws: [CT_HCOPIES][CHS_CT_WORDS], the integer words.  Copies: the 16 words of every workgroup added to one cache line,
// and the few bins of a smooth field's curvature added by every workgroup to one histogram, queue up (profiles/contour.txt);
// slots: [tiles][CHS_CT_SUMS]; map: [2][N-1][N-1] or null.
template <typename T, int V, bool NT>
__global__ __launch_bounds__(CT_THREADS) void k_ct_cells(const void* Uv, int N, double t, int bins, double kmax, double scale,
                                                         double* __restrict__ slots, ct_u64* __restrict__ hist,
                                                         ct_u64* __restrict__ iws, double* __restrict__ map) {
  constexpr int C0 = (CT_PAD - 1) / V * V;                          // the first staged column that is loaded
  constexpr int C1 = (CT_PAD + CT_TW + 2 + V - 1) / V * V;          // the end of the last
  constexpr int NV = (C1 - C0) / V, TOTAL = CT_LH * NV, ITER = (TOTAL + CT_THREADS - 1) / CT_THREADS;
  static_assert(C1 <= CT_LW, "the staged row holds the loaded columns");
  __shared__ double tile[CT_LH * CT_LW];
  __shared__ unsigned short queue[CT_TW * CT_TH];
  __shared__ unsigned lh[CHS_CT_MAX_BINS];
  __shared__ ct_u64 ll[CHS_CT_MAX_BINS];
  __shared__ ct_u64 wg[CHS_CT_WORDS];
  __shared__ int rowcnt[CT_TH], rowbase[CT_TH + 1];
  __shared__ double red[CT_NW * CHS_CT_SUMS];
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const int tid = threadIdx.x, lane = tid % CHS_WAVE, wave = tid / CHS_WAVE;
  const int i0 = blockIdx.y * CT_TH, j0 = blockIdx.x * CT_TW;

  // stage the tile and its halo: all loads first
  {
    T x[ITER][V];
    bool ok[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int idx = it * CT_THREADS + tid, r = idx / NV, c = C0 + (idx % NV) * V;
      const int i = i0 - 1 + r, j = j0 - CT_PAD + c;   // (j is a multiple of V, and so is N: a vector lies inside the row or outside)
      ok[it] = idx < TOTAL && i >= 0 && i < N && j >= 0 && j < N;
      chs_load<T, V, NT>(U + (ok[it] ? (size_t)i * N + j : 0), x[it]);
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int idx = it * CT_THREADS + tid, r = idx / NV, c = C0 + (idx % NV) * V;
      if (idx < TOTAL) {
#pragma unroll
        for (int e = 0; e < V; ++e) tile[r * CT_LW + c + e] = ok[it] ? (double)x[it][e] : 0.0;   // (outside the grid: never looked at by a cell that counts)
      }
    }
  }
  for (int i = tid; i < bins; i += CT_THREADS) { lh[i] = 0; ll[i] = 0; }
  if (tid < CHS_CT_WORDS) wg[tid] = 0;
  __syncthreads();

  // classify
  const size_t M = (size_t)(N - 1);
  const double nan = __builtin_nan("");
  ct_u64 p0 = 0, p1 = 0;   // 16-bit counters: cells_one, cells_two, saddles, vertices_rows; vertices_cols, ends, n_below, n_nonfinite
  ct_u64 crossed[CT_CPT];  // (the same in every lane)
  int code[CT_CPT];
#pragma unroll
  for (int k = 0; k < CT_CPT; ++k) {
    const int lr = k * CT_NW + wave, i = i0 + lr, j = j0 + lane;
    const bool valid = i < N - 1 && j < N - 1;
    const double* p = tile + (lr + 1) * CT_LW + CT_PAD + lane;
    const double a = p[0], b = p[1], c = p[CT_LW], d = p[CT_LW + 1];
    const bool ba = a < t, bb = b < t, bc = c < t, bd = d < t;
    const int cd = (int)ba + 2 * (int)bb + 4 * (int)bc + 8 * (int)bd;
    code[k] = cd;
    const int nb = (int)ba + (int)bb + (int)bc + (int)bd;
    const bool saddle = cd == 6 || cd == 9;
    const bool top = ba != bb, bottom = bc != bd, left = ba != bc, right = bb != bd;
    const bool lastrow = i == N - 2, lastcol = j == N - 2;
    const ct_u64 one = nb == 1 || nb == 3, two = nb == 2 && !saddle, sad = saddle;
    const ct_u64 vr = (ct_u64)top + (lastrow && bottom), vc = (ct_u64)left + (lastcol && right);
    const ct_u64 en = (ct_u64)(i == 0 && top) + (lastrow && bottom) + (j == 0 && left) + (lastcol && right);
    const ct_u64 be = (ct_u64)ba + (lastcol && bb) + (lastrow && bc) + (lastrow && lastcol && bd);
    const ct_u64 nf = (ct_u64)!ct_finite(a) + (lastcol && !ct_finite(b)) + (lastrow && !ct_finite(c)) + (lastrow && lastcol && !ct_finite(d));
    if (valid) {
      p0 += one | two << 16 | sad << 32 | vr << 48;
      p1 += vc | en << 16 | be << 32 | nf << 48;
    }
    const bool cr = valid && cd != 0 && cd != 15;
    crossed[k] = __ballot(cr);   // (every lane of the wavefront is here: nothing above branches)
    if (map && valid && !cr) {
      map[(size_t)i * M + j] = 0.0;
      map[M * M + (size_t)i * M + j] = nan;
    }
    if (lane == 0) rowcnt[lr] = __popcll(crossed[k]);
  }
  __syncthreads();
  if (wave == 0) {   // the rows' counts scanned: rowbase[r] = the crossed cells of the rows before r, rowbase[CT_TH] all
    const int own = lane < CT_TH ? rowcnt[lane] : 0;
    int incl = own;
#pragma unroll
    for (int off = 1; off < CT_TH; off <<= 1) {
      const int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane < CT_TH) rowbase[lane] = incl - own;
    if (lane == CT_TH - 1) rowbase[CT_TH] = incl;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CT_CPT; ++k) {
    const int lr = k * CT_NW + wave;
    if ((crossed[k] >> lane) & 1) {
      const int pos = rowbase[lr] + __popcll(crossed[k] & (((ct_u64)1 << lane) - 1));   // (< CT_TW CT_TH: a place per cell)
      queue[pos] = (unsigned short)((lr * CT_TW + lane) | code[k] << 10);
    }
  }
  __syncthreads();

  // the integers of the classification: a wavefront's sum per word into the workgroup's
  p0 = ct_wave_sum(p0); p1 = ct_wave_sum(p1);
  if (lane == 0) {
    atomicAdd(&wg[CHS_CT_CELLS_ONE], p0 & 0xffff); atomicAdd(&wg[CHS_CT_CELLS_TWO], (p0 >> 16) & 0xffff);
    atomicAdd(&wg[CHS_CT_SADDLES], (p0 >> 32) & 0xffff); atomicAdd(&wg[CHS_CT_VERTICES_ROWS], p0 >> 48);
    atomicAdd(&wg[CHS_CT_VERTICES_COLS], p1 & 0xffff); atomicAdd(&wg[CHS_CT_ENDS], (p1 >> 16) & 0xffff);
    atomicAdd(&wg[CHS_CT_N_BELOW], (p1 >> 32) & 0xffff); atomicAdd(&wg[CHS_CT_N_NONFINITE], p1 >> 48);
  }

  // work off the queue.  A tile that the contour does not cross -- most tiles of a coarsened field -- has nothing to
  // work off and nothing to join: its slot is zero.
  const int total = rowbase[CT_TH];   // (the same in every thread)
  const int wgid = blockIdx.y * gridDim.x + blockIdx.x;
  double* slot = slots + (size_t)wgid * CHS_CT_SUMS;
  if (total == 0) {
    if (tid < CHS_CT_SUMS) slot[tid] = 0.0;
    __syncthreads();   // (every wavefront's atomics on wg are done)
    if (tid < CHS_CT_WORDS && wg[tid]) atomicAdd(&iws[(wgid % CT_HCOPIES) * CHS_CT_WORDS + tid], wg[tid]);
    return;
  }
  double sxx = 0.0, sxy = 0.0, syy = 0.0, k1 = 0.0, ka = 0.0, k2 = 0.0;
  ct_u64 p2 = 0, p3 = 0;   // 16-bit counters: segments, cells_curv, cells_wall, cells_bad; hist_under, hist_over
  ct_u64 lfix = 0, lcurv = 0;
  for (int q = tid; q < total; q += CT_THREADS) {
#pragma clang fp contract(off)
    const int e = queue[q], cell = e & 1023, cd = e >> 10, lr = cell / CT_TW, lc = cell % CT_TW;
    const int i = i0 + lr, j = j0 + lc;
    const double* p = tile + (lr + 1) * CT_LW + CT_PAD + lc;
    const double a = p[0], b = p[1], c = p[CT_LW], d = p[CT_LW + 1];
    const bool saddle = cd == 6 || cd == 9;
    const CtSeg s0 = ct_segment((int)((CT_SEG0 >> (4 * cd)) & 15), a, b, c, d, t);
    double ell = s0.l;
    sxx += s0.txx; sxy += s0.txy; syy += s0.tyy;
    p2 += 1;
    if (saddle) {
      const CtSeg s1 = ct_segment(cd == 6 ? (CT_EDGE_L << 2 | CT_EDGE_B) : (CT_EDGE_B << 2 | CT_EDGE_R), a, b, c, d, t);
      ell = s0.l + s1.l;
      sxx += s1.txx; sxy += s1.txy; syy += s1.tyy;
      p2 += 1;
    }
    const ct_u64 fx = (ct_u64)(ct_i64)(ell * 0x1p30);
    lfix += fx;
    double kap = nan;
    if (!saddle) {
      if (i >= 1 && j >= 1 && i <= N - 3 && j <= N - 3) {
        double kv;
        const bool fin = ct_curvature(p, kv);
        if (fin && ct_finite(kv)) {
          kap = kv;
          p2 += (ct_u64)1 << 16;
          lcurv += fx;
          k1 += ell * kv; ka += ell * fabs(kv); k2 += ell * (kv * kv);
          if (kv < -kmax) p3 += 1;
          else if (kv > kmax) p3 += (ct_u64)1 << 16;
          else {
            const double pb = (kv + kmax) * scale;
            const int bin = pb >= 0.0 && pb < (double)bins ? (int)pb : bins - 1;
            atomicAdd(&lh[bin], 1u);
            atomicAdd(&ll[bin], fx);
          }
        } else p2 += (ct_u64)1 << 48;
      } else p2 += (ct_u64)1 << 32;
    }
    if (map) {
      map[(size_t)i * M + j] = ell;
      map[M * M + (size_t)i * M + j] = kap;
    }
  }

  // the integers of the queue: a wavefront's sum per word into the workgroup's, the workgroup's into the look's
  p2 = ct_wave_sum(p2); p3 = ct_wave_sum(p3);
  lfix = ct_wave_sum(lfix); lcurv = ct_wave_sum(lcurv);
  if (lane == 0) {
    atomicAdd(&wg[CHS_CT_SEGMENTS], p2 & 0xffff); atomicAdd(&wg[CHS_CT_CELLS_CURV], (p2 >> 16) & 0xffff);
    atomicAdd(&wg[CHS_CT_CELLS_WALL], (p2 >> 32) & 0xffff); atomicAdd(&wg[CHS_CT_CELLS_BAD], p2 >> 48);
    atomicAdd(&wg[CHS_CT_HIST_UNDER], p3 & 0xffff); atomicAdd(&wg[CHS_CT_HIST_OVER], (p3 >> 16) & 0xffff);
    atomicAdd(&wg[CHS_CT_L_FIX], lfix); atomicAdd(&wg[CHS_CT_L_CURV_FIX], lcurv);
  }
  // the doubles: a fixed tree into the workgroup's slot
  double v[CHS_CT_SUMS];
  v[CHS_CT_TXX] = sxx; v[CHS_CT_TXY] = sxy; v[CHS_CT_TYY] = syy; v[CHS_CT_K1] = k1; v[CHS_CT_KA] = ka; v[CHS_CT_K2] = k2;
  ct_block_sums<CT_NW>(v, red);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < CHS_CT_SUMS; ++k) slot[k] = v[k];
  }
  __syncthreads();   // (every wavefront's atomics on wg, lh and ll are done)
  if (tid < CHS_CT_WORDS && wg[tid]) atomicAdd(&iws[(wgid % CT_HCOPIES) * CHS_CT_WORDS + tid], wg[tid]);
  ct_u64* __restrict__ hc = hist + (size_t)(wgid % CT_HCOPIES) * 2 * bins;
  for (int i = tid; i < bins; i += CT_THREADS) {
    const unsigned n = lh[i];
    if (n) { atomicAdd(&hc[i], (ct_u64)n); atomicAdd(&hc[bins + i], ll[i]); }
  }
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------------
// One workgroup.  sums: [CHS_CT_SUMS]; words: [CHS_CT_WORDS]; xw: the histogram's cells and its lengths added up.  The
// copies of the histograms are added into copy 0, the look's snapshot: a bin is its thread's alone.
__global__ __launch_bounds__(CT_FIN_THREADS) void k_ct_fin(const double* __restrict__ slots, const ct_u64* __restrict__ iws,
                                                           int groups, int bins, ct_u64* __restrict__ hist,
                                                           double* __restrict__ sums, ct_u64* __restrict__ words,
                                                           ct_i64* __restrict__ xw) {
  constexpr int NW = CT_FIN_THREADS / CHS_WAVE;
  static_assert(CT_FIN_THREADS >= CT_HCOPIES * CHS_CT_WORDS, "a thread of k_ct_fin per word of every copy");
  __shared__ double red[NW];
  __shared__ ct_u64 hs[2], ws[CHS_CT_WORDS];
  if (threadIdx.x < 2) hs[threadIdx.x] = 0;
  if (threadIdx.x < CHS_CT_WORDS) ws[threadIdx.x] = 0;
  ct_u64 wacc = 0;   // integer sums: order-free
  if (threadIdx.x < CT_HCOPIES * CHS_CT_WORDS) wacc = iws[threadIdx.x];   // (word threadIdx.x mod CHS_CT_WORDS of a copy)
#pragma unroll 1
  for (int w = 0; w < CHS_CT_SUMS; ++w) {
    double acc = 0.0;
    for (int g = threadIdx.x; g < groups; g += CT_FIN_THREADS) acc += slots[(size_t)g * CHS_CT_SUMS + w];
    acc = ct_block_sum<NW>(acc, red);
    if (threadIdx.x == 0) sums[w] = acc;
  }
  ct_u64 hc = 0, hl = 0;
  for (int i = threadIdx.x; i < bins; i += CT_FIN_THREADS) {
    ct_u64 c = 0, l = 0;
    for (int k = 0; k < CT_HCOPIES; ++k) { c += hist[(size_t)k * 2 * bins + i]; l += hist[(size_t)k * 2 * bins + bins + i]; }
    hist[i] = c; hist[bins + i] = l;
    hc += c; hl += l;
  }
  hc = ct_wave_sum(hc); hl = ct_wave_sum(hl);
  __syncthreads();   // (hs and ws are cleared)
  if (threadIdx.x % CHS_WAVE == 0) { atomicAdd(&hs[0], hc); atomicAdd(&hs[1], hl); }
  atomicAdd(&ws[threadIdx.x % CHS_CT_WORDS], wacc);
  __syncthreads();
  if (threadIdx.x == 0) { xw[0] = (ct_i64)hs[0]; xw[1] = (ct_i64)hs[1]; }
  if (threadIdx.x < CHS_CT_WORDS) words[threadIdx.x] = ws[threadIdx.x];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct CtResult {   // pinned
  ct_i64 words[CHS_CT_WORDS];
  double sums[CHS_CT_SUMS];
  ct_i64 xw[CT_NX];
};

struct CtBuf : LookBase {   // have: hist (and map, if have_map) are the look's snapshot, bins the histogram's length
  int bins = 0, gx = 0, gy = 0;
  bool have_map = false;
  double* slots = nullptr;      // [gx gy][CHS_CT_SUMS]
  ct_u64* hist = nullptr;       // [CT_HCOPIES][2][CHS_CT_MAX_BINS] allocated, [CT_HCOPIES][2][bins] used; after the look [2][bins]
  ct_u64* iws = nullptr;        // [CT_HCOPIES][CHS_CT_WORDS]
  ct_u64* words = nullptr;      // [CHS_CT_WORDS]
  double* sums = nullptr;       // [CHS_CT_SUMS]
  ct_i64* xw = nullptr;         // [CT_NX]
  double* map = nullptr;        // [2][N-1][N-1]: only while the last look asked for it
  CtResult* hRes = nullptr;
};

void ct_release(CtBuf* s) {
  if (!s) return;
  hipFree(s->slots); hipFree(s->hist); hipFree(s->iws); hipFree(s->words); hipFree(s->sums); hipFree(s->xw); hipFree(s->map);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int ct_alloc(CtBuf* s) {
  const int M = s->N - 1;
  s->gx = (M + CT_TW - 1) / CT_TW;
  s->gy = (M + CT_TH - 1) / CT_TH;
  CHS_HIP(hipMalloc(&s->slots, sizeof(double) * CHS_CT_SUMS * (size_t)s->gx * s->gy));
  CHS_HIP(hipMalloc(&s->hist, sizeof(ct_u64) * CT_HCOPIES * 2 * CHS_CT_MAX_BINS));
  CHS_HIP(hipMalloc(&s->iws, sizeof(ct_u64) * CT_HCOPIES * CHS_CT_WORDS));
  CHS_HIP(hipMalloc(&s->words, sizeof(ct_u64) * CHS_CT_WORDS));
  CHS_HIP(hipMalloc(&s->sums, sizeof(double) * CHS_CT_SUMS));
  CHS_HIP(hipMalloc(&s->xw, sizeof(ct_i64) * CT_NX));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(CtResult), hipHostMallocDefault));
  return CHS_OK;
}

int64_t ct_map_size(int N) { return 2 * (int64_t)(N - 1) * (N - 1); }

struct CtArgs {
  double t, kmax, scale;
  int bins;
};

template <typename T, int V, bool NT>
int ct_launch(const CtBuf* s, const void* U, const CtArgs& a, hipStream_t st) {
  k_ct_cells<T, V, NT><<<dim3(s->gx, s->gy), CT_THREADS, 0, st>>>(U, s->N, a.t, a.bins, a.kmax, a.scale, s->slots, s->hist, s->iws,
                                                                 s->have_map ? s->map : nullptr);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

// The sweep in the instantiation the field asks for: 16-byte loads where N is a multiple of the vector, element loads
// otherwise; non-temporal where the step loop's arrays fill the Infinity Cache (a read-once sweep must not displace them).
template <typename T>
int ct_sweep(const CtBuf* s, const void* U, const CtArgs& a, hipStream_t st) {
  constexpr int V = ChsVec<T>::V;
  const bool nt = chs_grid_exceeds_cache((size_t)s->N, sizeof(T));
  if (s->N % V == 0) return nt ? ct_launch<T, V, true>(s, U, a, st) : ct_launch<T, V, false>(s, U, a, st);
  return nt ? ct_launch<T, 1, true>(s, U, a, st) : ct_launch<T, 1, false>(s, U, a, st);
}

int ct_run(CtBuf* s, Engine* E, hipStream_t st, const CtArgs& a, bool want_map, const std::string& who) {
  const int groups = s->gx * s->gy;
  look_forget(s);
  // the map goes with the look that asked for it: a look without one hands its memory back
  s->have_map = false;
  if (!want_map && s->map) { CHS_HIP(hipFree(s->map)); s->map = nullptr; }
  if (want_map && !s->map) CHS_HIP(hipMalloc(&s->map, sizeof(double) * (size_t)ct_map_size(s->N)));
  s->have_map = want_map;
  s->bins = a.bins;
  CHS_HIP(hipMemsetAsync(s->iws, 0, sizeof(ct_u64) * CT_HCOPIES * CHS_CT_WORDS, st));
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(ct_u64) * CT_HCOPIES * 2 * (size_t)a.bins, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  const int rc = E->dtype == CHS_F64 ? ct_sweep<double>(s, E->dU, a, st) : ct_sweep<float>(s, E->dU, a, st);
  if (rc) return rc;
  k_ct_fin<<<1, CT_FIN_THREADS, 0, st>>>(s->slots, s->iws, groups, a.bins, s->hist, s->sums, s->words, s->xw);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CtResult* r = s->hRes;
  CHS_HIP(hipMemcpyAsync(r->words, s->words, sizeof(ct_i64) * CHS_CT_WORDS, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(r->sums, s->sums, sizeof(double) * CHS_CT_SUMS, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(r->xw, s->xw, sizeof(ct_i64) * CT_NX, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const ct_i64* w = r->words;
  std::string m;
  if (w[CHS_CT_SEGMENTS] != w[CHS_CT_CELLS_ONE] + w[CHS_CT_CELLS_TWO] + 2 * w[CHS_CT_SADDLES])
    m += " the segments are not the cells with one, two and three corners below and twice the saddles;";
  if (2 * w[CHS_CT_SEGMENTS] != 2 * (w[CHS_CT_VERTICES_ROWS] + w[CHS_CT_VERTICES_COLS]) - w[CHS_CT_ENDS])
    m += " the segments' ends are not the vertices, the inner ones twice;";
  if (w[CHS_CT_CELLS_CURV] + w[CHS_CT_CELLS_WALL] + w[CHS_CT_CELLS_BAD] != w[CHS_CT_CELLS_ONE] + w[CHS_CT_CELLS_TWO])
    m += " curvature, wall and bad cells do not add up to the crossed cells without the saddles;";
  if (r->xw[0] + w[CHS_CT_HIST_UNDER] + w[CHS_CT_HIST_OVER] != w[CHS_CT_CELLS_CURV])
    m += " the histogram and the cells under and over it do not add up to the curvature cells;";
  if (r->xw[1] > w[CHS_CT_L_CURV_FIX] || (w[CHS_CT_HIST_UNDER] + w[CHS_CT_HIST_OVER] == 0 && r->xw[1] != w[CHS_CT_L_CURV_FIX]))
    m += " the histogram's lengths do not add up to the length of the curvature cells;";
  const double txx = r->sums[CHS_CT_TXX], tyy = r->sums[CHS_CT_TYY];
  if (std::isfinite(txx) && std::isfinite(tyy)) {
    // txx + tyy of a segment is its l within 4 roundings, a saddle's ell one more, TXX + TYY one more: E + D + 8 roundings
    // of 2^-53 on sums of terms that are not negative; fix() cuts off less than 2^-30 a cell
    const double Et = 2.0 * CT_CPT + (double)((groups + CT_FIN_THREADS - 1) / CT_FIN_THREADS) - 1.0, D = 8 + 10;
    const double slack = (Et + D + 8.0) * 0x1p-53 * (txx + tyy) + (double)w[CHS_CT_SEGMENTS] * 0x1p-30;
    if (!(std::fabs(txx + tyy - (double)w[CHS_CT_L_FIX] * 0x1p-30) <= slack)) m += " TXX + TYY is not the length;";
  }
  if (!m.empty()) { chs_set_error(who + ": self-check failed:" + m); return CHS_ECHECK; }
  return look_end(s);
}
}  // namespace

void chs_ct_free(void** buf) {
  if (!buf) return;
  ct_release((CtBuf*)*buf);
  *buf = nullptr;
}

void chs_ct_forget(void* buf) {
  if (buf) look_forget((CtBuf*)buf);
}

int chs_ct_look(Engine* E, hipStream_t st, void** buf, double threshold, int32_t bins, double kmax, int32_t want_map,
                int64_t* words, double* sums, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(words, threshold, who))) return rc;
  if (!sums) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (bins < 1 || bins > CHS_CT_MAX_BINS) { chs_set_error(who + ": bins = " + std::to_string(bins) + " is outside [1, " + std::to_string(CHS_CT_MAX_BINS) + "]"); return CHS_EINVAL; }
  if (!std::isfinite(kmax) || !(kmax > 0.0)) { chs_set_error(who + ": kmax must be finite and above 0"); return CHS_EINVAL; }
  if (E->N < 2) { chs_set_error(who + ": N below 2"); return CHS_EINVAL; }
  if ((rc = look_check_field(E, CT_MAX_N, who))) return rc;
  if ((rc = look_buffers<CtBuf>(buf, E->N, ct_alloc, ct_release))) return rc;
  CtBuf* s = (CtBuf*)*buf;
  CtArgs a;
  a.t = threshold; a.kmax = kmax; a.bins = bins;
  a.scale = (double)bins / (2.0 * kmax);
  if ((rc = ct_run(s, E, st, a, want_map != 0, who))) return rc;
  memcpy(words, s->hRes->words, sizeof(int64_t) * CHS_CT_WORDS);
  memcpy(sums, s->hRes->sums, sizeof(double) * CHS_CT_SUMS);
  return CHS_OK;
}

int chs_ct_hist(void* buf, int device, hipStream_t st, int32_t bins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const CtBuf* s = (const CtBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (bins != s->bins) { chs_set_error(who + ": bins = " + std::to_string(bins) + ", expected " + std::to_string(s->bins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * 2 * (size_t)bins);
}

int chs_ct_map(void* buf, int device, hipStream_t st, int64_t n, double* out, const char* who_) {
  const std::string who(who_);
  const CtBuf* s = (const CtBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (!s->have_map) { chs_set_error(who + ": the last look was taken without the map"); return CHS_ESTATE; }
  if (n != ct_map_size(s->N)) { chs_set_error(who + ": n = " + std::to_string(n) + ", expected " + std::to_string(ct_map_size(s->N))); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->map, sizeof(double) * (size_t)n);
}

int chs_ct_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const CtBuf*)buf, ms, what);
}

extern "C" int chs_contour(chs_handle h, double threshold, int32_t bins, double kmax, int32_t want_map, int64_t words[CHS_CT_WORDS],
                           double sums[CHS_CT_SUMS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_contour: null handle"); return CHS_EINVAL; }
  return chs_ct_look(E, E->stream, &E->ct, threshold, bins, kmax, want_map, words, sums, "chs_contour");
}

extern "C" int chs_contour_hist(chs_handle h, int32_t bins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_contour_hist: null handle"); return CHS_EINVAL; }
  return chs_ct_hist(E->ct, E->hc.device, E->stream, bins, out, "chs_contour_hist");
}

extern "C" int chs_contour_map(chs_handle h, int64_t n, double* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_contour_map: null handle"); return CHS_EINVAL; }
  return chs_ct_map(E->ct, E->hc.device, E->stream, n, out, "chs_contour_map");
}

extern "C" int chs_contour_last_ms(chs_handle h, double* ms) {
  return chs_ct_last_ms(h, h ? ((Engine*)h)->ct : nullptr, ms, "chs_contour");
}

extern "C" int chs_contour_tile(int32_t* tile_w, int32_t* tile_h, int32_t* threads, int32_t* fin_threads) {
  if (!tile_w || !tile_h || !threads || !fin_threads) { chs_set_error("chs_contour_tile: null argument"); return CHS_EINVAL; }
  *tile_w = CT_TW;
  *tile_h = CT_TH;
  *threads = CT_THREADS;
  *fin_threads = CT_FIN_THREADS;
  return CHS_OK;
}
