// chs_geodesic.hip -- geodesic look at a phase of the thresholded field on the device: for every foreground pixel the cost
// of the shortest path through the phase from one wall of the box, its histogram (the accessible amount of phase by
// depth), the profile by depth and sixteen summary words -- tortuosity and reach (the definition:
// include/chs_hip.h, chs_geodesic).
//
// A geodesic look is a components look first: chs_cc_look leaves the root label L of every pixel on the handle's
// component buffers, -1 for background.  L is the mask here; the field itself is never read.  Then:
//   1  k_geo_init    G <- 0 at the foreground of the source wall, CHS_GEO_INF at the other foreground, -1 at background;
//                    the 64 x 64 tiles that hold a source, or read one through their halo, are flagged for round 1 (a
//                    source is a changed pixel like any other), the components that hold one are marked.
//   2  k_geo_relax   one launch per round over all tiles.  A workgroup whose tile is not flagged for this round returns.
//                    An active one clears its flag, loads tile and halo into LDS, relaxes its own pixels to the fixed point
//                    with the halo held fixed (chs_geo::relax_segment, counted sweeps), stores the pixels that fell and
//                    flags, for the next round, every neighbour tile that reads a changed border pixel through its halo
//                    (chs_geo::wakes).  The flags are double-buffered by round parity.  No workgroup waits for another:
//                    a halo word may be any earlier value of that word, which is the cost of a real path and not below
//                    the final one, so a stale halo delays the result and never falsifies it -- the neighbour that lowers
//                    the word afterwards flags this tile for the next round.  A workgroup stores to its own tile alone.
//                    ROUNDS is raised to the round of every active workgroup, PENDING to the round a flag is set for.
//      The host issues rounds GEO_CHUNK at a time and reads both words after each chunk: PENDING <= the rounds issued means
//      no flag is left and the map is final.
//   3  k_geo_stats, k_geo_fin   one sweep over G: words, histogram and profile by integer reductions, and the certificate
//                    (a) to (d) of the definition, which proves G to be the shortest-path costs.
// Everything is an integer and every accumulation a minimum, a maximum or an integer add.
#include <algorithm>
#include <cstring>

#include "chs_geo_host.h"
#include "chs_look.h"

#define GEO_THREADS CHS_GEO_THREADS
#define GEO_LBINS 4096                      // bins of a workgroup's LDS histogram
#define GEO_CHUNK 32                        // rounds the host issues between two looks at PENDING
#define GEO_FACTOR 32ll                     // chs_geodesic_rounds_default(N) = GEO_FACTOR nt^2 + GEO_SLACK
#define GEO_SLACK 64ll
#define GEO_MAX_FACTOR 16ll                 // max_rounds at most that many defaults
// the counters of a look
#define GEO_C_ROUNDS 0                      // the last round with an active workgroup
#define GEO_C_PENDING 1                     // the last round a tile was flagged for
#define GEO_C_ERR 2
#define GEO_NC 3
#define GEO_ERR_SWEEPS 1                    // the in-tile loop reached its cap
#define GEO_ERR_MARK 2                      // a source pixel without a component number

static_assert(GEO_THREADS == 256 && CHS_WAVE == 64, "a wavefront per 64-pixel row of a slab");
static_assert(CHS_GEO_UNREACHED == CHS_GEO_INF, "one word for unreached");
static_assert(CHS_GEO_T == CHS_WAVE, "k_geo_stats: a lane per column of the tile");

typedef long long geo_i64;
typedef unsigned long long geo_u64;
static_assert(sizeof(geo_i64) == sizeof(int64_t), "the result words are int64");

// depth of pixel (i, j) from the source wall, and its position along a wall
__host__ __device__ inline int geo_depth(int source, int N, int i, int j) {
  return source == 0 ? i : source == 1 ? N - 1 - i : source == 2 ? j : N - 1 - j;
}
__host__ __device__ inline int geo_along(int source, int i, int j) { return source < 2 ? j : i; }

struct GeoSum {
  geo_i64 fg, sources, reached, tfg, treached, gmin, gminpos, gsumt, gmax, gmaxfirst, gsum;
  geo_i64 viol;                // violations of the certificate
  geo_i64 ccr, cca, cct;       // k_geo_fin: marked components, their area, those of them that touch the target wall
};

__host__ __device__ inline GeoSum geo_zero() { return GeoSum{0, 0, 0, 0, 0, -1, -1, 0, -1, -1, 0, 0, 0, 0, 0}; }

__host__ __device__ inline GeoSum geo_add(const GeoSum& x, const GeoSum& y) {
  GeoSum s;
  s.fg = x.fg + y.fg; s.sources = x.sources + y.sources; s.reached = x.reached + y.reached; s.tfg = x.tfg + y.tfg;
  s.treached = x.treached + y.treached; s.gsumt = x.gsumt + y.gsumt; s.gsum = x.gsum + y.gsum; s.viol = x.viol + y.viol;
  s.ccr = x.ccr + y.ccr; s.cca = x.cca + y.cca; s.cct = x.cct + y.cct;
  // the smallest G on the target wall, at the smallest position (-1: none)
  const bool xm = x.gmin >= 0 && (y.gmin < 0 || x.gmin < y.gmin || (x.gmin == y.gmin && x.gminpos < y.gminpos));
  s.gmin = xm ? x.gmin : y.gmin; s.gminpos = xm ? x.gminpos : y.gminpos;
  // the largest G, at the smallest linear index (-1: none)
  const bool xM = x.gmax > y.gmax || (x.gmax == y.gmax && x.gmaxfirst < y.gmaxfirst);
  s.gmax = xM ? x.gmax : y.gmax; s.gmaxfirst = xM ? x.gmaxfirst : y.gmaxfirst;
  return s;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GEO_THREADS) void k_geo_init(const int* __restrict__ L, const int* __restrict__ id, int N, int conn,
                                                          int source, int count, int* __restrict__ G, unsigned* __restrict__ flags,
                                                          int* __restrict__ mark, unsigned* __restrict__ cnt) {
  const unsigned n2 = (unsigned)N * (unsigned)N;
  const unsigned p = blockIdx.x * (unsigned)GEO_THREADS + threadIdx.x;
  if (p >= n2) return;
  const int i = (int)(p / (unsigned)N), j = (int)(p - (unsigned)i * (unsigned)N);
  const int l = L[p];
  const bool src = l >= 0 && geo_depth(source, N, i, j) == 0;
  G[p] = l < 0 ? -1 : (src ? 0 : CHS_GEO_INF);
  if (!src) return;
  // a source pixel counts as changed: its tile and the tiles that read it through their halo are active in round 1
  const int nt = chs_geo::tiles_of(N), ti = i / CHS_GEO_T, tj = j / CHS_GEO_T;
  unsigned* f1 = flags + (size_t)nt * nt;                                       // parity 1
  f1[(size_t)ti * nt + tj] = 1u;
  const unsigned wake = chs_geo::wakes(conn, i - ti * CHS_GEO_T, j - tj * CHS_GEO_T);
#pragma unroll
  for (int k = 0; k < CHS_GEO_NB; ++k) {
    int di, dj;
    chs_geo::nb_of(k, &di, &dj);
    const int ni = ti + di, nj = tj + dj;
    if ((wake >> k & 1u) && ni >= 0 && ni < nt && nj >= 0 && nj < nt) f1[(size_t)ni * nt + nj] = 1u;
  }
  atomicMax(&cnt[GEO_C_PENDING], 1u);
  const int c = (unsigned)l < n2 ? id[l] : -1;
  if (c >= 0 && c < count) mark[c] = 1;
  else atomicOr(&cnt[GEO_C_ERR], (unsigned)GEO_ERR_MARK);
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------
// grid nt * nt, a workgroup per tile; thread t owns the pixels (t / 4, 16 (t % 4) .. + 16) of it.
__global__ __launch_bounds__(GEO_THREADS) void k_geo_relax(int* __restrict__ G, int N, int nt, int conn, int round,
                                                           unsigned* __restrict__ flags, unsigned* __restrict__ cnt) {
  __shared__ int S[CHS_GEO_P * CHS_GEO_P];
  __shared__ unsigned sact, swake;
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int ntiles = nt * nt;
  if (tid == 0) {
    unsigned* mine = flags + (size_t)(round & 1) * ntiles + tile;
    sact = *mine;
    swake = 0;
    if (sact) {
      *mine = 0;                                   // nobody sets a flag of this parity during this round
      atomicMax(&cnt[GEO_C_ROUNDS], (unsigned)round);
    }
  }
  __syncthreads();
  if (!sact) return;                               // (uniform)
  const int ti = tile / nt, tj = tile - ti * nt;
  const int i0 = ti * CHS_GEO_T, j0 = tj * CHS_GEO_T;
  for (int q = tid; q < CHS_GEO_P * CHS_GEO_P; q += GEO_THREADS) {
    const int lr = q / CHS_GEO_P, lc = q - lr * CHS_GEO_P;
    const int gi = i0 + lr - 1, gj = j0 + lc - 1;
    S[q] = (gi >= 0 && gi < N && gj >= 0 && gj < N) ? G[(size_t)gi * N + gj] : -1;
  }
  __syncthreads();
  const int r = tid / (CHS_GEO_T / CHS_GEO_SEG), c0 = (tid % (CHS_GEO_T / CHS_GEO_SEG)) * CHS_GEO_SEG;
  int* own = S + (r + 1) * CHS_GEO_P + c0 + 1;
  int v[CHS_GEO_SEG];
#pragma unroll
  for (int k = 0; k < CHS_GEO_SEG; ++k) v[k] = own[k];
  unsigned ever = 0;
  bool done = false;
#pragma unroll 1
  for (int n = 0; n < CHS_GEO_SWEEP_CAP; ++n) {
    const unsigned fell = chs_geo::relax_segment(S, conn, r, c0, v);
    __syncthreads();                               // every thread has read
#pragma unroll
    for (int k = 0; k < CHS_GEO_SEG; ++k)
      if (fell >> k & 1u) own[k] = v[k];
    ever |= fell;
    if (!__syncthreads_or(fell != 0)) { done = true; break; }
  }
  if (!done && tid == 0) atomicOr(&cnt[GEO_C_ERR], (unsigned)GEO_ERR_SWEEPS);
  // a pixel that fell was foreground inside the grid: the rows and columns of the tile beyond it hold -1 for ever
  unsigned wake = 0;
#pragma unroll
  for (int k = 0; k < CHS_GEO_SEG; ++k) {
    if (!(ever >> k & 1u)) continue;
    G[(size_t)(i0 + r) * N + j0 + c0 + k] = v[k];
    wake |= chs_geo::wakes(conn, r, c0 + k);
  }
  if (wake) atomicOr(&swake, wake);
  __syncthreads();
  if (tid < CHS_GEO_NB && (swake >> tid & 1u)) {
    int di, dj;
    chs_geo::nb_of(tid, &di, &dj);
    const int ni = ti + di, nj = tj + dj;
    if (ni >= 0 && ni < nt && nj >= 0 && nj < nt) {
      flags[(size_t)((round + 1) & 1) * ntiles + (size_t)ni * nt + nj] = 1u;
      atomicMax(&cnt[GEO_C_PENDING], (unsigned)(round + 1));
    }
  }
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ GeoSum geo_block_sum(GeoSum mine, GeoSum* red) {
  red[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll 1
  for (int off = GEO_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = geo_add(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  return red[0];
}

// The certificate at pixel (i, j) with word g against its neighbour word q over a step of cost w: returns violations;
// *pred is set where q is a predecessor of g.
__device__ __forceinline__ int geo_cert(int g, int q, int w, bool* pred) {
  if (q < 0) return 0;                                       // background or outside
  if (g == CHS_GEO_INF) return q != CHS_GEO_INF ? 1 : 0;     // (d)
  if (q == CHS_GEO_INF || q > g + w) return 1;               // (a), and (d) from the reached side
  if (q + w == g) *pred = true;
  return 0;
}

// grid nt * nt, a workgroup per 64 x 64 tile in 16 slabs of 4 rows: wavefront w takes row 4 s + w of slab s, its lanes
// the columns.  part[block] <- the summary of the tile; hist and prof by integer atomics.
__global__ __launch_bounds__(GEO_THREADS) void k_geo_stats(const int* __restrict__ G, const int* __restrict__ L, int N, int nt, int conn,
                                                           int source, int nbins, geo_u64* __restrict__ hist,
                                                           geo_u64* __restrict__ prof, GeoSum* __restrict__ part) {
  __shared__ int lh[GEO_LBINS];
  __shared__ GeoSum red[GEO_THREADS];
  __shared__ geo_u64 col[CHS_GEO_T][3];
  for (int k = threadIdx.x; k < GEO_LBINS; k += GEO_THREADS) lh[k] = 0;
  if (threadIdx.x < CHS_GEO_T) { col[threadIdx.x][0] = 0; col[threadIdx.x][1] = 0; col[threadIdx.x][2] = 0; }
  __syncthreads();
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
  const int j = tj * CHS_GEO_T + lane;
  const int a = chs_geo::unit_of(conn), d = chs_geo::diag_of(conn);
  const bool by_row = source < 2;
  GeoSum s = geo_zero();
  geo_i64 cfg = 0, cre = 0, csum = 0;                         // this thread's column, where the depth runs along columns
#pragma unroll 1
  for (int sl = 0; sl < CHS_GEO_T / 4; ++sl) {
    const int i = ti * CHS_GEO_T + sl * 4 + wave;
    const bool inb = i < N && j < N;
    int g = -1;
    geo_i64 rfg = 0, rre = 0, rsum = 0;
    if (inb) {
      const size_t p = (size_t)i * N + j;
      g = G[p];
      if (g < -1 || (g == -1) != (L[p] < 0)) s.viol += 1;    // the mask is that of the components look
    }
    if (g >= 0) {
      const int* c = G + (size_t)i * N + j;
      const bool up = i > 0, down = i + 1 < N, left = j > 0, right = j + 1 < N;
      const int k = geo_depth(source, N, i, j);
      bool pred = false;
      int bad = 0;
      bad += geo_cert(g, up ? c[-N] : -1, a, &pred);
      bad += geo_cert(g, down ? c[N] : -1, a, &pred);
      bad += geo_cert(g, left ? c[-1] : -1, a, &pred);
      bad += geo_cert(g, right ? c[1] : -1, a, &pred);
      if (d) {
        bad += geo_cert(g, (up && left) ? c[-N - 1] : -1, d, &pred);
        bad += geo_cert(g, (up && right) ? c[-N + 1] : -1, d, &pred);
        bad += geo_cert(g, (down && left) ? c[N - 1] : -1, d, &pred);
        bad += geo_cert(g, (down && right) ? c[N + 1] : -1, d, &pred);
      }
      if ((g == 0) != (k == 0)) bad += 1;                                    // (c)
      if (g > 0 && g != CHS_GEO_INF && !pred) bad += 1;                      // (b)
      s.viol += bad;
      s.fg += 1; rfg = 1;
      if (k == 0) s.sources += 1;
      if (k == N - 1) s.tfg += 1;
      if (g != CHS_GEO_INF) {
        s.reached += 1; s.gsum += g; rre = 1; rsum = g;
        const geo_i64 first = (geo_i64)i * N + j;
        if (g > s.gmax) { s.gmax = g; s.gmaxfirst = first; }                 // (the thread's pixels come in ascending order)
        if (k == N - 1) {
          s.treached += 1; s.gsumt += g;
          const int pos = geo_along(source, i, j);
          if (s.gmin < 0 || g < s.gmin) { s.gmin = g; s.gminpos = pos; }
        }
        int b = g / a;
        b = b < nbins - 1 ? b : nbins - 1;
        if (b < GEO_LBINS) atomicAdd(&lh[b], 1);
        else atomicAdd(&hist[b], (geo_u64)1);
      }
    }
    if (by_row) {                                           // (uniform) the row of this wavefront is one depth
#pragma unroll
      for (int off = CHS_WAVE / 2; off > 0; off >>= 1) {
        rfg += __shfl_down(rfg, off, CHS_WAVE); rre += __shfl_down(rre, off, CHS_WAVE); rsum += __shfl_down(rsum, off, CHS_WAVE);
      }
      if (lane == 0 && i < N && rfg) {
        geo_u64* q = prof + (size_t)geo_depth(source, N, i, 0) * 3;
        atomicAdd(q, (geo_u64)rfg);
        if (rre) { atomicAdd(q + 1, (geo_u64)rre); atomicAdd(q + 2, (geo_u64)rsum); }
      }
    } else {
      cfg += rfg; cre += rre; csum += rsum;
    }
  }
  if (!by_row) {
    if (cfg) {
      atomicAdd(&col[lane][0], (geo_u64)cfg);
      if (cre) { atomicAdd(&col[lane][1], (geo_u64)cre); atomicAdd(&col[lane][2], (geo_u64)csum); }
    }
    __syncthreads();
    if (threadIdx.x < CHS_GEO_T && j < N && col[lane][0]) {
      geo_u64* q = prof + (size_t)geo_depth(source, N, 0, j) * 3;
      atomicAdd(q, col[lane][0]);
      if (col[lane][1]) { atomicAdd(q + 1, col[lane][1]); atomicAdd(q + 2, col[lane][2]); }
    }
  }
  __syncthreads();
  const int top = nbins < GEO_LBINS ? nbins : GEO_LBINS;
  for (int k = threadIdx.x; k < top; k += GEO_THREADS) {
    const int c = lh[k];
    if (c) atomicAdd(&hist[k], (geo_u64)c);
  }
  s = geo_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: the parts, and the marked rows of the component table
__global__ __launch_bounds__(GEO_THREADS) void k_geo_fin(const GeoSum* __restrict__ part, int nparts, const int* __restrict__ table,
                                                         const int* __restrict__ mark, int count, int N, int source,
                                                         GeoSum* __restrict__ out) {
  __shared__ GeoSum red[GEO_THREADS];
  GeoSum s = geo_zero();
  for (int r = threadIdx.x; r < nparts; r += GEO_THREADS) s = geo_add(s, part[r]);
  for (int r = threadIdx.x; r < count; r += GEO_THREADS) {
    if (!mark[r]) continue;
    const int* row = table + (size_t)r * CHS_CC_COLS;         // first, area, imin, imax, jmin, jmax
    s.ccr += 1; s.cca += row[1];
    const bool touch = source == 0 ? row[3] == N - 1 : source == 1 ? row[2] == 0 : source == 2 ? row[5] == N - 1 : row[4] == 0;
    s.cct += touch ? 1 : 0;
  }
  s = geo_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct GeoResult {   // pinned
  unsigned cnt[GEO_NC];
  GeoSum out;
  int64_t words[CHS_GEO_WORDS];
};

struct GeoBuf : LookBase {   // have: G, hist and prof are the look's snapshot
  int nbins = 0, nt = 0;
  int* G = nullptr;             // [N * N]
  unsigned* flags = nullptr;    // [2][nt * nt]
  unsigned* cnt = nullptr;      // [GEO_NC]
  geo_u64* hist = nullptr;      // [nbins]
  geo_u64* prof = nullptr;      // [N][3]
  int* mark = nullptr;          // [cap] a component holds a source pixel
  int64_t cap = 0;
  GeoSum* part = nullptr;       // [nt * nt]
  GeoSum* out = nullptr;        // [1]
  GeoResult* hRes = nullptr;
  hipEvent_t evr[2] = {nullptr, nullptr};   // around the rounds
  double relax_ms = -1.0;
};

void geo_release(GeoBuf* s) {
  if (!s) return;
  hipFree(s->G); hipFree(s->flags); hipFree(s->cnt); hipFree(s->hist); hipFree(s->prof); hipFree(s->mark); hipFree(s->part);
  hipFree(s->out);
  if (s->hRes) hipHostFree(s->hRes);
  for (auto e : s->evr) if (e) hipEventDestroy(e);
  look_release_events(s);
  delete s;
}

int geo_alloc(GeoBuf* s) {
  const size_t n2 = (size_t)s->N * s->N;
  s->nbins = chs_geodesic_bins(s->N);
  s->nt = chs_geo::tiles_of(s->N);
  const size_t ntiles = (size_t)s->nt * s->nt;
  CHS_HIP(hipMalloc(&s->G, sizeof(int) * n2));
  CHS_HIP(hipMalloc(&s->flags, sizeof(unsigned) * 2 * ntiles));
  CHS_HIP(hipMalloc(&s->cnt, sizeof(unsigned) * GEO_NC));
  CHS_HIP(hipMalloc(&s->hist, sizeof(geo_u64) * (size_t)s->nbins));
  CHS_HIP(hipMalloc(&s->prof, sizeof(geo_u64) * 3 * (size_t)s->N));
  CHS_HIP(hipMalloc(&s->part, sizeof(GeoSum) * ntiles));
  CHS_HIP(hipMalloc(&s->out, sizeof(GeoSum)));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(GeoResult), hipHostMallocDefault));
  for (auto& e : s->evr) CHS_HIP(hipEventCreate(&e));
  return CHS_OK;
}

// The phases behind a components look that has just succeeded and left `cc`.
int geo_run(GeoBuf* s, hipStream_t st, const ChsCcSnapshot& cc, const int64_t* ccw, int conn, int source, int64_t limit,
            const std::string& who) {
  const int N = s->N, nt = s->nt, ntiles = nt * nt;
  const int64_t C = cc.count;
  look_forget(s);
  s->relax_ms = -1.0;
  if (C > s->cap) {   // the marks grow with the component table
    CHS_HIP(hipFree(s->mark));
    s->mark = nullptr; s->cap = 0;
    const int64_t cap = C + C / 8 + 1024;
    CHS_HIP(hipMalloc(&s->mark, sizeof(int) * (size_t)cap));
    s->cap = cap;
  }
  CHS_HIP(hipMemsetAsync(s->cnt, 0, sizeof(unsigned) * GEO_NC, st));
  CHS_HIP(hipMemsetAsync(s->flags, 0, sizeof(unsigned) * 2 * (size_t)ntiles, st));
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(geo_u64) * (size_t)s->nbins, st));
  CHS_HIP(hipMemsetAsync(s->prof, 0, sizeof(geo_u64) * 3 * (size_t)N, st));
  if (C > 0) CHS_HIP(hipMemsetAsync(s->mark, 0, sizeof(int) * (size_t)C, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  const int n2 = N * N;
  k_geo_init<<<(n2 + GEO_THREADS - 1) / GEO_THREADS, GEO_THREADS, 0, st>>>(cc.L, cc.id, N, conn, source, (int)C, s->G, s->flags, s->mark, s->cnt);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->evr[0], st));
  int64_t issued = 0, pending = 0;
  while (issued < limit) {
    const int64_t chunk = std::min<int64_t>(GEO_CHUNK, limit - issued);
    for (int64_t k = 0; k < chunk; ++k) {
      k_geo_relax<<<ntiles, GEO_THREADS, 0, st>>>(s->G, N, nt, conn, (int)(issued + k + 1), s->flags, s->cnt);
      CHS_HIP(hipGetLastError());
    }
    issued += chunk;
    CHS_HIP(hipMemcpyAsync(s->hRes->cnt, s->cnt, sizeof(unsigned) * GEO_NC, hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    pending = s->hRes->cnt[GEO_C_PENDING];
    if (s->hRes->cnt[GEO_C_ERR] || pending <= issued) break;
  }
  CHS_HIP(hipEventRecord(s->evr[1], st));
  int64_t* w = s->hRes->words;
  memset(w, 0, sizeof(int64_t) * CHS_GEO_WORDS);
  w[CHS_GEO_ROUNDS] = s->hRes->cnt[GEO_C_ROUNDS]; w[CHS_GEO_LIMIT] = limit;
  if (s->hRes->cnt[GEO_C_ERR]) {
    std::string m;
    if (s->hRes->cnt[GEO_C_ERR] & GEO_ERR_SWEEPS) m += " the in-tile loop (k_geo_relax) reached its cap;";
    if (s->hRes->cnt[GEO_C_ERR] & GEO_ERR_MARK) m += " a source pixel has no component number;";
    chs_set_error(who + ": self-check failed:" + m);
    return CHS_ECHECK;
  }
  if (pending > issued) {
    chs_set_error(who + ": tiles are still active after ROUNDS = " + std::to_string(w[CHS_GEO_ROUNDS]) + " rounds, max_rounds = " +
                  std::to_string(limit) + "; there is no geodesic result (the components look of this call is complete)");
    return CHS_ELIMIT;
  }
  k_geo_stats<<<ntiles, GEO_THREADS, 0, st>>>(s->G, cc.L, N, nt, conn, source, s->nbins, s->hist, s->prof, s->part);
  CHS_HIP(hipGetLastError());
  k_geo_fin<<<1, GEO_THREADS, 0, st>>>(s->part, ntiles, cc.table, s->mark, (int)C, N, source, s->out);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(&s->hRes->out, s->out, sizeof(GeoSum), hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const GeoSum& o = s->hRes->out;
  if (o.viol) {
    chs_set_error(who + ": self-check failed: " + std::to_string(o.viol) + " violations of the shortest-path certificate");
    return CHS_ECHECK;
  }
  if (o.reached != o.cca || (o.treached > 0) != (o.cct > 0) || o.reached > o.fg || o.fg != ccw[CHS_CC_AREA]) {
    chs_set_error(who + ": self-check failed: FG, REACHED, TARGET_REACHED = " + std::to_string(o.fg) + ", " + std::to_string(o.reached) +
                  ", " + std::to_string(o.treached) + "; the components look has the area " + std::to_string(ccw[CHS_CC_AREA]) +
                  ", its components with a source pixel the area " + std::to_string(o.cca) + ", " + std::to_string(o.cct) +
                  " of them at the target wall");
    return CHS_ECHECK;
  }
  w[CHS_GEO_FG] = o.fg; w[CHS_GEO_SOURCES] = o.sources; w[CHS_GEO_REACHED] = o.reached; w[CHS_GEO_TARGET_FG] = o.tfg;
  w[CHS_GEO_TARGET_REACHED] = o.treached; w[CHS_GEO_GMIN_TARGET] = o.gmin; w[CHS_GEO_GMIN_TARGET_POS] = o.gminpos;
  w[CHS_GEO_GSUM_TARGET] = o.gsumt; w[CHS_GEO_GMAX] = o.gmax; w[CHS_GEO_GMAX_FIRST] = o.gmaxfirst; w[CHS_GEO_GSUM] = o.gsum;
  w[CHS_GEO_UNIT] = chs_geo::unit_of(conn); w[CHS_GEO_CC_COUNT] = C; w[CHS_GEO_CC_REACHED] = o.ccr;
  float rms = 0.f;
  CHS_HIP(hipEventElapsedTime(&rms, s->evr[0], s->evr[1]));
  int rc;
  if ((rc = look_end(s))) return rc;
  s->relax_ms = rms;
  s->ms += cc.ms;   // the components look inside
  return CHS_OK;
}
}  // namespace

void chs_geo_free(void** buf) {
  if (!buf) return;
  geo_release((GeoBuf*)*buf);
  *buf = nullptr;
}

void chs_geo_forget(void* buf) {
  if (buf) look_forget((GeoBuf*)buf);
}

int chs_geo_look(Engine* E, hipStream_t st, void** ccbuf, void** buf, double threshold, int32_t connectivity, int32_t side,
                 int32_t source, int64_t max_rounds, int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  // the order of the components look: arguments, connectivity, side -- then this look's own, then the field
  if ((rc = look_check_args(out, threshold, who))) return rc;
  if (connectivity != 4 && connectivity != 8) { chs_set_error(who + ": the connectivity is 4 or 8"); return CHS_EINVAL; }
  if (side != CHS_CC_BELOW && side != CHS_CC_ABOVE) { chs_set_error(who + ": the side is CHS_CC_BELOW (0) or CHS_CC_ABOVE (1)"); return CHS_EINVAL; }
  if (source < 0 || source > 3) { chs_set_error(who + ": the source is a wall, 0 to 3"); return CHS_EINVAL; }
  const int64_t def = chs_geodesic_rounds_default(E->N);
  if (max_rounds < 0 || max_rounds > GEO_MAX_FACTOR * def) {
    chs_set_error(who + ": max_rounds = " + std::to_string(max_rounds) + " is outside [0, " + std::to_string(GEO_MAX_FACTOR * def) +
                  "] (0: the default, " + std::to_string(def) + ")");
    return CHS_EINVAL;
  }
  if (max_rounds == 0) max_rounds = def;
  int64_t ccw[CHS_CC_WORDS];
  if ((rc = chs_cc_look(E, st, ccbuf, threshold, connectivity, side, ccw, who_))) return rc;
  if ((rc = look_buffers<GeoBuf>(buf, E->N, geo_alloc, geo_release))) return rc;
  GeoBuf* s = (GeoBuf*)*buf;
  ChsCcSnapshot cc;
  if ((rc = chs_cc_snapshot(*ccbuf, &cc, who_))) return rc;
  rc = geo_run(s, st, cc, ccw, connectivity, source, max_rounds, who);
  if (rc == CHS_OK || rc == CHS_ELIMIT) memcpy(out, s->hRes->words, sizeof(int64_t) * CHS_GEO_WORDS);   // refused: ROUNDS and LIMIT
  return rc;
}

int chs_geo_hist(void* buf, int device, hipStream_t st, int32_t nbins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const GeoBuf* s = (const GeoBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (nbins != s->nbins) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(s->nbins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * (size_t)nbins);
}

int chs_geo_profile(void* buf, int device, hipStream_t st, int64_t* out, const char* who_) {
  const std::string who(who_);
  const GeoBuf* s = (const GeoBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->prof, sizeof(int64_t) * 3 * (size_t)s->N);
}

int chs_geo_map(void* buf, int device, hipStream_t st, int32_t* out, const char* who_) {
  const std::string who(who_);
  const GeoBuf* s = (const GeoBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->G, sizeof(int32_t) * (size_t)s->N * s->N);
}

int chs_geo_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const GeoBuf*)buf, ms, what);
}

int chs_geo_relax_ms(const void* h, const void* buf, double* ms, const char* what) {
  const std::string who = std::string(what) + "_relax_ms";
  const GeoBuf* s = (const GeoBuf*)buf;
  if (!h || !ms) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (!s || !s->have || s->relax_ms < 0.0) { chs_set_error(who + ": no " + what + " call so far"); return CHS_ESTATE; }
  *ms = s->relax_ms;
  return CHS_OK;
}

extern "C" int32_t chs_geodesic_bins(int32_t N) { return N < 1 ? 0 : 4 * N; }

extern "C" int64_t chs_geodesic_rounds_default(int32_t N) {
  if (N < 1) return 0;
  const int64_t nt = chs_geo::tiles_of(N);
  return GEO_FACTOR * nt * nt + GEO_SLACK;
}

extern "C" int chs_geodesic(chs_handle h, double threshold, int32_t connectivity, int32_t side, int32_t source, int64_t max_rounds,
                            int64_t out[CHS_GEO_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_geodesic: null handle"); return CHS_EINVAL; }
  return chs_geo_look(E, E->stream, &E->cc, &E->geo, threshold, connectivity, side, source, max_rounds, out, "chs_geodesic");
}

extern "C" int chs_geodesic_hist(chs_handle h, int32_t nbins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_geodesic_hist: null handle"); return CHS_EINVAL; }
  return chs_geo_hist(E->geo, E->hc.device, E->stream, nbins, out, "chs_geodesic_hist");
}

extern "C" int chs_geodesic_profile(chs_handle h, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_geodesic_profile: null handle"); return CHS_EINVAL; }
  return chs_geo_profile(E->geo, E->hc.device, E->stream, out, "chs_geodesic_profile");
}

extern "C" int chs_geodesic_map(chs_handle h, int32_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_geodesic_map: null handle"); return CHS_EINVAL; }
  return chs_geo_map(E->geo, E->hc.device, E->stream, out, "chs_geodesic_map");
}

extern "C" int chs_geodesic_last_ms(chs_handle h, double* ms) {
  return chs_geo_last_ms(h, h ? ((Engine*)h)->geo : nullptr, ms, "chs_geodesic");
}

extern "C" int chs_geodesic_relax_ms(chs_handle h, double* ms) {
  return chs_geo_relax_ms(h, h ? ((Engine*)h)->geo : nullptr, ms, "chs_geodesic");
}
