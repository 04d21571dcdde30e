// chs_thickness.hip -- local thickness of a phase of the thresholded field on the device: for every foreground pixel the
// squared radius of the largest disc that fits inside the phase and covers it, the area-weighted histogram of those radii
// (the pore-size distribution) and seven summary words (the definition: include/chs_hip.h,
// chs_thickness).
//
// A thickness look is a distance look first: chs_dt_look leaves the exact squared distances D2 on the handle's distance
// buffers.  Then, here, each phase a launch of its own -- no workgroup waits for another, nothing is polled:
//   1  k_th_select   a thread per pixel reads the 3 x 3 neighbourhood of D2 and evaluates the pruning rule of the
//                    definition: a centre c with R = D2[c] is dropped iff one of its 8 neighbours c + (a, b) has
//                    D2 > E(R, a, b), E the largest |q - (a, b)|^2 over the lattice points q of the open disc |q|^2 < R
//                    (th_reach: one function for the axis neighbours, one for the diagonal ones).  Then the disc of c
//                    lies inside that of the neighbour, whose value is larger.  The kept centres go into a list of
//                    (i << 16 | j, R), eight bytes each, appended a workgroup's centres at a time; KEPT is the list's counter and
//                    WORK the sum of their bounding boxes (2 rho + 1)^2, rho = isqrt(R - 1), both integer atomics.  A
//                    pixel of a grid without background gets T2 = CHS_DT_INF here: such a grid has no centre.
//   2  k_th_paint    reads WORK first and returns where it is above the limit.  A wavefront takes 64 list entries at a
//                    time.  The discs with rho <= TH_SMALL_RHO are painted by the lane that holds them; the others one
//                    after the other by the whole wavefront, over the bounding box clipped to the grid: a box at most 64
//                    pixels wide is covered 64 / width rows a pass, a wider one a row a pass with the lanes along it,
//                    between the ends of the row's chord.  A pixel is raised with atomicMax on the unsigned map, no
//                    value returned; a plain load before it skips the pixels that are at R already (the map only rises,
//                    so a stale value is a smaller one and skips nothing it should not).
//   3  k_th_stats, k_th_fin   one sweep over T2: the radius bins into an LDS histogram per workgroup, flushed by integer
//                    atomics, and the summary by per-workgroup partials and a one-workgroup finish, a fixed tree.
// Everything is an integer and every accumulation a maximum or an integer add: map, histogram and words do not depend on
// the order of anything.  The kernels read D2 and write this look's own arrays alone.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "chs_look.h"

#define TH_THREADS 256
#define TH_WAVES (TH_THREADS / CHS_WAVE)
#define TH_LBINS 4096                       // bins of a workgroup's LDS histogram
#define TH_PARTS 1024                       // workgroups of k_th_stats at most
#define TH_PAINT_GROUPS 2048                // workgroups of k_th_paint at most
#define TH_MAX_N 16384                      // that of the distance look: i and j fit 16 bits
#define TH_SEL_PIXELS 8                     // pixels of a thread of k_th_select
#define TH_SMALL_RHO 2                      // a disc up to 5 x 5 is painted by one lane
#define TH_K 16384ll                        // chs_thickness_work_default(N) = TH_K N^2: by the measured paint rate (DESIGN.md
                                            // section 3m, profiles/thickness.txt), inside [1024, 65536]
#define TH_MAX_FACTOR 16ll                  // max_work at most that many defaults
// the counters of a look
#define TH_C_KEPT 0                         // the kept centres found; the list holds min(KEPT, cap) of them
#define TH_C_ERR 1
#define TH_NC 2
#define TH_ERR_LIST 1                       // the list was full
#define TH_ERR_REACH 2                      // a scan of th_reach reached its cap

static_assert(CHS_WAVE == 64, "the ballots are 64-bit words");
static_assert(TH_MAX_N <= 65536, "i and j share a word of the list");

typedef long long th_i64;
typedef unsigned long long th_u64;
static_assert(sizeof(th_i64) == sizeof(int64_t), "the result words are int64");

struct ThSummary {
  th_i64 fg, t2max, nmax, sumt2, ninf, kept, work;
};
static_assert(sizeof(ThSummary) == CHS_TH_WORDS * sizeof(int64_t), "the summary is the seven int64 words");

__host__ __device__ inline ThSummary th_zero() { return ThSummary{0, 0, 0, 0, 0, 0, 0}; }
// the maximum and how often it occurs; every other word a sum
__host__ __device__ inline ThSummary th_add(const ThSummary& x, const ThSummary& y) {
  ThSummary s;
  s.fg = x.fg + y.fg; s.sumt2 = x.sumt2 + y.sumt2; s.ninf = x.ninf + y.ninf; s.kept = x.kept + y.kept; s.work = x.work + y.work;
  s.t2max = x.t2max > y.t2max ? x.t2max : y.t2max;
  s.nmax = (x.t2max == s.t2max ? x.nmax : 0) + (y.t2max == s.t2max ? y.nmax : 0);
  return s;
}

// k with k^2 <= v < (k+1)^2 for 0 <= v <= 2^30: the float root is off by one at most, two integer comparisons settle it
__host__ __device__ inline int th_isqrt(int v) {
  int k = (int)sqrtf((float)v);
  k -= (k * k > v) ? 1 : 0;
  k += ((k + 1) * (k + 1) <= v) ? 1 : 0;
  return k;
}

// E(R, a, b) for 1 <= R < CHS_DT_INF: the maximum of |q - (a, b)|^2 over the lattice points q with |q|^2 < R, for
// (a, b) an axis neighbour (diagonal == 0) or a diagonal one.  *capped is set where a scan ends at its cap (it cannot).
//   axis      with q = (-x, y), x >= 0: |q|^2 + 2 x + 1, and for a given x the largest |y| is y(x) = isqrt(R - 1 - x^2).
//             x down from rho: |q|^2 <= R - 1, so no x' <= x gives more than R + 2 x -- the scan stops there.
//   diagonal  with q = (-x, -y), x, y >= 0: |q|^2 + 2 (x + y) + 2, for a given x again at y(x).  The expression is
//             symmetric in x and y and rises with either, so the pairs with x >= y(x) suffice (a pair with x < y(x) is
//             below its mirror image (y(x), y(y(x))), whose first entry is larger: the chain ends at a pair with
//             x >= y).  These are the x from s = isqrt((R - 1) / 2) or s + 1 on: y(s) >= s and y(s + 1) <= s.  x up from
//             s: with r^2 = R - 1 and x > y(x), x lies beyond r / sqrt(2), where x + sqrt(r^2 - x^2) falls, so every
//             x' >= x has x' + y(x') <= x + sqrt(r^2 - x^2) < x + y(x) + 1 and gives less than R + 3 + 2 (x + y(x)) --
//             the scan stops there.  Near the diagonal x + y falls by about (x - r / sqrt(2))^2 sqrt(2) / r, so the scan
//             is a few sqrt(r) steps long.
// Both loops are counted: rho + 1 steps at most.
__host__ __device__ inline int th_reach(int R, int diagonal, int* capped) {
  const int rho = th_isqrt(R - 1);
  int best = 0;
  bool done = false;
  if (!diagonal) {
    int x = rho;
#pragma unroll 1
    for (int n = 0; n <= rho; ++n, --x) {
      if (R + 2 * x <= best) { done = true; break; }
      const int y = th_isqrt(R - 1 - x * x);
      const int v = x * x + y * y + 2 * x + 1;
      best = v > best ? v : best;
    }
    done = done || x < 0;
  } else {
    int x = th_isqrt((R - 1) / 2);
#pragma unroll 1
    for (int n = 0; n <= rho; ++n, ++x) {
      if (x > rho) { done = true; break; }
      const int y = th_isqrt(R - 1 - x * x);
      if (x > y && R + 3 + 2 * (x + y) <= best) { done = true; break; }
      const int v = x * x + y * y + 2 * (x + y) + 2;
      best = v > best ? v : best;
    }
    done = done || x > rho;
  }
  if (!done) *capped = 1;
  return best;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------
// Is the finite foreground pixel (i, j) with R = D2 a centre the rule keeps?  A neighbour outside the grid is masked; the
// background has D2 = 0, which is above no E: it drops nobody.
__device__ __forceinline__ bool th_keeps(const int* __restrict__ c, int N, int i, int j, int R, int rho, int* err) {
  const bool up = i > 0, down = i + 1 < N, left = j > 0, right = j + 1 < N;
  const int au = up ? c[-N] : 0, ad = down ? c[N] : 0, al = left ? c[-1] : 0, ar = right ? c[1] : 0;
  const int dul = (up && left) ? c[-N - 1] : 0, dur = (up && right) ? c[-N + 1] : 0;
  const int ddl = (down && left) ? c[N - 1] : 0, ddr = (down && right) ? c[N + 1] : 0;
  const int ma = max(max(au, ad), max(al, ar)), md = max(max(dul, dur), max(ddl, ddr));
  const int least = (rho + 1) * (rho + 1);   // both E are at least that: q = (-rho, 0)
  if (ma > least && ma > th_reach(R, 0, err)) return false;
  if (md > least && md > th_reach(R, 1, err)) return false;
  return true;
}

// grid ceil(N^2 / (TH_THREADS TH_SEL_PIXELS)): a workgroup owns TH_THREADS TH_SEL_PIXELS consecutive pixels, thread t the
// pixels t, t + TH_THREADS, ... of them.  It finds its centres first and then takes its part of the list with ONE
// atomicAdd on the list's counter (a prefix sum over the threads' counts places every centre) and adds its boxes to WORK
// with one more: two atomics on one address per wavefront made the kernel ten times slower at N = 4096.
__global__ __launch_bounds__(TH_THREADS) void k_th_select(const int* __restrict__ D2, int N, unsigned* __restrict__ T2,
                                                          uint2* __restrict__ list, unsigned cap, unsigned* __restrict__ cnt,
                                                          th_u64* __restrict__ work) {
  __shared__ unsigned wsum[TH_WAVES];
  __shared__ th_i64 wbox[TH_WAVES];
  __shared__ unsigned sbase;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const unsigned n2 = (unsigned)N * (unsigned)N;
  const unsigned p0 = blockIdx.x * (unsigned)(TH_THREADS * TH_SEL_PIXELS) + threadIdx.x;
  unsigned at[TH_SEL_PIXELS];   // i << 16 | j of the thread's pixels ...
  int Rs[TH_SEL_PIXELS];        // ... and D2 there, 0 where the pixel is no kept centre
  int err = 0;
  unsigned mine = 0;
  th_i64 box = 0;
#pragma unroll
  for (int k = 0; k < TH_SEL_PIXELS; ++k) {
    const unsigned p = p0 + (unsigned)(k * TH_THREADS);
    const bool inb = p < n2;
    const unsigned pc = inb ? p : n2 - 1;
    const int i = (int)(pc / (unsigned)N), j = (int)(pc - (unsigned)i * (unsigned)N);
    const int R = D2[pc];
    at[k] = ((unsigned)i << 16) | (unsigned)j;
    Rs[k] = 0;
    if (inb && R >= CHS_DT_INF) T2[pc] = (unsigned)CHS_DT_INF;
    if (inb && R > 0 && R < CHS_DT_INF) {
      const int rho = th_isqrt(R - 1);
      if (th_keeps(D2 + pc, N, i, j, R, rho, &err)) {
        Rs[k] = R;
        mine += 1;
        box += (th_i64)(2 * rho + 1) * (2 * rho + 1);
      }
    }
  }
  // the threads' counts: an inclusive prefix sum inside the wavefront, the wavefronts' sums through LDS
  unsigned incl = mine;
#pragma unroll
  for (int off = 1; off < CHS_WAVE; off <<= 1) {
    const unsigned v = __shfl_up(incl, off, CHS_WAVE);
    if (lane >= off) incl += v;
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) box += __shfl_down(box, off, CHS_WAVE);
  if (lane == CHS_WAVE - 1) wsum[wave] = incl;
  if (lane == 0) wbox[wave] = box;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < TH_WAVES; ++w) {
    before += w < wave ? wsum[w] : 0u;
    total += wsum[w];
  }
  if (threadIdx.x == 0 && total) {
    th_i64 b = 0;
#pragma unroll
    for (int w = 0; w < TH_WAVES; ++w) b += wbox[w];
    sbase = atomicAdd(&cnt[TH_C_KEPT], total);
    atomicAdd(work, (th_u64)b);
  }
  __syncthreads();
  if (total) {   // (uniform)
    unsigned slot = sbase + before + incl - mine;
#pragma unroll
    for (int k = 0; k < TH_SEL_PIXELS; ++k) {
      if (Rs[k] == 0) continue;
      if (slot < cap) list[slot] = make_uint2(at[k], (unsigned)Rs[k]);
      else err |= TH_ERR_LIST << 8;
      ++slot;
    }
  }
  if (err) atomicOr(&cnt[TH_C_ERR], (unsigned)(((err & 0xff) ? TH_ERR_REACH : 0) | (err >> 8)));
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void th_raise(unsigned* __restrict__ T2, int N, int y, int x, unsigned R) {
  unsigned* q = T2 + (size_t)y * N + x;
  if (*q < R) atomicMax(q, R);
}

// grid: at most TH_PAINT_GROUPS workgroups; wavefront g of all of them takes the list entries [64 c, 64 c + 64) for
// c = g, g + waves, ...  Every row and column is clipped to the grid before anything is addressed.
__global__ __launch_bounds__(TH_THREADS) void k_th_paint(const uint2* __restrict__ list, unsigned cap, const unsigned* __restrict__ cnt,
                                                         const th_u64* __restrict__ work, th_u64 max_work, int N,
                                                         unsigned* __restrict__ T2) {
  if (*work > max_work) return;   // (uniform over the grid) a refused look paints nothing
  const int lane = threadIdx.x & (CHS_WAVE - 1);
  const unsigned found = cnt[TH_C_KEPT];
  const unsigned kept = found < cap ? found : cap;
  const unsigned waves = gridDim.x * TH_WAVES, wave = blockIdx.x * TH_WAVES + threadIdx.x / CHS_WAVE;
  const unsigned chunks = (kept + CHS_WAVE - 1) / CHS_WAVE;
#pragma unroll 1
  for (unsigned c = wave; c < chunks; c += waves) {
    const unsigned e = c * CHS_WAVE + (unsigned)lane;
    const bool have = e < kept;
    const uint2 ent = list[have ? e : kept - 1];
    const int ci = (int)(ent.x >> 16), cj = (int)(ent.x & 0xffffu), R = (int)ent.y;
    const int rho = th_isqrt(R - 1);
    if (have && rho <= TH_SMALL_RHO) {
#pragma unroll 1
      for (int dy = -rho; dy <= rho; ++dy) {
        const int y = ci + dy;
        if (y < 0 || y >= N) continue;
        const int rem = R - 1 - dy * dy;
#pragma unroll 1
        for (int dx = -rho; dx <= rho; ++dx) {
          const int x = cj + dx;
          if (x >= 0 && x < N && dx * dx <= rem) th_raise(T2, N, y, x, (unsigned)R);
        }
      }
    }
    th_u64 big = __ballot(have && rho > TH_SMALL_RHO);
#pragma unroll 1
    for (int n = 0; n < CHS_WAVE; ++n) {   // a disc a step, CHS_WAVE of them at most
      if (!big) break;   // (uniform)
      const int src = __ffsll((long long)big) - 1;
      big &= big - 1;
      const int bi = __shfl(ci, src, CHS_WAVE), bj = __shfl(cj, src, CHS_WAVE), bR = __shfl(R, src, CHS_WAVE);
      const int brho = __shfl(rho, src, CHS_WAVE);
      const int dyLo = max(-brho, -bi), dyHi = min(brho, N - 1 - bi);
      const int dxLo = max(-brho, -bj), dxHi = min(brho, N - 1 - bj);
      const int w = dxHi - dxLo + 1;           // >= 1: the centre is inside
      if (w <= CHS_WAVE) {
        const int rpp = CHS_WAVE / w, lr = lane / w, lc = lane - lr * w;
        const int dx = dxLo + lc;
#pragma unroll 1
        for (int dy0 = dyLo; dy0 <= dyHi; dy0 += rpp) {
          const int dy = dy0 + lr;
          if (lr < rpp && dy <= dyHi && dx * dx <= bR - 1 - dy * dy) th_raise(T2, N, bi + dy, bj + dx, (unsigned)bR);
        }
      } else {
#pragma unroll 1
        for (int dy = dyLo; dy <= dyHi; ++dy) {
          const int span = th_isqrt(bR - 1 - dy * dy);
          const int lo = max(dxLo, -span), hi = min(dxHi, span);
#pragma unroll 1
          for (int dx = lo + lane; dx <= hi; dx += CHS_WAVE) th_raise(T2, N, bi + dy, bj + dx, (unsigned)bR);
        }
      }
    }
  }
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ ThSummary th_block_sum(ThSummary mine, ThSummary* red) {
  red[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll 1
  for (int off = TH_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = th_add(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  return red[0];
}

// part[block] <- the summary of pixels block TH_THREADS + tid, + gridDim.x TH_THREADS, ...; hist[k] += the block's
// foreground pixels of bin k.  A foreground pixel is one with T2 > 0.
__global__ __launch_bounds__(TH_THREADS) void k_th_stats(const unsigned* __restrict__ T2, int n2, int nbins, th_u64* __restrict__ hist,
                                                         ThSummary* __restrict__ part) {
  __shared__ int lh[TH_LBINS];
  __shared__ ThSummary red[TH_THREADS];
  for (int k = threadIdx.x; k < TH_LBINS; k += TH_THREADS) lh[k] = 0;
  __syncthreads();
  ThSummary s = th_zero();
  const int stride = gridDim.x * TH_THREADS;   // (at most TH_PARTS * TH_THREADS = 2^18: p + stride stays inside int32)
  for (int p = blockIdx.x * TH_THREADS + threadIdx.x; p < n2; p += stride) {
    const int d = (int)T2[p];
    if (d <= 0) continue;
    s.fg += 1;
    if (d >= CHS_DT_INF) { s.ninf += 1; continue; }
    s.sumt2 += d;
    if (d > s.t2max) { s.t2max = d; s.nmax = 1; }
    else if (d == s.t2max) s.nmax += 1;
    const int k = th_isqrt(d);
    if (k < TH_LBINS) atomicAdd(&lh[k], 1);
    else if (k < nbins) atomicAdd(&hist[k], (th_u64)1);
  }
  __syncthreads();
  const int top = nbins < TH_LBINS ? nbins : TH_LBINS;
  for (int k = threadIdx.x; k < top; k += TH_THREADS) {
    const int c = lh[k];
    if (c) atomicAdd(&hist[k], (th_u64)c);
  }
  s = th_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(TH_THREADS) void k_th_fin(const ThSummary* __restrict__ part, int nparts, const unsigned* __restrict__ cnt,
                                                       const th_u64* __restrict__ work, ThSummary* __restrict__ out) {
  __shared__ ThSummary red[TH_THREADS];
  ThSummary s = th_zero();
  for (int r = threadIdx.x; r < nparts; r += TH_THREADS) s = th_add(s, part[r]);
  s = th_block_sum(s, red);
  if (threadIdx.x == 0) {
    s.kept = cnt[TH_C_KEPT];
    s.work = (th_i64)*work;
    out[0] = s;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct ThResult {   // pinned
  unsigned cnt[TH_NC];
  ThSummary out;
};

struct ThBuf : LookBase {   // have: T2 and hist are the look's snapshot
  int nbins = 0;
  unsigned* T2 = nullptr;       // [N * N]
  uint2* list = nullptr;        // [N * N] the kept centres: every foreground pixel can be one (a field of isolated pixels)
  unsigned* cnt = nullptr;      // [TH_NC]
  th_u64* work = nullptr;       // [1]
  th_u64* hist = nullptr;       // [nbins]
  ThSummary* part = nullptr;    // [TH_PARTS]
  ThSummary* out = nullptr;     // [1]
  ThResult* hRes = nullptr;
};

void th_release(ThBuf* s) {
  if (!s) return;
  hipFree(s->T2); hipFree(s->list); hipFree(s->cnt); hipFree(s->work); hipFree(s->hist); hipFree(s->part); hipFree(s->out);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int th_alloc(ThBuf* s) {
  const size_t n2 = (size_t)s->N * s->N;
  s->nbins = chs_distance_bins(s->N);
  CHS_HIP(hipMalloc(&s->T2, sizeof(unsigned) * n2));
  CHS_HIP(hipMalloc(&s->list, sizeof(uint2) * n2));
  CHS_HIP(hipMalloc(&s->cnt, sizeof(unsigned) * TH_NC));
  CHS_HIP(hipMalloc(&s->work, sizeof(th_u64)));
  CHS_HIP(hipMalloc(&s->hist, sizeof(th_u64) * (size_t)s->nbins));
  CHS_HIP(hipMalloc(&s->part, sizeof(ThSummary) * TH_PARTS));
  CHS_HIP(hipMalloc(&s->out, sizeof(ThSummary)));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(ThResult), hipHostMallocDefault));
  return CHS_OK;
}

// The three phases behind a distance look that has just succeeded and left `dt`.
int th_run(ThBuf* s, hipStream_t st, const ChsDtSnapshot& dt, const int64_t* dtw, int64_t max_work, const std::string& who) {
  const int N = s->N, n2 = N * N;
  look_forget(s);
  CHS_HIP(hipMemsetAsync(s->cnt, 0, sizeof(unsigned) * TH_NC, st));
  CHS_HIP(hipMemsetAsync(s->work, 0, sizeof(th_u64), st));
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(th_u64) * (size_t)s->nbins, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  CHS_HIP(hipMemsetAsync(s->T2, 0, sizeof(unsigned) * (size_t)n2, st));
  const int blocks = (n2 + TH_THREADS - 1) / TH_THREADS;
  k_th_select<<<(blocks + TH_SEL_PIXELS - 1) / TH_SEL_PIXELS, TH_THREADS, 0, st>>>(dt.D2, N, s->T2, s->list, (unsigned)n2, s->cnt, s->work);
  CHS_HIP(hipGetLastError());
  const int groups = std::min((blocks + TH_WAVES - 1) / TH_WAVES, TH_PAINT_GROUPS);   // a wavefront per 64 pixels is enough
  k_th_paint<<<groups, TH_THREADS, 0, st>>>(s->list, (unsigned)n2, s->cnt, s->work, (th_u64)max_work, N, s->T2);
  CHS_HIP(hipGetLastError());
  const int parts = std::min(blocks, TH_PARTS);
  k_th_stats<<<parts, TH_THREADS, 0, st>>>(s->T2, n2, s->nbins, s->hist, s->part);
  CHS_HIP(hipGetLastError());
  k_th_fin<<<1, TH_THREADS, 0, st>>>(s->part, parts, s->cnt, s->work, s->out);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->cnt, s->cnt, sizeof(unsigned) * TH_NC, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(&s->hRes->out, s->out, sizeof(ThSummary), hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const ThSummary& o = s->hRes->out;
  if (s->hRes->cnt[TH_C_ERR]) {
    std::string m;
    if (s->hRes->cnt[TH_C_ERR] & TH_ERR_LIST) m += " the list of centres was full;";
    if (s->hRes->cnt[TH_C_ERR] & TH_ERR_REACH) m += " a scan of the reach (k_th_select) reached its cap;";
    chs_set_error(who + ": self-check failed:" + m);
    return CHS_ECHECK;
  }
  if (o.work > max_work) {
    chs_set_error(who + ": the look needs WORK = " + std::to_string(o.work) + " disc pixels, max_work = " + std::to_string(max_work) +
                  "; nothing was painted (the distance look of this call is complete)");
    return CHS_ELIMIT;
  }
  if (o.fg != dtw[CHS_DT_FG] || o.t2max != dtw[CHS_DT_D2MAX] || o.ninf != dtw[CHS_DT_NINF]) {
    chs_set_error(who + ": self-check failed: FG, T2MAX, NINF = " + std::to_string(o.fg) + ", " + std::to_string(o.t2max) + ", " +
                  std::to_string(o.ninf) + ", the distance look has " + std::to_string(dtw[CHS_DT_FG]) + ", " +
                  std::to_string(dtw[CHS_DT_D2MAX]) + ", " + std::to_string(dtw[CHS_DT_NINF]));
    return CHS_ECHECK;
  }
  int rc;
  if ((rc = look_end(s))) return rc;
  s->ms += dt.ms;   // the distance look inside
  return CHS_OK;
}
}  // namespace

void chs_th_free(void** buf) {
  if (!buf) return;
  th_release((ThBuf*)*buf);
  *buf = nullptr;
}

void chs_th_forget(void* buf) {
  if (buf) look_forget((ThBuf*)buf);
}

int chs_th_look(Engine* E, hipStream_t st, void** dtbuf, void** buf, double threshold, int32_t side, int64_t max_work,
                int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  const int64_t def = chs_thickness_work_default(E->N);
  if (max_work < 0 || max_work > TH_MAX_FACTOR * def) {
    chs_set_error(who + ": max_work = " + std::to_string(max_work) + " is outside [0, " + std::to_string(TH_MAX_FACTOR * def) +
                  "] (0: the default, " + std::to_string(def) + ")");
    return CHS_EINVAL;
  }
  if (max_work == 0) max_work = def;
  int64_t dtw[CHS_DT_WORDS];
  // the distance look: its own checks of side and field, in its own order, under this look's name
  if ((rc = chs_dt_look(E, st, dtbuf, threshold, side, dtw, who_))) return rc;
  if ((rc = look_buffers<ThBuf>(buf, E->N, th_alloc, th_release))) return rc;
  ThBuf* s = (ThBuf*)*buf;
  ChsDtSnapshot dt;
  if ((rc = chs_dt_snapshot(*dtbuf, &dt, who_))) return rc;
  rc = th_run(s, st, dt, dtw, max_work, who);
  if (rc == CHS_ELIMIT) {   // what the refusal is about, for the caller; no other word means anything
    memset(out, 0, sizeof(int64_t) * CHS_TH_WORDS);
    out[CHS_TH_KEPT] = s->hRes->out.kept; out[CHS_TH_WORK] = s->hRes->out.work;
  }
  if (rc) return rc;
  memcpy(out, &s->hRes->out, sizeof(int64_t) * CHS_TH_WORDS);
  return CHS_OK;
}

int chs_th_hist(void* buf, int device, hipStream_t st, int32_t nbins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const ThBuf* s = (const ThBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (nbins != s->nbins) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(s->nbins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * (size_t)nbins);
}

int chs_th_map(void* buf, int device, hipStream_t st, int32_t* out, const char* who_) {
  const std::string who(who_);
  const ThBuf* s = (const ThBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->T2, sizeof(int32_t) * (size_t)s->N * s->N);
}

int chs_th_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const ThBuf*)buf, ms, what);
}

extern "C" int64_t chs_thickness_work_default(int32_t N) {
  if (N < 1) return 0;
  return TH_K * (int64_t)N * (int64_t)N;
}

extern "C" int32_t chs_thickness_reach(int32_t R, int32_t diagonal) {
  if (R < 1 || R >= CHS_DT_INF) return 0;
  int capped = 0;
  return th_reach(R, diagonal ? 1 : 0, &capped);
}

extern "C" int chs_thickness(chs_handle h, double threshold, int32_t side, int64_t max_work, int64_t out[CHS_TH_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_thickness: null handle"); return CHS_EINVAL; }
  return chs_th_look(E, E->stream, &E->dt, &E->th, threshold, side, max_work, out, "chs_thickness");
}

extern "C" int chs_thickness_hist(chs_handle h, int32_t nbins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_thickness_hist: null handle"); return CHS_EINVAL; }
  return chs_th_hist(E->th, E->hc.device, E->stream, nbins, out, "chs_thickness_hist");
}

extern "C" int chs_thickness_map(chs_handle h, int32_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_thickness_map: null handle"); return CHS_EINVAL; }
  return chs_th_map(E->th, E->hc.device, E->stream, out, "chs_thickness_map");
}

extern "C" int chs_thickness_last_ms(chs_handle h, double* ms) {
  return chs_th_last_ms(h, h ? ((Engine*)h)->th : nullptr, ms, "chs_thickness");
}
