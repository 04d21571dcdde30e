// chs_distance.hip -- exact squared Euclidean distance transform of the thresholded field on the device: domain widths,
// the widest point, the histogram of local radii (the definition: include/chs_hip.h, chs_distance).
//
// The separable transform: a vertical pass gives G[i][j], the distance from (i, j) to the nearest background pixel of
// column j (CHS_DT_INF if the column has none); a horizontal pass gives D2[i][j] = min over l of (j - l)^2 + G[i][l]^2.
// Phases that depend on each other are separate launches: no workgroup ever waits for another one, nothing is polled.
//   1a k_dt_mask   a workgroup thresholds one band of CHS_DT_BAND rows of a column strip (16-byte loads where N allows,
//                  no load guarded by a branch).  A band of a column is ONE 64-bit word, bit r = row r of the band is
//                  background: the scan inside the band is then two bit counts per pixel (the leading zeros above, the
//                  trailing zeros below), and what the pass stores is N^2 / 8 bytes instead of an N x N array.
//   1b k_dt_carry  the bands joined: a thread per column and direction walks the column's N / CHS_DT_BAND words down, or
//                  up, and leaves, per band, the nearest background row before the band, or the nearest one behind it.
//   2  k_dt_rows   a workgroup owns a whole row.  It combines word and carries into G and stages h[l] = G[i][l]^2 in
//                  LDS (INF stays INF) -- G itself is never written: the third launch of the vertical pass and the
//                  staging of the horizontal one are the same sweep.  Then, per pixel j, one lane:
//                      best = h[j];  for d = 1, 2, ...: stop when d^2 >= best or both j - d and j + d are outside;
//                      best = min(best, d^2 + h[j - d], d^2 + h[j + d])
//                  `best` never rises and every candidate at distance d is at least d^2, so nothing beyond the stop can
//                  improve it: exact.  The search covers ceil(sqrt(D2)) distances -- the pixel's own -- and at most
//                  N - 1, two of them per step of its loop; the loop's cap cannot be reached, and reaching it all the
//                  same sets a bit of the error word.
//                  A row without a finite h (a grid without background) is written as INF without a search.
//   3  k_dt_stats, k_dt_fin   one sweep over D2: the radius bins into an LDS histogram per workgroup (integer atomics;
//                  bins beyond it straight to global memory), flushed into the int64 histogram by atomicAdd -- integer
//                  sums, order-free -- and the five summary words by per-workgroup partials and a one-workgroup finish:
//                  a fixed tree, the widest point being the maximum of (D2, -index), a total order.
// Nothing of the handle is written and nothing the step loop owns is read: its field alone.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "chs_look.h"
#include "chs_cc_host.h"   // chs_cc::fg_of: the foreground is that of chs_components

#define CHS_DT_BAND 64                      // rows of a band: the bits of one word
#define CHS_DT_CHUNK CHS_WAVE               // consecutive pixels of a row one wavefront pass of k_dt_rows covers
#define DT_THREADS 256
#define DT_LBINS 4096                       // bins of a workgroup's LDS histogram
#define DT_PARTS 1024                       // workgroups of k_dt_stats at most
#define DT_MAX_N 16384                      // 4 N bytes of LDS hold a row; 2 (N-1)^2 < CHS_DT_INF
#define DT_UP_NONE (-CHS_DT_INF)            // no background row before the band: i - DT_UP_NONE >= CHS_DT_INF
#define DT_DN_NONE (CHS_DT_INF + DT_MAX_N)  // none behind it: DT_DN_NONE - i >= CHS_DT_INF
// the words of a look
#define DT_W_ERR 0
#define DT_NW 2
#define DT_ERR_ROW 1                        // the search of k_dt_rows reached its cap

static_assert(CHS_DT_BAND == 64, "a band of a column is one 64-bit word");
static_assert(2ll * (DT_MAX_N - 1) * (DT_MAX_N - 1) < CHS_DT_INF, "every finite D2 is below CHS_DT_INF");
static_assert((long long)DT_DN_NONE < (1ll << 31) && (long long)DT_MAX_N + CHS_DT_INF < (1ll << 31), "the carries stay inside int32");

typedef long long dt_i64;
typedef unsigned long long dt_u64;
static_assert(sizeof(dt_i64) == sizeof(int64_t), "the result words are int64");

struct DtSummary {
  dt_i64 fg, d2max, first, sumd2, ninf;
};
static_assert(sizeof(DtSummary) == CHS_DT_WORDS * sizeof(int64_t), "the summary is the five int64 words");

__host__ __device__ inline DtSummary dt_zero() { return DtSummary{0, 0, -1, 0, 0}; }
// the widest point: the maximum of (D2, -index); a partial without a finite foreground pixel has first == -1
__host__ __device__ inline DtSummary dt_add(const DtSummary& x, const DtSummary& y) {
  DtSummary s;
  s.fg = x.fg + y.fg; s.sumd2 = x.sumd2 + y.sumd2; s.ninf = x.ninf + y.ninf;
  const bool xw = x.d2max > y.d2max || (x.d2max == y.d2max && (y.first < 0 || (x.first >= 0 && x.first < y.first)));
  s.d2max = xw ? x.d2max : y.d2max;
  s.first = xw ? x.first : y.first;
  return s;
}

// (dt_isqrt, the radius bin: chs_look.h)

// ---- phase 1a --------------------------------------------------------------------------------------------------------
// grid (column strips, bands).  V: pixels per load (16 bytes where N is a multiple of V, else 1); a thread owns the V
// columns from (blockIdx.x DT_THREADS + tid) V on and the band's 64 rows of them.  A row or column outside the grid is
// clamped to one inside and masked: its bit stays 0, as if it were foreground, so it is nobody's nearest background.
template <typename T, int V, bool NT>
__global__ __launch_bounds__(DT_THREADS) void k_dt_mask(const void* Uv, int N, double t, int above, dt_u64* __restrict__ mask) {
  typedef const typename ChsVec<T>::type CHS_GLOBAL* VP;
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const int j = (blockIdx.x * DT_THREADS + threadIdx.x) * V, i0 = blockIdx.y * CHS_DT_BAND;
  const bool inside = j < N;   // (V > 1: N and j are multiples of V, so j < N is j + V - 1 < N)
  const T CHS_GLOBAL* col = U + (inside ? j : N - V);
  dt_u64 m[V];
#pragma unroll
  for (int e = 0; e < V; ++e) m[e] = 0;
#pragma unroll 8
  for (int r = 0; r < CHS_DT_BAND; ++r) {
    const int i = i0 + r;
    const T CHS_GLOBAL* src = col + (size_t)(i < N ? i : N - 1) * N;
    T x[V];
    // (chs_load of chs_look.h, written out: behind the call the compiler schedules this unrolled loop otherwise)
    if constexpr (V == 1) {
      x[0] = NT ? __builtin_nontemporal_load(src) : *src;
    } else {
      const typename ChsVec<T>::type v = NT ? __builtin_nontemporal_load(reinterpret_cast<VP>(src)) : *reinterpret_cast<VP>(src);
#pragma unroll
      for (int e = 0; e < V; ++e) x[e] = v[e];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool bg = i < N && !chs_cc::fg_of((double)x[e], t, above);
      m[e] |= (dt_u64)(bg ? 1 : 0) << r;
    }
  }
  if (inside) {
#pragma unroll
    for (int e = 0; e < V; ++e) mask[(size_t)blockIdx.y * N + j + e] = m[e];
  }
}

// ---- phase 1b --------------------------------------------------------------------------------------------------------
// grid (column blocks, 2): blockIdx.y == 0 walks the bands down and leaves up[b][j], the last background row of column
// j before band b (DT_UP_NONE without one); blockIdx.y == 1 walks them up and leaves dn[b][j], the first one behind band
// b (DT_DN_NONE).  A thread owns a column.  The words are loaded DT_CARRY_AHEAD at a time before they are used: the walk
// is nb steps long, and with one load per step it is nb memory latencies long (29 us of a 0.21 ms look at N = 4096).
// Counted loops; a band beyond the last is clamped for the load and skipped.
#define DT_CARRY_AHEAD 8
__global__ __launch_bounds__(DT_THREADS) void k_dt_carry(const dt_u64* __restrict__ mask, int N, int nb, int* __restrict__ up,
                                                         int* __restrict__ dn) {
  const int j = blockIdx.x * DT_THREADS + threadIdx.x;
  if (j >= N) return;
  const bool down = blockIdx.y == 0;   // (uniform)
  int* __restrict__ out = down ? up : dn;
  int carry = down ? DT_UP_NONE : DT_DN_NONE;
  for (int s0 = 0; s0 < nb; s0 += DT_CARRY_AHEAD) {
    dt_u64 m[DT_CARRY_AHEAD];
#pragma unroll
    for (int k = 0; k < DT_CARRY_AHEAD; ++k) {
      const int s = s0 + k < nb ? s0 + k : nb - 1;
      m[k] = mask[(size_t)(down ? s : nb - 1 - s) * N + j];
    }
#pragma unroll
    for (int k = 0; k < DT_CARRY_AHEAD; ++k) {
      if (s0 + k >= nb) break;
      const int b = down ? s0 + k : nb - 1 - (s0 + k);
      out[(size_t)b * N + j] = carry;
      if (m[k]) carry = b * CHS_DT_BAND + (down ? 63 - __clzll((dt_i64)m[k]) : __ffsll((dt_i64)m[k]) - 1);
    }
  }
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------------
// grid N: workgroup i owns row i; N ints of dynamic LDS.  Pixel l of the row is thread l % DT_THREADS's: a wavefront
// pass covers CHS_DT_CHUNK consecutive pixels, whose searches are about equally long and whose LDS reads h[l -+ d] are
// consecutive words.
__global__ __launch_bounds__(DT_THREADS) void k_dt_rows(const dt_u64* __restrict__ mask, const int* __restrict__ up,
                                                        const int* __restrict__ dn, int N, int* __restrict__ D2,
                                                        int* __restrict__ words) {
  extern __shared__ int h[];
  const int i = blockIdx.x, b = i / CHS_DT_BAND, r = i % CHS_DT_BAND;
  const size_t band = (size_t)b * N, row = (size_t)i * N;
  int finite = 0;
  for (int l = threadIdx.x; l < N; l += DT_THREADS) {
    const dt_u64 m = mask[band + l];
    // The carries are loaded whatever the word says -- three loads in flight, not a wait for the word and then a branch
    // around each of the other two, which is where the compiler would sink them.
    int cu = up[band + l], cd = dn[band + l];
    asm volatile("" : "+v"(cu), "+v"(cd));
    const int before = i - cu, behind = cd - i;
    const dt_u64 low = m << (63 - r), high = m >> r;   // the band's rows up to i, from i on
    const int upd = low ? __clzll((dt_i64)low) : before;
    const int dnd = high ? __ffsll((dt_i64)high) - 1 : behind;
    const int g = upd < dnd ? upd : dnd;
    const int gc = g < (1 << 15) ? g : (1 << 15);      // (g < N where it is finite; the product stays inside int32)
    const int v = g >= CHS_DT_INF ? CHS_DT_INF : gc * gc;
    h[l] = v;
    finite |= (v < CHS_DT_INF) ? 1 : 0;
  }
  finite = __syncthreads_or(finite);
  if (!finite) {   // (uniform) no column of the grid has a background pixel
    for (int l = threadIdx.x; l < N; l += DT_THREADS) D2[row + l] = CHS_DT_INF;
    return;
  }
  // A side that has left the row is clamped to the row's end instead of being branched around: the end pixel is
  // nearer than d, so d^2 + h[end] is above a candidate the search has seen already and changes nothing.
  int err = 0;
  const int last = N - 1;
  for (int l = threadIdx.x; l < N; l += DT_THREADS) {
    int best = h[l];
    const int dmax = l > last - l ? l : last - l;   // beyond it both sides are outside
    int d = 1, dd = 1;
    bool done = false;
#pragma unroll 1
    // Two distances a step, d and d + 1 -- four LDS reads in flight behind one wait.  The candidates of d + 1 are taken
    // even where d + 1 is beyond the stop: every candidate is the squared distance to a background pixel (or above
    // one), so a candidate more never puts `best` below D2.
    for (int n = 0; n < N + 2; n += 2) {   // d = n + 1 and dmax <= N - 1: at n = N at the latest d > dmax, the cap is never used up
      if (dd >= best || d > dmax) { done = true; break; }
      const int lo = l - d > 0 ? l - d : 0, hi = l + d < last ? l + d : last;
      const int lo2 = lo > 0 ? lo - 1 : 0, hi2 = hi < last ? hi + 1 : last;
      const int a = h[lo], b = h[hi], a2 = h[lo2], b2 = h[hi2];
      const int c = dd + (a < b ? a : b), c2 = dd + 2 * d + 1 + (a2 < b2 ? a2 : b2);
      best = c < best ? c : best;
      best = c2 < best ? c2 : best;
      dd += 4 * d + 4;
      d += 2;
    }
    if (!done) err |= DT_ERR_ROW;
    D2[row + l] = best;
  }
  if (err) atomicOr(&words[DT_W_ERR], err);
}

// ---- phase 3 ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ DtSummary dt_block_sum(DtSummary mine, DtSummary* red) {
  red[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll 1
  for (int off = DT_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = dt_add(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  return red[0];
}

// part[block] <- the summary of pixels block DT_THREADS + tid, + gridDim.x DT_THREADS, ... (a thread adds its pixels in
// ascending order); hist[k] += the block's foreground pixels of bin k.  A foreground pixel is one with D2 > 0.
__global__ __launch_bounds__(DT_THREADS) void k_dt_stats(const int* __restrict__ D2, int n2, int nbins, dt_u64* __restrict__ hist,
                                                         DtSummary* __restrict__ part) {
  __shared__ int lh[DT_LBINS];
  __shared__ DtSummary red[DT_THREADS];
  for (int k = threadIdx.x; k < DT_LBINS; k += DT_THREADS) lh[k] = 0;
  __syncthreads();
  DtSummary s = dt_zero();
  const int stride = gridDim.x * DT_THREADS;   // (at most DT_PARTS * DT_THREADS = 2^18: p + stride stays inside int32)
  for (int p = blockIdx.x * DT_THREADS + threadIdx.x; p < n2; p += stride) {
    const int d = D2[p];
    if (d <= 0) continue;
    s.fg += 1;
    if (d >= CHS_DT_INF) { s.ninf += 1; continue; }
    s.sumd2 += d;
    if (d > s.d2max) { s.d2max = d; s.first = p; }   // (ascending p: the first index of the maximum stays)
    const int k = dt_isqrt(d);
    if (k < DT_LBINS) atomicAdd(&lh[k], 1);
    else if (k < nbins) atomicAdd(&hist[k], (dt_u64)1);
  }
  __syncthreads();
  const int top = nbins < DT_LBINS ? nbins : DT_LBINS;
  for (int k = threadIdx.x; k < top; k += DT_THREADS) {
    const int c = lh[k];
    if (c) atomicAdd(&hist[k], (dt_u64)c);
  }
  s = dt_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(DT_THREADS) void k_dt_fin(const DtSummary* __restrict__ part, int nparts, DtSummary* __restrict__ out) {
  __shared__ DtSummary red[DT_THREADS];
  DtSummary s = dt_zero();
  for (int r = threadIdx.x; r < nparts; r += DT_THREADS) s = dt_add(s, part[r]);
  s = dt_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct DtResult {   // pinned
  int words[DT_NW];
  DtSummary out;
};

struct DtBuf : LookBase {   // have: D2 and hist are the look's snapshot
  int nb = 0, nbins = 0;
  int* D2 = nullptr;            // [N * N]
  dt_u64* mask = nullptr;       // [nb][N] the background bits of every band of every column
  int* up = nullptr;            // [nb][N] the carries
  int* dn = nullptr;
  dt_u64* hist = nullptr;       // [nbins]
  DtSummary* part = nullptr;    // [DT_PARTS]
  DtSummary* out = nullptr;     // [1]
  int* words = nullptr;         // [DT_NW]
  DtResult* hRes = nullptr;
};

void dt_release(DtBuf* s) {
  if (!s) return;
  hipFree(s->D2); hipFree(s->mask); hipFree(s->up); hipFree(s->dn); hipFree(s->hist); hipFree(s->part); hipFree(s->out); hipFree(s->words);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int dt_alloc(DtBuf* s) {
  const int N = s->N;
  s->nb = (N + CHS_DT_BAND - 1) / CHS_DT_BAND;
  s->nbins = chs_distance_bins(N);
  const size_t n2 = (size_t)N * N, nc = (size_t)s->nb * N;
  CHS_HIP(hipMalloc(&s->D2, sizeof(int) * n2));
  CHS_HIP(hipMalloc(&s->mask, sizeof(dt_u64) * nc));
  CHS_HIP(hipMalloc(&s->up, sizeof(int) * nc));
  CHS_HIP(hipMalloc(&s->dn, sizeof(int) * nc));
  CHS_HIP(hipMalloc(&s->hist, sizeof(dt_u64) * (size_t)s->nbins));
  CHS_HIP(hipMalloc(&s->part, sizeof(DtSummary) * DT_PARTS));
  CHS_HIP(hipMalloc(&s->out, sizeof(DtSummary)));
  CHS_HIP(hipMalloc(&s->words, sizeof(int) * DT_NW));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(DtResult), hipHostMallocDefault));
  return CHS_OK;
}

template <typename T>
int launch_mask(const DtBuf* s, const void* U, double t, int side, hipStream_t st) {
  constexpr int V = ChsVec<T>::V;
  const int N = s->N;
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  const bool nt = chs_grid_exceeds_cache((size_t)N, sizeof(T));
  if (N % V == 0) {
    const dim3 grid((N / V + DT_THREADS - 1) / DT_THREADS, s->nb);
    if (nt) k_dt_mask<T, V, true><<<grid, DT_THREADS, 0, st>>>(U, N, t, side, s->mask);
    else k_dt_mask<T, V, false><<<grid, DT_THREADS, 0, st>>>(U, N, t, side, s->mask);
  } else {
    const dim3 grid((N + DT_THREADS - 1) / DT_THREADS, s->nb);
    if (nt) k_dt_mask<T, 1, true><<<grid, DT_THREADS, 0, st>>>(U, N, t, side, s->mask);
    else k_dt_mask<T, 1, false><<<grid, DT_THREADS, 0, st>>>(U, N, t, side, s->mask);
  }
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

int dt_run(DtBuf* s, Engine* E, hipStream_t st, double t, int side, const std::string& who) {
  const int N = s->N, n2 = N * N;
  look_forget(s);
  CHS_HIP(hipMemsetAsync(s->words, 0, sizeof(int) * DT_NW, st));
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(dt_u64) * (size_t)s->nbins, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  const int rc = E->dtype == CHS_F64 ? launch_mask<double>(s, E->dU, t, side, st) : launch_mask<float>(s, E->dU, t, side, st);
  if (rc) return rc;
  k_dt_carry<<<dim3((N + DT_THREADS - 1) / DT_THREADS, 2), DT_THREADS, 0, st>>>(s->mask, N, s->nb, s->up, s->dn);
  CHS_HIP(hipGetLastError());
  k_dt_rows<<<N, DT_THREADS, sizeof(int) * (size_t)N, st>>>(s->mask, s->up, s->dn, N, s->D2, s->words);
  CHS_HIP(hipGetLastError());
  const int parts = std::min((n2 + DT_THREADS - 1) / DT_THREADS, DT_PARTS);
  k_dt_stats<<<parts, DT_THREADS, 0, st>>>(s->D2, n2, s->nbins, s->hist, s->part);
  CHS_HIP(hipGetLastError());
  k_dt_fin<<<1, DT_THREADS, 0, st>>>(s->part, parts, s->out);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->words, s->words, sizeof(int) * DT_NW, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(&s->hRes->out, s->out, sizeof(DtSummary), hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  if (s->hRes->words[DT_W_ERR]) {
    std::string m;
    if (s->hRes->words[DT_W_ERR] & DT_ERR_ROW) m += " the search along a row (k_dt_rows) reached its cap;";
    chs_set_error(who + ": self-check failed:" + m);
    return CHS_ECHECK;
  }
  return look_end(s);
}
}  // namespace

void chs_dt_free(void** buf) {
  if (!buf) return;
  dt_release((DtBuf*)*buf);
  *buf = nullptr;
}

void chs_dt_forget(void* buf) {
  if (buf) look_forget((DtBuf*)buf);
}

int chs_dt_snapshot(const void* buf, ChsDtSnapshot* out, const char* who_) {
  const DtBuf* s = (const DtBuf*)buf;
  if (!s || !s->have) { chs_set_error(std::string(who_) + ": no distance look to build on"); return CHS_ESTATE; }
  out->D2 = s->D2; out->ms = s->ms;
  return CHS_OK;
}

int chs_dt_look(Engine* E, hipStream_t st, void** buf, double threshold, int32_t side, int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  if (side != CHS_CC_BELOW && side != CHS_CC_ABOVE) { chs_set_error(who + ": the side is CHS_CC_BELOW (0) or CHS_CC_ABOVE (1)"); return CHS_EINVAL; }
  if ((rc = look_check_field(E, DT_MAX_N, who))) return rc;
  if ((rc = look_buffers<DtBuf>(buf, E->N, dt_alloc, dt_release))) return rc;
  DtBuf* s = (DtBuf*)*buf;
  if ((rc = dt_run(s, E, st, threshold, side, who))) return rc;
  memcpy(out, &s->hRes->out, sizeof(int64_t) * CHS_DT_WORDS);
  return CHS_OK;
}

int chs_dt_hist(void* buf, int device, hipStream_t st, int32_t nbins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const DtBuf* s = (const DtBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (nbins != s->nbins) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(s->nbins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * (size_t)nbins);
}

int chs_dt_map(void* buf, int device, hipStream_t st, int32_t* out, const char* who_) {
  const std::string who(who_);
  const DtBuf* s = (const DtBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->D2, sizeof(int32_t) * (size_t)s->N * s->N);
}

extern "C" int32_t chs_distance_bins(int32_t N) {
  if (N < 1) return 0;
  const long long v = 2ll * (N - 1) * (N - 1);
  long long k = (long long)std::sqrt((double)v);
  while (k * k > v) --k;
  while ((k + 1) * (k + 1) <= v) ++k;
  return (int32_t)(k + 1);
}

extern "C" int chs_distance(chs_handle h, double threshold, int32_t side, int64_t out[CHS_DT_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_distance: null handle"); return CHS_EINVAL; }
  return chs_dt_look(E, E->stream, &E->dt, threshold, side, out, "chs_distance");
}

extern "C" int chs_distance_hist(chs_handle h, int32_t nbins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_distance_hist: null handle"); return CHS_EINVAL; }
  return chs_dt_hist(E->dt, E->hc.device, E->stream, nbins, out, "chs_distance_hist");
}

extern "C" int chs_distance_map(chs_handle h, int32_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_distance_map: null handle"); return CHS_EINVAL; }
  return chs_dt_map(E->dt, E->hc.device, E->stream, out, "chs_distance_map");
}

extern "C" int chs_distance_last_ms(chs_handle h, double* ms) {
  return look_last_ms(h, h ? (const DtBuf*)((Engine*)h)->dt : nullptr, ms, "chs_distance");
}

extern "C" int chs_distance_tile(int32_t* band_rows, int32_t* row_chunk) {
  if (!band_rows || !row_chunk) { chs_set_error("chs_distance_tile: null argument"); return CHS_EINVAL; }
  *band_rows = CHS_DT_BAND;
  *row_chunk = CHS_DT_CHUNK;
  return CHS_OK;
}
