// chs_skeleton.hip -- skeleton look: the medial network of a phase of the thresholded field on the device, by a
// topology-preserving parallel thinning of its bit plane, with the network's seventeen summary words, the histogram of the
// widths along it and the packed plane itself (the definition: include/chs_hip.h, chs_skeleton).
//
// A skeleton look is a distance look first: chs_dt_look leaves the exact squared distances D2 on the handle's distance
// buffers, and the phase is D2 > 0.  Then, here, each phase a launch of its own -- no workgroup waits for another, nothing
// is polled on the device:
//   1  k_sk_mask     a wavefront per 64 pixels of a row: D2 > 0 by a 64-lane ballot is the word of the plane; FG by
//                    popcount, one atomic per workgroup.  k_sk_euler then takes the Euler number of the phase from the
//                    plane, a thread per word.
//   2  k_sk_thin<d>  one launch per sub-iteration, ping-pong between two planes.  A thread owns a word: it loads the
//                    3 x 3 words about it (a word outside the plane is 0), and chs_sk::deletes of chs_skel_host.h gives
//                    the pixels the sub-iteration deletes, in plain boolean algebra on the eight shifted neighbour
//                    planes -- no loop over pixels, no divergence.  A workgroup that deleted raises LAST to the
//                    sub-iteration's index by one atomic maximum.  A launch behind the fixed point copies the plane.
//                    The host issues SK_CHUNK launches, reads LAST from a pinned word and stops at LAST + 4 <= issued.
//   3  k_sk_stats    one sweep over the final plane, a thread per word: popcounts of the masks of chs_sk::kinds_of
//                    (B, the Yokoi number, the adjacent pairs, the 2 x 2 windows), and a loop over the set bits of the
//                    word for D2: the LDS histogram by isqrt(D2), sum, maximum and the minimum over the links.  A
//                    workgroup adds each of its sums with one integer atomic.
// Everything is an integer and every accumulation a maximum, a minimum or an integer add: plane, histogram and words do not
// depend on the order of anything.  The kernels read D2 and write this look's own arrays alone; they never read the field.
#include <algorithm>
#include <cstring>

#include "chs_look.h"
#include "chs_skel_host.h"

#define SK_THREADS 256
#define SK_WAVES (SK_THREADS / CHS_WAVE)
#define SK_LBINS 4096                       // bins of a workgroup's LDS histogram
#define SK_MASK_GROUPS 4096                 // workgroups of k_sk_mask at most
#define SK_CHUNK 32                         // sub-iterations the host issues between two reads of LAST
#define SK_FACTOR 4ll                       // chs_skeleton_subiters_default(N) = SK_FACTOR N + SK_SLACK
#define SK_SLACK 64ll
#define SK_MAX_FACTOR 16ll                  // max_subiters at most that many defaults
// the counters of a look, 64-bit words
#define SK_C_FG 0
#define SK_C_EULER0 1                       // the Euler number of the phase (two's complement)
#define SK_C_PIXELS 2
#define SK_C_ISOLATED 3
#define SK_C_ENDS 4
#define SK_C_B2 5
#define SK_C_Y1 6                           // .. Y4 = 9
#define SK_C_AXIAL 10
#define SK_C_DIAGONAL 11
#define SK_C_TRI 12
#define SK_C_FULL 13
#define SK_C_SUMD2 14
#define SK_C_NINF 15
#define SK_C_SUMS 16                        // the counters below this are sums
#define SK_C_D2MAX 16
#define SK_C_D2MIN 17                       // starts at all ones
#define SK_C_LAST 18
#define SK_NC 19

static_assert(CHS_WAVE == 64, "a ballot is a word of the plane");

typedef chs_sk::u64 sk_u64;
static_assert(sizeof(sk_u64) == sizeof(int64_t), "the result words are int64");

// the 3 x 3 words about word w of row i; a word outside the plane is 0
__device__ __forceinline__ chs_sk::Nine sk_load9(const sk_u64* __restrict__ P, int N, int W, int i, int w) {
  chs_sk::Nine n;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int ii = i + r - 1;
    const bool row = ii >= 0 && ii < N;
    const sk_u64* base = P + (size_t)(row ? ii : i) * W;
    n.c[r] = row ? base[w] : 0ull;
    n.l[r] = (row && w > 0) ? base[w - 1] : 0ull;
    n.r[r] = (row && w + 1 < W) ? base[w + 1] : 0ull;
  }
  return n;
}

// the sum of v over the workgroup, in thread 0; red: SK_WAVES words
__device__ __forceinline__ sk_u64 sk_block_sum(sk_u64 v, sk_u64* red) {
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, CHS_WAVE);
  __syncthreads();   // (red is free again)
  if ((threadIdx.x & (CHS_WAVE - 1)) == 0) red[threadIdx.x / CHS_WAVE] = v;
  __syncthreads();
  sk_u64 s = 0;
#pragma unroll
  for (int k = 0; k < SK_WAVES; ++k) s += red[k];
  return s;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------
// Wavefront g of the grid takes the words g, g + waves, ... of the plane; lane j is column 64 w + j.
__global__ __launch_bounds__(SK_THREADS) void k_sk_mask(const int* __restrict__ D2, int N, int W, sk_u64* __restrict__ plane,
                                                        sk_u64* __restrict__ cnt) {
  __shared__ sk_u64 red[SK_WAVES];
  const int lane = threadIdx.x & (CHS_WAVE - 1);
  const int total = N * W;
  const int waves = gridDim.x * SK_WAVES;
  sk_u64 fg = 0;
#pragma unroll 1
  for (int word = blockIdx.x * SK_WAVES + threadIdx.x / CHS_WAVE; word < total; word += waves) {   // (uniform in the wavefront)
    const int i = word / W, w = word - i * W;
    const int col = w * 64 + lane;
    const bool in = col < N;
    const int d = D2[(size_t)i * N + (in ? col : N - 1)];
    const sk_u64 m = __ballot(in && d > 0);
    if (lane == 0) { plane[word] = m; fg += (sk_u64)chs_sk::popc(m); }
  }
  const sk_u64 s = sk_block_sum(fg, red);
  if (threadIdx.x == 0 && s) atomicAdd(&cnt[SK_C_FG], s);
}

// the Euler number of the plane P into cnt[SK_C_EULER0]: a thread per word, a workgroup's part by one atomic
__global__ __launch_bounds__(SK_THREADS) void k_sk_euler(const sk_u64* __restrict__ P, int N, int W, sk_u64* __restrict__ cnt) {
  __shared__ sk_u64 red[SK_WAVES];
  const int idx = blockIdx.x * SK_THREADS + threadIdx.x;
  long long e = 0;
  if (idx < N * W) {
    const int i = idx / W, w = idx - i * W;
    const chs_sk::Kinds k = chs_sk::kinds_of(sk_load9(P, N, W, i, w));
    e = chs_sk::euler8_of(chs_sk::popc(P[idx]), chs_sk::popc(k.axial_e) + chs_sk::popc(k.axial_s),
                          chs_sk::popc(k.diag_se) + chs_sk::popc(k.diag_sw), chs_sk::popc(k.tri), chs_sk::popc(k.full));
  }
  const sk_u64 s = sk_block_sum((sk_u64)e, red);
  if (threadIdx.x == 0 && s) atomicAdd(&cnt[SK_C_EULER0], s);
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------
// dst <- src after sub-iteration `iter` of direction DIR; a thread per word
template <int DIR>
__global__ __launch_bounds__(SK_THREADS) void k_sk_thin(const sk_u64* __restrict__ src, sk_u64* __restrict__ dst, int N, int W,
                                                        sk_u64 iter, sk_u64* __restrict__ cnt) {
  const int idx = blockIdx.x * SK_THREADS + threadIdx.x;
  sk_u64 del = 0;
  if (idx < N * W) {
    const int i = idx / W, w = idx - i * W;
    const chs_sk::Nine n = sk_load9(src, N, W, i, w);
    del = chs_sk::deletes(n, DIR);
    dst[idx] = n.c[1] & ~del;
  }
  const int any = __syncthreads_or(del != 0);
  if (threadIdx.x == 0 && any) atomicMax(&cnt[SK_C_LAST], iter);
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------
// a thread per word of the final plane
__global__ __launch_bounds__(SK_THREADS) void k_sk_stats(const sk_u64* __restrict__ P, const int* __restrict__ D2, int N, int W, int nbins,
                                                         sk_u64* __restrict__ hist, sk_u64* __restrict__ cnt) {
  __shared__ int lh[SK_LBINS];
  __shared__ sk_u64 red[SK_WAVES][SK_C_SUMS];
  for (int k = threadIdx.x; k < SK_LBINS; k += SK_THREADS) lh[k] = 0;
  __syncthreads();
  const int idx = blockIdx.x * SK_THREADS + threadIdx.x;
  sk_u64 sum[SK_C_SUMS];
#pragma unroll
  for (int k = 0; k < SK_C_SUMS; ++k) sum[k] = 0;
  unsigned d2max = 0, d2min = 0xffffffffu;
  if (idx < N * W) {
    const int i = idx / W, w = idx - i * W;
    const chs_sk::Nine n = sk_load9(P, N, W, i, w);
    const chs_sk::Kinds kd = chs_sk::kinds_of(n);
    const sk_u64 c = n.c[1];
    sum[SK_C_PIXELS] = chs_sk::popc(c);
    sum[SK_C_ISOLATED] = chs_sk::popc(kd.isolated);
    sum[SK_C_ENDS] = chs_sk::popc(kd.ends);
    sum[SK_C_B2] = chs_sk::popc(kd.b2);
#pragma unroll
    for (int y = 1; y <= 4; ++y) sum[SK_C_Y1 + y - 1] = chs_sk::popc(kd.y[y]);
    sum[SK_C_AXIAL] = chs_sk::popc(kd.axial_e) + chs_sk::popc(kd.axial_s);
    sum[SK_C_DIAGONAL] = chs_sk::popc(kd.diag_se) + chs_sk::popc(kd.diag_sw);
    sum[SK_C_TRI] = chs_sk::popc(kd.tri);
    sum[SK_C_FULL] = chs_sk::popc(kd.full);
    const int* row = D2 + (size_t)i * N + w * 64;   // (a set bit j is a column 64 w + j < N)
    sk_u64 m = c;
#pragma unroll 1
    for (int step = 0; step < 64 && m; ++step) {
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int d = row[j];
      if ((kd.y[2] >> j) & 1ull) d2min = min(d2min, (unsigned)d);
      if (d >= CHS_DT_INF) { sum[SK_C_NINF] += 1; continue; }
      sum[SK_C_SUMD2] += (sk_u64)d;
      d2max = max(d2max, (unsigned)d);
      const int k = dt_isqrt(d);   // the distance look's own bin (chs_look.h)
      if (k < SK_LBINS) atomicAdd(&lh[k], 1);
      else if (k < nbins) atomicAdd(&hist[k], (sk_u64)1);
    }
  }
  __syncthreads();
  const int top = nbins < SK_LBINS ? nbins : SK_LBINS;
  for (int k = threadIdx.x; k < top; k += SK_THREADS) {
    const int v = lh[k];
    if (v) atomicAdd(&hist[k], (sk_u64)v);
  }
  // the sums: inside the wavefront by shuffles, the wavefronts' through LDS; thread k adds the workgroup's sum k.  The
  // maximum and the minimum ride in the two slots below SK_C_PIXELS, which are no sums of this kernel.
  static_assert(SK_C_PIXELS >= 2, "two free slots");
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) {
    d2max = max(d2max, (unsigned)__shfl_down(d2max, off, CHS_WAVE));
    d2min = min(d2min, (unsigned)__shfl_down(d2min, off, CHS_WAVE));
  }
  const bool first = (threadIdx.x & (CHS_WAVE - 1)) == 0;
  if (first) { red[threadIdx.x / CHS_WAVE][0] = d2max; red[threadIdx.x / CHS_WAVE][1] = d2min; }
#pragma unroll
  for (int k = SK_C_PIXELS; k < SK_C_SUMS; ++k) {
    sk_u64 v = sum[k];
#pragma unroll
    for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, CHS_WAVE);
    if (first) red[threadIdx.x / CHS_WAVE][k] = v;
  }
  __syncthreads();
  if (threadIdx.x >= SK_C_PIXELS && threadIdx.x < SK_C_SUMS) {
    sk_u64 s = 0;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) s += red[w][threadIdx.x];
    if (s) atomicAdd(&cnt[threadIdx.x], s);
  }
  if (threadIdx.x == 0) {
    sk_u64 m = 0;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) m = max(m, red[w][0]);
    if (m) atomicMax(&cnt[SK_C_D2MAX], m);
  }
  if (threadIdx.x == 1) {
    sk_u64 m = 0xffffffffull;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) m = min(m, red[w][1]);
    if (m != 0xffffffffull) atomicMin(&cnt[SK_C_D2MIN], m);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct SkResult {   // pinned
  sk_u64 cnt[SK_NC];
  int64_t words[CHS_SK_WORDS];
};

struct SkBuf : LookBase {   // have: plane[final] and hist are the look's snapshot
  int nbins = 0, W = 0, final = 0;
  sk_u64* plane[2] = {nullptr, nullptr};   // [N * W] each
  sk_u64* cnt = nullptr;                   // [SK_NC]
  sk_u64* hist = nullptr;                  // [nbins]
  SkResult* hRes = nullptr;
  hipEvent_t evr[2] = {nullptr, nullptr};   // around the sub-iterations
  double thin_ms = -1.0;
};

void sk_release(SkBuf* s) {
  if (!s) return;
  hipFree(s->plane[0]); hipFree(s->plane[1]); hipFree(s->cnt); hipFree(s->hist);
  if (s->hRes) hipHostFree(s->hRes);
  for (auto e : s->evr) if (e) hipEventDestroy(e);
  look_release_events(s);
  delete s;
}

int sk_alloc(SkBuf* s) {
  s->W = chs_sk::words_of(s->N);
  s->nbins = chs_distance_bins(s->N);
  const size_t words = (size_t)s->N * s->W;
  for (auto& p : s->plane) CHS_HIP(hipMalloc(&p, sizeof(sk_u64) * words));
  CHS_HIP(hipMalloc(&s->cnt, sizeof(sk_u64) * SK_NC));
  CHS_HIP(hipMalloc(&s->hist, sizeof(sk_u64) * (size_t)s->nbins));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(SkResult), hipHostMallocDefault));
  for (auto& e : s->evr) CHS_HIP(hipEventCreate(&e));
  return CHS_OK;
}

void sk_thin(int dir, int groups, hipStream_t st, const sk_u64* src, sk_u64* dst, int N, int W, sk_u64 iter, sk_u64* cnt) {
  switch (dir) {
    case CHS_SK_DIR_N: k_sk_thin<CHS_SK_DIR_N><<<groups, SK_THREADS, 0, st>>>(src, dst, N, W, iter, cnt); break;
    case CHS_SK_DIR_S: k_sk_thin<CHS_SK_DIR_S><<<groups, SK_THREADS, 0, st>>>(src, dst, N, W, iter, cnt); break;
    case CHS_SK_DIR_E: k_sk_thin<CHS_SK_DIR_E><<<groups, SK_THREADS, 0, st>>>(src, dst, N, W, iter, cnt); break;
    default: k_sk_thin<CHS_SK_DIR_W><<<groups, SK_THREADS, 0, st>>>(src, dst, N, W, iter, cnt); break;
  }
}

// The phases behind a distance look that has just succeeded and left `dt`.
int sk_run(SkBuf* s, hipStream_t st, const ChsDtSnapshot& dt, const int64_t* dtw, int64_t limit, const std::string& who) {
  const int N = s->N, W = s->W, total = N * W;
  const int groups = (total + SK_THREADS - 1) / SK_THREADS;
  look_forget(s);
  s->thin_ms = -1.0;
  CHS_HIP(hipMemsetAsync(s->cnt, 0, sizeof(sk_u64) * SK_NC, st));
  CHS_HIP(hipMemsetAsync(s->cnt + SK_C_D2MIN, 0xff, sizeof(sk_u64), st));
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(sk_u64) * (size_t)s->nbins, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  k_sk_mask<<<std::min((total + SK_WAVES - 1) / SK_WAVES, SK_MASK_GROUPS), SK_THREADS, 0, st>>>(dt.D2, N, W, s->plane[0], s->cnt);
  CHS_HIP(hipGetLastError());
  k_sk_euler<<<groups, SK_THREADS, 0, st>>>(s->plane[0], N, W, s->cnt);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->evr[0], st));
  int64_t issued = 0, last = 0;
  while (issued < limit) {
    const int64_t chunk = std::min<int64_t>(SK_CHUNK, limit - issued);
    for (int64_t k = 0; k < chunk; ++k) {
      const int64_t it = issued + k + 1;   // plane[(it - 1) & 1] -> plane[it & 1]
      sk_thin(chs_sk::dir_of(it), groups, st, s->plane[(it - 1) & 1], s->plane[it & 1], N, W, (sk_u64)it, s->cnt);
      CHS_HIP(hipGetLastError());
    }
    issued += chunk;
    CHS_HIP(hipMemcpyAsync(&s->hRes->cnt[SK_C_LAST], s->cnt + SK_C_LAST, sizeof(sk_u64), hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    last = (int64_t)s->hRes->cnt[SK_C_LAST];
    if (last + 4 <= issued) break;
  }
  CHS_HIP(hipEventRecord(s->evr[1], st));
  int64_t* w = s->hRes->words;
  memset(w, 0, sizeof(int64_t) * CHS_SK_WORDS);
  w[CHS_SK_SUBITERS] = last; w[CHS_SK_LIMIT] = limit;
  if (last + 4 > issued) {
    chs_set_error(who + ": a pixel was deleted in sub-iteration " + std::to_string(last) + ", max_subiters = " + std::to_string(limit) +
                  "; there is no skeleton result (the distance look of this call is complete)");
    return CHS_ELIMIT;
  }
  const int fin = (int)(issued & 1);   // (both planes are equal by now)
  k_sk_stats<<<groups, SK_THREADS, 0, st>>>(s->plane[fin], dt.D2, N, W, s->nbins, s->hist, s->cnt);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->cnt, s->cnt, sizeof(sk_u64) * SK_NC, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const sk_u64* c = s->hRes->cnt;
  const int64_t fg = (int64_t)c[SK_C_FG], pixels = (int64_t)c[SK_C_PIXELS], euler0 = (int64_t)c[SK_C_EULER0];
  const int64_t euler = chs_sk::euler8_of(pixels, (int64_t)c[SK_C_AXIAL], (int64_t)c[SK_C_DIAGONAL], (int64_t)c[SK_C_TRI],
                                          (int64_t)c[SK_C_FULL]);
  const int64_t parts = (int64_t)(c[SK_C_ISOLATED] + c[SK_C_ENDS] + c[SK_C_B2]);
  if (euler != euler0 || pixels > fg || fg != dtw[CHS_DT_FG] || pixels != parts || (int64_t)c[SK_C_LAST] != last || last + 4 > issued) {
    chs_set_error(who + ": self-check failed: EULER8 = " + std::to_string(euler) + ", the phase has " + std::to_string(euler0) +
                  "; PIXELS, FG = " + std::to_string(pixels) + ", " + std::to_string(fg) + ", the distance look has FG = " +
                  std::to_string(dtw[CHS_DT_FG]) + "; ISOLATED + ENDS + (B >= 2) = " + std::to_string(parts) + "; SUBITERS = " +
                  std::to_string((int64_t)c[SK_C_LAST]) + " of " + std::to_string(issued) + " issued");
    return CHS_ECHECK;
  }
  w[CHS_SK_FG] = fg; w[CHS_SK_PIXELS] = pixels; w[CHS_SK_ISOLATED] = (int64_t)c[SK_C_ISOLATED]; w[CHS_SK_ENDS] = (int64_t)c[SK_C_ENDS];
  for (int y = 0; y < 4; ++y) w[CHS_SK_Y1 + y] = (int64_t)c[SK_C_Y1 + y];
  w[CHS_SK_AXIAL] = (int64_t)c[SK_C_AXIAL]; w[CHS_SK_DIAGONAL] = (int64_t)c[SK_C_DIAGONAL];
  w[CHS_SK_SUMD2] = (int64_t)c[SK_C_SUMD2]; w[CHS_SK_D2MAX] = (int64_t)c[SK_C_D2MAX];
  w[CHS_SK_D2MIN_LINK] = c[SK_C_Y1 + 1] ? (int64_t)c[SK_C_D2MIN] : 0;
  w[CHS_SK_NINF] = (int64_t)c[SK_C_NINF]; w[CHS_SK_EULER8] = euler;
  float tms = 0.f;
  CHS_HIP(hipEventElapsedTime(&tms, s->evr[0], s->evr[1]));
  int rc;
  if ((rc = look_end(s))) return rc;
  s->final = fin;
  s->thin_ms = tms;
  s->ms += dt.ms;   // the distance look inside
  return CHS_OK;
}
}  // namespace

void chs_sk_free(void** buf) {
  if (!buf) return;
  sk_release((SkBuf*)*buf);
  *buf = nullptr;
}

void chs_sk_forget(void* buf) {
  if (buf) look_forget((SkBuf*)buf);
}

int chs_sk_look(Engine* E, hipStream_t st, void** dtbuf, void** buf, double threshold, int32_t side, int64_t max_subiters,
                int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  const int64_t def = chs_skeleton_subiters_default(E->N);
  if (max_subiters < 0 || max_subiters > SK_MAX_FACTOR * def) {
    chs_set_error(who + ": max_subiters = " + std::to_string(max_subiters) + " is outside [0, " + std::to_string(SK_MAX_FACTOR * def) +
                  "] (0: the default, " + std::to_string(def) + ")");
    return CHS_EINVAL;
  }
  if (max_subiters == 0) max_subiters = def;
  int64_t dtw[CHS_DT_WORDS];
  // the distance look: its own checks of side and field, in its own order, under this look's name
  if ((rc = chs_dt_look(E, st, dtbuf, threshold, side, dtw, who_))) return rc;
  if ((rc = look_buffers<SkBuf>(buf, E->N, sk_alloc, sk_release))) return rc;
  SkBuf* s = (SkBuf*)*buf;
  ChsDtSnapshot dt;
  if ((rc = chs_dt_snapshot(*dtbuf, &dt, who_))) return rc;
  rc = sk_run(s, st, dt, dtw, max_subiters, who);
  if (rc == CHS_OK || rc == CHS_ELIMIT) memcpy(out, s->hRes->words, sizeof(int64_t) * CHS_SK_WORDS);   // refused: SUBITERS and LIMIT
  return rc;
}

int chs_sk_hist(void* buf, int device, hipStream_t st, int32_t nbins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const SkBuf* s = (const SkBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (nbins != s->nbins) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(s->nbins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * (size_t)nbins);
}

int chs_sk_plane(void* buf, int device, hipStream_t st, uint64_t* out, const char* who_) {
  const std::string who(who_);
  const SkBuf* s = (const SkBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->plane[s->final], sizeof(uint64_t) * (size_t)s->N * s->W);
}

int chs_sk_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const SkBuf*)buf, ms, what);
}

int chs_sk_thin_ms(const void* h, const void* buf, double* ms, const char* what) {
  const std::string who = std::string(what) + "_thin_ms";
  const SkBuf* s = (const SkBuf*)buf;
  if (!h || !ms) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (!s || !s->have || s->thin_ms < 0.0) { chs_set_error(who + ": no " + what + " call so far"); return CHS_ESTATE; }
  *ms = s->thin_ms;
  return CHS_OK;
}

extern "C" int64_t chs_skeleton_subiters_default(int32_t N) {
  if (N < 1) return 0;
  return SK_FACTOR * (int64_t)N + SK_SLACK;
}

extern "C" int chs_skeleton(chs_handle h, double threshold, int32_t side, int64_t max_subiters, int64_t out[CHS_SK_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_skeleton: null handle"); return CHS_EINVAL; }
  return chs_sk_look(E, E->stream, &E->dt, &E->sk, threshold, side, max_subiters, out, "chs_skeleton");
}

extern "C" int chs_skeleton_hist(chs_handle h, int32_t nbins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_skeleton_hist: null handle"); return CHS_EINVAL; }
  return chs_sk_hist(E->sk, E->hc.device, E->stream, nbins, out, "chs_skeleton_hist");
}

extern "C" int chs_skeleton_plane(chs_handle h, uint64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_skeleton_plane: null handle"); return CHS_EINVAL; }
  return chs_sk_plane(E->sk, E->hc.device, E->stream, out, "chs_skeleton_plane");
}

extern "C" int chs_skeleton_last_ms(chs_handle h, double* ms) {
  return chs_sk_last_ms(h, h ? ((Engine*)h)->sk : nullptr, ms, "chs_skeleton");
}

extern "C" int chs_skeleton_thin_ms(chs_handle h, double* ms) {
  return chs_sk_thin_ms(h, h ? ((Engine*)h)->sk : nullptr, ms, "chs_skeleton");
}
