// chs_two_point.hip -- two-point correlation of both phases of the thresholded field on the device: the pair counts of
// every displacement (dy, dx) with 0 <= dy <= rmax, |dx| <= rmax (the definition:
// include/chs_hip.h, chs_two_point).
//
// Phases that depend on each other are separate launches: no workgroup ever waits for another one, nothing is polled.
//   1  k_tp_mask   one sweep over U gives the row plane of either phase as 32-bit words, row-major [N][nw], nw =
//                  ceil(N / 32): bit b of word w of row i is pixel (i, 32 w + b).  A wavefront takes 64 consecutive pixels
//                  of TP_MASK_ROWS rows (the loads of the rows are independent of each other); the ballot of a row is two
//                  words of phase 0, the ballot of the complement inside the grid two words of phase 1.  Four lanes store
//                  the four words.  The bits beyond N of a row's last word are zero in both planes.
//   2  k_tp_pairs  a work item is (a band of TP_H rows and a chunk of TP_CW words of them, one dy, one phase).  The
//                  workgroup stages the chunk's words of the rows i + dy in LDS with TP_PAD words on either side, zero
//                  where the row or the word lies outside the grid -- that is the whole of "no wrap-around".  A lane owns
//                  TP_K consecutive words of one row i and keeps them in registers.  For dx = 32 q + s (0 <= s < 32) the
//                  partner of word w is bits s .. s + 31 of the words w + q and w + q + 1 of row i + dy: one alignbit;
//                  then an AND and a population count that adds to the accumulator of this dx.  The TP_K + 1 partner
//                  words are read from LDS once per q and serve its 32 values of s.  The accumulator of a dx is summed
//                  over the wavefront by a shuffle tree in registers (tp_wave_sum), the wavefronts' sums meet in LDS,
//                  and a workgroup adds what is not zero to the int64 table with one atomicAdd per dx: integer sums,
//                  order-free.
//   3  k_tp_fin    one workgroup forms the 8 words, sums both tables and checks the look: N_BELOW + N_ABOVE = N^2, the
//                  row dy = 0 of both tables is symmetric in dx, c0 + c1 <= pairs entry by entry.
// Nothing of the handle is written and nothing the step loop owns is read: its field alone.
#include <cstring>

#include "chs_look.h"
#include "chs_cc_host.h"   // chs_cc::fg_of: phase 0 is the foreground of chs_components with CHS_CC_BELOW

#define TP_WORD 32                          // pixels of a row in one word
#define TP_THREADS 256                      // k_tp_mask, k_tp_pairs
#define TP_FIN_THREADS 1024                 // k_tp_fin: one workgroup
#define TP_MASK_ROWS 4                      // rows of a wavefront of k_tp_mask
#define TP_H 64                             // rows of a band of k_tp_pairs
#define TP_K 16                             // consecutive words of a row that a lane of k_tp_pairs owns
#define TP_CW (TP_THREADS / TP_H * TP_K)    // words of a row in a chunk: 64 = 2048 pixels
#define TP_PAD (CHS_TP_MAX_R / TP_WORD)     // words of padding on either side of a staged row: q is in [-TP_PAD, TP_PAD]
#define TP_STRIDE (TP_CW + 2 * TP_PAD + 1)  // words of a staged row: local words -TP_PAD .. TP_CW + TP_PAD; odd
#define TP_MAX_N 16384                      // N of chs_create at most, as chs_chords
#define TP_W_ERR 0
#define TP_NW 2
#define TP_ERR_TOTAL 1                      // N_BELOW + N_ABOVE is not N^2
#define TP_ERR_SYM 2                        // the row dy = 0 of a table is not symmetric in dx
#define TP_ERR_PAIRS 4                      // c0 + c1 > pairs at some displacement, or a negative entry

static_assert(TP_WORD == 32 && CHS_WAVE == 2 * TP_WORD, "a ballot is two words");
static_assert(TP_THREADS % CHS_WAVE == 0 && TP_THREADS % TP_H == 0, "whole wavefronts; the lanes of a row of a band");
static_assert(TP_FIN_THREADS % CHS_WAVE == 0 && TP_FIN_THREADS <= 1024, "whole wavefronts, one workgroup");
static_assert(CHS_TP_MAX_R % TP_WORD == 0 && TP_STRIDE % 2 == 1, "dx = CHS_TP_MAX_R is q = TP_PAD, s = 0");
static_assert(TP_CW * TP_WORD == CHS_TP_CHUNK, "the chunk the header names");
static_assert((long long)TP_H * TP_CW * TP_WORD < (1ll << 31), "a workgroup's count of one dx fits 32 bits");
static_assert(CHS_TP_WORDS == 8, "the summary words");

typedef long long tp_i64;
typedef unsigned long long tp_u64;
static_assert(sizeof(tp_i64) == sizeof(int64_t), "the result words are int64");

// ---- phase 1 ---------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64) / 4 rounded up, ceil(N / TP_MASK_ROWS)): wavefront v of workgroup (bx, by) takes pixels 64 g .. 64 g +
// 63, g = 4 bx + v, of rows TP_MASK_ROWS by ...  planes: phase 0 [N][nw], then phase 1.
template <typename T, bool NT>
__global__ __launch_bounds__(TP_THREADS) void k_tp_mask(const void* Uv, int N, int nw, double t, unsigned* __restrict__ planes) {
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const int lane = threadIdx.x % CHS_WAVE, g = blockIdx.x * (TP_THREADS / CHS_WAVE) + threadIdx.x / CHS_WAVE;
  const int j = g * CHS_WAVE + lane, i0 = blockIdx.y * TP_MASK_ROWS;
  const bool inside = j < N;
  const T CHS_GLOBAL* col = U + (inside ? j : N - 1);
  T x[TP_MASK_ROWS][1];
#pragma unroll
  for (int r = 0; r < TP_MASK_ROWS; ++r) {   // (clamped: no load guarded by a branch)
    const int i = i0 + r < N ? i0 + r : N - 1;
    chs_load<T, 1, NT>(col + (size_t)i * N, x[r]);
  }
  const int w = 2 * g + (lane & 1);          // lanes 0 .. 3 store: phase lane / 2, word lane % 2 of the ballot
  unsigned* __restrict__ dst = planes + (size_t)(lane >> 1) * N * nw;
#pragma unroll
  for (int r = 0; r < TP_MASK_ROWS; ++r) {
    const int i = i0 + r;
    const bool p0 = chs_cc::fg_of((double)x[r][0], t, 0);
    const tp_u64 b0 = __ballot(inside && p0), b1 = __ballot(inside && !p0);   // (every lane of the wavefront is here)
    const tp_u64 b = (lane & 2) ? b1 : b0;
    const unsigned v = (unsigned)((lane & 1) ? b >> 32 : b);
    if (lane < 4 && i < N && w < nw) dst[(size_t)i * nw + w] = v;
  }
}

// ---- phase 2 ---------------------------------------------------------------------------------------------------------
// The sum of v over the wavefront, the same in every lane (all 64 are active): a butterfly inside each row of 16 lanes by
// DPP -- the neighbour, the other pair of the quad, the other quad of the half row, the other half row -- then the four
// rows by readlane.  No LDS round trip; measured no faster than six __shfl_xor steps.
__device__ __forceinline__ int tp_wave_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1, 0, 3, 2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2, 3, 0, 1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);   // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);   // row_mirror
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}

// grid (bands x chunks, rmax + 1, 2): blockIdx.y is dy, blockIdx.z the phase.  counts is [2][rmax + 1][2 rmax + 1].
__global__ __launch_bounds__(TP_THREADS) void k_tp_pairs(const unsigned* __restrict__ planes, int N, int nw, int nchunks, int rmax,
                                                         tp_u64* __restrict__ counts) {
  __shared__ unsigned rowsB[TP_H * TP_STRIDE];                     // the rows i + dy: local words -TP_PAD .. TP_CW + TP_PAD
  __shared__ int wsum[TP_THREADS / CHS_WAVE][2 * CHS_TP_MAX_R + 1];   // the wavefronts' sums by dx + rmax
  const int band = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks, dy = blockIdx.y, phase = blockIdx.z;
  const int i0 = band * TP_H, w0 = chunk * TP_CW;
  if (i0 + dy >= N) return;   // (the whole workgroup: no row of the band has a partner row)
  const unsigned* __restrict__ plane = planes + (size_t)phase * N * nw;
  for (int idx = threadIdx.x; idx < TP_H * TP_STRIDE; idx += TP_THREADS) {
    const int r = idx / TP_STRIDE, c = idx % TP_STRIDE;
    const int i = i0 + r + dy, w = w0 + c - TP_PAD;
    rowsB[idx] = (i < N && w >= 0 && w < nw) ? plane[(size_t)i * nw + w] : 0u;
  }
  // the lane's own words: TP_K consecutive ones of row i0 + r, zero outside the grid
  const int r = threadIdx.x / (TP_CW / TP_K), k0 = (threadIdx.x % (TP_CW / TP_K)) * TP_K;
  unsigned a[TP_K];
#pragma unroll
  for (int k = 0; k < TP_K; ++k) {
    const int i = i0 + r, w = w0 + k0 + k;
    a[k] = (i < N && w < nw) ? plane[(size_t)i * nw + w] : 0u;
  }
  __syncthreads();
  const int wave = threadIdx.x / CHS_WAVE, lane = threadIdx.x % CHS_WAVE;
  const int qlo = -((rmax + TP_WORD - 1) / TP_WORD), qhi = rmax / TP_WORD;   // floor(-rmax / 32) .. floor(rmax / 32)
#pragma unroll 1
  for (int q = qlo; q <= qhi; ++q) {
    unsigned b[TP_K + 1];
    const unsigned* src = rowsB + r * TP_STRIDE + TP_PAD + k0 + q;   // local words k0 + q .. k0 + q + TP_K: inside the padding
#pragma unroll
    for (int k = 0; k <= TP_K; ++k) b[k] = src[k];
    const int slo = -rmax - q * TP_WORD > 0 ? -rmax - q * TP_WORD : 0;
    const int shi = rmax - q * TP_WORD < TP_WORD - 1 ? rmax - q * TP_WORD : TP_WORD - 1;
    for (int s = slo; s <= shi; ++s) {
      int acc = 0;
#pragma unroll
      for (int k = 0; k < TP_K; ++k) acc += __popc(a[k] & __builtin_amdgcn_alignbit(b[k + 1], b[k], (unsigned)s));
      const int sum = tp_wave_sum(acc);
      if (lane == 0) wsum[wave][q * TP_WORD + s + rmax] = sum;
    }
  }
  __syncthreads();
  tp_u64* __restrict__ dst = counts + ((size_t)phase * (rmax + 1) + dy) * (2 * rmax + 1);
  for (int d = threadIdx.x; d <= 2 * rmax; d += TP_THREADS) {
    int c = 0;
#pragma unroll
    for (int v = 0; v < TP_THREADS / CHS_WAVE; ++v) c += wsum[v][d];
    if (c) atomicAdd(&dst[d], (tp_u64)c);
  }
}

// ---- phase 3 ---------------------------------------------------------------------------------------------------------
// One workgroup: every thread walks its share of the displacements, a shuffle tree inside the wavefront, thread 0 joins
// the wavefronts' sums in a fixed order and writes the words.
__global__ __launch_bounds__(TP_FIN_THREADS) void k_tp_fin(const tp_u64* __restrict__ counts, int N, int rmax, tp_i64* __restrict__ out,
                                                       int* __restrict__ words) {
  __shared__ tp_i64 red[TP_FIN_THREADS / CHS_WAVE][2];
  __shared__ int rerr[TP_FIN_THREADS / CHS_WAVE];
  const int nx = 2 * rmax + 1, per = (rmax + 1) * nx;
  tp_i64 s0 = 0, s1 = 0;
  int err = 0;
  for (int e = threadIdx.x; e < per; e += TP_FIN_THREADS) {
    const int dy = e / nx, dx = e % nx - rmax;
    const tp_i64 c0 = (tp_i64)counts[e], c1 = (tp_i64)counts[per + e];
    const tp_i64 pairs = (tp_i64)(N - dy) * (N - (dx < 0 ? -dx : dx));
    if (c0 < 0 || c1 < 0 || c0 + c1 > pairs) err |= TP_ERR_PAIRS;
    if (dy == 0 && (c0 != (tp_i64)counts[rmax - dx] || c1 != (tp_i64)counts[per + rmax - dx])) err |= TP_ERR_SYM;
    s0 += c0; s1 += c1;
  }
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); err |= __shfl_down(err, off);
  }
  if (threadIdx.x % CHS_WAVE == 0) {
    red[threadIdx.x / CHS_WAVE][0] = s0; red[threadIdx.x / CHS_WAVE][1] = s1; rerr[threadIdx.x / CHS_WAVE] = err;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tp_i64 t0 = 0, t1 = 0;
    int e = 0;
    for (int v = 0; v < TP_FIN_THREADS / CHS_WAVE; ++v) { t0 += red[v][0]; t1 += red[v][1]; e |= rerr[v]; }
    const tp_u64* c0 = counts;
    const tp_u64* c1 = counts + per;
    out[CHS_TP_N_BELOW] = (tp_i64)c0[rmax]; out[CHS_TP_N_ABOVE] = (tp_i64)c1[rmax];
    out[CHS_TP_ADJ_ROWS_BELOW] = (tp_i64)c0[rmax + 1]; out[CHS_TP_ADJ_COLS_BELOW] = (tp_i64)c0[nx + rmax];
    out[CHS_TP_ADJ_ROWS_ABOVE] = (tp_i64)c1[rmax + 1]; out[CHS_TP_ADJ_COLS_ABOVE] = (tp_i64)c1[nx + rmax];
    out[CHS_TP_SUM_BELOW] = t0; out[CHS_TP_SUM_ABOVE] = t1;
    if ((tp_i64)c0[rmax] + (tp_i64)c1[rmax] != (tp_i64)N * N) e |= TP_ERR_TOTAL;
    if (e) atomicOr(&words[TP_W_ERR], e);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct TpResult {   // pinned
  int words[TP_NW];
  tp_i64 out[CHS_TP_WORDS];
};

struct TpBuf : LookBase {   // have: counts is the look's snapshot
  int nw = 0, rmax = 0;
  unsigned* planes = nullptr;   // [2][N][nw]: the row plane of phase 0, then that of phase 1
  tp_u64* counts = nullptr;     // [2][rmax + 1][2 rmax + 1], re-sized when a look has another rmax
  tp_i64* out = nullptr;        // [CHS_TP_WORDS]
  int* words = nullptr;         // [TP_NW]
  TpResult* hRes = nullptr;
};

void tp_release(TpBuf* s) {
  if (!s) return;
  hipFree(s->planes); hipFree(s->counts); hipFree(s->out); hipFree(s->words);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int tp_alloc(TpBuf* s) {   // what depends on N alone; the count table: tp_resize
  const int N = s->N;
  s->nw = (N + TP_WORD - 1) / TP_WORD;
  CHS_HIP(hipMalloc(&s->planes, sizeof(unsigned) * 2 * (size_t)N * s->nw));
  CHS_HIP(hipMalloc(&s->out, sizeof(tp_i64) * CHS_TP_WORDS));
  CHS_HIP(hipMalloc(&s->words, sizeof(int) * TP_NW));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(TpResult), hipHostMallocDefault));
  return CHS_OK;
}

int tp_resize(TpBuf* s, int rmax) {
  if (s->counts && s->rmax == rmax) return CHS_OK;
  look_forget(s);   // (the snapshot goes with its table)
  hipFree(s->counts);
  s->counts = nullptr; s->rmax = 0;
  CHS_HIP(hipMalloc(&s->counts, sizeof(tp_u64) * (size_t)chs_two_point_size(s->N, rmax)));
  s->rmax = rmax;
  return CHS_OK;
}

template <typename T>
int launch_mask(const TpBuf* s, const void* U, double t, hipStream_t st) {
  const int N = s->N, groups = (N + CHS_WAVE - 1) / CHS_WAVE, per = TP_THREADS / CHS_WAVE;
  const dim3 grid((groups + per - 1) / per, (N + TP_MASK_ROWS - 1) / TP_MASK_ROWS);
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  if (chs_grid_exceeds_cache((size_t)N, sizeof(T))) k_tp_mask<T, true><<<grid, TP_THREADS, 0, st>>>(U, N, s->nw, t, s->planes);
  else k_tp_mask<T, false><<<grid, TP_THREADS, 0, st>>>(U, N, s->nw, t, s->planes);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

int tp_run(TpBuf* s, Engine* E, hipStream_t st, double t, const std::string& who) {
  const int N = s->N, rmax = s->rmax;
  const size_t n = (size_t)chs_two_point_size(N, rmax);
  look_forget(s);
  CHS_HIP(hipMemsetAsync(s->words, 0, sizeof(int) * TP_NW, st));
  CHS_HIP(hipMemsetAsync(s->counts, 0, sizeof(tp_u64) * n, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  const int rc = E->dtype == CHS_F64 ? launch_mask<double>(s, E->dU, t, st) : launch_mask<float>(s, E->dU, t, st);
  if (rc) return rc;
  const int bands = (N + TP_H - 1) / TP_H, nchunks = (s->nw + TP_CW - 1) / TP_CW;
  k_tp_pairs<<<dim3(bands * nchunks, rmax + 1, 2), TP_THREADS, 0, st>>>(s->planes, N, s->nw, nchunks, rmax, s->counts);
  CHS_HIP(hipGetLastError());
  k_tp_fin<<<1, TP_FIN_THREADS, 0, st>>>(s->counts, N, rmax, s->out, s->words);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(s->hRes->words, s->words, sizeof(int) * TP_NW, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(s->hRes->out, s->out, sizeof(tp_i64) * CHS_TP_WORDS, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const int err = s->hRes->words[TP_W_ERR];
  if (err) {
    std::string m;
    if (err & TP_ERR_TOTAL) m += " N_BELOW + N_ABOVE is not N^2;";
    if (err & TP_ERR_SYM) m += " the row dy = 0 of a table is not symmetric in dx;";
    if (err & TP_ERR_PAIRS) m += " c0 + c1 exceeds pairs(dy, dx) at some displacement, or an entry is negative;";
    chs_set_error(who + ": self-check failed:" + m);
    return CHS_ECHECK;
  }
  return look_end(s);
}
}  // namespace

void chs_tp_free(void** buf) {
  if (!buf) return;
  tp_release((TpBuf*)*buf);
  *buf = nullptr;
}

void chs_tp_forget(void* buf) {
  if (buf) look_forget((TpBuf*)buf);
}

int chs_tp_look(Engine* E, hipStream_t st, void** buf, double threshold, int32_t rmax, int64_t* out, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(out, threshold, who))) return rc;
  if (rmax < 1 || rmax > chs_two_point_max_r(E->N)) {
    chs_set_error(who + ": rmax = " + std::to_string(rmax) + " outside [1, " + std::to_string(chs_two_point_max_r(E->N)) + "]");
    return CHS_EINVAL;
  }
  if ((rc = look_check_field(E, TP_MAX_N, who))) return rc;
  if ((rc = look_buffers<TpBuf>(buf, E->N, tp_alloc, tp_release))) return rc;
  TpBuf* s = (TpBuf*)*buf;
  if ((rc = tp_resize(s, rmax))) return rc;
  if ((rc = tp_run(s, E, st, threshold, who))) return rc;
  memcpy(out, s->hRes->out, sizeof(int64_t) * CHS_TP_WORDS);
  return CHS_OK;
}

int chs_tp_counts(void* buf, int device, hipStream_t st, int64_t n, int64_t* out, const char* who_) {
  const std::string who(who_);
  const TpBuf* s = (const TpBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  const int64_t want = chs_two_point_size(s->N, s->rmax);
  if (n != want) { chs_set_error(who + ": n = " + std::to_string(n) + ", expected " + std::to_string(want)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->counts, sizeof(int64_t) * (size_t)n);
}

int chs_tp_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const TpBuf*)buf, ms, what);
}

extern "C" int32_t chs_two_point_max_r(int32_t N) { return N < 2 ? 0 : (N - 1 < CHS_TP_MAX_R ? N - 1 : CHS_TP_MAX_R); }

extern "C" int64_t chs_two_point_size(int32_t N, int32_t rmax) {
  return rmax < 1 || rmax > chs_two_point_max_r(N) ? 0 : 2 * (int64_t)(rmax + 1) * (2 * rmax + 1);
}

extern "C" int chs_two_point(chs_handle h, double threshold, int32_t rmax, int64_t out[CHS_TP_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_two_point: null handle"); return CHS_EINVAL; }
  return chs_tp_look(E, E->stream, &E->tp, threshold, rmax, out, "chs_two_point");
}

extern "C" int chs_two_point_counts(chs_handle h, int64_t n, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_two_point_counts: null handle"); return CHS_EINVAL; }
  return chs_tp_counts(E->tp, E->hc.device, E->stream, n, out, "chs_two_point_counts");
}

extern "C" int chs_two_point_last_ms(chs_handle h, double* ms) {
  return chs_tp_last_ms(h, h ? ((Engine*)h)->tp : nullptr, ms, "chs_two_point");
}

extern "C" int chs_two_point_tile(int32_t* word_bits, int32_t* band_rows, int32_t* lanes) {
  if (!word_bits || !band_rows || !lanes) { chs_set_error("chs_two_point_tile: null argument"); return CHS_EINVAL; }
  *word_bits = TP_WORD;
  *band_rows = TP_H;
  *lanes = TP_THREADS;
  return CHS_OK;
}
