// chs_morphology.hip -- area, interface length and Euler number of the thresholded field, on the device (DESIGN.md
// section 3c; the definition: include/chs_hip.h, chs_morphology).
//
//   X[i][j] = ((double)U[i][j] < t), one ring of background around it; window (i, j), 0 <= i, j <= N, holds
//   X[i-1][j-1], X[i-1][j], X[i][j-1], X[i][j].  The (N+1)^2 windows are counted by their number of foreground
//   pixels, the two-pixel windows apart by diagonal and adjacent: Q0, Q1, Q2, QD, Q3, Q4, and `border`, the
//   foreground pixels of rows 0, N-1 and columns 0, N-1.  Integers only: the same bits at every call.
//
// One sweep over U, nothing N x N written.  A workgroup owns a tile of MORPH_TR x MORPH_TC windows; each of its four
// wavefronts walks MORPH_TR / 4 rows of it downward, the whole width of the tile per row (pixel j is at lane
// (j - j0) / V of load (j - j0) / (64 V), as in k_spec_bins).  A lane keeps one bit per pixel: the row's and the row
// above's, and beside each its left neighbour's -- from the lane before (__shfl_up), from the last lane of the load
// before (lane 0), from a load of its own (lane 0 of the first load: the halo column).  A row is thus loaded once per
// tile, plus one halo row per wavefront (TR / 4 + 1 rows read for TR / 4).  The four masks are classified as bit
// slices, a popcount per class and row; the 32-bit counters of a lane are added over the wavefront, the wavefronts'
// in LDS, and one [CHS_MORPH_WORDS] int64 partial per tile goes to HBM.  k_morph_fin adds the tiles.
#include <cstring>

#include "chs_look.h"

#define MORPH_THREADS 256
#define MORPH_WAVES (MORPH_THREADS / CHS_WAVE)
#define MORPH_TR 128                      // window rows of a tile: MORPH_RW per wavefront
#define MORPH_TC 512                      // window columns of a tile
#define MORPH_RW (MORPH_TR / MORPH_WAVES)
#define MORPH_NCNT 6                      // counters of a lane: Q1, Q2 + QD, QD, Q3, Q4, border

typedef long long morph_i64;
static_assert(sizeof(morph_i64) == sizeof(int64_t), "the result words are int64");

// one member of a launch: the single handle's launch has one
struct MorphMember {
  const void* U;       // the field
  double threshold;
  int dtype;           // CHS_F64 / CHS_F32 (one launch has one type: its kernel's)
  int pad_;
};

// Row i of the field, the tile's MORPH_TC columns from j0 on: x[c][k] = U[i][j0 + (64 c + lane) V + k] and
// h = U[i][j0 - 1].  No branch guards a load: a row or a column outside the grid is clamped to the nearest one inside
// -- a load more of a cache line that is read anyway -- and the caller masks what it stands for, so that the loop around
// is straight-line code and the next row's loads stay in flight behind the counted waits for this row's.
template <typename T, int V, bool NT>
__device__ __forceinline__ void morph_load(const T CHS_GLOBAL* U, int N, int i, int j0, int lane,
                                           T (&x)[MORPH_TC / (CHS_WAVE * V)][V], T& h) {
  constexpr int CHUNK = CHS_WAVE * V, NCH = MORPH_TC / CHUNK;
  const T CHS_GLOBAL* row = U + (size_t)(i < 0 ? 0 : (i < N ? i : N - 1)) * N;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    int j = j0 + c * CHUNK + lane * V;
    j = j < N ? j : N - V;   // (V > 1: N is a multiple of V and so is j -- j < N is j + V - 1 < N -- and every row starts aligned)
    chs_load<T, V, NT>(row + j, x[c]);
  }
  // The halo pixel has one address for the wavefront, which the compiler would fetch with a scalar load; scalar loads
  // share their counter with the cross-lane moves, whose waits would then wait for the next row's halo.  A vector load.
  int jh = j0 > 0 ? j0 - 1 : 0;
  asm volatile("" : "+v"(jh));
  h = row[jh];
}

// part[member][tile][CHS_MORPH_WORDS] <- the tile's counts.  grid (column tiles, row tiles, members) over the
// (N+1) x (N+1) windows.  V: pixels per lane and load (16 bytes where N is a multiple of V).
template <typename T, int V, bool NT>
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_quads(const MorphMember* __restrict__ mem, int N,
                                                               morph_i64* __restrict__ part) {
  __shared__ int red[MORPH_WAVES][MORPH_NCNT];
  constexpr int CHUNK = CHS_WAVE * V, NCH = MORPH_TC / CHUNK, NB = NCH * V;   // NB = 8 bits of a lane per row
  constexpr unsigned ALL = (1u << NB) - 1u;
  unsigned k0 = 0;   // the bits of the first pixel of every load
#pragma unroll
  for (int c = 0; c < NCH; ++c) k0 |= 1u << (c * V);
  const MorphMember m = mem[blockIdx.z];
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)m.U;
  const double t = m.threshold;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = chs_wave_id();   // (an SGPR: the row loop's branches are scalar)
  const int i0 = blockIdx.y * MORPH_TR + wave * MORPH_RW, j0 = blockIdx.x * MORPH_TC;

  unsigned colv = 0, col0 = 0, colN = 0;   // this lane's bits inside the grid, in column 0, in column N - 1
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int j = j0 + c * CHUNK + lane * V + k;
      const unsigned bit = 1u << (c * V + k);
      if (j < N) colv |= bit;
      if (j == 0) col0 |= bit;
      if (j == N - 1) colN |= bit;
    }

  // the foreground bits of a loaded row (bit c V + k: pixel x[c][k]; `in`: the row is one of the grid's) and their left
  // neighbours'
  auto bits_of = [&](const T (&x)[NCH][V], bool in) -> unsigned {
    unsigned b = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int k = 0; k < V; ++k) b |= ((double)x[c][k] < t) ? (1u << (c * V + k)) : 0u;
    return in ? (b & colv) : 0u;
  };
  auto left_of = [&](unsigned b, T h, bool in) -> unsigned {
    const unsigned up = __shfl_up(b, 1, CHS_WAVE), last = __shfl(b, CHS_WAVE - 1, CHS_WAVE);
    const unsigned own = (b << 1) & ~k0 & ALL;                          // pixel k - 1 of the same load
    const unsigned edge = (lane != 0) ? (up >> (V - 1))                 // the lane before: its pixel V - 1 of every load
                                      : (((last >> (V - 1)) << V) | ((in && j0 > 0 && (double)h < t) ? 1u : 0u));
    return own | (edge & k0);
  };

  int cnt[MORPH_NCNT] = {0, 0, 0, 0, 0, 0};
  if (i0 <= N) {   // (uniform in the wavefront)
    T x[NCH][V], h;
    bool in = i0 >= 1;   // (row i0 - 1 <= N - 1)
    morph_load<T, V, NT>(U, N, i0 - 1, j0, lane, x, h);
    unsigned pb = bits_of(x, in);
    unsigned pl = left_of(pb, h, in);
    morph_load<T, V, NT>(U, N, i0, j0, lane, x, h);
#pragma unroll 2
    for (int r = 0; r < MORPH_RW; ++r) {
      const int i = i0 + r;
      if (i > N) break;   // (uniform)
      in = i < N;
      T nx[NCH][V], nh;   // the next row is on its way while this one is counted
      morph_load<T, V, NT>(U, N, i + 1, j0, lane, nx, nh);
      const unsigned cb = bits_of(x, in);
      const unsigned cl = left_of(cb, h, in);
      // bit slices of n = pl + pb + cl + cb per window
      const unsigned x1 = pl ^ pb, a1 = pl & pb, x2 = cl ^ cb, a2 = cl & cb;
      const unsigned s0 = x1 ^ x2, s1 = a1 ^ a2 ^ (x1 & x2);
      cnt[0] += __popc(s0 & ~s1);                                       // n = 1
      cnt[1] += __popc(~s0 & s1);                                       // n = 2, both kinds
      cnt[2] += __popc((pl & cb & ~pb & ~cl) | (pb & cl & ~pl & ~cb));  // the diagonal ones among them
      cnt[3] += __popc(s0 & s1);                                        // n = 3
      cnt[4] += __popc(a1 & a2);                                        // n = 4
      cnt[5] += __popc(cb & col0) + __popc(cb & colN) + ((i == 0) ? __popc(cb) : 0) + ((i == N - 1) ? __popc(cb) : 0);
      pb = cb; pl = cl;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int k = 0; k < V; ++k) x[c][k] = nx[c][k];
      h = nh;
    }
  }
#pragma unroll
  for (int q = 0; q < MORPH_NCNT; ++q) {
    int v = cnt[q];
#pragma unroll
    for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, CHS_WAVE);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    morph_i64 s[MORPH_NCNT];
#pragma unroll
    for (int q = 0; q < MORPH_NCNT; ++q) {
      s[q] = 0;
#pragma unroll
      for (int w = 0; w < MORPH_WAVES; ++w) s[q] += red[w][q];
    }
    const int ti = blockIdx.y * MORPH_TR;
    const morph_i64 rows = (N + 1 - ti < MORPH_TR) ? (N + 1 - ti) : MORPH_TR;
    const morph_i64 cols = (N + 1 - j0 < MORPH_TC) ? (N + 1 - j0) : MORPH_TC;
    morph_i64* out = part + ((size_t)blockIdx.z * (gridDim.x * gridDim.y) + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * CHS_MORPH_WORDS;
    out[CHS_MORPH_Q0] = rows * cols - (s[0] + s[1] + s[3] + s[4]);      // the tile's windows that are none of the others
    out[CHS_MORPH_Q1] = s[0];
    out[CHS_MORPH_Q2] = s[1] - s[2];
    out[CHS_MORPH_QD] = s[2];
    out[CHS_MORPH_Q3] = s[3];
    out[CHS_MORPH_Q4] = s[4];
    out[CHS_MORPH_BORDER] = s[5];
  }
}

// out[member][CHS_MORPH_WORDS] <- the sum over the member's tiles: lane l adds tiles l, l + 64, ... in that order, the
// lanes by a fixed tree (integers: any order gives these bits).  One wavefront per member.
__global__ __launch_bounds__(CHS_WAVE) void k_morph_fin(const morph_i64* __restrict__ part, int ntiles,
                                                         morph_i64* __restrict__ out) {
  const morph_i64* p = part + (size_t)blockIdx.x * ntiles * CHS_MORPH_WORDS;
  morph_i64 s[CHS_MORPH_WORDS];
#pragma unroll
  for (int w = 0; w < CHS_MORPH_WORDS; ++w) s[w] = 0;
  for (int tl = threadIdx.x; tl < ntiles; tl += CHS_WAVE)
#pragma unroll
    for (int w = 0; w < CHS_MORPH_WORDS; ++w) s[w] += p[(size_t)tl * CHS_MORPH_WORDS + w];
#pragma unroll
  for (int w = 0; w < CHS_MORPH_WORDS; ++w) {
    morph_i64 v = s[w];
#pragma unroll
    for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, CHS_WAVE);
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * CHS_MORPH_WORDS + w] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct MorphBuf {
  int B = 0, N = 0, tx = 0, ty = 0;
  MorphMember* mem = nullptr;   // [B] device records
  morph_i64* part = nullptr;    // [B][tx * ty][CHS_MORPH_WORDS]
  morph_i64* out = nullptr;     // [B][CHS_MORPH_WORDS]
  morph_i64* hOut = nullptr;    // pinned [B][CHS_MORPH_WORDS]
  hipEvent_t ev[2] = {nullptr, nullptr};   // around the two kernels of the last look
  double ms = -1.0;
};

void morph_release(MorphBuf* s) {
  if (!s) return;
  hipFree(s->mem); hipFree(s->part); hipFree(s->out);
  if (s->hOut) hipHostFree(s->hOut);
  for (auto e : s->ev) if (e) hipEventDestroy(e);
  delete s;
}

int morph_buffers(void** buf, int B, int N) {
  MorphBuf* s = (MorphBuf*)*buf;
  if (s && s->B == B && s->N == N) return CHS_OK;
  morph_release(s);
  *buf = nullptr;
  s = new (std::nothrow) MorphBuf();
  if (!s) { chs_set_error("out of host memory"); return CHS_EINVAL; }
  *buf = s;   // (freed with its owner whatever fails below)
  s->B = B; s->N = N;
  s->tx = (N + 1 + MORPH_TC - 1) / MORPH_TC; s->ty = (N + 1 + MORPH_TR - 1) / MORPH_TR;
  const size_t nt = (size_t)s->tx * s->ty;
  CHS_HIP(hipMalloc(&s->mem, sizeof(MorphMember) * (size_t)B));
  CHS_HIP(hipMalloc(&s->part, sizeof(morph_i64) * (size_t)B * nt * CHS_MORPH_WORDS));
  CHS_HIP(hipMalloc(&s->out, sizeof(morph_i64) * (size_t)B * CHS_MORPH_WORDS));
  CHS_HIP(hipHostMalloc((void**)&s->hOut, sizeof(morph_i64) * (size_t)B * CHS_MORPH_WORDS, hipHostMallocDefault));
  for (auto& e : s->ev) CHS_HIP(hipEventCreate(&e));
  return CHS_OK;
}

template <typename T>
int launch_quads(const MorphBuf* s, hipStream_t st) {
  constexpr int V = ChsVec<T>::V;
  const dim3 grid(s->tx, s->ty, s->B);
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  const bool nt = chs_grid_exceeds_cache((size_t)s->N, sizeof(T));
  if (s->N % V == 0) {
    if (nt) k_morph_quads<T, V, true><<<grid, MORPH_THREADS, 0, st>>>(s->mem, s->N, s->part);
    else k_morph_quads<T, V, false><<<grid, MORPH_THREADS, 0, st>>>(s->mem, s->N, s->part);
  } else {
    if (nt) k_morph_quads<T, 1, true><<<grid, MORPH_THREADS, 0, st>>>(s->mem, s->N, s->part);
    else k_morph_quads<T, 1, false><<<grid, MORPH_THREADS, 0, st>>>(s->mem, s->N, s->part);
  }
  CHS_HIP(hipGetLastError());
  k_morph_fin<<<s->B, CHS_WAVE, 0, st>>>(s->part, s->tx * s->ty, s->out);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

// The look at B members (one N, one element type) on one stream: two launches, one copy, one wait.  Nothing of the
// members is written and nothing the step loop owns is read (no state, no halt flag): their fields alone.
int morph_run(Engine* const* m, int B, hipStream_t st, void** buf, const double* threshold, int64_t* out) {
  Engine* E0 = m[0];
  int rc;
  if ((rc = morph_buffers(buf, B, E0->N))) return rc;
  MorphBuf* s = (MorphBuf*)*buf;
  std::vector<MorphMember> rec((size_t)B);   // (the records outlive the stream's work: the wait below)
  for (int i = 0; i < B; ++i) rec[(size_t)i] = MorphMember{m[i]->dU, threshold[i], m[i]->dtype, 0};
  CHS_HIP(hipMemcpyAsync(s->mem, rec.data(), sizeof(MorphMember) * (size_t)B, hipMemcpyHostToDevice, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  rc = E0->dtype == CHS_F64 ? launch_quads<double>(s, st) : launch_quads<float>(s, st);
  if (!rc) {
    hipError_t e = hipEventRecord(s->ev[1], st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->hOut, s->out, sizeof(morph_i64) * (size_t)B * CHS_MORPH_WORDS, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) rc = chs_hip_fail(e, "chs_morphology: event / copy", __FILE__, __LINE__);
  }
  CHS_HIP(hipStreamSynchronize(st));   // (also behind a failure: `rec` is not read any longer when it goes)
  if (rc) return rc;
  float ms = 0.f;
  CHS_HIP(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->ms = ms;
  memcpy(out, s->hOut, sizeof(morph_i64) * (size_t)B * CHS_MORPH_WORDS);
  return CHS_OK;
}

int check_args(const double* threshold, int B, const int64_t* out, const std::string& who) {
  if (!threshold || !out) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  for (int i = 0; i < B; ++i)
    if (!std::isfinite(threshold[i])) { chs_set_error(who + ": the threshold must be finite"); return CHS_EINVAL; }
  return CHS_OK;
}
}  // namespace

void chs_morph_free(void** buf) {
  if (!buf) return;
  morph_release((MorphBuf*)*buf);
  *buf = nullptr;
}

void chs_morph_forget(void* buf) {
  if (buf) ((MorphBuf*)buf)->ms = -1.0;
}

int chs_morph_one(Engine* E, const double* threshold, int64_t* out, const char* who) {
  int rc;
  if ((rc = check_args(threshold, 1, out, who))) return rc;
  if (!E->have_U) { chs_set_error(std::string(who) + ": no field (chs_set_U / chs_init_U_pcg64 first)"); return CHS_ESTATE; }
  CHS_HIP(hipSetDevice(E->hc.device));
  Engine* one[1] = {E};
  return morph_run(one, 1, E->stream, &E->morph, threshold, out);
}

int chs_morph_all(Engine* const* m, int B, hipStream_t s, void** buf, const double* threshold, int64_t* out, const char* who) {
  int rc;
  if ((rc = check_args(threshold, B, out, who))) return rc;
  for (int i = 0; i < B; ++i)
    if (!m[i]->have_U) { chs_set_error(std::string(who) + ": member " + std::to_string(i) + " has no field"); return CHS_ESTATE; }
  CHS_HIP(hipSetDevice(m[0]->hc.device));
  return morph_run(m, B, s, buf, threshold, out);
}

extern "C" int chs_morphology(chs_handle h, double threshold, int64_t out[CHS_MORPH_WORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_morphology: null handle"); return CHS_EINVAL; }
  return chs_morph_one(E, &threshold, out, "chs_morphology");
}

extern "C" int chs_morphology_last_ms(chs_handle h, double* ms) {
  Engine* E = (Engine*)h;
  if (!E || !ms) { chs_set_error("chs_morphology_last_ms: null argument"); return CHS_EINVAL; }
  const MorphBuf* s = (const MorphBuf*)E->morph;
  if (!s || s->ms < 0.0) { chs_set_error("chs_morphology_last_ms: no chs_morphology call so far"); return CHS_ESTATE; }
  *ms = s->ms;
  return CHS_OK;
}
