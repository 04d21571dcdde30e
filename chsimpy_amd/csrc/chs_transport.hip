// chs_transport.hip -- transport look at a phase of the thresholded field on the device: the steady diffusion problem through
// the spanning components of the phase between two opposite walls of the box, solved matrix-free by conjugate gradients in
// fp64: effective diffusivity, formation factor, tortuosity factor (the definition: include/chs_hip.h,
// chs_transport).
//
// A transport look is a components look at connectivity 4 first: chs_cc_look leaves the root label L of every pixel, the
// component number at a root and the table of bounding boxes on the handle's component buffers.  The field itself is
// never read.  Then, with 64 x 64 tiles, thread t of 256 owning the pixels (4 k + t / 64, t % 64), k = 0 .. 15, of a tile:
//   1  k_trn_span    per component: does its bounding box touch both walls?
//      k_trn_setup   a byte per pixel (four bond bits, two wall bits, the active bit), x <- 0 / -1 / -2 (active, background,
//                    foreground that is not active), r <- b; the integer words by integer adds; a flag per tile.
//      k_trn_list    the tiles that hold an active pixel, in index order, and the scalars of the iteration.
//   2  per iteration k, over the listed tiles alone:
//      k_trn_ap      p_k = r + beta p_(k-1) on the fly for the tile and its four halo edges (p is double-buffered by the
//                    parity of k: a workgroup reads the old buffer of its neighbours while they write the new one),
//                    q = A p_k from LDS, the partial sum of p.q; the last workgroup to arrive forms alpha.
//      k_trn_update  x += alpha p, r -= alpha q, the partial sums of r.r, |r|_1, F_in, F_out; the last workgroup to
//                    arrive forms beta, counts the iteration and sets `done` when the recurrence residual meets the
//                    acceptance rule.  Kernels launched after that return at once.
//      The host issues TRN_CHUNK iterations at a time and reads the scalars after each chunk.  No workgroup waits for
//      another; the host never supplies a scalar.
//   3  k_trn_close, k_trn_fin   the closing sweep: the true residual b - A x into q, its norms, the sum of x and the
//                    lines of the profile; the host accepts the look on these.  Where the true residual fails the rule the
//                    recurrence passed, k_trn_resume puts it in the place of r, p stays, and the iteration goes on.
// Every float sum has a fixed order: a thread over its pixels in k order, a wavefront by shuffles, the four wavefronts in
// order, the tiles by a strided sum in list order and the same tree.  No float atomics.
#include <algorithm>
#include <cfloat>
#include <cstring>

#include "chs_look.h"

#define TRN_T 64                            // tile edge
#define TRN_P (TRN_T + 2)                   // ... with its halo
#define TRN_THREADS 256
#define TRN_K (TRN_T * TRN_T / TRN_THREADS) // pixels of a thread
#define TRN_CHUNK 32                        // iterations the host issues between two looks at the scalars
#define TRN_FACTOR 48ll                     // chs_transport_iters_default(N) = TRN_FACTOR N + TRN_SLACK
#define TRN_SLACK 64ll
#define TRN_MAX_FACTOR 16ll                 // max_iters at most that many defaults
#define TRN_TOL_MIN 1e-12
#define TRN_TOL_MAX 1e-2
// the byte of a pixel
#define TRN_UP 1u
#define TRN_DOWN 2u
#define TRN_LEFT 4u
#define TRN_RIGHT 8u
#define TRN_SRC 16u
#define TRN_TGT 32u
#define TRN_ACT 64u
// the integer counters of a look
#define TRN_C_FG 0
#define TRN_C_ACTIVE 1
#define TRN_C_SPANNING 2
#define TRN_C_SRC 3
#define TRN_C_TGT 4
#define TRN_C_BONDS 5
#define TRN_C_ERR 6
#define TRN_C_NTL 7
#define TRN_NC 8
// partial sums of a workgroup
#define TRN_NB 4                            // k_trn_update: r.r, |r|_1, F_in, F_out
#define TRN_NS 3                            // k_trn_close: |r|_1, r.r, sum of x (and the maximum of |r| behind them)
#define TRN_NL 4                            // a line of the profile: cut, sum of x, active pixels, flux into the target wall

static_assert(TRN_THREADS == 4 * CHS_WAVE && TRN_T == CHS_WAVE, "a wavefront per row of a slab of four");

typedef unsigned long long trn_u64;
typedef unsigned char trn_byte;

struct TrnScal {      // the scalars of the iteration, on the device
  double rr, pq, alpha, beta, res1, fin, fout, tol;
  unsigned done, iters, ticket, pad;
};

struct TrnOut {       // the closing sweep
  double fin, fout, res1, resinf, cutmin, cutmax, csum, rr;
};

__host__ __device__ inline int trn_depth(int source, int N, int i, int j) {
  return source == 0 ? i : source == 1 ? N - 1 - i : source == 2 ? j : N - 1 - j;
}

// ---- the pieces of a reduction ------------------------------------------------------------------------------------------
__device__ __forceinline__ double trn_ld(const double* p) {   // a word another workgroup of this launch wrote
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const trn_u64*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// v[m] of thread 0 <- the sum over the workgroup, wavefront by wavefront
template <int M>
__device__ __forceinline__ void trn_block_sum(double (&v)[M], double (*red)[M]) {
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v[m] += __shfl_down(v[m], off, CHS_WAVE);
    if (lane == 0) red[wave][m] = v[m];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = ((red[0][m] + red[1][m]) + red[2][m]) + red[3][m];
  }
}

__device__ __forceinline__ double trn_block_max(double v, double* red) {
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, CHS_WAVE));
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// Thread 0 has stored this workgroup's partial sums.  True, in every thread, for the workgroup that arrives last: release
// and acquire at agent scope around the ticket, explicit waits on both sides as in k_colmin_slices (chs_pointwise.hip).
__device__ __forceinline__ bool trn_arrive(unsigned* ticket, unsigned nblocks, unsigned* slast) {
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool last = atomicAdd(ticket, 1u) == nblocks - 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *slast = last ? 1u : 0u;
  }
  __syncthreads();
  return *slast != 0u;
}

// v[m] of thread 0 <- the sum of part[b][m] over the workgroups b in a fixed order (the last workgroup calls this)
template <int M>
__device__ __forceinline__ void trn_total(const double* part, int nparts, double (&v)[M], double (*red)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) v[m] = 0.0;
  for (int b = threadIdx.x; b < nparts; b += TRN_THREADS) {
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] += trn_ld(part + (size_t)b * M + m);
  }
  trn_block_sum<M>(v, red);
}

__device__ __forceinline__ double trn_dir(double beta, double pold, double r) { return fma(beta, pold, r); }

__device__ __forceinline__ double trn_diag(unsigned c) {
  return (double)(__popc(c & 15u) + ((c & TRN_SRC) ? 2 : 0) + ((c & TRN_TGT) ? 2 : 0));
}

// (A v) at a pixel with byte c whose value v0 and neighbours lie in LDS around s
__device__ __forceinline__ double trn_apply(unsigned c, double v0, const double* s) {
  double a = trn_diag(c) * v0;
  if (c & TRN_UP) a -= s[-TRN_P];
  if (c & TRN_DOWN) a -= s[TRN_P];
  if (c & TRN_LEFT) a -= s[-1];
  if (c & TRN_RIGHT) a -= s[1];
  return a;
}

// the halo pixel of thread t: side t / 64 (top, bottom, left, right), position t % 64; *q: its place in LDS
__device__ __forceinline__ bool trn_halo(int i0, int j0, int N, int* gi, int* gj, int* q) {
  const int side = threadIdx.x / TRN_T, pos = threadIdx.x % TRN_T;
  *gi = side == 0 ? i0 - 1 : side == 1 ? i0 + TRN_T : i0 + pos;
  *gj = side == 2 ? j0 - 1 : side == 3 ? j0 + TRN_T : j0 + pos;
  *q = side == 0 ? pos + 1 : side == 1 ? (TRN_P - 1) * TRN_P + pos + 1 : side == 2 ? (pos + 1) * TRN_P : (pos + 1) * TRN_P + TRN_P - 1;
  return *gi >= 0 && *gi < N && *gj >= 0 && *gj < N;
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRN_THREADS) void k_trn_span(const int* __restrict__ table, int count, int N, int source,
                                                          trn_byte* __restrict__ span, trn_u64* __restrict__ cnt) {
  const int c = blockIdx.x * TRN_THREADS + threadIdx.x;
  if (c >= count) return;
  const int* row = table + (size_t)c * CHS_CC_COLS;           // first, area, imin, imax, jmin, jmax
  const bool sp = source < 2 ? (row[2] == 0 && row[3] == N - 1) : (row[4] == 0 && row[5] == N - 1);
  span[c] = sp ? 1 : 0;
  if (sp) atomicAdd(&cnt[TRN_C_SPANNING], (trn_u64)1);
}

// grid nt * nt, a workgroup per tile
__global__ __launch_bounds__(TRN_THREADS) void k_trn_setup(const int* __restrict__ L, const int* __restrict__ id,
                                                           const trn_byte* __restrict__ span, int count, int N, int nt, int source,
                                                           trn_byte* __restrict__ code, double* __restrict__ x, double* __restrict__ r,
                                                           unsigned* __restrict__ tflag, trn_u64* __restrict__ cnt) {
  __shared__ unsigned sum[6];
  if (threadIdx.x < 6) sum[threadIdx.x] = 0;
  __syncthreads();
  const int ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = tj * TRN_T + lane;
  const unsigned n2 = (unsigned)N * (unsigned)N;
  unsigned fg = 0, act = 0, src = 0, tgt = 0, bonds = 0, err = 0;
#pragma unroll 1
  for (int k = 0; k < TRN_K; ++k) {
    const int i = ti * TRN_T + 4 * k + wave;
    if (i >= N || j >= N) continue;
    const size_t p = (size_t)i * N + j;
    const int l = L[p];
    unsigned c = 0;
    double xv = -1.0, rv = 0.0;
    if (l >= 0) {
      fg += 1;
      const int comp = (unsigned)l < n2 ? id[l] : -1;
      if (comp < 0 || comp >= count) err = 1;
      else if (span[comp]) {
        // 4-adjacent foreground pixels are one component: a foreground neighbour of an active pixel is active
        c = TRN_ACT;
        if (i > 0 && L[p - N] >= 0) c |= TRN_UP;
        if (i + 1 < N && L[p + N] >= 0) c |= TRN_DOWN;
        if (j > 0 && L[p - 1] >= 0) c |= TRN_LEFT;
        if (j + 1 < N && L[p + 1] >= 0) c |= TRN_RIGHT;
        const int d = trn_depth(source, N, i, j);
        if (d == 0) c |= TRN_SRC;
        if (d == N - 1) c |= TRN_TGT;
        act += 1; src += (c & TRN_SRC) ? 1 : 0; tgt += (c & TRN_TGT) ? 1 : 0;
        bonds += ((c & TRN_DOWN) ? 1 : 0) + ((c & TRN_RIGHT) ? 1 : 0);
        xv = 0.0; rv = (c & TRN_SRC) ? 2.0 : 0.0;
      } else {
        xv = -2.0;
      }
    }
    code[p] = (trn_byte)c; x[p] = xv; r[p] = rv;
  }
  if (fg) atomicAdd(&sum[0], fg);
  if (act) atomicAdd(&sum[1], act);
  if (src) atomicAdd(&sum[2], src);
  if (tgt) atomicAdd(&sum[3], tgt);
  if (bonds) atomicAdd(&sum[4], bonds);
  if (err) atomicOr(&sum[5], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    tflag[blockIdx.x] = sum[1] ? 1u : 0u;
    if (sum[0]) atomicAdd(&cnt[TRN_C_FG], (trn_u64)sum[0]);
    if (sum[1]) atomicAdd(&cnt[TRN_C_ACTIVE], (trn_u64)sum[1]);
    if (sum[2]) atomicAdd(&cnt[TRN_C_SRC], (trn_u64)sum[2]);
    if (sum[3]) atomicAdd(&cnt[TRN_C_TGT], (trn_u64)sum[3]);
    if (sum[4]) atomicAdd(&cnt[TRN_C_BONDS], (trn_u64)sum[4]);
    if (sum[5]) atomicOr(&cnt[TRN_C_ERR], (trn_u64)1);
  }
}

// one wavefront: list[0 .. ntl) <- the flagged tiles in index order, slot[tile] <- its place or -1; the scalars at x = 0
__global__ __launch_bounds__(CHS_WAVE) void k_trn_list(const unsigned* __restrict__ tflag, int ntiles, int* __restrict__ list,
                                                       int* __restrict__ slot, trn_u64* __restrict__ cnt, TrnScal* __restrict__ sc,
                                                       double tol) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int base = 0; base < ntiles; base += CHS_WAVE) {
    const int t = base + lane;
    const bool f = t < ntiles && tflag[t] != 0u;
    const trn_u64 m = __ballot(f);
    const int at = n + __popcll(m & (((trn_u64)1 << lane) - 1));
    if (f) list[at] = t;
    if (t < ntiles) slot[t] = f ? at : -1;
    n += __popcll(m);
  }
  if (lane == 0) {
    cnt[TRN_C_NTL] = (trn_u64)n;
    TrnScal s;
    s.rr = 4.0 * (double)cnt[TRN_C_SRC];          // b.b: the setup kernel is complete
    s.pq = 0.0; s.alpha = 0.0; s.beta = 0.0; s.res1 = 2.0 * (double)cnt[TRN_C_SRC]; s.fin = s.res1; s.fout = 0.0; s.tol = tol;
    s.done = 0; s.iters = 0; s.ticket = 0; s.pad = 0;
    *sc = s;
  }
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------
// grid ntl.  p_new = r + beta p_old on tile and halo edges, q = A p_new, part[b] <- p_new . q of the tile
__global__ __launch_bounds__(TRN_THREADS) void k_trn_ap(const trn_byte* code_, const double* r_, const double* pold_, double* pnew_,
                                                        double* q_, const int* __restrict__ list, TrnScal* sc, double* part, int N,
                                                        int nt) {
  __shared__ double S[TRN_P * TRN_P];          // (the four corners are never written and never read: a five-point stencil)
  __shared__ double red[4][1], red2[4][1];
  __shared__ unsigned slast;
  if (sc->done) return;                            // (uniform)
  const double beta = sc->beta;
  const trn_byte CHS_GLOBAL* code = (const trn_byte CHS_GLOBAL*)code_;
  const double CHS_GLOBAL* r = (const double CHS_GLOBAL*)r_;
  const double CHS_GLOBAL* pold = (const double CHS_GLOBAL*)pold_;
  double CHS_GLOBAL* pnew = (double CHS_GLOBAL*)pnew_;
  double CHS_GLOBAL* q = (double CHS_GLOBAL*)q_;
  const int tile = list[blockIdx.x];
  const int ti = tile / nt, tj = tile - ti * nt;
  const int i0 = ti * TRN_T, j0 = tj * TRN_T;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = j0 + lane;
  unsigned cd[TRN_K];
  double pv[TRN_K];
#pragma unroll
  for (int k = 0; k < TRN_K; ++k) {
    const int i = i0 + 4 * k + wave;
    cd[k] = 0; pv[k] = 0.0;
    if (i < N && j < N) {
      const size_t p = (size_t)i * N + j;
      cd[k] = code[p];
      if (cd[k] & TRN_ACT) pv[k] = trn_dir(beta, pold[p], r[p]);
    }
    S[(4 * k + wave + 1) * TRN_P + lane + 1] = pv[k];
  }
  {
    int gi, gj, at;
    double v = 0.0;                                  // r and p are 0 off the active set
    if (trn_halo(i0, j0, N, &gi, &gj, &at)) {
      const size_t p = (size_t)gi * N + gj;
      v = trn_dir(beta, pold[p], r[p]);
    }
    S[at] = v;
  }
  __syncthreads();
  double s[1] = {0.0};
#pragma unroll
  for (int k = 0; k < TRN_K; ++k) {
    if (!(cd[k] & TRN_ACT)) continue;
    const int row = 4 * k + wave;
    const double a = trn_apply(cd[k], pv[k], S + (row + 1) * TRN_P + lane + 1);
    const size_t p = (size_t)(i0 + row) * N + j;
    pnew[p] = pv[k]; q[p] = a;
    s[0] = fma(pv[k], a, s[0]);
  }
  trn_block_sum<1>(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
  if (!trn_arrive(&sc->ticket, gridDim.x, &slast)) return;
  double t[1];
  trn_total<1>(part, (int)gridDim.x, t, red2);
  if (threadIdx.x == 0) {
    sc->pq = t[0];
    sc->alpha = t[0] != 0.0 ? sc->rr / t[0] : 0.0;   // a zero denominator: a zero step
    sc->ticket = 0;                                  // (for the next launch: kernel boundaries order it)
  }
}

// grid ntl.  x += alpha p, r -= alpha q; part[b][] <- r.r, |r|_1, F_in, F_out of the tile
__global__ __launch_bounds__(TRN_THREADS) void k_trn_update(const trn_byte* code_, double* x_, double* r_, const double* p_,
                                                            const double* q_, const int* __restrict__ list, TrnScal* sc,
                                                            double* part, int N, int nt) {
  __shared__ double red[4][TRN_NB], red2[4][TRN_NB];
  __shared__ unsigned slast;
  if (sc->done) return;                            // (uniform)
  const double alpha = sc->alpha;
  const trn_byte CHS_GLOBAL* code = (const trn_byte CHS_GLOBAL*)code_;
  double CHS_GLOBAL* x = (double CHS_GLOBAL*)x_;
  double CHS_GLOBAL* r = (double CHS_GLOBAL*)r_;
  const double CHS_GLOBAL* pp = (const double CHS_GLOBAL*)p_;
  const double CHS_GLOBAL* q = (const double CHS_GLOBAL*)q_;
  const int tile = list[blockIdx.x];
  const int ti = tile / nt, tj = tile - ti * nt;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = tj * TRN_T + lane;
  double s[TRN_NB] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < TRN_K; ++k) {
    const int i = ti * TRN_T + 4 * k + wave;
    if (i >= N || j >= N) continue;
    const size_t p = (size_t)i * N + j;
    const unsigned c = code[p];
    if (!(c & TRN_ACT)) continue;
    const double xv = fma(alpha, pp[p], x[p]);
    const double rv = fma(-alpha, q[p], r[p]);
    x[p] = xv; r[p] = rv;
    s[0] = fma(rv, rv, s[0]);
    s[1] += fabs(rv);
    if (c & TRN_SRC) s[2] += 2.0 * (1.0 - xv);
    if (c & TRN_TGT) s[3] += 2.0 * xv;
  }
  trn_block_sum<TRN_NB>(s, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < TRN_NB; ++m) part[(size_t)blockIdx.x * TRN_NB + m] = s[m];
  }
  if (!trn_arrive(&sc->ticket, gridDim.x, &slast)) return;
  double t[TRN_NB];
  trn_total<TRN_NB>(part, (int)gridDim.x, t, red2);
  if (threadIdx.x == 0) {
    const double was = sc->rr;
    sc->beta = was != 0.0 ? t[0] / was : 0.0;
    sc->rr = t[0]; sc->res1 = t[1]; sc->fin = t[2]; sc->fout = t[3];
    sc->iters += 1;
    if (t[1] <= sc->tol * fmin(t[2], t[3])) sc->done = 1;   // the recurrence residual; the closing sweep decides
    sc->ticket = 0;
  }
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------
// grid ntl.  rt = b - A x of the tile; part[b][] <- |rt|_1, rt.rt, sum of x; pmax[b] <- max |rt|; lines[b][64][] <- the
// tile's part of the profile lines that cross it.
__global__ __launch_bounds__(TRN_THREADS) void k_trn_close(const trn_byte* code_, const double* x_, double* rt_,
                                                           const int* __restrict__ list, double* __restrict__ part,
                                                           double* __restrict__ pmax, double* __restrict__ lines, int N, int nt,
                                                           int source) {
  __shared__ double S[TRN_P * TRN_P];          // (the four corners are never written and never read: a five-point stencil)
  __shared__ trn_byte C[TRN_T * TRN_T];
  __shared__ double red[4][TRN_NS], redm[4];
  const trn_byte CHS_GLOBAL* code = (const trn_byte CHS_GLOBAL*)code_;
  const double CHS_GLOBAL* x = (const double CHS_GLOBAL*)x_;
  double CHS_GLOBAL* rt = (double CHS_GLOBAL*)rt_;
  const int tile = list[blockIdx.x];
  const int ti = tile / nt, tj = tile - ti * nt;
  const int i0 = ti * TRN_T, j0 = tj * TRN_T;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x / CHS_WAVE;
  const int j = j0 + lane;
  unsigned cd[TRN_K];
  double xv[TRN_K];
#pragma unroll
  for (int k = 0; k < TRN_K; ++k) {
    const int i = i0 + 4 * k + wave;
    cd[k] = 0; xv[k] = 0.0;
    if (i < N && j < N) {
      const size_t p = (size_t)i * N + j;
      cd[k] = code[p];
      if (cd[k] & TRN_ACT) xv[k] = x[p];
    }
    S[(4 * k + wave + 1) * TRN_P + lane + 1] = xv[k];
    C[(4 * k + wave) * TRN_T + lane] = (trn_byte)cd[k];
  }
  {
    int gi, gj, at;
    double v = 0.0;                                  // (read through a bond alone: an active pixel then)
    if (trn_halo(i0, j0, N, &gi, &gj, &at)) v = x[(size_t)gi * N + gj];
    S[at] = v;
  }
  __syncthreads();
  double s[TRN_NS] = {0.0, 0.0, 0.0};
  double big = 0.0;
#pragma unroll
  for (int k = 0; k < TRN_K; ++k) {
    if (!(cd[k] & TRN_ACT)) continue;
    const int row = 4 * k + wave;
    const double a = trn_apply(cd[k], xv[k], S + (row + 1) * TRN_P + lane + 1);
    const double v = ((cd[k] & TRN_SRC) ? 2.0 : 0.0) - a;
    rt[(size_t)(i0 + row) * N + j] = v;
    s[0] += fabs(v);
    s[1] = fma(v, v, s[1]);
    s[2] += xv[k];
    big = fmax(big, fabs(v));
  }
  // the profile: thread l < 64 walks line l of the tile (a row for the sources 0 and 1, a column for 2 and 3) in order
  if (threadIdx.x < TRN_T) {
    const int l = threadIdx.x;
    const bool by_row = source < 2;
    const unsigned toward = source == 0 ? TRN_UP : source == 1 ? TRN_DOWN : source == 2 ? TRN_LEFT : TRN_RIGHT;
    const int step = source == 0 ? -TRN_P : source == 1 ? TRN_P : source == 2 ? -1 : 1;
    double cut = 0.0, cs = 0.0, cnt = 0.0, outf = 0.0;
#pragma unroll 1
    for (int m = 0; m < TRN_T; ++m) {
      const int lr = by_row ? l : m, lc = by_row ? m : l;
      const unsigned c = C[lr * TRN_T + lc];
      if (!(c & TRN_ACT)) continue;
      const double* sp = S + (lr + 1) * TRN_P + lc + 1;
      const double v = sp[0];
      cnt += 1.0; cs += v;
      if (c & TRN_SRC) cut += 2.0 * (1.0 - v);
      else if (c & toward) cut += sp[step] - v;
      if (c & TRN_TGT) outf += 2.0 * v;
    }
    double* o = lines + ((size_t)blockIdx.x * TRN_T + l) * TRN_NL;
    o[0] = cut; o[1] = cs; o[2] = cnt; o[3] = outf;
  }
  big = trn_block_max(big, redm);
  trn_block_sum<TRN_NS>(s, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < TRN_NS; ++m) part[(size_t)blockIdx.x * TRN_NS + m] = s[m];
    pmax[blockIdx.x] = big;
  }
}

// one workgroup: the sums over the listed tiles in a fixed order; prof[k][] for k = 0 .. N from the lines of the tiles of
// a tile row (or column) in index order.  F_in is cut[0] and F_out is cut[N].
__global__ __launch_bounds__(TRN_THREADS) void k_trn_fin(const double* __restrict__ part, const double* __restrict__ pmax, int ntl,
                                                         const double* __restrict__ lines, const int* __restrict__ slot, int N, int nt,
                                                         int source, double* __restrict__ prof, TrnOut* __restrict__ out) {
  __shared__ double red[4][TRN_NS], redm[4], redn[4];
  __shared__ double ends[2];
  const bool by_row = source < 2;
  double lo = DBL_MAX, hi = -DBL_MAX;
  for (int k = threadIdx.x; k < N; k += TRN_THREADS) {
    const int a = (source == 0 || source == 2) ? k : N - 1 - k;
    const int tl = a / TRN_T, l = a - tl * TRN_T;
    double v[TRN_NL] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < nt; ++t) {
      const int sl = slot[by_row ? tl * nt + t : t * nt + tl];
      if (sl < 0) continue;
      const double* o = lines + ((size_t)sl * TRN_T + l) * TRN_NL;
#pragma unroll
      for (int m = 0; m < TRN_NL; ++m) v[m] += o[m];
    }
    double* pr = prof + (size_t)k * 3;
    pr[0] = v[0]; pr[1] = v[1]; pr[2] = v[2];
    lo = fmin(lo, v[0]); hi = fmax(hi, v[0]);
    if (k == 0) ends[0] = v[0];
    if (k == N - 1) {
      pr[3] = v[3]; pr[4] = 0.0; pr[5] = 0.0;        // row N
      ends[1] = v[3];
      lo = fmin(lo, v[3]); hi = fmax(hi, v[3]);
    }
  }
  double s[TRN_NS] = {0.0, 0.0, 0.0};
  double big = 0.0;
  for (int b = threadIdx.x; b < ntl; b += TRN_THREADS) {
#pragma unroll
    for (int m = 0; m < TRN_NS; ++m) s[m] += part[(size_t)b * TRN_NS + m];
    big = fmax(big, pmax[b]);
  }
  big = trn_block_max(big, redm);
  hi = trn_block_max(hi, redn);
  __syncthreads();
  lo = -trn_block_max(-lo, redn);
  trn_block_sum<TRN_NS>(s, red);
  if (threadIdx.x == 0) {
    TrnOut o;
    o.fin = ends[0]; o.fout = ends[1]; o.res1 = s[0]; o.resinf = big; o.cutmin = lo; o.cutmax = hi; o.csum = s[2]; o.rr = s[1];
    *out = o;
  }
}

// the true residual takes the place of the recurrence's: r.r is its own, the direction stays
__global__ void k_trn_resume(TrnScal* sc, const TrnOut* out) {
  sc->rr = out->rr;
  sc->done = 0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct TrnResult {   // pinned
  trn_u64 cnt[TRN_NC];
  TrnScal sc;
  TrnOut out;
  int64_t words[CHS_TRN_WORDS];
  double vals[CHS_TRN_VALS];
};

struct TrnBuf : LookBase {   // have: x and prof are the look's snapshot
  int nt = 0;
  trn_byte* code = nullptr;     // [N * N]
  double* x = nullptr;          // [N * N] the map
  double* r = nullptr;          // [N * N]
  double* p[2] = {nullptr, nullptr};   // [N * N] the direction, by the parity of the iteration
  double* q = nullptr;          // [N * N] A p; the true residual of a closing sweep
  unsigned* tflag = nullptr;    // [nt * nt]
  int* list = nullptr;          // [nt * nt] the active tiles in index order
  int* slot = nullptr;          // [nt * nt] a tile's place in the list, -1
  trn_u64* cnt = nullptr;       // [TRN_NC]
  TrnScal* sc = nullptr;
  double* part = nullptr;       // [nt * nt][TRN_NB]
  double* pmax = nullptr;       // [nt * nt]
  double* lines = nullptr;      // [nt * nt][64][TRN_NL]
  double* prof = nullptr;       // [N + 1][3]
  TrnOut* out = nullptr;
  trn_byte* span = nullptr;     // [cap] a component touches both walls
  int64_t cap = 0;
  TrnResult* hRes = nullptr;
  hipEvent_t evs[2] = {nullptr, nullptr};   // around the iterations and the closing sweeps
  double solve_ms = -1.0;
};

void trn_release(TrnBuf* s) {
  if (!s) return;
  hipFree(s->code); hipFree(s->x); hipFree(s->r); hipFree(s->p[0]); hipFree(s->p[1]); hipFree(s->q); hipFree(s->tflag);
  hipFree(s->list); hipFree(s->slot); hipFree(s->cnt); hipFree(s->sc); hipFree(s->part); hipFree(s->pmax); hipFree(s->lines);
  hipFree(s->prof); hipFree(s->out); hipFree(s->span);
  if (s->hRes) hipHostFree(s->hRes);
  for (auto e : s->evs) if (e) hipEventDestroy(e);
  look_release_events(s);
  delete s;
}

int trn_alloc(TrnBuf* s) {
  const size_t n2 = (size_t)s->N * s->N;
  s->nt = (s->N + TRN_T - 1) / TRN_T;
  const size_t ntiles = (size_t)s->nt * s->nt;
  CHS_HIP(hipMalloc(&s->code, n2));
  CHS_HIP(hipMalloc(&s->x, sizeof(double) * n2));
  CHS_HIP(hipMalloc(&s->r, sizeof(double) * n2));
  CHS_HIP(hipMalloc(&s->p[0], sizeof(double) * n2));
  CHS_HIP(hipMalloc(&s->p[1], sizeof(double) * n2));
  CHS_HIP(hipMalloc(&s->q, sizeof(double) * n2));
  CHS_HIP(hipMalloc(&s->tflag, sizeof(unsigned) * ntiles));
  CHS_HIP(hipMalloc(&s->list, sizeof(int) * ntiles));
  CHS_HIP(hipMalloc(&s->slot, sizeof(int) * ntiles));
  CHS_HIP(hipMalloc(&s->cnt, sizeof(trn_u64) * TRN_NC));
  CHS_HIP(hipMalloc(&s->sc, sizeof(TrnScal)));
  CHS_HIP(hipMalloc(&s->part, sizeof(double) * TRN_NB * ntiles));
  CHS_HIP(hipMalloc(&s->pmax, sizeof(double) * ntiles));
  CHS_HIP(hipMalloc(&s->lines, sizeof(double) * TRN_NL * TRN_T * ntiles));
  CHS_HIP(hipMalloc(&s->prof, sizeof(double) * 3 * ((size_t)s->N + 1)));
  CHS_HIP(hipMalloc(&s->out, sizeof(TrnOut)));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(TrnResult), hipHostMallocDefault));
  for (auto& e : s->evs) CHS_HIP(hipEventCreate(&e));
  return CHS_OK;
}

// The phases behind a components look that has just succeeded and left `cc`.
int trn_run(TrnBuf* s, hipStream_t st, const ChsCcSnapshot& cc, const int64_t* ccw, int source, double tol, int64_t limit,
            const std::string& who) {
  const int N = s->N, nt = s->nt, ntiles = nt * nt;
  const size_t n2 = (size_t)N * N;
  const int64_t C = cc.count;
  look_forget(s);
  s->solve_ms = -1.0;
  if (C > s->cap) {   // the flags grow with the component table
    CHS_HIP(hipFree(s->span));
    s->span = nullptr; s->cap = 0;
    const int64_t cap = C + C / 8 + 1024;
    CHS_HIP(hipMalloc(&s->span, (size_t)cap));
    s->cap = cap;
  }
  CHS_HIP(hipMemsetAsync(s->cnt, 0, sizeof(trn_u64) * TRN_NC, st));
  CHS_HIP(hipMemsetAsync(s->prof, 0, sizeof(double) * 3 * ((size_t)N + 1), st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  if (C > 0) {
    k_trn_span<<<(int)((C + TRN_THREADS - 1) / TRN_THREADS), TRN_THREADS, 0, st>>>(cc.table, (int)C, N, source, s->span, s->cnt);
    CHS_HIP(hipGetLastError());
  }
  k_trn_setup<<<ntiles, TRN_THREADS, 0, st>>>(cc.L, cc.id, s->span, (int)C, N, nt, source, s->code, s->x, s->r, s->tflag, s->cnt);
  CHS_HIP(hipGetLastError());
  k_trn_list<<<1, CHS_WAVE, 0, st>>>(s->tflag, ntiles, s->list, s->slot, s->cnt, s->sc, tol);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipMemcpyAsync(s->hRes->cnt, s->cnt, sizeof(trn_u64) * TRN_NC, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  const trn_u64* c = s->hRes->cnt;
  int64_t* w = s->hRes->words;
  double* v = s->hRes->vals;
  memset(w, 0, sizeof(int64_t) * CHS_TRN_WORDS);
  memset(v, 0, sizeof(double) * CHS_TRN_VALS);
  w[CHS_TRN_LIMIT] = limit;
  const int ntl = (int)c[TRN_C_NTL];
  if (c[TRN_C_ERR] || (int64_t)c[TRN_C_FG] != ccw[CHS_CC_AREA] || (c[TRN_C_ACTIVE] == 0) != (c[TRN_C_SPANNING] == 0) ||
      (c[TRN_C_ACTIVE] == 0) != (ntl == 0) || (c[TRN_C_ACTIVE] > 0 && (c[TRN_C_SRC] == 0 || c[TRN_C_TGT] == 0))) {
    chs_set_error(who + ": self-check failed: FG, ACTIVE, CC_SPANNING, SRC_PIXELS, TGT_PIXELS = " + std::to_string(c[TRN_C_FG]) + ", " +
                  std::to_string(c[TRN_C_ACTIVE]) + ", " + std::to_string(c[TRN_C_SPANNING]) + ", " + std::to_string(c[TRN_C_SRC]) + ", " +
                  std::to_string(c[TRN_C_TGT]) + "; the components look has the area " + std::to_string(ccw[CHS_CC_AREA]) +
                  (c[TRN_C_ERR] ? "; a foreground pixel has no component number" : ""));
    return CHS_ECHECK;
  }
  CHS_HIP(hipEventRecord(s->evs[0], st));
  if (ntl > 0) {
    // p and q are 0 off the active set: k_trn_ap reads its halo edges without the pixel's byte, and the first iteration
    // multiplies p by beta = 0.  Every look zeroes them: the pixels that were active in the last look need not be now.
    CHS_HIP(hipMemsetAsync(s->p[0], 0, sizeof(double) * n2, st));
    CHS_HIP(hipMemsetAsync(s->p[1], 0, sizeof(double) * n2, st));
    CHS_HIP(hipMemsetAsync(s->q, 0, sizeof(double) * n2, st));
  }
  int64_t iters = 0, checks = 0;
  bool accepted = ntl == 0;                          // no spanning component: D_eff = 0 is the answer
  const TrnOut& o = s->hRes->out;
  while (!accepted && iters < limit) {
    const int64_t chunk = std::min<int64_t>(TRN_CHUNK, limit - iters);
    for (int64_t k = iters + 1; k <= iters + chunk; ++k) {   // iteration k reads p[(k - 1) & 1] and writes p[k & 1]
      k_trn_ap<<<ntl, TRN_THREADS, 0, st>>>(s->code, s->r, s->p[(k - 1) & 1], s->p[k & 1], s->q, s->list, s->sc, s->part, N, nt);
      CHS_HIP(hipGetLastError());
      k_trn_update<<<ntl, TRN_THREADS, 0, st>>>(s->code, s->x, s->r, s->p[k & 1], s->q, s->list, s->sc, s->part, N, nt);
      CHS_HIP(hipGetLastError());
    }
    CHS_HIP(hipMemcpyAsync(&s->hRes->sc, s->sc, sizeof(TrnScal), hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    iters = s->hRes->sc.iters;                       // the kernels behind `done` returned at once
    if (!s->hRes->sc.done) continue;
    k_trn_close<<<ntl, TRN_THREADS, 0, st>>>(s->code, s->x, s->q, s->list, s->part, s->pmax, s->lines, N, nt, source);
    CHS_HIP(hipGetLastError());
    k_trn_fin<<<1, TRN_THREADS, 0, st>>>(s->part, s->pmax, ntl, s->lines, s->slot, N, nt, source, s->prof, s->out);
    CHS_HIP(hipGetLastError());
    CHS_HIP(hipMemcpyAsync(&s->hRes->out, s->out, sizeof(TrnOut), hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    checks += 1;
    if (!(std::isfinite(o.res1) && std::isfinite(o.fin) && std::isfinite(o.fout))) {
      chs_set_error(who + ": self-check failed: the closing sweep gave RES1, F_IN, F_OUT = " + std::to_string(o.res1) + ", " +
                    std::to_string(o.fin) + ", " + std::to_string(o.fout));
      return CHS_ECHECK;
    }
    if (o.res1 <= tol * std::min(o.fin, o.fout)) { accepted = true; break; }
    // the recurrence passed and the true residual does not: go on from the true one
    CHS_HIP(hipMemcpyAsync(s->r, s->q, sizeof(double) * n2, hipMemcpyDeviceToDevice, st));
    k_trn_resume<<<1, 1, 0, st>>>(s->sc, s->out);
    CHS_HIP(hipGetLastError());
  }
  CHS_HIP(hipEventRecord(s->evs[1], st));
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipStreamSynchronize(st));
  w[CHS_TRN_ITERS] = iters;
  if (!accepted) {
    chs_set_error(who + ": the solve is not accepted after ITERS = " + std::to_string(iters) + " iterations, max_iters = " +
                  std::to_string(limit) + "; there is no transport result (the components look of this call is complete)");
    return CHS_ELIMIT;
  }
  w[CHS_TRN_FG] = (int64_t)c[TRN_C_FG]; w[CHS_TRN_ACTIVE] = (int64_t)c[TRN_C_ACTIVE]; w[CHS_TRN_CC_COUNT] = C;
  w[CHS_TRN_CC_SPANNING] = (int64_t)c[TRN_C_SPANNING]; w[CHS_TRN_SRC_PIXELS] = (int64_t)c[TRN_C_SRC];
  w[CHS_TRN_TGT_PIXELS] = (int64_t)c[TRN_C_TGT]; w[CHS_TRN_BONDS] = (int64_t)c[TRN_C_BONDS]; w[CHS_TRN_CHECKS] = checks;
  if (ntl > 0) {
    v[CHS_TRN_TOL] = tol;
    // the certificate: every cut lies within RES1 of F_out, up to the rounding of the sums
    const double slack = 64.0 * DBL_EPSILON * ((double)c[TRN_C_ACTIVE] + (double)N + 1.0);
    if (!(std::max(o.cutmax - o.fout, o.fout - o.cutmin) <= o.res1 + slack) || !(o.resinf <= o.res1)) {
      chs_set_error(who + ": self-check failed: the cuts span [" + std::to_string(o.cutmin) + ", " + std::to_string(o.cutmax) +
                    "] with RES1 = " + std::to_string(o.res1));
      return CHS_ECHECK;
    }
    v[CHS_TRN_F_IN] = o.fin; v[CHS_TRN_F_OUT] = o.fout; v[CHS_TRN_RES1] = o.res1; v[CHS_TRN_RESINF] = o.resinf;
    v[CHS_TRN_CUT_MIN] = o.cutmin; v[CHS_TRN_CUT_MAX] = o.cutmax; v[CHS_TRN_CSUM] = o.csum;
  }
  float sms = 0.f;
  CHS_HIP(hipEventElapsedTime(&sms, s->evs[0], s->evs[1]));
  int rc;
  if ((rc = look_end(s))) return rc;
  s->solve_ms = sms;
  s->ms += cc.ms;   // the components look inside
  return CHS_OK;
}
}  // namespace

void chs_trn_free(void** buf) {
  if (!buf) return;
  trn_release((TrnBuf*)*buf);
  *buf = nullptr;
}

void chs_trn_forget(void* buf) {
  if (buf) look_forget((TrnBuf*)buf);
}

int chs_trn_look(Engine* E, hipStream_t st, void** ccbuf, void** buf, double threshold, int32_t side, int32_t source, double tol,
                 int64_t max_iters, int64_t* words, double* vals, const char* who_) {
  const std::string who(who_);
  int rc;
  // the order of the components look: arguments, side -- then this look's own, then the field
  if (!vals) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if ((rc = look_check_args(words, threshold, who))) return rc;
  if (side != CHS_CC_BELOW && side != CHS_CC_ABOVE) { chs_set_error(who + ": the side is CHS_CC_BELOW (0) or CHS_CC_ABOVE (1)"); return CHS_EINVAL; }
  if (source < 0 || source > 3) { chs_set_error(who + ": the source is a wall, 0 to 3"); return CHS_EINVAL; }
  if (!(tol >= TRN_TOL_MIN && tol <= TRN_TOL_MAX)) { chs_set_error(who + ": tol is outside [1e-12, 1e-2]"); return CHS_EINVAL; }
  const int64_t def = chs_transport_iters_default(E->N);
  if (max_iters < 0 || max_iters > TRN_MAX_FACTOR * def) {
    chs_set_error(who + ": max_iters = " + std::to_string(max_iters) + " is outside [0, " + std::to_string(TRN_MAX_FACTOR * def) +
                  "] (0: the default, " + std::to_string(def) + ")");
    return CHS_EINVAL;
  }
  if (max_iters == 0) max_iters = def;
  int64_t ccw[CHS_CC_WORDS];
  if ((rc = chs_cc_look(E, st, ccbuf, threshold, 4, side, ccw, who_))) return rc;
  if ((rc = look_buffers<TrnBuf>(buf, E->N, trn_alloc, trn_release))) return rc;
  TrnBuf* s = (TrnBuf*)*buf;
  ChsCcSnapshot cc;
  if ((rc = chs_cc_snapshot(*ccbuf, &cc, who_))) return rc;
  rc = trn_run(s, st, cc, ccw, source, tol, max_iters, who);
  if (rc == CHS_OK || rc == CHS_ELIMIT) {   // refused: ITERS and LIMIT
    memcpy(words, s->hRes->words, sizeof(int64_t) * CHS_TRN_WORDS);
    memcpy(vals, s->hRes->vals, sizeof(double) * CHS_TRN_VALS);
  }
  return rc;
}

int chs_trn_profile(void* buf, int device, hipStream_t st, double* out, const char* who_) {
  const std::string who(who_);
  const TrnBuf* s = (const TrnBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->prof, sizeof(double) * 3 * ((size_t)s->N + 1));
}

int chs_trn_map(void* buf, int device, hipStream_t st, double* out, const char* who_) {
  const std::string who(who_);
  const TrnBuf* s = (const TrnBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  return look_fetch(device, st, out, s->x, sizeof(double) * (size_t)s->N * s->N);
}

int chs_trn_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const TrnBuf*)buf, ms, what);
}

int chs_trn_solve_ms(const void* h, const void* buf, double* ms, const char* what) {
  const std::string who = std::string(what) + "_solve_ms";
  const TrnBuf* s = (const TrnBuf*)buf;
  if (!h || !ms) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (!s || !s->have || s->solve_ms < 0.0) { chs_set_error(who + ": no " + what + " call so far"); return CHS_ESTATE; }
  *ms = s->solve_ms;
  return CHS_OK;
}

extern "C" int64_t chs_transport_iters_default(int32_t N) { return N < 1 ? 0 : TRN_FACTOR * (int64_t)N + TRN_SLACK; }

extern "C" int chs_transport(chs_handle h, double threshold, int32_t side, int32_t source, double tol, int64_t max_iters,
                             int64_t words[CHS_TRN_WORDS], double vals[CHS_TRN_VALS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_transport: null handle"); return CHS_EINVAL; }
  return chs_trn_look(E, E->stream, &E->cc, &E->trn, threshold, side, source, tol, max_iters, words, vals, "chs_transport");
}

extern "C" int chs_transport_profile(chs_handle h, double* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_transport_profile: null handle"); return CHS_EINVAL; }
  return chs_trn_profile(E->trn, E->hc.device, E->stream, out, "chs_transport_profile");
}

extern "C" int chs_transport_map(chs_handle h, double* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_transport_map: null handle"); return CHS_EINVAL; }
  return chs_trn_map(E->trn, E->hc.device, E->stream, out, "chs_transport_map");
}

extern "C" int chs_transport_last_ms(chs_handle h, double* ms) {
  return chs_trn_last_ms(h, h ? ((Engine*)h)->trn : nullptr, ms, "chs_transport");
}

extern "C" int chs_transport_solve_ms(chs_handle h, double* ms) {
  return chs_trn_solve_ms(h, h ? ((Engine*)h)->trn : nullptr, ms, "chs_transport");
}
