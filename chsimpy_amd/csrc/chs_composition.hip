// chs_composition.hip -- the values of the field themselves on the device: range, sums, histogram, central moments and
// exact order statistics (the definition: include/chs_hip.h, chs_composition).
//
// Phases that depend on each other are separate launches: no workgroup ever waits for another one, nothing is polled.
// Every sweep walks the field the same way: a tile is CMP_THREADS * CMP_EPT consecutive elements, workgroup g takes the
// tiles g, g + groups, ... (groups = min(tiles, CMP_MAX_GROUPS)), and within a tile thread t loads the CMP_EPT / V
// vectors (k CMP_THREADS + t) V -- all of them before it looks at one -- and handles them k-major, element-minor.  That
// is the fixed order of a thread's sums.
//   composition
//   1  k_cmp_range   sweep A: min, max, sum, sum below the threshold, counts of NaN, infinite, below.  A workgroup
//                    reduces its threads' numbers by a fixed tree and stores them into slot g.
//   2  k_cmp_fin_a   one workgroup reduces the slots by a fixed tree and writes what sweep B needs: centre, lo, hi, scale.
//   3  k_cmp_hist    sweep B: the histogram and the sums of (x - centre)^p.  Bins go through cmp_wave_add into the
//                    workgroup's LDS histogram, which is flushed by integer atomicAdd; the sums into slot g as in 1.
//   4  k_cmp_fin_b   one workgroup reduces those slots and adds up the histogram for the look's check.
//   select
//   1  k_cmp_digits  one sweep per digit of the order-preserving key, most significant first: a pixel whose key begins
//                    with the prefix a rank has so far adds 1 to that prefix's table of digit counts, in LDS, flushed by
//                    integer atomicAdd.  Ranks that share a prefix share a table (in the first pass all of them do).
//   2  k_cmp_scan    one workgroup, a wavefront per rank: the digit in which the rank falls, the rank within it, the new
//                    prefix; then the distinct prefixes for the next sweep, and the tables cleared.
// cmp_wave_add is where a constant or phase-separated field would otherwise pile every lane onto one LDS address: the
// wavefront peels off CMP_ROUNDS groups of lanes that agree with the first remaining lane -- one lane adds the
// popcount -- and only what is left adds lane by lane.
// Nothing of the handle is written and nothing the step loop owns is read: its field alone.
#include <cmath>
#include <cstring>
#include <limits>

#include "chs_look.h"

#define CMP_THREADS 256                     // the sweeps
#define CMP_EPT 16                          // elements of a tile per thread
#define CMP_MAX_GROUPS 2048                 // workgroups of a sweep at most: the slots
#define CMP_FIN_THREADS 1024                // k_cmp_fin_a, k_cmp_fin_b: one workgroup, two slots a thread
#define CMP_DIGIT_BITS 11
#define CMP_DIGITS (1 << CMP_DIGIT_BITS)
#define CMP_ROUNDS 2                        // groups of agreeing lanes a wavefront peels off before it adds lane by lane
#define CMP_SCAN_THREADS (CHS_CMP_MAX_RANKS * CHS_WAVE)
#define CMP_MAX_N 16384                     // N of chs_create at most: N^2 <= 2^28, a workgroup's counts fit 32 bits
// slots of sweep A and of sweep B
#define CMP_PA_MIN 0
#define CMP_PA_MAX 1
#define CMP_PA_SUM 2
#define CMP_PA_SUMB 3
#define CMP_PF 4                            // doubles of a slot
#define CMP_PI 3                            // int64 of a slot of sweep A: NaN, infinite, below
// the words the kernels leave beside iw and fw
#define CMP_X_HSUM 0                        // the histogram added up
#define CMP_NX 1
#define CMP_ERR_SCAN 1                      // k_cmp_scan: a rank fell into no digit

static_assert(CMP_THREADS % CHS_WAVE == 0 && CMP_FIN_THREADS % CHS_WAVE == 0, "whole wavefronts");
static_assert(CMP_MAX_GROUPS == 2 * CMP_FIN_THREADS, "two slots a thread of the finishing workgroup");
static_assert(CMP_THREADS == 1 << 8 && CMP_MAX_GROUPS == 1 << 11, "the trees above a thread's sum are 8 + 11 deep (cmp_run)");
static_assert(CMP_EPT % 4 == 0, "whole 16-byte vectors of either type");
static_assert(CMP_DIGITS % CHS_WAVE == 0, "a lane of k_cmp_scan owns whole digits");
static_assert((size_t)CHS_CMP_MAX_RANKS * CMP_DIGITS * sizeof(unsigned) <= 65536, "the tables of all ranks fit 64 KB of LDS");
static_assert(CHS_CMP_MAX_BINS * sizeof(unsigned) <= 65536, "the histogram fits LDS");

typedef long long cmp_i64;
typedef unsigned long long cmp_u64;
static_assert(sizeof(cmp_i64) == sizeof(int64_t), "the result words are int64");

// ---- what the kernels share -------------------------------------------------------------------------------------------
enum { CMP_OP_SUM, CMP_OP_MIN, CMP_OP_MAX };
template <int OP, typename X>
__device__ __forceinline__ X cmp_op(X a, X b) {
  if constexpr (OP == CMP_OP_SUM) return a + b;
  else if constexpr (OP == CMP_OP_MIN) return b < a ? b : a;
  else return b > a ? b : a;
}

// The workgroup's v joined by a fixed tree, log2(64 NW) deep: shuffles inside the wavefront, the NW wavefronts' results
// through red[NW], shuffles over those in the first wavefront.  Thread 0 has the result.
template <int OP, int NW, typename X>
__device__ __forceinline__ X cmp_block(X v, X* red) {
#pragma unroll
  for (int off = CHS_WAVE / 2; off > 0; off >>= 1) v = cmp_op<OP>(v, __shfl_down(v, off));
  const int lane = threadIdx.x % CHS_WAVE, w = threadIdx.x / CHS_WAVE;
  __syncthreads();   // (red is free again)
  if (lane == 0) red[w] = v;
  __syncthreads();
  if (w == 0) {
    v = red[lane < NW ? lane : 0];
#pragma unroll
    for (int off = NW / 2; off > 0; off >>= 1) v = cmp_op<OP>(v, __shfl_down(v, off));   // (lane 0 reaches lanes < NW only)
  }
  return v;
}

// lh[key] += 1 for every lane with `valid`, all lanes of the wavefront being here.  CMP_ROUNDS times the lanes that have
// the first remaining lane's key leave together, that lane adding their number; the others add one by one.
__device__ __forceinline__ void cmp_wave_add(unsigned* lh, int key, bool valid) {
  const int lane = threadIdx.x % CHS_WAVE;
  cmp_u64 rest = __ballot(valid);
#pragma unroll
  for (int r = 0; r < CMP_ROUNDS; ++r) {
    if (rest == 0) break;   // (the same in every lane)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((cmp_i64)rest) - 1);
    const int lk = __builtin_amdgcn_readlane(key, leader);
    const cmp_u64 m = __ballot(valid && key == lk) & rest;
    if (lane == leader) atomicAdd(&lh[lk], (unsigned)__popcll(m));
    rest &= ~m;
  }
  if ((rest >> lane) & 1) atomicAdd(&lh[key], 1u);
}

// the tile `tile` of the field of `total` elements: x[k][e] of this thread, ok[k]: inside the field
template <typename T, int V, bool NT>
__device__ __forceinline__ void cmp_load_tile(const T CHS_GLOBAL* U, size_t total, size_t tile, T (&x)[CMP_EPT / V][V],
                                              bool (&ok)[CMP_EPT / V]) {
  const size_t base = tile * (size_t)(CMP_THREADS * CMP_EPT);
#pragma unroll
  for (int k = 0; k < CMP_EPT / V; ++k) {
    const size_t i = base + ((size_t)k * CMP_THREADS + threadIdx.x) * V;   // (total is a multiple of V)
    ok[k] = i < total;
    chs_load<T, V, NT>(U + (ok[k] ? i : 0), x[k]);
  }
}

// the order-preserving key of a value: the bits of a non-negative number with the sign bit set, those of a negative one
// inverted, all ones for a NaN of either sign
__device__ __forceinline__ cmp_u64 cmp_key(double x) {
  const cmp_u64 b = (cmp_u64)__double_as_longlong(x);
  return x != x ? ~(cmp_u64)0 : (b >> 63 ? ~b : b | ((cmp_u64)1 << 63));
}
__device__ __forceinline__ unsigned cmp_key(float x) {
  const unsigned b = __float_as_uint(x);
  return x != x ? ~0u : (b >> 31 ? ~b : b | (1u << 31));
}
template <typename T> struct CmpKey;
template <> struct CmpKey<double> { typedef cmp_u64 type; static constexpr int BITS = 64; };
template <> struct CmpKey<float> { typedef unsigned type; static constexpr int BITS = 32; };

// ---- composition: sweep A ---------------------------------------------------------------------------------------------
template <typename T, int V, bool NT>
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_range(const void* Uv, cmp_i64 total_, int tiles, double t,
                                                           double* __restrict__ pf, cmp_i64* __restrict__ pi) {
  constexpr int NW = CMP_THREADS / CHS_WAVE;
  __shared__ double redf[NW];
  __shared__ cmp_i64 redi[NW];
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const size_t total = (size_t)total_;
  const double inf = __builtin_inf();
  double mn = inf, mx = -inf, sum = 0.0, sumb = 0.0;
  unsigned nnan = 0, ninf = 0, nbelow = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    T x[CMP_EPT / V][V];
    bool ok[CMP_EPT / V];
    cmp_load_tile<T, V, NT>(U, total, (size_t)tile, x, ok);
#pragma unroll
    for (int k = 0; k < CMP_EPT / V; ++k) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double v = (double)x[k][e];
        const bool nan = v != v, fin = ok[k] && fabs(v) < inf, below = ok[k] && v < t;
        nnan += ok[k] && nan;
        ninf += ok[k] && !nan && !(fabs(v) < inf);
        nbelow += below;
        mn = fin && v < mn ? v : mn;
        mx = fin && v > mx ? v : mx;
        sum += fin ? v : 0.0;
        sumb += fin && below ? v : 0.0;
      }
    }
  }
  mn = cmp_block<CMP_OP_MIN, NW>(mn, redf);
  mx = cmp_block<CMP_OP_MAX, NW>(mx, redf);
  sum = cmp_block<CMP_OP_SUM, NW>(sum, redf);
  sumb = cmp_block<CMP_OP_SUM, NW>(sumb, redf);
  const cmp_i64 cn = cmp_block<CMP_OP_SUM, NW>((cmp_i64)nnan, redi), ci = cmp_block<CMP_OP_SUM, NW>((cmp_i64)ninf, redi),
                cb = cmp_block<CMP_OP_SUM, NW>((cmp_i64)nbelow, redi);
  if (threadIdx.x == 0) {
    double* f = pf + (size_t)blockIdx.x * CMP_PF;
    f[CMP_PA_MIN] = mn; f[CMP_PA_MAX] = mx; f[CMP_PA_SUM] = sum; f[CMP_PA_SUMB] = sumb;
    cmp_i64* c = pi + (size_t)blockIdx.x * CMP_PI;
    c[0] = cn; c[1] = ci; c[2] = cb;
  }
}

// the slots s and s + CMP_FIN_THREADS of this thread joined (a slot past `groups` is the identity), then the tree
template <int OP, typename X>
__device__ __forceinline__ X cmp_fin(const X* __restrict__ p, int stride, int groups, X id, X* red) {
  const int a = threadIdx.x, b = threadIdx.x + CMP_FIN_THREADS;
  const X va = a < groups ? p[(size_t)a * stride] : id, vb = b < groups ? p[(size_t)b * stride] : id;
  return cmp_block<OP, CMP_FIN_THREADS / CHS_WAVE>(cmp_op<OP>(va, vb), red);
}

__global__ __launch_bounds__(CMP_FIN_THREADS) void k_cmp_fin_a(const double* __restrict__ pf, const cmp_i64* __restrict__ pi,
                                                               int groups, cmp_i64 total, int nbins, int own_range, double lo,
                                                               double hi, cmp_i64* __restrict__ iw, double* __restrict__ fw) {
  __shared__ double redf[CMP_FIN_THREADS / CHS_WAVE];
  __shared__ cmp_i64 redi[CMP_FIN_THREADS / CHS_WAVE];
  const double inf = __builtin_inf();
  double mn = cmp_fin<CMP_OP_MIN>(pf + CMP_PA_MIN, CMP_PF, groups, inf, redf);
  double mx = cmp_fin<CMP_OP_MAX>(pf + CMP_PA_MAX, CMP_PF, groups, -inf, redf);
  const double sum = cmp_fin<CMP_OP_SUM>(pf + CMP_PA_SUM, CMP_PF, groups, 0.0, redf);
  const double sumb = cmp_fin<CMP_OP_SUM>(pf + CMP_PA_SUMB, CMP_PF, groups, 0.0, redf);
  const cmp_i64 nnan = cmp_fin<CMP_OP_SUM>(pi + 0, CMP_PI, groups, (cmp_i64)0, redi);
  const cmp_i64 ninf = cmp_fin<CMP_OP_SUM>(pi + 1, CMP_PI, groups, (cmp_i64)0, redi);
  const cmp_i64 nbelow = cmp_fin<CMP_OP_SUM>(pi + 2, CMP_PI, groups, (cmp_i64)0, redi);
  if (threadIdx.x == 0) {
    const cmp_i64 nfin = total - nnan - ninf;
    const double nan = __builtin_nan("");
    if (nfin == 0) mn = mx = nan;
    if (own_range) { lo = mn; hi = mx; }
    iw[CHS_CMP_N_TOTAL] = total; iw[CHS_CMP_N_NAN] = nnan; iw[CHS_CMP_N_INF] = ninf; iw[CHS_CMP_N_BELOW] = nbelow;
    iw[CHS_CMP_NBINS] = nbins;
    fw[CHS_CMP_MIN] = mn; fw[CHS_CMP_MAX] = mx; fw[CHS_CMP_SUM] = sum; fw[CHS_CMP_SUM_BELOW] = sumb;
    // the mean of the finite pixels lies in [min, max]; the rounded quotient of the rounded sum may lie an ulp outside (a
    // constant field): it is brought back, which moves it towards the mean
    const double q = sum / (double)nfin;
    fw[CHS_CMP_CENTER] = nfin ? (q < mn ? mn : q > mx ? mx : q) : nan;
    fw[CHS_CMP_LO] = lo; fw[CHS_CMP_HI] = hi;
    fw[CHS_CMP_SCALE] = hi > lo ? (double)nbins / (hi - lo) : 0.0;   // (0 for hi == lo and for a range of NaN)
  }
}

// ---- composition: sweep B ---------------------------------------------------------------------------------------------
// pf: slots of CMP_PF doubles (M2, M3, M4); cnt: under, over
template <typename T, int V, bool NT>
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_hist(const void* Uv, cmp_i64 total_, int tiles, int nbins,
                                                          const double* __restrict__ fw, double* __restrict__ pf,
                                                          cmp_u64* __restrict__ hist, cmp_u64* __restrict__ cnt) {
  constexpr int NW = CMP_THREADS / CHS_WAVE;
  __shared__ unsigned lh[CHS_CMP_MAX_BINS];
  __shared__ double redf[NW];
  __shared__ cmp_i64 redi[NW];
  for (int i = threadIdx.x; i < nbins; i += CMP_THREADS) lh[i] = 0;
  __syncthreads();
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const size_t total = (size_t)total_;
  const double inf = __builtin_inf();
  const double c = fw[CHS_CMP_CENTER], lo = fw[CHS_CMP_LO], hi = fw[CHS_CMP_HI], scale = fw[CHS_CMP_SCALE];
  double s2 = 0.0, s3 = 0.0, s4 = 0.0;
  unsigned under = 0, over = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    T x[CMP_EPT / V][V];
    bool ok[CMP_EPT / V];
    cmp_load_tile<T, V, NT>(U, total, (size_t)tile, x, ok);
#pragma unroll
    for (int k = 0; k < CMP_EPT / V; ++k) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double v = (double)x[k][e];
        const bool fin = ok[k] && fabs(v) < inf;
        const double d = fin ? v - c : 0.0, d2 = d * d;
        s2 += d2; s3 += d2 * d; s4 += d2 * d2;
        under += ok[k] && (v < lo || v == -inf);
        over += ok[k] && (v > hi || v == inf);
        const bool in = fin && v >= lo && v <= hi;
        const double p = (v - lo) * scale;   // a subtraction, then a multiplication: nothing to contract
        const int b = p >= 0.0 && p < (double)nbins ? (int)p : nbins - 1;
        cmp_wave_add(lh, in ? b : 0, in);
      }
    }
  }
  s2 = cmp_block<CMP_OP_SUM, NW>(s2, redf);
  s3 = cmp_block<CMP_OP_SUM, NW>(s3, redf);
  s4 = cmp_block<CMP_OP_SUM, NW>(s4, redf);
  const cmp_i64 cu = cmp_block<CMP_OP_SUM, NW>((cmp_i64)under, redi), co = cmp_block<CMP_OP_SUM, NW>((cmp_i64)over, redi);
  if (threadIdx.x == 0) {
    double* f = pf + (size_t)blockIdx.x * CMP_PF;
    f[0] = s2; f[1] = s3; f[2] = s4;
    if (cu) atomicAdd(&cnt[0], (cmp_u64)cu);
    if (co) atomicAdd(&cnt[1], (cmp_u64)co);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += CMP_THREADS) {
    const unsigned n = lh[i];
    if (n) atomicAdd(&hist[i], (cmp_u64)n);
  }
}

__global__ __launch_bounds__(CMP_FIN_THREADS) void k_cmp_fin_b(const double* __restrict__ pf, int groups, int nbins,
                                                               const cmp_u64* __restrict__ hist, const cmp_u64* __restrict__ cnt,
                                                               cmp_i64* __restrict__ iw, double* __restrict__ fw,
                                                               cmp_i64* __restrict__ xw) {
  __shared__ double redf[CMP_FIN_THREADS / CHS_WAVE];
  __shared__ cmp_i64 redi[CMP_FIN_THREADS / CHS_WAVE];
  const double m2 = cmp_fin<CMP_OP_SUM>(pf + 0, CMP_PF, groups, 0.0, redf);
  const double m3 = cmp_fin<CMP_OP_SUM>(pf + 1, CMP_PF, groups, 0.0, redf);
  const double m4 = cmp_fin<CMP_OP_SUM>(pf + 2, CMP_PF, groups, 0.0, redf);
  cmp_i64 h = 0;
  for (int i = threadIdx.x; i < nbins; i += CMP_FIN_THREADS) h += (cmp_i64)hist[i];
  h = cmp_block<CMP_OP_SUM, CMP_FIN_THREADS / CHS_WAVE>(h, redi);
  if (threadIdx.x == 0) {
    fw[CHS_CMP_M2] = m2; fw[CHS_CMP_M3] = m3; fw[CHS_CMP_M4] = m4;
    iw[CHS_CMP_N_UNDER] = (cmp_i64)cnt[0]; iw[CHS_CMP_N_OVER] = (cmp_i64)cnt[1];
    xw[CMP_X_HSUM] = h;
  }
}

// ---- select -----------------------------------------------------------------------------------------------------------
// What the passes hand on, on the device.  prefix[q]: the digits of rank q's key found so far; rem[q]: its rank among the
// keys with that prefix; equal[q]: the count of its last digit (after the last pass: of the keys equal to the one found);
// slot[q]: the table of its prefix; nuniq tables, uprefix[u] the prefix of table u.
struct CmpSel {
  cmp_u64 prefix[CHS_CMP_MAX_RANKS], uprefix[CHS_CMP_MAX_RANKS];
  cmp_i64 rem[CHS_CMP_MAX_RANKS], equal[CHS_CMP_MAX_RANKS];
  int slot[CHS_CMP_MAX_RANKS];
  int nuniq, err;
};

// Pass `pass` looks at the `width` bits above bit `shift` of the key; the bits above those are the prefix (pass 0: none,
// every pixel counts).  tables: [CHS_CMP_MAX_RANKS][CMP_DIGITS]; LDS: nq tables.
template <typename T, int V, bool NT>
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_digits(const void* Uv, cmp_i64 total_, int tiles, int pass, int shift,
                                                            int width, int nq, const CmpSel* __restrict__ sel,
                                                            cmp_u64* __restrict__ tables) {
  typedef typename CmpKey<T>::type K;
  extern __shared__ __attribute__((aligned(16))) unsigned cmp_lds[];
  const int nuniq = __builtin_amdgcn_readfirstlane(sel->nuniq), nu = nuniq < nq ? nuniq : nq;   // (the launch has LDS for nq tables)
  for (int i = threadIdx.x; i < nu * CMP_DIGITS; i += CMP_THREADS) cmp_lds[i] = 0;
  __syncthreads();
  const T CHS_GLOBAL* U = (const T CHS_GLOBAL*)Uv;
  const size_t total = (size_t)total_;
  const K mask = (K)((1u << width) - 1);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    T x[CMP_EPT / V][V];
    bool ok[CMP_EPT / V];
    cmp_load_tile<T, V, NT>(U, total, (size_t)tile, x, ok);
    K key[CMP_EPT / V][V];
#pragma unroll
    for (int k = 0; k < CMP_EPT / V; ++k) {
#pragma unroll
      for (int e = 0; e < V; ++e) key[k][e] = cmp_key(x[k][e]);
    }
    // the tables one after the other (a loop, not unrolled: the tile's 16 adds once in the code), the tile's keys in registers
#pragma unroll 1
    for (int u = 0; u < nu; ++u) {
      const K up = (K)sel->uprefix[u];   // (the same in every lane: a scalar load)
      unsigned* lh = cmp_lds + u * CMP_DIGITS;
#pragma unroll
      for (int k = 0; k < CMP_EPT / V; ++k) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int digit = (int)((key[k][e] >> shift) & mask);
          const K head = pass ? (K)(key[k][e] >> (shift + width)) : (K)0;   // (pass 0 has shift + width = the key's bits)
          cmp_wave_add(lh, digit, ok[k] && (pass == 0 || head == up));
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nu * CMP_DIGITS; i += CMP_THREADS) {
    const unsigned n = cmp_lds[i];
    if (n) atomicAdd(&tables[i], (cmp_u64)n);
  }
}

// One workgroup, wavefront q for rank q.  A lane owns CMP_DIGITS / 64 consecutive digits of the rank's table.
__global__ __launch_bounds__(CMP_SCAN_THREADS) void k_cmp_scan(int nq, int width, CmpSel* sel, cmp_u64* tables) {
  constexpr int PER = CMP_DIGITS / CHS_WAVE;
  const int lane = threadIdx.x % CHS_WAVE, q = threadIdx.x / CHS_WAVE;
  const int ndig = 1 << width;
  if (q < nq) {
    const cmp_u64* tb = tables + (size_t)sel->slot[q] * CMP_DIGITS;
    const cmp_i64 rem = sel->rem[q];
    cmp_i64 c[PER], own = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int d = lane * PER + j;
      c[j] = d < ndig ? (cmp_i64)tb[d] : 0;
      own += c[j];
    }
    cmp_i64 incl = own;   // the digits of this lane and of the lanes before it
#pragma unroll
    for (int off = 1; off < CHS_WAVE; off <<= 1) {
      const cmp_i64 o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    cmp_i64 before = incl - own;
    const bool mine = before <= rem && rem < incl;   // one lane at the most
    if (mine) {
      int d = lane * PER;
#pragma unroll
      for (int j = 0; j < PER - 1; ++j) {
        if (before + c[j] <= rem && d == lane * PER + j) { before += c[j]; ++d; }
      }
      sel->prefix[q] = (sel->prefix[q] << width) | (cmp_u64)d;
      sel->rem[q] = rem - before;
      sel->equal[q] = (cmp_i64)tb[d];
    }
    if (__ballot(mine) == 0 && lane == 0) atomicOr(&sel->err, CMP_ERR_SCAN);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CHS_CMP_MAX_RANKS * CMP_DIGITS; i += CMP_SCAN_THREADS) tables[i] = 0;
  if (threadIdx.x == 0) {   // the distinct prefixes, in the order of their first rank
    int nu = 0;
    for (int a = 0; a < nq; ++a) {
      int u = 0;
      while (u < nu && sel->uprefix[u] != sel->prefix[a]) ++u;
      if (u == nu) sel->uprefix[nu++] = sel->prefix[a];
      sel->slot[a] = u;
    }
    sel->nuniq = nu;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct CmpResult {   // pinned
  cmp_i64 iw[CHS_CMP_IWORDS];
  double fw[CHS_CMP_FWORDS];
  cmp_i64 xw[CMP_NX];
  CmpSel sel;
};

struct CmpBuf : LookBase {   // have: hist is the snapshot of the last chs_composition, nbins its length
  int nbins = 0;
  double* pf = nullptr;         // [CMP_MAX_GROUPS][CMP_PF]: the slots of the sweep that runs
  cmp_i64* pi = nullptr;        // [CMP_MAX_GROUPS][CMP_PI]
  cmp_u64* hist = nullptr;      // [CHS_CMP_MAX_BINS]
  cmp_u64* cnt = nullptr;       // [2]: under, over
  cmp_i64* iw = nullptr;        // [CHS_CMP_IWORDS]
  double* fw = nullptr;         // [CHS_CMP_FWORDS]
  cmp_i64* xw = nullptr;        // [CMP_NX]
  cmp_u64* tables = nullptr;    // [CHS_CMP_MAX_RANKS][CMP_DIGITS] of the select
  CmpSel* sel = nullptr;
  CmpResult* hRes = nullptr;
};

void cmp_release(CmpBuf* s) {
  if (!s) return;
  hipFree(s->pf); hipFree(s->pi); hipFree(s->hist); hipFree(s->cnt); hipFree(s->iw); hipFree(s->fw); hipFree(s->xw);
  hipFree(s->tables); hipFree(s->sel);
  if (s->hRes) hipHostFree(s->hRes);
  look_release_events(s);
  delete s;
}

int cmp_alloc(CmpBuf* s) {
  CHS_HIP(hipMalloc(&s->pf, sizeof(double) * CMP_MAX_GROUPS * CMP_PF));
  CHS_HIP(hipMalloc(&s->pi, sizeof(cmp_i64) * CMP_MAX_GROUPS * CMP_PI));
  CHS_HIP(hipMalloc(&s->hist, sizeof(cmp_u64) * CHS_CMP_MAX_BINS));
  CHS_HIP(hipMalloc(&s->cnt, sizeof(cmp_u64) * 2));
  CHS_HIP(hipMalloc(&s->iw, sizeof(cmp_i64) * CHS_CMP_IWORDS));
  CHS_HIP(hipMalloc(&s->fw, sizeof(double) * CHS_CMP_FWORDS));
  CHS_HIP(hipMalloc(&s->xw, sizeof(cmp_i64) * CMP_NX));
  CHS_HIP(hipMalloc(&s->tables, sizeof(cmp_u64) * CHS_CMP_MAX_RANKS * CMP_DIGITS));
  CHS_HIP(hipMalloc(&s->sel, sizeof(CmpSel)));
  CHS_HIP(hipHostMalloc((void**)&s->hRes, sizeof(CmpResult), hipHostMallocDefault));
  return CHS_OK;
}

struct CmpGrid {
  cmp_i64 total;
  int tiles, groups;
};

CmpGrid cmp_grid(int N) {
  CmpGrid g;
  g.total = (cmp_i64)N * N;
  g.tiles = (int)((g.total + CMP_THREADS * CMP_EPT - 1) / (CMP_THREADS * CMP_EPT));
  g.groups = g.tiles < CMP_MAX_GROUPS ? g.tiles : CMP_MAX_GROUPS;
  return g;
}

// A sweep in the instantiation the field asks for: 16-byte loads where N is a multiple of the vector, element loads
// otherwise; non-temporal where the step loop's arrays fill the Infinity Cache (a read-once sweep must not displace them).
// kernel: 0 k_cmp_range, 1 k_cmp_hist, 2 k_cmp_digits
struct CmpSweep {
  int kernel;
  double t;                     // 0
  int nbins;                    // 1
  int pass, shift, width, nq;   // 2
};

template <typename T, int V, bool NT>
int cmp_launch(const CmpBuf* s, const void* U, const CmpSweep& w, hipStream_t st) {
  const CmpGrid g = cmp_grid(s->N);
  if (w.kernel == 0) k_cmp_range<T, V, NT><<<g.groups, CMP_THREADS, 0, st>>>(U, g.total, g.tiles, w.t, s->pf, s->pi);
  else if (w.kernel == 1) k_cmp_hist<T, V, NT><<<g.groups, CMP_THREADS, 0, st>>>(U, g.total, g.tiles, w.nbins, s->fw, s->pf, s->hist, s->cnt);
  else k_cmp_digits<T, V, NT><<<g.groups, CMP_THREADS, sizeof(unsigned) * CMP_DIGITS * (size_t)w.nq, st>>>(
      U, g.total, g.tiles, w.pass, w.shift, w.width, w.nq, s->sel, s->tables);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

template <typename T>
int cmp_sweep(const CmpBuf* s, const void* U, const CmpSweep& w, hipStream_t st) {
  constexpr int V = ChsVec<T>::V;
  const bool nt = chs_grid_exceeds_cache((size_t)s->N, sizeof(T));
  if (s->N % V == 0) return nt ? cmp_launch<T, V, true>(s, U, w, st) : cmp_launch<T, V, false>(s, U, w, st);
  return nt ? cmp_launch<T, 1, true>(s, U, w, st) : cmp_launch<T, 1, false>(s, U, w, st);
}

int cmp_sweep(const CmpBuf* s, const Engine* E, const CmpSweep& w, hipStream_t st) {
  return E->dtype == CHS_F64 ? cmp_sweep<double>(s, E->dU, w, st) : cmp_sweep<float>(s, E->dU, w, st);
}

int cmp_run(CmpBuf* s, Engine* E, hipStream_t st, double t, int nbins, bool own_range, double lo, double hi, const std::string& who) {
  const CmpGrid g = cmp_grid(s->N);
  look_forget(s);
  s->nbins = nbins;
  CHS_HIP(hipMemsetAsync(s->hist, 0, sizeof(cmp_u64) * (size_t)nbins, st));
  CHS_HIP(hipMemsetAsync(s->cnt, 0, sizeof(cmp_u64) * 2, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  int rc;
  CmpSweep w{};
  w.kernel = 0; w.t = t;
  if ((rc = cmp_sweep(s, E, w, st))) return rc;
  k_cmp_fin_a<<<1, CMP_FIN_THREADS, 0, st>>>(s->pf, s->pi, g.groups, g.total, nbins, own_range ? 1 : 0, lo, hi, s->iw, s->fw);
  CHS_HIP(hipGetLastError());
  w.kernel = 1; w.nbins = nbins;
  if ((rc = cmp_sweep(s, E, w, st))) return rc;
  k_cmp_fin_b<<<1, CMP_FIN_THREADS, 0, st>>>(s->pf, g.groups, nbins, s->hist, s->cnt, s->iw, s->fw, s->xw);
  CHS_HIP(hipGetLastError());
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CmpResult* r = s->hRes;
  CHS_HIP(hipMemcpyAsync(r->iw, s->iw, sizeof(cmp_i64) * CHS_CMP_IWORDS, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(r->fw, s->fw, sizeof(double) * CHS_CMP_FWORDS, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipMemcpyAsync(r->xw, s->xw, sizeof(cmp_i64) * CMP_NX, hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  std::string m;
  const cmp_i64 nfin = r->iw[CHS_CMP_N_TOTAL] - r->iw[CHS_CMP_N_NAN] - r->iw[CHS_CMP_N_INF];
  if (r->xw[CMP_X_HSUM] + r->iw[CHS_CMP_N_UNDER] + r->iw[CHS_CMP_N_OVER] + r->iw[CHS_CMP_N_NAN] != g.total)
    m += " the histogram, the pixels under and over it and the NaN pixels do not add up to N^2;";
  if (r->iw[CHS_CMP_N_BELOW] < 0 || r->iw[CHS_CMP_N_BELOW] > g.total || nfin < 0) m += " more pixels below the threshold, or NaN and infinite, than N^2;";
  if (nfin > 0 && std::isfinite(r->fw[CHS_CMP_SUM])) {   // (a sum that overflowed has no mean to check)
    // SUM / nfin before k_cmp_fin_a brought it into [min, max]: outside by no more than the error bound of SUM allows
    // (E + D + 3 roundings of 2^-53 on a mean of absolute values that is max(|min|, |max|) at the most)
    const double q = r->fw[CHS_CMP_SUM] / (double)nfin, mn = r->fw[CHS_CMP_MIN], mx = r->fw[CHS_CMP_MAX];
    const double E = (double)CMP_EPT * (double)((g.tiles + g.groups - 1) / g.groups), D = 8 + 11;
    const double slack = (E + D + 3.0) * 0x1p-53 * std::fmax(std::fabs(mn), std::fabs(mx));
    if (!(mn - slack <= q && q <= mx + slack) || !(mn <= r->fw[CHS_CMP_CENTER] && r->fw[CHS_CMP_CENTER] <= mx))
      m += " the mean is not between min and max;";
  }
  if (!m.empty()) { chs_set_error(who + ": self-check failed:" + m); return CHS_ECHECK; }
  return look_end(s);
}

template <typename K> double cmp_value_of(cmp_u64 key);
template <> double cmp_value_of<cmp_u64>(cmp_u64 key) {
  if (key == ~(cmp_u64)0) return std::numeric_limits<double>::quiet_NaN();
  const cmp_u64 b = key >> 63 ? key & ~((cmp_u64)1 << 63) : ~key;
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
}
template <> double cmp_value_of<unsigned>(cmp_u64 key64) {
  const unsigned key = (unsigned)key64;
  if (key == ~0u) return std::numeric_limits<double>::quiet_NaN();
  const unsigned b = key >> 31 ? key & ~(1u << 31) : ~key;
  float x;
  memcpy(&x, &b, sizeof x);
  return (double)x;
}

int cmp_select_run(CmpBuf* s, Engine* E, hipStream_t st, int nq, const int64_t* ranks, double* values, const std::string& who) {
  const int bits = E->dtype == CHS_F64 ? 64 : 32;
  CmpResult* r = s->hRes;
  s->ms = -1.0;   // (the histogram of the last chs_composition stays: `have` is not touched)
  memset(&r->sel, 0, sizeof(CmpSel));
  for (int q = 0; q < nq; ++q) r->sel.rem[q] = ranks[q];
  r->sel.nuniq = 1;
  CHS_HIP(hipMemcpyAsync(s->sel, &r->sel, sizeof(CmpSel), hipMemcpyHostToDevice, st));
  CHS_HIP(hipMemsetAsync(s->tables, 0, sizeof(cmp_u64) * CHS_CMP_MAX_RANKS * CMP_DIGITS, st));
  CHS_HIP(hipEventRecord(s->ev[0], st));
  int pass = 0;
  for (int top = bits; top > 0; top -= CMP_DIGIT_BITS, ++pass) {
    CmpSweep w{};
    w.kernel = 2; w.pass = pass; w.nq = nq;
    w.shift = top > CMP_DIGIT_BITS ? top - CMP_DIGIT_BITS : 0;
    w.width = top - w.shift;
    int rc;
    if ((rc = cmp_sweep(s, E, w, st))) return rc;
    k_cmp_scan<<<1, CMP_SCAN_THREADS, 0, st>>>(nq, w.width, s->sel, s->tables);
    CHS_HIP(hipGetLastError());
  }
  CHS_HIP(hipEventRecord(s->ev[1], st));
  CHS_HIP(hipMemcpyAsync(&r->sel, s->sel, sizeof(CmpSel), hipMemcpyDeviceToHost, st));
  CHS_HIP(hipStreamSynchronize(st));
  std::string m;
  if (r->sel.err & CMP_ERR_SCAN) m += " a rank fell into no digit of its table;";
  for (int q = 0; q < nq; ++q) {   // below = ranks[q] - rem keys lie below the one found, equal are equal to it
    const cmp_i64 below = ranks[q] - r->sel.rem[q], equal = r->sel.equal[q];
    if (below < 0 || below > ranks[q] || !(ranks[q] < below + equal)) {
      m += " rank " + std::to_string(ranks[q]) + ": " + std::to_string(below) + " keys below the one found, " + std::to_string(equal) + " equal to it;";
      break;
    }
  }
  if (!m.empty()) { chs_set_error(who + ": self-check failed:" + m); return CHS_ECHECK; }
  for (int q = 0; q < nq; ++q)
    values[q] = bits == 64 ? cmp_value_of<cmp_u64>(r->sel.prefix[q]) : cmp_value_of<unsigned>(r->sel.prefix[q]);
  float ms = 0.f;
  CHS_HIP(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
  s->ms = ms;
  return CHS_OK;
}
}  // namespace

void chs_cmp_free(void** buf) {
  if (!buf) return;
  cmp_release((CmpBuf*)*buf);
  *buf = nullptr;
}

void chs_cmp_forget(void* buf) {
  if (buf) look_forget((CmpBuf*)buf);
}

int chs_cmp_look(Engine* E, hipStream_t st, void** buf, double threshold, int32_t nbins, double lo, double hi, int64_t* iw,
                 double* fw, const char* who_) {
  const std::string who(who_);
  int rc;
  if ((rc = look_check_args(iw, threshold, who))) return rc;
  if (!fw) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (nbins < 1 || nbins > CHS_CMP_MAX_BINS) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + " is outside [1, " + std::to_string(CHS_CMP_MAX_BINS) + "]"); return CHS_EINVAL; }
  const bool own_range = std::isnan(lo) && std::isnan(hi);
  if (!own_range) {
    if (std::isnan(lo) || std::isnan(hi)) { chs_set_error(who + ": lo and hi are both NaN (the field's own range) or both numbers"); return CHS_EINVAL; }
    if (std::isinf(lo) || std::isinf(hi)) { chs_set_error(who + ": an infinite bound"); return CHS_EINVAL; }
    if (lo > hi) { chs_set_error(who + ": lo > hi"); return CHS_EINVAL; }
  }
  if ((rc = look_check_field(E, CMP_MAX_N, who))) return rc;
  if ((rc = look_buffers<CmpBuf>(buf, E->N, cmp_alloc, cmp_release))) return rc;
  CmpBuf* s = (CmpBuf*)*buf;
  if ((rc = cmp_run(s, E, st, threshold, nbins, own_range, lo, hi, who))) return rc;
  memcpy(iw, s->hRes->iw, sizeof(int64_t) * CHS_CMP_IWORDS);
  memcpy(fw, s->hRes->fw, sizeof(double) * CHS_CMP_FWORDS);
  return CHS_OK;
}

int chs_cmp_hist(void* buf, int device, hipStream_t st, int32_t nbins, int64_t* out, const char* who_) {
  const std::string who(who_);
  const CmpBuf* s = (const CmpBuf*)buf;
  int rc;
  if ((rc = look_ready(s, out, who))) return rc;
  if (nbins != s->nbins) { chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(s->nbins)); return CHS_EINVAL; }
  return look_fetch(device, st, out, s->hist, sizeof(int64_t) * (size_t)nbins);
}

int chs_cmp_select(Engine* E, hipStream_t st, void** buf, int32_t nq, const int64_t* ranks, double* values, const char* who_) {
  const std::string who(who_);
  if (!ranks || !values) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  if (nq < 1 || nq > CHS_CMP_MAX_RANKS) { chs_set_error(who + ": nq = " + std::to_string(nq) + " is outside [1, " + std::to_string(CHS_CMP_MAX_RANKS) + "]"); return CHS_EINVAL; }
  for (int q = 0; q < nq; ++q) {
    if (ranks[q] < 0 || ranks[q] >= (int64_t)E->N * E->N) { chs_set_error(who + ": rank " + std::to_string(ranks[q]) + " is outside [0, N^2)"); return CHS_EINVAL; }
  }
  int rc;
  if ((rc = look_check_field(E, CMP_MAX_N, who))) return rc;
  if ((rc = look_buffers<CmpBuf>(buf, E->N, cmp_alloc, cmp_release))) return rc;
  return cmp_select_run((CmpBuf*)*buf, E, st, nq, ranks, values, who);
}

int chs_cmp_last_ms(const void* h, const void* buf, double* ms, const char* what) {
  return look_last_ms(h, (const CmpBuf*)buf, ms, what);
}

extern "C" int chs_composition(chs_handle h, double threshold, int32_t nbins, double lo, double hi, int64_t iw[CHS_CMP_IWORDS],
                               double fw[CHS_CMP_FWORDS]) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_composition: null handle"); return CHS_EINVAL; }
  return chs_cmp_look(E, E->stream, &E->cmp, threshold, nbins, lo, hi, iw, fw, "chs_composition");
}

extern "C" int chs_composition_hist(chs_handle h, int32_t nbins, int64_t* out) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_composition_hist: null handle"); return CHS_EINVAL; }
  return chs_cmp_hist(E->cmp, E->hc.device, E->stream, nbins, out, "chs_composition_hist");
}

extern "C" int chs_composition_select(chs_handle h, int32_t nq, const int64_t* ranks, double* values) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_composition_select: null handle"); return CHS_EINVAL; }
  return chs_cmp_select(E, E->stream, &E->cmp, nq, ranks, values, "chs_composition_select");
}

extern "C" int chs_composition_last_ms(chs_handle h, double* ms) {
  return chs_cmp_last_ms(h, h ? ((Engine*)h)->cmp : nullptr, ms, "chs_composition");
}

extern "C" int chs_composition_tile(int32_t* elems_per_thread, int32_t* threads, int32_t* max_groups, int32_t* digit_bits) {
  if (!elems_per_thread || !threads || !max_groups || !digit_bits) { chs_set_error("chs_composition_tile: null argument"); return CHS_EINVAL; }
  *elems_per_thread = CMP_EPT;
  *threads = CMP_THREADS;
  *max_groups = CMP_MAX_GROUPS;
  *digit_bits = CMP_DIGIT_BITS;
  return CHS_OK;
}
