// chs_chirp_kernels.h -- the device code of the chirp engine (chs_chirp.hip): the line kernel, the tiled transpose and
// their arguments.
// chs_chirp.hip instantiates the single handle's kernels.  chs_chirp_batch.hip instantiates the batched ones, which
// take a NatSel behind the arguments (chs_nat_batch.h).  One body, two kernels: a member of a batch computes what its
// single handle computes.  A translation unit each: the single handle's code stays what it was.
// The algorithm and the LDS layout: chs_chirp_host.h and the head of chs_chirp.hip.
#pragma once
#include "chs_common.h"
#include "chs_cx.h"
#include "chs_fast_core.h"
#include "chs_chirp_host.h"
#include "chs_nat_batch.h"

namespace {

template <typename T>
struct ChirpArgs {
  const T* tw;    // [P]  exp(-2 pi i m/P)
  const T* bhat;  // [P]  at the forward FFT's output positions, 1/P included
  const T* tin;   // [N]  input factors of this direction
  const T* tout;  // [N]  output factors of this direction
  int N, P, logP, nt, rl;
  int lgLanes;    // log2(P/8)
  int items;      // LDS items of one plane of a line
  T dc;           // the constant part on its way round the convolution: sqrt(N) forward, 1/sqrt(N) inverse
};

struct ChirpDev {
  ChirpPlan plan;
  void* tables = nullptr;  // one allocation: tw, bhat, fin, fout, iin, iout
  size_t off[6] = {0, 0, 0, 0, 0, 0};  // element offsets (in T) of the six tables
  size_t ldsBytes = 0;
  int threads = 256;
};

__device__ __forceinline__ int chirp_pad(int i) { return i + (i >> 5); }

// one line's LDS: fp64 two planes of doubles, fp32 one plane of pairs
template <typename T>
struct LineLds;
template <>
struct LineLds<double> {
  double* re;
  double* im;
  __device__ __forceinline__ LineLds(unsigned char* smem, int line, int items) {
    re = reinterpret_cast<double*>(smem) + (size_t)line * 2 * items;
    im = re + items;
  }
  __device__ __forceinline__ void st(int pos, D2 v) const { const int a = chirp_pad(pos); re[a] = v.x; im[a] = v.y; }
  __device__ __forceinline__ D2 ld(int pos) const { const int a = chirp_pad(pos); return cx_make(re[a], im[a]); }
  __device__ __forceinline__ double* real() const { return re; }
};
template <>
struct LineLds<float> {
  v2f* p;
  __device__ __forceinline__ LineLds(unsigned char* smem, int line, int items) {
    p = reinterpret_cast<v2f*>(smem) + (size_t)line * items;
  }
  __device__ __forceinline__ void st(int pos, v2f v) const { p[chirp_pad(pos)] = v; }
  __device__ __forceinline__ v2f ld(int pos) const { return p[chirp_pad(pos)]; }
  __device__ __forceinline__ float* real() const { return reinterpret_cast<float*>(p); }
};

// the last forward pass / first inverse pass on the 8 neighbouring positions of a lane
template <class V, bool INV>
__device__ __forceinline__ void chirp_last(V* z, int rl) {
  if (rl == 0) {
    Dft<V, 8, INV>::run(z);
  } else if (rl == 2) {
    Dft<V, 4, INV>::run(z);
    Dft<V, 4, INV>::run(z + 4);
  } else {
#pragma unroll
    for (int e = 0; e < 8; e += 2) Dft<V, 2, INV>::run(z + e);
  }
}

// Batch...: empty for the single handle's kernel; one NatSel for a batch (chs_nat_batch.h), grid (blocks, B): the
// member's arrays sel.src / sel.dst stand in for in / out, the tables `a` are member 0's
template <typename T, bool INV, int MAXT, class... Batch>
__global__ __launch_bounds__(MAXT) void k_chirp_lines(const T* __restrict__ in, T* __restrict__ out, const ChirpArgs<T> a,
                                                      const DevState* __restrict__ st, int ignore_halt, Batch... sel) {
  if constexpr (sizeof...(Batch) != 0) {
    const NatSel b = NatSel{sel...};
    ConstNatMember& m = nat_member(b, blockIdx.y);
    if (nat_sits_out(m)) return;
    in = (const T*)m.arr[b.src]; out = (T*)m.arr[b.dst];
  } else {
    if (!ignore_halt && st->halt) return;
  }
  using V = Cx<T>;
  extern __shared__ __align__(16) unsigned char chirp_smem[];
  const int N = a.N, logP = a.logP;
  const int lanes = 1 << a.lgLanes;
  const int lineInBlock = (int)threadIdx.x >> a.lgLanes;
  const int t = (int)threadIdx.x & (lanes - 1);
  const int line = (int)blockIdx.x * ((int)blockDim.x >> a.lgLanes) + lineInBlock;
  const bool active = line < N;   // (a line past the grid takes part in the barriers only)
  const size_t row = (size_t)(active ? line : 0) * N;
  const LineLds<T> lds(chirp_smem, lineInBlock, a.items);
  const V zero = cx_make(T(0), T(0));
  const int ls0 = logP - 3;

  V z[8];
  const T ref = active ? in[row] : T(0);   // forward: the line's first value; inverse: X[0]
  if constexpr (!INV) {
    // (x[i] - ref) * w[pos(i)] to its Makhoul position
    for (int i = t; i < N; i += lanes) {
      const int pos = (i & 1) ? N - 1 - ((i - 1) >> 1) : (i >> 1);
      const T x = active ? in[row + i] - ref : T(0);
      const V w = ldc<T>(a.tin, pos);
      lds.st(pos, cx_make(x * cx_re(w), x * cx_im(w)));
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pos = t + (q << ls0);
      z[q] = (pos < N) ? lds.ld(pos) : zero;
    }
  } else {
    // a[n] = iin[n] * (X[n] + i X[N-n]),  X[N] := 0; X[0] goes round the convolution
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = t + (q << ls0);
      z[q] = zero;
      if (active && n < N) {
        const T xr = n ? in[row + n] : T(0);
        const T xi = n ? in[row + (N - n)] : T(0);
        z[q] = cx_mul(cx_make(xr, xi), ldc<T>(a.tin, n));
      }
    }
  }
#pragma unroll
  for (int q = 4; q < 8; ++q) z[q] = zero;   // N <= P/2: the upper half of the padded line

  // forward FFT, decimation in frequency
  int ls = ls0;
  for (int i = 0; i < a.nt; ++i) {
    Dft<V, 8, false>::run(z);
    const int j = t & ((1 << ls) - 1);
    const int sh = logP - ls - 3;
#pragma unroll
    for (int k = 1; k < 8; ++k) z[k] = cx_mul(z[k], ldc<T>(a.tw, (j * k) << sh));
    int base = ((t >> ls) << (ls + 3)) + j;
#pragma unroll
    for (int k = 0; k < 8; ++k) lds.st(base + (k << ls), z[k]);
    __syncthreads();
    ls = (i + 1 < a.nt) ? ls - 3 : 0;
    base = ((t >> ls) << (ls + 3)) + (t & ((1 << ls) - 1));
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = lds.ld(base + (q << ls));
  }
  chirp_last<V, false>(z, a.rl);
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = cx_mul(z[e], ldc<T>(a.bhat, 8 * t + e));
  chirp_last<V, true>(z, a.rl);
  // inverse FFT, decimation in time: the same network backwards
  ls = 0;
  for (int i = a.nt - 1; i >= 0; --i) {
    int base = ((t >> ls) << (ls + 3)) + (t & ((1 << ls) - 1));
#pragma unroll
    for (int k = 0; k < 8; ++k) lds.st(base + (k << ls), z[k]);
    __syncthreads();
    ls = ls0 - 3 * i;
    const int j = t & ((1 << ls) - 1);
    const int sh = 3 * i;
    base = ((t >> ls) << (ls + 3)) + j;
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = lds.ld(base + (q << ls));
#pragma unroll
    for (int k = 1; k < 8; ++k) z[k] = cx_mulc(z[k], ldc<T>(a.tw, (j * k) << sh));
    Dft<V, 8, true>::run(z);
  }

  // c[k] at k = t + q P/8: the output factor and the real part
  T r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = t + (q << ls0);
    r[q] = T(0);
    if (k < N) {
      const V f = ldc<T>(a.tout, k);
      r[q] = cx_re(f) * cx_re(z[q]) - cx_im(f) * cx_im(z[q]);
      if (INV || k == 0) r[q] += ref * a.dc;
    }
  }
  if constexpr (!INV) {
    if (active) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = t + (q << ls0);
        if (k < N) out[row + k] = r[q];
      }
    }
  } else {
    // undo the reorder on the way out: x[i] = v[pos(i)]
    T* v = lds.real();
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = t + (q << ls0);
      if (k < N) v[k] = r[q];
    }
    __syncthreads();
    if (active) {
      for (int i = t; i < N; i += lanes) {
        const int pos = (i & 1) ? N - 1 - ((i - 1) >> 1) : (i >> 1);
        out[row + i] = v[pos];
      }
    }
  }
}

#define CT_TILE 32
// out = in^T, N x N, 32 x 32 tiles through LDS: rows of 32 elements on both sides
// (Batch... as above; grid (nt, nt, B))
template <typename T, class... Batch>
__global__ __launch_bounds__(256) void k_chirp_transpose(const T* __restrict__ in, T* __restrict__ out, int N,
                                                         const DevState* __restrict__ st, int ignore_halt, Batch... sel) {
  if constexpr (sizeof...(Batch) != 0) {
    const NatSel b = NatSel{sel...};
    ConstNatMember& m = nat_member(b, blockIdx.z);
    if (nat_sits_out(m)) return;
    in = (const T*)m.arr[b.src]; out = (T*)m.arr[b.dst];
  } else {
    if (!ignore_halt && st->halt) return;
  }
  __shared__ T tile[CT_TILE][CT_TILE + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8 threads
  const int r0 = blockIdx.y * CT_TILE, c0 = blockIdx.x * CT_TILE;
#pragma unroll
  for (int y = ty; y < CT_TILE; y += 8) {
    const int r = r0 + y, c = c0 + tx;
    if (r < N && c < N) tile[y][tx] = in[(size_t)r * N + c];
  }
  __syncthreads();
#pragma unroll
  for (int y = ty; y < CT_TILE; y += 8) {
    const int r = c0 + y, c = r0 + tx;   // out[r][c] = in[c][r]
    if (r < N && c < N) out[(size_t)r * N + c] = tile[tx][y];
  }
}

template <typename T>
ChirpArgs<T> chirp_args(const ChirpDev* D, int N, bool inverse) {
  const T* base = (const T*)D->tables;
  ChirpArgs<T> a;
  a.tw = base + D->off[0];
  a.bhat = base + D->off[1];
  a.tin = base + D->off[inverse ? 4 : 2];
  a.tout = base + D->off[inverse ? 5 : 3];
  a.N = N; a.P = D->plan.P; a.logP = D->plan.logP; a.nt = D->plan.nt; a.rl = D->plan.rl;
  a.lgLanes = D->plan.logP - 3;
  a.items = chirp_lds_items(D->plan.P);
  a.dc = (T)(inverse ? 1.0L / sqrtl((long double)N) : sqrtl((long double)N));
  return a;
}

}  // namespace
