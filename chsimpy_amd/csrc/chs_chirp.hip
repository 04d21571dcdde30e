// chs_chirp.hip -- "chirp" transform engine: the 2-D orthonormal DCT-II/III for ANY N in [8, 4096], line by line with
// Bluestein's chirp-z algorithm on a power-of-two FFT of length P >= 2N-1 held in LDS.  O(N^2 log N) per transform
// where the direct engine (chs_direct.hip) spends O(N^3).  Natural order in and out, so that the step is the direct
// engine's unfused sequence with another dct2d (chs_api.hip: one_step).
//
// The algorithm, its tables and the LDS layout: chs_chirp_host.h; the index maps as numpy: tools/chirp_model.py.
//
// k_chirp_lines<T, INV>: P/8 lanes own a line, a workgroup carries as many lines as fill 256 threads (P = 4096, 8192:
// one line of 512, 1024 threads).  A lane keeps 8 complex values in registers through a radix-8 pass; between passes
// the values change hands through LDS (one barrier per exchange: a pass reads and writes the same positions).  The
// forward FFT is decimation in frequency, its last pass works on the 8 neighbouring positions of a lane (one radix 8,
// two radix 4 or four radix 2), Bhat is stored at those digit-reversed positions and the inverse FFT is the same
// network backwards: no permutation pass, and the last forward pass, the product and the first inverse pass never
// leave the registers.  P, the pass count and the strides are run-time arguments: one kernel per direction and type.
// The constant part of a line does not go through the convolution: the solver's fields are a mean plus fluctuations a
// thousand times smaller, the chirp spreads the mean over every frequency of the FFT, and the rounding of that part
// would land on every coefficient (in fp32 several times the direct engine's error, which rounds coefficient by
// coefficient).  Forward, the line's first value is subtracted from all of them and comes back as ref*sqrt(N) in X[0]
// (the DCT-II of a constant line); inverse, X[0] is left out of the spectrum and comes back as X[0]/sqrt(N) in every
// point.
// Global traffic is coalesced: the Makhoul reorder happens between the global order and the LDS position, the zero
// padding is never loaded.  The column direction is the same kernel between two tiled transposes.
#include <cmath>
#include <cstring>
#include <new>
#include "chs_common.h"
#include "chs_cx.h"
#include "chs_fast_core.h"
#include "chs_chirp_host.h"

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

template <typename T, bool INV, int MAXT>
__global__ __launch_bounds__(MAXT) void k_chirp_lines(const T* __restrict__ in, T* __restrict__ out, const ChirpArgs<T> a,
                                                      const DevState* __restrict__ st, int ignore_halt) {
  if (!ignore_halt && st->halt) return;
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
template <typename T>
__global__ __launch_bounds__(256) void k_chirp_transpose(const T* __restrict__ in, T* __restrict__ out, int N,
                                                         const DevState* __restrict__ st, int ignore_halt) {
  if (!ignore_halt && st->halt) return;
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

template <typename T, bool INV>
int launch_lines(Engine* E, const ChirpDev* D, const void* in, void* out, int ignore_halt) {
  const ChirpArgs<T> a = chirp_args<T>(D, E->N, INV);
  const int lpb = chirp_lines_per_block(D->plan.P);
  const int blocks = (E->N + lpb - 1) / lpb;
  if (D->threads <= 256)
    k_chirp_lines<T, INV, 256><<<blocks, D->threads, D->ldsBytes, E->stream>>>((const T*)in, (T*)out, a, E->dState, ignore_halt);
  else
    k_chirp_lines<T, INV, 1024><<<blocks, D->threads, D->ldsBytes, E->stream>>>((const T*)in, (T*)out, a, E->dState, ignore_halt);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

template <typename T>
int launch_transpose(Engine* E, const void* in, void* out, int ignore_halt) {
  const int nt = (E->N + CT_TILE - 1) / CT_TILE;
  k_chirp_transpose<T><<<dim3(nt, nt), 256, 0, E->stream>>>((const T*)in, (T*)out, E->N, E->dState, ignore_halt);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

template <typename T, bool INV>
int dct2d_t(Engine* E, const ChirpDev* D, const void* in, void* out, void* tmp) {
  int rc;
  const int ih = 0;
  if ((rc = launch_lines<T, INV>(E, D, in, tmp, ih))) return rc;    // along the rows
  if ((rc = launch_transpose<T>(E, tmp, out, ih))) return rc;
  if ((rc = launch_lines<T, INV>(E, D, out, tmp, ih))) return rc;   // along the columns
  return launch_transpose<T>(E, tmp, out, ih);
}

template <typename T>
int set_lds_all(size_t bytes) {
  const int b = (int)bytes;
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, false, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, true, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, false, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, true, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  return CHS_OK;
}

}  // namespace

bool chs_chirp_supported(int N) { return N >= CHS_CHIRP_MIN_N && N <= CHS_CHIRP_MAX_N; }

int chs_chirp_init(Engine* E) {
  ChirpDev* D = new (std::nothrow) ChirpDev();
  if (!D) { chs_set_error("out of host memory"); return CHS_EINVAL; }
  E->chirp = D;
  const ChirpTablesLd t = chirp_tables_ld(E->N);
  D->plan = t.plan;
  D->threads = chirp_block_threads(t.plan.P);
  D->ldsBytes = chirp_lds_bytes(t.plan.P, (int)E->esz);
  const std::vector<ChirpCx>* tabs[6] = {&t.tw, &t.bhat, &t.fin, &t.fout, &t.iin, &t.iout};
  size_t total = 0;
  for (int i = 0; i < 6; ++i) { D->off[i] = total; total += 2 * tabs[i]->size(); }
  std::vector<char> host(total * E->esz);
  for (int i = 0; i < 6; ++i) {
    if (E->dtype == CHS_F64) {
      const std::vector<double> r = chirp_round<double>(*tabs[i]);
      memcpy(host.data() + D->off[i] * 8, r.data(), r.size() * 8);
    } else {
      const std::vector<float> r = chirp_round<float>(*tabs[i]);
      memcpy(host.data() + D->off[i] * 4, r.data(), r.size() * 4);
    }
  }
  CHS_HIP(hipMalloc(&D->tables, host.size()));
  CHS_HIP(hipMemcpy(D->tables, host.data(), host.size(), hipMemcpyHostToDevice));
  // a line of P = 8192 needs 132 KiB of the CU's 160 KiB: above the default limit of a launch.  The limit belongs to
  // the kernel, not to the engine: always that of the largest P, whatever this engine's is
  const size_t most = chirp_lds_bytes(2 * CHS_CHIRP_MAX_N, 8);
  return E->dtype == CHS_F64 ? set_lds_all<double>(most) : set_lds_all<float>(most);
}

void chs_chirp_free(Engine* E) {
  ChirpDev* D = (ChirpDev*)E->chirp;
  if (!D) return;
  if (D->tables) hipFree(D->tables);
  delete D;
  E->chirp = nullptr;
}

// out = dctn(in) (forward) or idctn(in) (inverse), norm='ortho'; tmp is an N x N scratch; in, out, tmp distinct.
int chs_chirp_dct2d(Engine* E, const void* in, void* out, void* tmp, bool inverse) {
  const ChirpDev* D = (const ChirpDev*)E->chirp;
  if (E->dtype == CHS_F64)
    return inverse ? dct2d_t<double, true>(E, D, in, out, tmp) : dct2d_t<double, false>(E, D, in, out, tmp);
  return inverse ? dct2d_t<float, true>(E, D, in, out, tmp) : dct2d_t<float, false>(E, D, in, out, tmp);
}
