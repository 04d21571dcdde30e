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
#include "chs_chirp_kernels.h"

namespace {

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
