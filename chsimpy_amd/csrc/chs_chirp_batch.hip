// chs_chirp_batch.hip -- the chirp engine's transform for a batch (chs_batch.hip): the 2-D DCT of EVERY member in four
// launches, the member as the grid's slowest dimension.  The kernels are those of chs_chirp_kernels.h instantiated
// with a NatSel behind their arguments (chs_nat_batch.h): a workgroup takes source and destination from its member's
// record, everything else -- the lines of a workgroup, the block size, the LDS layout, the tables -- is the single
// handle's launch (chs_chirp.hip: launch_lines, launch_transpose); the tables are member 0's, all members share N and
// the element type.  In a translation unit of its own, beside the instantiations of the single handle they would share
// nothing but the source text with.
#include "chs_common.h"
#include "chs_chirp_kernels.h"

namespace {

template <typename T, bool INV>
int launch_lines_batch(Engine* E0, const ChirpDev* D, hipStream_t s, const NatMember* mem, int B, int src, int dst) {
  const ChirpArgs<T> a = chirp_args<T>(D, E0->N, INV);
  const int lpb = chirp_lines_per_block(D->plan.P);
  const dim3 grid((E0->N + lpb - 1) / lpb, B);
  const NatSel sel{mem, src, dst};
  if (D->threads <= 256)
    k_chirp_lines<T, INV, 256, NatSel><<<grid, D->threads, D->ldsBytes, s>>>(nullptr, nullptr, a, nullptr, 0, sel);
  else
    k_chirp_lines<T, INV, 1024, NatSel><<<grid, D->threads, D->ldsBytes, s>>>(nullptr, nullptr, a, nullptr, 0, sel);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

template <typename T>
int launch_transpose_batch(Engine* E0, hipStream_t s, const NatMember* mem, int B, int src, int dst) {
  const int nt = (E0->N + CT_TILE - 1) / CT_TILE;
  k_chirp_transpose<T, NatSel><<<dim3(nt, nt, B), 256, 0, s>>>(nullptr, nullptr, E0->N, nullptr, 0, NatSel{mem, src, dst});
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

// the sequence of dct2d_t (chs_chirp.hip): rows, transpose, columns, transpose
template <typename T, bool INV>
int dct2d_batch_t(Engine* E0, const ChirpDev* D, hipStream_t s, const NatMember* mem, int B, int src, int dst, int tmp) {
  int rc;
  if ((rc = launch_lines_batch<T, INV>(E0, D, s, mem, B, src, tmp))) return rc;
  if ((rc = launch_transpose_batch<T>(E0, s, mem, B, tmp, dst))) return rc;
  if ((rc = launch_lines_batch<T, INV>(E0, D, s, mem, B, dst, tmp))) return rc;
  return launch_transpose_batch<T>(E0, s, mem, B, tmp, dst);
}

template <typename T>
int set_lds_batch(size_t bytes) {
  const int b = (int)bytes;
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, false, 256, NatSel>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, true, 256, NatSel>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, false, 1024, NatSel>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  CHS_HIP(hipFuncSetAttribute((const void*)k_chirp_lines<T, true, 1024, NatSel>, hipFuncAttributeMaxDynamicSharedMemorySize, b));
  return CHS_OK;
}

}  // namespace

// the limit belongs to the kernel: that of the largest P, as in chs_chirp_init
int chs_chirp_batch_init(Engine* E0) {
  if (E0->engine != CHS_ENGINE_CHIRP || !E0->chirp) { chs_set_error("chs_chirp_batch_init: not a chirp engine"); return CHS_EINVAL; }
  const size_t most = chirp_lds_bytes(2 * CHS_CHIRP_MAX_N, 8);
  return E0->dtype == CHS_F64 ? set_lds_batch<double>(most) : set_lds_batch<float>(most);
}

int chs_chirp_batch_dct2d(Engine* E0, hipStream_t s, const NatMember* mem, int B, int src, int dst, int tmp, bool inverse) {
  const ChirpDev* D = (const ChirpDev*)E0->chirp;
  if (E0->dtype == CHS_F64)
    return inverse ? dct2d_batch_t<double, true>(E0, D, s, mem, B, src, dst, tmp)
                   : dct2d_batch_t<double, false>(E0, D, s, mem, B, src, dst, tmp);
  return inverse ? dct2d_batch_t<float, true>(E0, D, s, mem, B, src, dst, tmp)
                 : dct2d_batch_t<float, false>(E0, D, s, mem, B, src, dst, tmp);
}
