// chs_mathhook.hip -- chs_test_math_cols: the inline functions of chs_math.h, each called elementwise through one
// test kernel (accuracy tests only; no step kernel lives here).  The kernel calls the very functions the step kernels
// call; the codes and the meaning of the columns are those of include/chs_hip.h.
#include "chs_common.h"
#include "chs_math.h"

#define MH_THREADS 256
#define MH_NIN 4
#define MH_NOUT 2
#define MH_NCONST 8
#define MH_FIRST 10
#define MH_LAST 36

struct MhConsts { double c[MH_NCONST]; };

// T-typed forms of the column functions: the inputs are doubles that hold T values exactly (the host rounded them),
// the arithmetic is T's and the result is widened on the way out.
template <typename T, int WHICH>
__device__ __forceinline__ double mh_from_logs(double U, double Uinv, double lU, double lV, const MhConsts& k) {
  const T RT = (T)k.c[0], B = (T)k.c[1], BRT = (T)k.c[2], A0 = (T)k.c[3], A1 = (T)k.c[4];
  if constexpr (WHICH == 0) return (double)chs_energy_from_logs<T>((T)U, (T)Uinv, (T)lU, (T)lV, RT, B, A0, A1);
  else if constexpr (WHICH == 1) return (double)chs_mu_from_logs<T>((T)U, (T)Uinv, (T)lU, (T)lV, RT, BRT, A0, A1);
  else if constexpr (WHICH == 2) return (double)chs_energy_from_logs_fast<T>((T)U, (T)Uinv, (T)lU, (T)lV, RT, B, A0, A1);
  else return (double)chs_mu_from_logs_fast<T>((T)U, (T)Uinv, (T)lU, (T)lV, RT, BRT, A0, A1);
}

__global__ __launch_bounds__(MH_THREADS) void k_test_math_cols(int which, const double* __restrict__ in, MhConsts k,
                                                               double* __restrict__ out, long long n) {
  __shared__ double2 ltab[CHS_LOGTAB_N];
  for (int t = threadIdx.x; t < CHS_LOGTAB_N; t += blockDim.x) ltab[t] = reinterpret_cast<const double2*>(chs_log_table)[t];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = in[i], b = in[n + i], c = in[2 * n + i], d = in[3 * n + i];
  double r0 = 0.0, r1 = 0.0;
  unsigned dom = 0;
  switch (which) {
    case 10: r0 = chs_div_pos(a, b); r1 = __builtin_amdgcn_rcp(b); break;
    case 11: r0 = chs_div_pos1(a, b); r1 = __builtin_amdgcn_rcp(b); break;
    case 12: case 13: case 14: {
      const PwConsts pwk = chs_pw_consts(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4]);
      r0 = k.c[5];
      if (which == 12) chs_energy_mu_from_logs<true, true>(a, b, c, d, pwk, r0, r1);
      else if (which == 13) chs_energy_mu_from_logs<true, false>(a, b, c, d, pwk, r0, r1);
      else chs_energy_mu_from_logs<false, true>(a, b, c, d, pwk, r0, r1);
    } break;
    case 15: case 16: {  // one grid point as the fused fp64 row kernel forms it (chs_fast_kernels.h, `point`)
      const PwConsts pwk = chs_pw_consts(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4]);
      const double u = a, uinv = 1.0 - u;
      const double lU = chs_log_unit_tab<double>(u, ltab, dom), lV = chs_log_unit_tab<double>(uinv, ltab, dom);
      double sE = k.c[5], m = 0.0;
      chs_energy_mu_from_logs<true, true>(u, uinv, lU, lV, pwk, sE, m);
      if (which == 15) { r0 = sE; r1 = m; }
      else { r0 = m; r1 = chs_log_dom_bad(dom) ? 1.0 : 0.0; }
    } break;
    case 17: r0 = mh_from_logs<double, 0>(a, b, c, d, k); break;
    case 18: r0 = mh_from_logs<double, 1>(a, b, c, d, k); break;
    case 19: r0 = mh_from_logs<double, 2>(a, b, c, d, k); break;
    case 20: r0 = mh_from_logs<double, 3>(a, b, c, d, k); break;
    case 21: r0 = mh_from_logs<float, 0>(a, b, c, d, k); break;
    case 22: r0 = mh_from_logs<float, 1>(a, b, c, d, k); break;
    case 23: r0 = mh_from_logs<float, 2>(a, b, c, d, k); break;
    case 24: r0 = mh_from_logs<float, 3>(a, b, c, d, k); break;
    case 25: r0 = chs_dt_integrand(a, k.c[0]); break;
    case 26: r0 = chs_dt_integrand_fast(a, k.c[0]); break;
    case 27: r0 = (double)chs_dt_integrand_fast((float)a, (float)k.c[0]); break;
    case 28: r0 = chs_spectral<double>(a, b, c, d, k.c[0], k.c[1]); break;
    case 29: r0 = (double)chs_spectral<float, false>((float)a, (float)b, c, d, k.c[0], k.c[1]); break;
    case 30: r0 = (double)chs_spectral_f32((float)a, (float)b, c, d, k.c[0], k.c[1]); break;
    case 31: r0 = (double)chs_logf((float)a); break;
    case 32: r0 = (double)chs_log_ratio<float>((float)a, (float)b); break;
    case 33: r0 = (double)chs_mu<float>((float)a, (float)k.c[0], (float)k.c[2], (float)k.c[3], (float)k.c[4]); break;
    case 34: r0 = (double)chs_energy_density<float>((float)a, (float)k.c[0], (float)k.c[1], (float)k.c[3], (float)k.c[4]); break;
    case 35: r0 = (double)chs_log_unit_tab<float>((float)a, ltab, dom); r1 = chs_log_dom_bad(dom) ? 1.0 : 0.0; break;
    default: r0 = chs_log_unit_tab<double>(a, ltab, dom); r1 = chs_log_dom_bad(dom) ? 1.0 : 0.0; break;  // 36
  }
  out[i] = r0;
  out[n + i] = r1;
}

extern "C" int chs_test_math_cols(int device, int which, const double* in, const double* consts, double* out, int64_t n) {
  if (!in || !consts || !out || n <= 0 || n > (int64_t)1 << 28 || which < MH_FIRST || which > MH_LAST) {
    chs_set_error("chs_test_math_cols: bad argument");
    return CHS_EINVAL;
  }
  CHS_HIP(hipSetDevice(device));
  MhConsts k;
  for (int j = 0; j < MH_NCONST; ++j) k.c[j] = consts[j];
  double *din = nullptr, *dout = nullptr;
  CHS_HIP(hipMalloc(&din, sizeof(double) * MH_NIN * n));
  if (hipMalloc(&dout, sizeof(double) * MH_NOUT * n) != hipSuccess) {
    hipFree(din);
    chs_set_error("chs_test_math_cols: out of device memory");
    return CHS_EHIP;
  }
  auto run = [&]() -> int {   // (CHS_HIP returns: the buffers are freed behind it either way)
    CHS_HIP(hipMemcpy(din, in, sizeof(double) * MH_NIN * n, hipMemcpyHostToDevice));
    k_test_math_cols<<<(unsigned)((n + MH_THREADS - 1) / MH_THREADS), MH_THREADS>>>(which, din, k, dout, (long long)n);
    CHS_HIP(hipGetLastError());
    CHS_HIP(hipDeviceSynchronize());
    CHS_HIP(hipMemcpy(out, dout, sizeof(double) * MH_NOUT * n, hipMemcpyDeviceToHost));
    return CHS_OK;
  };
  const int rc = run();
  hipFree(din);
  hipFree(dout);
  return rc;
}
