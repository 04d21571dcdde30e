// chs_spectrum.hip -- the radially averaged structure factor of the field, on the device.
//
//   C = dctn(U - mean(U), norm='ortho');  Ssum[b] = sum of C[i][j]^2 over the modes whose bin is b,
//   bin(i, j) = the integer nearest to sqrt(i^2 + j^2), decided in integers: b^2 - b < i^2 + j^2 <= b^2 + b
// (no tie exists: b^2 + b + 1/4 is no integer); the power of mode (0, 0) counts as 0.  Always float64.
//
// Four stages on the handle's stream, all on arrays that are dead between two calls in every mode (U, hat_U, T1 and
// the partial sums of the continuing loop are read at the most):
//   k_sum / k_sum_fin (chs_pointwise.hip)  mean(U) into a state of this file's own -- the engine's meanU is not written
//   k_spec_center      MU <- U - mean, in the handle's element type: the mean leaves BEFORE the transform, whose error
//                      scales with the largest coefficient (the field is a mean plus fluctuations 1000 times smaller)
//   the engine's natural-order forward transform: fast MU -> (T2) -> MU, direct / chirp MU -> (T1) -> T2
//   k_spec_bins, k_spec_fin   the binning, below
//
// The binning is deterministic: no floating-point atomics anywhere.  A workgroup owns a tile of SPEC_TR x SPEC_TC
// coefficients, whose bins are a contiguous window of at most sqrt(SPEC_TR^2 + SPEC_TC^2) + 2 bins from bin(i0, j0) on
// (the bin grows with i and with j, and sqrt(i^2 + j^2) is 1-Lipschitz) -- 17 KB of LDS at every N instead of all
// 1.415 N bins.  Each wavefront has a window of its own and walks its rows of the tile in order; along a row the bin
// never decreases, so the 64 lanes of a load are runs of equal bins: a segmented sum over the lanes (a fixed tree) and
// the first lane of every run adds to the wavefront's window, one lane per bin and instruction.  The four windows are
// added in wavefront order, the tile's window goes to HBM, and k_spec_fin adds up the tiles of a bin in tile order.
#include <cstring>
#include <new>

#include "chs_look.h"
#include "chs_nat_batch.h"

#define SPEC_THREADS 256
#define SPEC_WAVES (SPEC_THREADS / CHS_WAVE)
#define SPEC_TR 32                      // rows of a tile: SPEC_TR / SPEC_WAVES per wavefront
#define SPEC_TC 512                     // columns of a tile
#define SPEC_WIN (SPEC_TC + SPEC_TR)    // bins of a tile's window (>= sqrt(SPEC_TR^2 + SPEC_TC^2) + 2)

// The bin of mode (i, j).  The float square root is a first guess only (off by one at the most for N <= 16384);
// the two integer comparisons decide.
__host__ __device__ inline int spec_bin(int i, int j) {
  const unsigned s = (unsigned)i * (unsigned)i + (unsigned)j * (unsigned)j;
  if (s == 0) return 0;
  int b = (int)(sqrtf((float)s) + 0.5f);
  while ((unsigned)(b * b - b) >= s) --b;
  while (s > (unsigned)(b * b + b)) ++b;
  return b;
}

extern "C" int32_t chs_structure_factor_bins(int32_t N) {
  if (N < 1 || N > 16384) { chs_set_error("chs_structure_factor_bins: N must be in [1, 16384]"); return CHS_EINVAL; }
  return spec_bin(N - 1, N - 1) + 1;
}

// one member of a launch: the single handle's launch has one
struct SpecMember {
  const void* U;       // the field
  void* work;          // U - mean, then (fast engine) its transform
  const void* coef;    // the natural-order coefficients the binning reads
  const DevState* st;  // st->meanU: the mean of U
};

// work <- U - mean(U).  V elements (16 bytes) per thread where N * N is a multiple of V, else one.
template <typename T, int V>
__global__ __launch_bounds__(SPEC_THREADS) void k_spec_center(const SpecMember* __restrict__ mem, size_t total) {
  const SpecMember m = mem[blockIdx.y];
  const double mean = m.st->meanU;
  const size_t idx = ((size_t)blockIdx.x * SPEC_THREADS + threadIdx.x) * V;
  if (idx >= total) return;
  const T* u = (const T*)m.U + idx;
  T* w = (T*)m.work + idx;
  if constexpr (V == 1) {
    *w = (T)((double)*u - mean);
  } else {
    typedef typename ChsVec<T>::type VT;
    const VT x = *reinterpret_cast<const VT*>(u);
    VT y;
#pragma unroll
    for (int k = 0; k < V; ++k) y[k] = (T)((double)x[k] - mean);
    *reinterpret_cast<VT*>(w) = y;
  }
}

// Sum of v over the lanes to the right that share this lane's bin, the lane itself included (`room` of them follow):
// a fixed tree over the lane numbers.
__device__ __forceinline__ double spec_run_sum(double v, int room) {
#pragma unroll
  for (int off = 1; off < CHS_WAVE; off <<= 1) {
    const double o = __shfl_down(v, off, CHS_WAVE);
    if (off <= room) v += o;
  }
  return v;
}

// part[member][tile][0 .. SPEC_WIN) <- the tile's power per bin, from bin(i0, j0) on.  grid (column tiles, row tiles,
// members).  V: elements per lane and load (16 bytes where N is a multiple of V, so that every row starts aligned).
template <typename T, int V, bool NT>
__global__ __launch_bounds__(SPEC_THREADS) void k_spec_bins(const SpecMember* __restrict__ mem, int N,
                                                             double* __restrict__ part) {
  __shared__ double acc[SPEC_WAVES][SPEC_WIN];
  typedef typename ChsVec<T>::type VT;
  constexpr int CHUNK = CHS_WAVE * V;        // columns of one load of a wavefront
  constexpr int NCH = SPEC_TC / CHUNK;
  const T* __restrict__ C = (const T*)mem[blockIdx.z].coef;
  const int lane = threadIdx.x & (CHS_WAVE - 1), wave = threadIdx.x >> 6;
  const int i0 = blockIdx.y * SPEC_TR, j0 = blockIdx.x * SPEC_TC;
  const int b0 = spec_bin(i0, j0);
  for (int t = threadIdx.x; t < SPEC_WAVES * SPEC_WIN; t += SPEC_THREADS) (&acc[0][0])[t] = 0.0;
  __syncthreads();
  double* mine = acc[wave];
  for (int r = wave; r < SPEC_TR; r += SPEC_WAVES) {
    const int i = i0 + r;
    if (i >= N) break;   // (uniform in the wavefront)
    const T* row = C + (size_t)i * N;
    T x[NCH][V];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = j0 + c * CHUNK + lane * V;
      if constexpr (V == 1) {
        x[c][0] = (j < N) ? (NT ? __builtin_nontemporal_load(row + j) : row[j]) : T(0);
      } else {
        VT v = {};
        if (j < N) v = NT ? __builtin_nontemporal_load(reinterpret_cast<const VT*>(row + j)) : *reinterpret_cast<const VT*>(row + j);
#pragma unroll
        for (int k = 0; k < V; ++k) x[c][k] = v[k];
      }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (j0 + c * CHUNK >= N) break;   // (uniform) nothing of the row is left
#pragma unroll
      for (int k = 0; k < V; ++k) {
        // the lanes hold columns j, j + V, j + 2V, ...: bins that never decrease from lane to lane
        const int j = j0 + c * CHUNK + lane * V + k;
        const bool valid = j < N;
        const int b = valid ? spec_bin(i, j) : 0x7fffffff;
        const double xd = (double)x[c][k];
        const double p = (valid && (i | j) != 0) ? xd * xd : 0.0;
        const int left = __shfl_up(b, 1, CHS_WAVE);
        const bool head = (lane == 0) || (left != b);
        const unsigned long long heads = __ballot(head);
        const unsigned long long later = (lane == CHS_WAVE - 1) ? 0ull : (heads >> (lane + 1));
        const int room = later ? (__ffsll((long long)later) - 1) : (CHS_WAVE - 1 - lane);
        const double s = spec_run_sum(p, room);
        const unsigned w = (unsigned)(b - b0);
        if (head && valid && w < (unsigned)SPEC_WIN) mine[w] += s;   // one lane per bin; the wavefront's own window
      }
    }
  }
  __syncthreads();
  double* out = part + ((size_t)blockIdx.z * (gridDim.x * gridDim.y) + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * SPEC_WIN;
  for (int t = threadIdx.x; t < SPEC_WIN; t += SPEC_THREADS) {
    double s = acc[0][t];
#pragma unroll
    for (int w = 1; w < SPEC_WAVES; ++w) s += acc[w][t];
    out[t] = s;
  }
}

// ssum[member][b] <- the tiles' shares of bin b in tile order.  tile[t] = {first bin, bins in use} of tile t.
__global__ __launch_bounds__(SPEC_THREADS) void k_spec_fin(const double* __restrict__ part, const int2* __restrict__ tile,
                                                            int ntiles, int nb, double* __restrict__ ssum) {
  const int b = blockIdx.x * SPEC_THREADS + threadIdx.x;
  if (b >= nb) return;
  const double* p = part + (size_t)blockIdx.y * ntiles * SPEC_WIN;
  double s = 0.0;
  for (int t = 0; t < ntiles; ++t) {
    const int2 w = tile[t];
    const unsigned k = (unsigned)(b - w.x);
    if (k < (unsigned)w.y) s += p[(size_t)t * SPEC_WIN + k];
  }
  ssum[(size_t)blockIdx.y * nb + b] = s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {
struct SpecBuf {
  int B = 0, N = 0, nb = 0, tx = 0, ty = 0;
  DevState* st = nullptr;       // [B] zeroed states: meanU lands here; never halted, no step done (batched transforms)
  SpecMember* mem = nullptr;    // [B] device records
  NatMember* nat = nullptr;     // [B] records of the batched chirp transform
  double* part = nullptr;       // [B][tx * ty][SPEC_WIN]
  int2* tile = nullptr;         // [tx * ty]
  double* out = nullptr;        // [B][nb]
  double* hOut = nullptr;       // pinned [B][nb]
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // sweep | transform | binning of the last call
  double ms[3] = {-1.0, -1.0, -1.0};
};

void spec_release(SpecBuf* s) {
  if (!s) return;
  hipFree(s->st); hipFree(s->mem); hipFree(s->nat); hipFree(s->part); hipFree(s->tile); hipFree(s->out);
  if (s->hOut) hipHostFree(s->hOut);
  for (auto e : s->ev) if (e) hipEventDestroy(e);
  delete s;
}

int spec_buffers(void** buf, int B, int N, bool chirp_batch, hipStream_t stream) {
  SpecBuf* s = (SpecBuf*)*buf;
  if (s && s->B == B && s->N == N) return CHS_OK;
  spec_release(s);
  *buf = nullptr;
  s = new (std::nothrow) SpecBuf();
  if (!s) { chs_set_error("out of host memory"); return CHS_EINVAL; }
  *buf = s;   // (freed with its owner whatever fails below)
  s->B = B; s->N = N;
  s->nb = spec_bin(N - 1, N - 1) + 1;
  s->tx = (N + SPEC_TC - 1) / SPEC_TC; s->ty = (N + SPEC_TR - 1) / SPEC_TR;
  const size_t nt = (size_t)s->tx * s->ty;
  CHS_HIP(hipMalloc(&s->st, sizeof(DevState) * (size_t)B));
  CHS_HIP(hipMemsetAsync(s->st, 0, sizeof(DevState) * (size_t)B, stream));
  CHS_HIP(hipMalloc(&s->mem, sizeof(SpecMember) * (size_t)B));
  if (chirp_batch) CHS_HIP(hipMalloc(&s->nat, sizeof(NatMember) * (size_t)B));
  CHS_HIP(hipMalloc(&s->part, sizeof(double) * (size_t)B * nt * SPEC_WIN));
  CHS_HIP(hipMalloc(&s->tile, sizeof(int2) * nt));
  CHS_HIP(hipMalloc(&s->out, sizeof(double) * (size_t)B * s->nb));
  CHS_HIP(hipHostMalloc((void**)&s->hOut, sizeof(double) * (size_t)B * s->nb, hipHostMallocDefault));
  for (auto& e : s->ev) CHS_HIP(hipEventCreate(&e));
  std::vector<int2> tile(nt);
  for (int y = 0; y < s->ty; ++y)
    for (int x = 0; x < s->tx; ++x) {
      const int i0 = y * SPEC_TR, j0 = x * SPEC_TC;
      const int i1 = (i0 + SPEC_TR < N ? i0 + SPEC_TR : N) - 1, j1 = (j0 + SPEC_TC < N ? j0 + SPEC_TC : N) - 1;
      const int b0 = spec_bin(i0, j0);
      tile[(size_t)y * s->tx + x] = make_int2(b0, spec_bin(i1, j1) - b0 + 1);
    }
  CHS_HIP(hipMemcpy(s->tile, tile.data(), sizeof(int2) * nt, hipMemcpyHostToDevice));
  return CHS_OK;
}

int check_args(const Engine* E, const double* ssum, int32_t nbins, const std::string& who) {
  if (!ssum) { chs_set_error(who + ": null argument"); return CHS_EINVAL; }
  const int nb = spec_bin(E->N - 1, E->N - 1) + 1;
  if (nbins != nb) {
    chs_set_error(who + ": nbins = " + std::to_string(nbins) + ", expected " + std::to_string(nb) + " for N = " +
                  std::to_string(E->N) + " (chs_structure_factor_bins)");
    return CHS_EINVAL;
  }
  return CHS_OK;
}

// The transform kernels of a single handle return at once when the state says `halt` (a call that a stop rule ended
// leaves it set): it is taken down for the look and put back, the state otherwise byte for byte what it was.
int halt_down(Engine* E, DevState* saved, bool* was) {
  if (E->stateCached) {
    *saved = E->hState[0];   // (what the last call fetched behind its last kernel; nothing has run since)
  } else {
    CHS_HIP(hipStreamSynchronize(E->stream));
    CHS_HIP(hipMemcpy(saved, E->dState, sizeof(DevState), hipMemcpyDeviceToHost));
  }
  *was = saved->halt != 0;
  if (*was) {
    DevState s = *saved;
    s.halt = 0;
    CHS_HIP(hipStreamSynchronize(E->stream));
    CHS_HIP(hipMemcpy(E->dState, &s, sizeof s, hipMemcpyHostToDevice));
  }
  return CHS_OK;
}
int halt_up(Engine* E, const DevState* saved, bool was) {
  if (was) CHS_HIP(hipMemcpy(E->dState, saved, sizeof(DevState), hipMemcpyHostToDevice));
  return CHS_OK;
}

// the coefficients of member E's centred field: direct / chirp MU -> (T1) -> T2, fast MU -> (T2) -> MU
int transform_one(Engine* E) {
  if (chs_natural_engine(E)) return chs_natural_dct2d(E, E->dMU, E->dT2, E->dT1, false);
  return chs_fast_dct2d_fwd_using(E, E->dMU, E->dMU, E->dT2);
}

template <typename T>
int launch_center(const SpecBuf* s, hipStream_t st) {
  const size_t total = (size_t)s->N * s->N;
  constexpr int V = ChsVec<T>::V;
  if (total % V == 0) {
    const size_t threads = total / V;
    k_spec_center<T, V><<<dim3((unsigned)((threads + SPEC_THREADS - 1) / SPEC_THREADS), s->B), SPEC_THREADS, 0, st>>>(s->mem, total);
  } else {
    k_spec_center<T, 1><<<dim3((unsigned)((total + SPEC_THREADS - 1) / SPEC_THREADS), s->B), SPEC_THREADS, 0, st>>>(s->mem, total);
  }
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

template <typename T>
int launch_bins(const SpecBuf* s, hipStream_t st) {
  constexpr int V = ChsVec<T>::V;
  const dim3 grid(s->tx, s->ty, s->B);
  // a read-once sweep: where the step loop's arrays fill the Infinity Cache it must not displace them
  const bool nt = chs_grid_exceeds_cache((size_t)s->N, sizeof(T));
  if (s->N % V == 0) {
    if (nt) k_spec_bins<T, V, true><<<grid, SPEC_THREADS, 0, st>>>(s->mem, s->N, s->part);
    else k_spec_bins<T, V, false><<<grid, SPEC_THREADS, 0, st>>>(s->mem, s->N, s->part);
  } else {
    if (nt) k_spec_bins<T, 1, true><<<grid, SPEC_THREADS, 0, st>>>(s->mem, s->N, s->part);
    else k_spec_bins<T, 1, false><<<grid, SPEC_THREADS, 0, st>>>(s->mem, s->N, s->part);
  }
  CHS_HIP(hipGetLastError());
  k_spec_fin<<<dim3((s->nb + SPEC_THREADS - 1) / SPEC_THREADS, s->B), SPEC_THREADS, 0, st>>>(s->part, s->tile, s->tx * s->ty,
                                                                                          s->nb, s->out);
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

// The look at B members on one stream.  Members of a chirp batch are transformed together (chs_chirp_batch_dct2d,
// on states of this file's own: no member's halt flag or step count is in the way); every other member by its own
// engine's launch, its halt flag taken down for the time.
int spectrum_run(Engine* const* m, int B, hipStream_t st, bool chirp_batch, void** buf, double* ssum) {
  Engine* E0 = m[0];
  int rc;
  if ((rc = spec_buffers(buf, B, E0->N, chirp_batch, st))) return rc;
  SpecBuf* s = (SpecBuf*)*buf;
  std::vector<DevState> saved(chirp_batch ? 0 : (size_t)B);
  std::vector<char> was((size_t)B, 0);
  for (int i = 0; !chirp_batch && i < B; ++i) {
    bool w = false;
    if ((rc = halt_down(m[i], &saved[(size_t)i], &w))) return rc;
    was[(size_t)i] = w;
  }
  auto restore = [&]() {
    int r = CHS_OK;
    for (int i = 0; !chirp_batch && i < B; ++i) {
      const int ri = halt_up(m[i], &saved[(size_t)i], was[(size_t)i] != 0);
      if (ri) r = ri;
    }
    return r;
  };
  std::vector<SpecMember> rec((size_t)B);   // (the records outlive the stream's work: the waits below)
  std::vector<NatMember> nat(chirp_batch ? (size_t)B : 0);
  auto run = [&]() -> int {
    for (int i = 0; i < B; ++i) {
      Engine* E = m[i];
      rec[(size_t)i] = SpecMember{E->dU, E->dMU, chs_natural_engine(E) ? E->dT2 : E->dMU, s->st + i};
      if (chirp_batch) {
        NatMember& r = nat[(size_t)i];
        memset((void*)&r, 0, sizeof r);
        r.dc = E->dc; r.st = s->st + i; r.nsteps = 1;   // (rows_written = 0 < 1 and halt = 0: the member takes part)
        r.arr[NAT_U] = E->dU; r.arr[NAT_MU] = E->dMU; r.arr[NAT_T1] = E->dT1; r.arr[NAT_T2] = E->dT2; r.arr[NAT_HAT] = E->dHat;
      }
    }
    CHS_HIP(hipMemcpyAsync(s->mem, rec.data(), sizeof(SpecMember) * (size_t)B, hipMemcpyHostToDevice, st));
    if (chirp_batch) CHS_HIP(hipMemcpyAsync(s->nat, nat.data(), sizeof(NatMember) * (size_t)B, hipMemcpyHostToDevice, st));
    CHS_HIP(hipEventRecord(s->ev[0], st));
    int r;
    for (int i = 0; i < B; ++i)
      if ((r = chs_launch_sum_to(m[i], s->st + i))) return r;
    if ((r = E0->dtype == CHS_F64 ? launch_center<double>(s, st) : launch_center<float>(s, st))) return r;
    CHS_HIP(hipEventRecord(s->ev[1], st));
    if (chirp_batch) {
      if ((r = chs_chirp_batch_dct2d(E0, st, s->nat, B, NAT_MU, NAT_T2, NAT_T1, false))) return r;
    } else {
      for (int i = 0; i < B; ++i)
        if ((r = transform_one(m[i]))) return r;
    }
    CHS_HIP(hipEventRecord(s->ev[2], st));
    if ((r = E0->dtype == CHS_F64 ? launch_bins<double>(s, st) : launch_bins<float>(s, st))) return r;
    CHS_HIP(hipEventRecord(s->ev[3], st));
    CHS_HIP(hipMemcpyAsync(s->hOut, s->out, sizeof(double) * (size_t)B * s->nb, hipMemcpyDeviceToHost, st));
    CHS_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) {
      float ms = 0.f;
      CHS_HIP(hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
      s->ms[k] = ms;
    }
    memcpy(ssum, s->hOut, sizeof(double) * (size_t)B * s->nb);
    return CHS_OK;
  };
  rc = run();
  if (rc) hipStreamSynchronize(st);   // nothing of this call is in flight when the states go back
  const int rr = restore();
  return rc ? rc : rr;
}
}  // namespace

void chs_spectrum_free(void** buf) {
  if (!buf) return;
  spec_release((SpecBuf*)*buf);
  *buf = nullptr;
}

void chs_spectrum_forget(void* buf) {
  if (!buf) return;
  SpecBuf* s = (SpecBuf*)buf;
  s->ms[0] = s->ms[1] = s->ms[2] = -1.0;
}

int chs_spectrum_one(Engine* E, double* ssum, int32_t nbins, const char* who) {
  int rc;
  if ((rc = check_args(E, ssum, nbins, who))) return rc;
  if (!E->have_U) { chs_set_error(std::string(who) + ": no field (chs_set_U / chs_init_U_pcg64 first)"); return CHS_ESTATE; }
  CHS_HIP(hipSetDevice(E->hc.device));
  Engine* one[1] = {E};
  return spectrum_run(one, 1, E->stream, false, &E->spec, ssum);
}

int chs_spectrum_all(Engine* const* m, int B, hipStream_t s, bool chirp, void** buf, double* ssum, int32_t nbins, const char* who) {
  int rc;
  if ((rc = check_args(m[0], ssum, nbins, who))) return rc;
  for (int i = 0; i < B; ++i)
    if (!m[i]->have_U) { chs_set_error(std::string(who) + ": member " + std::to_string(i) + " has no field"); return CHS_ESTATE; }
  CHS_HIP(hipSetDevice(m[0]->hc.device));
  return spectrum_run(m, B, s, chirp, buf, ssum);
}

extern "C" int chs_structure_factor(chs_handle h, double* ssum, int32_t nbins) {
  Engine* E = (Engine*)h;
  if (!E) { chs_set_error("chs_structure_factor: null handle"); return CHS_EINVAL; }
  return chs_spectrum_one(E, ssum, nbins, "chs_structure_factor");
}

extern "C" int chs_structure_factor_last_ms(chs_handle h, double ms[3]) {
  Engine* E = (Engine*)h;
  if (!E || !ms) { chs_set_error("chs_structure_factor_last_ms: null argument"); return CHS_EINVAL; }
  const SpecBuf* s = (const SpecBuf*)E->spec;
  if (!s || s->ms[0] < 0.0) { chs_set_error("chs_structure_factor_last_ms: no chs_structure_factor call so far"); return CHS_ESTATE; }
  for (int k = 0; k < 3; ++k) ms[k] = s->ms[k];
  return CHS_OK;
}
