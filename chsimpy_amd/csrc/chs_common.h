// chs_common.h -- internal declarations shared by the HIP translation units.
// gfx950 (MI355X) only: 64-wide wavefronts are assumed throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "chs_hip.h"
#include "chs_step_host.h"

#define CHS_WAVE 64

// Cache policy of the step loop: T and hat_U together against the 256 MiB Infinity Cache of an
// MI355X.  Where they exceed it, what is touched once per step (hat_U, the partial rows of the adaptive step) is moved
// with non-temporal accesses and T, which both kernels read and write, keeps the cache.
__host__ __device__ constexpr bool chs_grid_exceeds_cache(size_t N, size_t elem_bytes) {
  return 2 * N * N * elem_bytes > ((size_t)256 << 20);
}

// ---------------------------------------------------------------------------
// Device-resident scalar state of one simulation: what chsimpy/solver.py keeps
// in `self.*` / `self.solution.*` between iterations, plus the reduction
// results handed from one kernel of a step to the next.
// ---------------------------------------------------------------------------
struct DevState {
  double delt;            // solver.py:54,185-188
  double time_delta_sum;  // solver.py:51,195
  double time_passed;     // solver.py:52,196
  double tau0, t0;        // solver.py:243-244
  double E2_0, E2_prev;   // timedata.py:63 operands
  double L2_cur;          // ||EnergieEut||_F / N^2 of the running step (solver.py:225)
  double meanU;           // mean of the field the next statistics sweep refers to (solver.py:223)
  double lam1, lam2;      // utils.py:41-42 for delt_coef
  double delt_coef;       // the delt the coefficient grids CHeig/Seig stand for: params.delt from the entry of
                          // every solve_or_resume call (solver.py:154-155 reloads solution.Seig/CHeig, which
                          // solution.py:52-55 built once) until the adaptive step regenerates them (189-193)
  long long computed_steps;  // solver.py:134,240
  long long rows_written;    // rows produced by the running chs_step_n call
  int skip_check;            // solver.py:50,249
  int stop_reason;           // CHS_STOP_*
  int nan_flag;              // timedata.py:10
  int halt;                  // != 0: every later kernel of the call is a no-op
  // Gated tail (chs_fast.hip, k_col<MODE_STEP>): the sequence number of the last bookkeeping that rode in
  // a k_col as its extra workgroup and has been published (agent-scope release); the other workgroups of
  // that launch wait for it in front of their spectral stage.  gate_timeout: a wait gave up (never seen).
  unsigned long long decided;
  int gate_timeout;
  int colmin_ticket;      // arrivals of k_colmin_slices' blocks when the last of them decides the coming step's coefficients
};

// Read-only scalars, passed to kernels by value.
struct DevConsts {
  int N;
  int adaptive_time;
  int full_sim;
  int pad_;
  double RT, BRT, B, A0, A1, Amr, kappa_tilde, L, delx, delx2;
  double delt0;  // params.delt (lower bound of the adaptive step, solver.py:184)
  double delt_max, M_tilde, threshold, time_limit_s;
  double invN2;  // 1/N^2
};

// ---------------------------------------------------------------------------
// Deterministic block reductions (fixed tree: DPP/shuffle inside a wave, LDS
// across waves).  Callers pass a __shared__ scratch of >= 32 doubles.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  return v;
}
// Returns the block total in every thread.  All threads of the block must call.
__device__ __forceinline__ double block_sum(double v, double* scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nw; ++w) t += scratch[w];
  return t;
}
__device__ __forceinline__ double block_min(double v, double* scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  v = wave_min(v);
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double t = scratch[0];
  for (int w = 1; w < nw; ++w) t = fmin(t, scratch[w]);
  return t;
}

// Wavefront and lane number WITHOUT keeping threadIdx.x alive in a VGPR across a register-heavy kernel.  A kernel at its
// register limit spills such a long-lived index, and a 4-byte spill reload sits in the in-order vmcnt queue behind every
// store issued before it.  The wavefront's number goes to an SGPR once; the lane number is two v_mbcnt wherever it is
// needed (volatile: never carried from one use to the next either).  One-dimensional blocks of whole wavefronts only.
__device__ __forceinline__ int chs_wave_id() {
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  __builtin_assume(w >= 0 && w < 16);   // (what is derived from it stays unsigned 32-bit offset arithmetic)
  return w;
}
__device__ __forceinline__ int chs_lane_id() {
  int x;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(x));
  __builtin_assume(x >= 0 && x < 64);
  return x;
}
// wave_sum with the lane number taken afresh: __shfl_down computes its own lane number with a pure builtin, which the
// compiler hoists out of loops and keeps (or spills) like any other loop invariant.  Same tree, same sums in lane 0.
__device__ __forceinline__ double wave_sum_fresh(double v) {
  const int ln = chs_lane_id();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int src = ((ln + off) & 63) << 2;
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(src, (int)(b & 0xffffffffll));
    const int hi = __builtin_amdgcn_ds_bpermute(src, (int)(b >> 32));
    v += __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  }
  return v;  // valid in lane 0
}
// block_sum with the caller's wavefront number (SGPR) instead of threadIdx.x
__device__ __forceinline__ double block_sum_w(double v, double* scratch, int wave, int nw) {
  v = wave_sum_fresh(v);
  __syncthreads();
  if (chs_lane_id() == 0) scratch[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nw; ++w) t += scratch[w];
  return t;
}
// block_sum_store in two halves: `begin` right where the values are complete (wavefront sums into `red`: no register
// holds them any longer -- in the fused row kernel that is five accumulators less across the whole forward transform),
// `end` behind a barrier at the end of the kernel (wavefront 0's lane 0 adds up and gets out[]; returns true there).
template <int NV, bool FRESH = true>
__device__ __forceinline__ void block_reduce_begin(const double (&v)[NV], double* red /* >= NW*NV */, int wave) {
  double w[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) w[i] = FRESH ? wave_sum_fresh(v[i]) : wave_sum(v[i]);
  if (chs_lane_id() == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[wave * NV + i] = w[i];
  }
}
template <int NV, int NW>
__device__ __forceinline__ bool block_reduce_end(const double* red, double* __restrict__ out, int wave) {
  __syncthreads();
  const bool first = (wave == 0) && (chs_lane_id() == 0);
  if (first) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double t = red[i];
#pragma unroll
      for (int w = 1; w < NW; ++w) t += red[w * NV + i];
      out[i] = t;
    }
  }
  return first;
}

// NV per-thread values -> block totals (NW waves per block), left in out[0..NV) of thread 0.
// One barrier, no loops with run-time trip counts: meant for the END of a register-heavy
// kernel, where control flow around live register arrays would cost spills.
template <int NV, int NW>
__device__ __forceinline__ void block_sum_store(const double (&v)[NV], double* red /* >= NW*NV */,
                                                double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double w[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) w[i] = wave_sum(v[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[wave * NV + i] = w[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double t = red[i];
#pragma unroll
      for (int w = 1; w < NW; ++w) t += red[w * NV + i];
      out[i] = t;
    }
  }
}

// ---------------------------------------------------------------------------
// Host-side engine object behind chs_handle.
// ---------------------------------------------------------------------------
struct Engine;

// Per-step kernel slots for chs_profile_steps / chs_kernel_name.
struct StepTimer {
  bool on = false;
  double ms[CHS_NKERNELS];
  long long calls[CHS_NKERNELS];
  struct Span { int slot; hipEvent_t a, b; };
  std::vector<Span> pending;     // recorded, not yet harvested
  std::vector<hipEvent_t> pool;  // free events
  hipEvent_t cur = nullptr;      // start event of the open span
};

// The partial sums a step leaves for its record and for the time-step control of the next step.
struct PartialSums {
  double* diag = nullptr;  // per-block [sE, sG, sPS, cSA]
  double* mu = nullptr;    // per-block sum(mu^2)
  double* e2 = nullptr;    // per-column-tile spectral gradient sums (fast engine)
  double* ra = nullptr;    // Ra of the step, written by the row kernel (fast engine)
};

#define CHS_STAGE_BYTES (8u << 20)
struct Engine {
  // two pinned staging chunks of this handle for field up/downloads (allocated at the first transfer)
  void* stageBuf[2] = {nullptr, nullptr};
  hipEvent_t stageEv[2] = {nullptr, nullptr};
  chs_consts hc;       // as given
  DevConsts dc;        // device view
  int engine = 0;      // resolved CHS_ENGINE_*
  int N = 0;
  int dtype = CHS_F64;
  size_t esz = 8;
  hipStream_t stream = nullptr;
  bool prepared = false;
  bool have_U = false;
  bool hat_valid = false;  // dHat matches dU's history (CHS_STEP_CARRY_HAT)
  bool resident = false;   // ... and T1 / partMu hold the row transform of EnergieEut(U) and its sum of squares: the
                           // next call continues without an entry pass (the last fused step left them, chs_fast_step)
  bool lamByColmin = true;    // CHS_LAM_BY_COLMIN (chs_fast_rearm): the reduction's last block sets the coming step's coefficients
  bool gateEarly = false;     // CHS_GATE_EARLY=1 (chs_fast_rearm): experiment, measured equal
  bool adaptSparse = true;    // CHS_ADAPT_SPARSE (chs_fast_rearm)
  long long csHost = -1;      // the device's computed_steps as the host can follow it (prepare / set_state / end of a call, +1 per
                              // issued step): lets the adaptive path issue the step-size machinery only on the steps whose rule
                              // fires (chs_fast_step); -1 = not known
  bool stateCached = false;   // hState[0] is the device state as the last call left it (chs_get_state without a round trip)

  // device buffers (element type per dtype)
  void* dU = nullptr;      // field U, row-major N x N
  void* dMU = nullptr;     // EnergieEut (direct engine) / scratch
  void* dT1 = nullptr;     // transform scratch
  void* dT2 = nullptr;     // transform scratch
  void* dHat = nullptr;    // hat_U (direct: natural order; fast: engine-native order)
  void* dHat2 = nullptr;   // second hat_U buffer of the small grids' stop-rule runs (chs_fast_step), allocated on demand
  void* dNoise = nullptr;  // jitter noise (optional)
  double jitter = 0.0;
  double* dLambda = nullptr;   // lam_i, N doubles
  void* dD = nullptr;          // direct engine: orthonormal DCT-II matrix D[k][n]
  void* dTw = nullptr;         // fast engine: twiddle tables
  void* chirp = nullptr;       // chirp engine: its plan and tables (chs_chirp.hip)
  void* spec = nullptr;        // structure factor: partial bins, result, events (chs_spectrum.hip), at the first call
  void* morph = nullptr;       // morphology: tile partials, result, events (chs_morphology.hip), at the first look
  void* cc = nullptr;          // connected components: labels, numbers, table, result, events (chs_components.hip), at the first look
  void* dt = nullptr;          // distance transform: band masks, carries, D2, histogram, result, events (chs_distance.hip), at the first look
  void* ch = nullptr;          // chord lengths: bit planes, histograms, result, events (chs_chords.hip), at the first look
  void* cmp = nullptr;         // composition: partial slots, histogram, select tables, result, events (chs_composition.hip), at the first look
  void* tp = nullptr;          // two-point correlation: bit plane, pair counts, result, events (chs_two_point.hip), at the first look
  void* ct = nullptr;          // contour: slots, histograms, map, result, events (chs_contour.hip), at the first look
  void* sh = nullptr;          // droplet shapes: table, result, events (chs_shapes.hip), at the first look
  DevState* dState = nullptr;
  double* dRows = nullptr;     // timedata rows of the running call
  long long rowsCap = 0;
  double* dPartCol = nullptr;  // per-band column sums for the adaptive step
  double* dPartColMin = nullptr;
  double* dPartSum = nullptr;  // per-block sum(U)
  double* dSinSq = nullptr;    // sin^2(pi k/N), k = 0..N-1 (fast engine)
  int nPartE2 = 0;
  int nRowBlocks = 0;          // workgroups of the fast row kernels (diag partials)
  int nBands = 0;              // row bands used by the pointwise kernels
  int nPartMu = 0;             // number of sum(mu^2) partials the running engine produces
  double* dPartMuAux = nullptr; // scratch partials of the column-sum-only sweep
  int nDiagBlocks = 0;
  int nColMinBlocks = 0;
  int nColMinCur = 0;  // entries of dPartColMin the last column-sum launch wrote

  // The partial sums.  The natural engines have set 0 alone (chs_pointwise_alloc).  The fast engine has two
  // (chs_fast_init): the bookkeeping of step s rides as one extra workgroup in k_col of step s+1, and the sums
  // ping-pong between the sets so that step s+1 does not overwrite what that workgroup reads.  Both are freed by
  // chs_pointwise_free.
  PartialSums part[2];
  int parity = 0;             // the set the running step writes; always 0 without the second set
  // Every kernel launched outside a riding tail takes its partial sums from here.  `parity` flips only behind a step
  // whose tail rides (chs_fast_step), and the next thing to touch the sums is then the next step of the same call: a
  // call's last step runs its tail at once (StepIssue::tail_now) and never flips.  So everything between two calls
  // -- prepare's k_diag / k_fin pair, the entry of the next call, the batch's call_enter behind chs_fast_enter_fused
  // -- sees the set that the last step wrote; a call that a stop cut short leaves nothing in either set that is
  // read again (Engine::resident is off then).
  PartialSums& sums() { return part[parity]; }
  const PartialSums& sums() const { return part[parity]; }
  PendingTail pending;        // the tail of the previous step of the running call, where it is still to run (chs_fast_step)
  unsigned long long gateSeq = 0;
  bool testGateWithhold = false;  // test hook (CHS_TEST_GATE_WITHHOLD=1, read by chs_step_n in builds with -DCHS_TEST_HOOKS=1): gated tails never publish
  unsigned stepCount = 0;     // k_col<MODE_STEP> launches so far (tile walk direction alternates)
  // jitter noise generated on the device: numpy's PCG64 stream continued from the host generator's state
  bool jitterPcg = false;
  unsigned long long pcgState[2] = {0, 0}, pcgInc[2] = {0, 0};  // {hi, lo}
  bool adaptOk = false;       // the configuration has the fused adaptive row kernel
  bool fusedAdapt = false;    // the fused row kernel adds up the adaptive-step integrand itself
  void* dPartColRows = nullptr;    // [nRowBlocks][N] partial column sums of that integrand, in the engine's element type
  double* dColSlices = nullptr;    // [CS_SLICES][N] first stage of their reduction (chs_launch_colmin_rows)
  hipEvent_t evA = nullptr, evB = nullptr;
  // pinned host mirror of the device state: slot 0 = the state at the end of a call, slots 1..4 = the
  // polls behind the batches of a long call (run_steps)
  DevState* hState = nullptr;
  double* hRows = nullptr;    // pinned staging of the rows of a short call
  hipEvent_t evPoll[4] = {nullptr, nullptr, nullptr, nullptr};
  int batchSteps = 1024;      // steps issued between two looks at the device's halt flag (run_steps)
  double lastStepMs = 0.0;
  StepTimer timer;
  std::vector<double> hLambda;  // the eigenvalue table the engine was created with (engine pool: chs_create)
  void* tr = nullptr;          // droplet tracking: the frame, hash table, rows, events (chs_track.hip), at the first track look
  void* th = nullptr;          // local thickness: map, centre list, histogram, result, events (chs_thickness.hip), at the first look
  void* geo = nullptr;         // geodesic look: map, tile flags, histogram, profile, result, events (chs_geodesic.hip), at the first look
  void* sk = nullptr;          // skeleton look: two bit planes, histogram, counters, result, events (chs_skeleton.hip), at the first look
  void* trn = nullptr;         // transport look: pixel bytes, the vectors of the iteration, tile list, profile, result, events (chs_transport.hip), at the first look
};

void chs_set_error(const std::string& s);
int chs_hip_fail(hipError_t e, const char* what, const char* file, int line);

#define CHS_HIP(call)                                                    \
  do {                                                                   \
    hipError_t e__ = (call);                                             \
    if (e__ != hipSuccess) return chs_hip_fail(e__, #call, __FILE__, __LINE__); \
  } while (0)

// kernel-slot bracket used by the launchers
void chs_slot_begin(Engine* E, int slot);
void chs_slot_end(Engine* E, int slot);

// slots
enum {
  SLOT_MU = 0,      // direct: pointwise EnergieEut           | fast: row pass forward (mu + DCT-II rows)
  SLOT_PRE = 1,     // k_pre (+ the column-sum minimum): L2, adaptive dt, time bookkeeping
  SLOT_FWD = 2,     // direct: the two forward products       | fast: (unused)
  SLOT_SPEC = 3,    // direct: spectral update                | fast: column pass (DCT-II, update, DCT-III)
  SLOT_INV = 4,     // direct: the two inverse products       | fast: row pass inverse (DCT-III rows)
  SLOT_DIAG = 5,    // energy / statistics sweep
  SLOT_FIN = 6,     // k_fin: timedata row, stop rule
  SLOT_MISC = 7
};

// ---- pointwise / reduction launchers (chs_pointwise.hip) -------------------
int chs_launch_mu(Engine* E);                 // dU -> dMU, partials
int chs_launch_mu_colsums(Engine* E, int cs_offset);
int chs_fast_rearm(Engine* E);
int chs_launch_colmin_rows(Engine* E, int cs_offset, bool decide = false);  // min over the columns of sum(dPartColRows)  // dU -> column-sum minimum of the adaptive-step integrand only
struct TailArgs;
struct BatchMember;
// the batch's column-minimum reduction: the members' partial rows (chs_fast_kernels.h: k_row_inv<ADAPT>) -> partColMin
int chs_colmin_batch_buffers(Engine* E, BatchMember* r);
int chs_launch_colmin_rows_batch(hipStream_t s, const BatchMember* mem, int B, int N, bool rows_f32);
TailArgs chs_tail_args(const Engine* E, const PartialSums& sums, int do_pre);
int chs_launch_step_tail(Engine* E, int do_pre);  // fused pipeline: record of step s + time-step control of step s+1
int chs_launch_pre(Engine* E);                // partials -> state (L2, delt, time)
int chs_launch_call_begin(Engine* E);         // entry of a solve_or_resume call: re-arm the loop, coefficients of params.delt
int chs_launch_spectral(Engine* E, const void* hmu);  // dHat <- (dHat + Seig*hmu)/CHeig (natural order)
int chs_launch_sum(Engine* E, int ignore_halt);  // meanU <- mean(dU)
int chs_launch_sum_to(Engine* E, DevState* st);  // st->meanU <- mean(dU) for a state of the caller's, whatever E's halt flag
int chs_launch_diag(Engine* E, int ignore_halt);  // dU -> diag partials
int chs_launch_fin(Engine* E, int prepare_mode, int fused = 0);
int chs_launch_jitter(Engine* E);
int chs_launch_jitter_pcg(Engine* E);
int chs_launch_init_pcg(Engine* E, double base, double scale, const unsigned long long state[2], const unsigned long long inc[2]);  // U += jitter*(2*r-1), r from the PCG64 stream; advances E->pcgState by N*N
int chs_pointwise_alloc(Engine* E);
void chs_pointwise_free(Engine* E);

// ---- direct engine (chs_direct.hip) ----------------------------------------
int chs_direct_init(Engine* E);
void chs_direct_free(Engine* E);
int chs_direct_dct2d(Engine* E, const void* in, void* out, void* tmp, bool inverse);

// ---- chirp engine (chs_chirp.hip) -------------------------------------------
bool chs_chirp_supported(int N);
int chs_chirp_init(Engine* E);
void chs_chirp_free(Engine* E);
int chs_chirp_dct2d(Engine* E, const void* in, void* out, void* tmp, bool inverse);

// can the energy rule or the time limit end the run; does the run perturb U between the inverse transform and the
// record (solver.py:210-211: no fusion across the perturbation)
inline bool chs_stop_armed(const Engine* E) { return stop_armed(E->dc.full_sim != 0, E->dc.time_limit_s); }
inline bool chs_jitter_on(const Engine* E) { return (E->dNoise || E->jitterPcg) && E->jitter > 0.0 && E->jitter < 0.1; }

// The direct and the chirp engine are one family: natural order in every array, the unfused step of chs_api.hip
// (one_step); they differ in dct2d alone.
inline bool chs_natural_engine(const Engine* E) { return E->engine == CHS_ENGINE_DIRECT || E->engine == CHS_ENGINE_CHIRP; }
inline int chs_natural_dct2d(Engine* E, const void* in, void* out, void* tmp, bool inverse) {
  return E->engine == CHS_ENGINE_CHIRP ? chs_chirp_dct2d(E, in, out, tmp, inverse) : chs_direct_dct2d(E, in, out, tmp, inverse);
}

// ---- fast engine (chs_fast.hip) ---------------------------------------------
bool chs_fast_supported(int N, int dtype);
int chs_fast_recover_u(Engine* E);  // U <- idctn(hat_U): the field of the last completed step
// (chs_api.hip, shared by chs_step_n and the batch) a call that the energy rule or the time limit ended before its last
// step: the test (stored_u: the row kernel wrote the field on every step, nothing to rebuild), and the rebuild of the
// field through chs_fast_recover_u around the fetched state s
bool chs_stopped_short(const DevState& s, int64_t nsteps, bool stored_u);
int chs_rebuild_stopped_u(Engine* E, const DevState& s);
int chs_copy_rows_out(Engine* E, double* rows, int64_t from, int64_t to);  // rows [from, to) of the ring -> rows[from*9 ...]
int chs_fast_init(Engine* E);
void chs_fast_free(Engine* E);
int chs_fast_dct2d(Engine* E, const void* in, void* out, bool inverse);  // natural in/out (tests)
// out <- dctn(in), natural order, the row pass into `tmp` instead of T1: neither T1 nor hat_U is touched (out may be in)
int chs_fast_dct2d_fwd_using(Engine* E, const void* in, void* out, void* tmp);
int chs_fast_enter(Engine* E);   // hat_U <- dctn(U) in engine-native order (solver.py:159)
int chs_fast_enter_fused(Engine* E);       // both of them with one sweep of U
int chs_fast_enter_hat(Engine* E);         // hat_U <- dctn(U) alone: the first step's operand T1 is still on the device
int chs_fast_prologue(Engine* E);          // T1 <- row DCT of EnergieEut(U) for the first step of a call
int chs_fast_step(Engine* E, const StepMode& mode, bool first, bool last); // [k_pre,] k_col, fused row kernel, k_step_tail: step_issue
int chs_fast_step_unfused(Engine* E);      // jitter path: every kernel separate, U complete in HBM

// ---- structure factor (chs_spectrum.hip) -------------------------------------
// Radially binned power of dctn(U - mean(U)) from the arrays that are dead between two calls.
int chs_spectrum_one(Engine* E, double* ssum, int32_t nbins, const char* who);
// all members of a batch (one stream `s`, one N and element type): sweep and binning launched once for all of them;
// *buf is the batch's own buffer set, allocated here at the first call and freed by chs_spectrum_free
int chs_spectrum_all(Engine* const* m, int B, hipStream_t s, bool chirp, void** buf, double* ssum, int32_t nbins, const char* who);
void chs_spectrum_free(void** buf);
void chs_spectrum_forget(void* buf);   // the buffers stay, the times of the last call go

// ---- morphology (chs_morphology.hip) ------------------------------------------
// Bit-quad counts of the thresholded field: out[CHS_MORPH_WORDS] of one handle at *threshold ...
int chs_morph_one(Engine* E, const double* threshold, int64_t* out, const char* who);
// ... and out[B][CHS_MORPH_WORDS] of all members of a batch (one stream `s`, one N and element type) at threshold[B], one
// launch pair; *buf is the batch's own buffer set, allocated here at the first look and freed by chs_morph_free
int chs_morph_all(Engine* const* m, int B, hipStream_t s, void** buf, const double* threshold, int64_t* out, const char* who);
void chs_morph_free(void** buf);
void chs_morph_forget(void* buf);   // the buffers stay, the time of the last look goes

// ---- connected components (chs_components.hip) ---------------------------------
// The components of E's field thresholded at `threshold` on stream `s` with the buffer set *buf
// (the handle's own, or the batch's one set for whichever member it looks at), allocated here at the first look:
// out[CHS_CC_WORDS].  Table and labels of the last look of a buffer set: chs_cc_table, chs_cc_labels.
int chs_cc_look(Engine* E, hipStream_t s, void** buf, double threshold, int32_t connectivity, int32_t side, int64_t* out,
                const char* who);
int chs_cc_table(void* buf, int device, hipStream_t s, int64_t rows, int32_t* out, const char* who);
int chs_cc_labels(void* buf, int device, hipStream_t s, int32_t* out, const char* who);
void chs_cc_free(void** buf);
void chs_cc_forget(void* buf);   // the buffers stay, the last look goes
// What the last look of a buffer set left on the device, for a look that builds on it (chs_shapes.hip): the root label of
// every pixel, the number at every root, the table and its row count.  Read-only; CHS_ESTATE without a look.
struct ChsCcSnapshot {
  const int* L = nullptr;       // [N * N] the root's linear index, -1 for background
  const int* id = nullptr;      // [N * N] at a root: its component number
  const int* table = nullptr;   // [count][CHS_CC_COLS]
  int64_t count = 0;
  double ms = 0.0;              // the look's device time
};
int chs_cc_snapshot(const void* buf, ChsCcSnapshot* out, const char* who);

// ---- geodesic look (chs_geodesic.hip) ------------------------------------------
// The geodesic map of E's field thresholded at `threshold` from the wall `source` on stream `s`: a
// components look with the buffer set *ccbuf first (it stays that look's snapshot), then the relaxation rounds and the
// statistics with the buffer set *buf, both allocated here at the first look: out[CHS_GEO_WORDS].  max_rounds: 0 for
// chs_geodesic_rounds_default(N); a look that needs more returns CHS_ELIMIT and leaves no geodesic result.  Histogram,
// profile and map of the last look of a buffer set: chs_geo_hist, chs_geo_profile, chs_geo_map.
int chs_geo_look(Engine* E, hipStream_t s, void** ccbuf, void** buf, double threshold, int32_t connectivity, int32_t side,
                 int32_t source, int64_t max_rounds, int64_t* out, const char* who);
int chs_geo_hist(void* buf, int device, hipStream_t s, int32_t nbins, int64_t* out, const char* who);
int chs_geo_profile(void* buf, int device, hipStream_t s, int64_t* out, const char* who);
int chs_geo_map(void* buf, int device, hipStream_t s, int32_t* out, const char* who);
int chs_geo_last_ms(const void* h, const void* buf, double* ms, const char* what);
int chs_geo_relax_ms(const void* h, const void* buf, double* ms, const char* what);   // the rounds alone
void chs_geo_free(void** buf);
void chs_geo_forget(void* buf);   // the buffers stay, the last look goes

// ---- droplet shapes (chs_shapes.hip) -------------------------------------------
// The shape table of E's field thresholded at `threshold` on stream `s`: a components look with
// the buffer set *ccbuf first (it stays that look's snapshot), then the sweep with the buffer set *buf, both allocated
// here at the first look: out[CHS_SH_WORDS].  The table of the last look of a buffer set: chs_sh_table.
int chs_sh_look(Engine* E, hipStream_t s, void** ccbuf, void** buf, double threshold, int32_t connectivity, int32_t side,
                int64_t* out, const char* who);
int chs_sh_table(void* buf, int device, hipStream_t s, int64_t rows, int64_t* out, const char* who);
int chs_sh_last_ms(const void* h, const void* buf, double* ms, const char* what);
void chs_sh_free(void** buf);
void chs_sh_forget(void* buf);   // the buffers stay, the last look goes

// ---- droplet tracking (chs_track.hip) -------------------------------------------
// The pair table of E's field thresholded at `threshold` against the frame an earlier track look kept (DESIGN.md section
// 3l) on stream `s`: a shapes look with *ccbuf and *shbuf first (they stay that look's snapshot), then the overlap.
// *frame holds the frame -- the handle's own, in a batch the member's -- and *work the hash table, the row list and the
// last look's rows -- the same set for a single handle, the batch's one set otherwise; both are allocated here at the
// first look: out[CHS_TR_WORDS].  The rows of the last look of a working set: chs_tr_pairs.
int chs_tr_look(Engine* E, hipStream_t s, void** ccbuf, void** shbuf, void** frame, void** work, double threshold,
                int32_t connectivity, int32_t side, int32_t keep, int64_t* out, const char* who);
int chs_tr_pairs(void* work, int64_t rows, int64_t* out, const char* who);
void chs_tr_reset(void* frame);   // the frame goes; the buffers, the last pair table and the last time stay
void chs_tr_free(void** buf);
void chs_tr_forget(void* buf);    // the buffers stay, the frame and the last look go

// ---- distance transform (chs_distance.hip) -----------------------------------
// The squared distances of E's field thresholded at `threshold` on stream `s` with the buffer set
// *buf (the handle's own, or the batch's one set), allocated here at the first look: out[CHS_DT_WORDS].  Histogram and
// map of the last look of a buffer set: chs_dt_hist, chs_dt_map.
int chs_dt_look(Engine* E, hipStream_t s, void** buf, double threshold, int32_t side, int64_t* out, const char* who);
int chs_dt_hist(void* buf, int device, hipStream_t s, int32_t nbins, int64_t* out, const char* who);
int chs_dt_map(void* buf, int device, hipStream_t s, int32_t* out, const char* who);
void chs_dt_free(void** buf);
void chs_dt_forget(void* buf);   // the buffers stay, the last look goes
// What the last look of a buffer set left on the device, for a look that builds on it (chs_thickness.hip): the squared
// distances and the look's device time.  Read-only; CHS_ESTATE without a look.
struct ChsDtSnapshot {
  const int* D2 = nullptr;      // [N * N]
  double ms = 0.0;
};
int chs_dt_snapshot(const void* buf, ChsDtSnapshot* out, const char* who);

// ---- local thickness (chs_thickness.hip) ---------------------------------------
// The local thickness of E's field thresholded at `threshold` on stream `s`: a distance look with
// the buffer set *dtbuf first (it stays that look's snapshot), then the selection of the centres, the painting of their
// discs and the statistics with the buffer set *buf, both allocated here at the first look: out[CHS_TH_WORDS].  max_work:
// 0 for chs_thickness_work_default(N); a look that needs more returns CHS_ELIMIT and leaves no thickness result.
// Histogram and map of the last look of a buffer set: chs_th_hist, chs_th_map.
int chs_th_look(Engine* E, hipStream_t s, void** dtbuf, void** buf, double threshold, int32_t side, int64_t max_work,
                int64_t* out, const char* who);
int chs_th_hist(void* buf, int device, hipStream_t s, int32_t nbins, int64_t* out, const char* who);
int chs_th_map(void* buf, int device, hipStream_t s, int32_t* out, const char* who);
int chs_th_last_ms(const void* h, const void* buf, double* ms, const char* what);
void chs_th_free(void** buf);
void chs_th_forget(void* buf);   // the buffers stay, the last look goes

// ---- skeleton look (chs_skeleton.hip) -------------------------------------------
// The skeleton of a phase of E's field thresholded at `threshold` on stream `s`: a distance look
// with the buffer set *dtbuf first (it stays that look's snapshot), then the bit plane of D2 > 0, its thinning to the fixed
// point and the statistics with the buffer set *buf, both allocated here at the first look: out[CHS_SK_WORDS].
// max_subiters: 0 for chs_skeleton_subiters_default(N); a look that needs more returns CHS_ELIMIT and leaves no skeleton
// result.  Histogram and packed plane of the last look of a buffer set: chs_sk_hist, chs_sk_plane.
int chs_sk_look(Engine* E, hipStream_t s, void** dtbuf, void** buf, double threshold, int32_t side, int64_t max_subiters,
                int64_t* out, const char* who);
int chs_sk_hist(void* buf, int device, hipStream_t s, int32_t nbins, int64_t* out, const char* who);
int chs_sk_plane(void* buf, int device, hipStream_t s, uint64_t* out, const char* who);
int chs_sk_last_ms(const void* h, const void* buf, double* ms, const char* what);
int chs_sk_thin_ms(const void* h, const void* buf, double* ms, const char* what);   // the sub-iterations alone
void chs_sk_free(void** buf);
void chs_sk_forget(void* buf);   // the buffers stay, the last look goes

// ---- transport look (chs_transport.hip) -----------------------------------------
// The steady diffusion problem through the spanning components of a phase of E's field thresholded at `threshold`, from
// the wall `source` to the opposite one on stream `s`: a components look at connectivity 4 with the
// buffer set *ccbuf first (it stays that look's snapshot), then setup, conjugate-gradient iterations and closing sweep with
// the buffer set *buf, both allocated here at the first look: words[CHS_TRN_WORDS], vals[CHS_TRN_VALS].  max_iters: 0 for
// chs_transport_iters_default(N); a solve that is not accepted by then returns CHS_ELIMIT and leaves no transport result.
// Profile and map of the last look of a buffer set: chs_trn_profile, chs_trn_map.
int chs_trn_look(Engine* E, hipStream_t s, void** ccbuf, void** buf, double threshold, int32_t side, int32_t source, double tol,
                 int64_t max_iters, int64_t* words, double* vals, const char* who);
int chs_trn_profile(void* buf, int device, hipStream_t s, double* out, const char* who);
int chs_trn_map(void* buf, int device, hipStream_t s, double* out, const char* who);
int chs_trn_last_ms(const void* h, const void* buf, double* ms, const char* what);
int chs_trn_solve_ms(const void* h, const void* buf, double* ms, const char* what);   // iterations and closing sweeps alone
void chs_trn_free(void** buf);
void chs_trn_forget(void* buf);   // the buffers stay, the last look goes

// ---- chord lengths (chs_chords.hip) -------------------------------------------
// The chord lengths of both phases of E's field thresholded at `threshold`, along rows and columns (DESIGN.md section
// 3f), on stream `s` with the buffer set *buf (the handle's own, or the batch's one set), allocated here at the first
// look: out[CHS_CH_WORDS].  The histograms of the last look of a buffer set: chs_ch_hist.
int chs_ch_look(Engine* E, hipStream_t s, void** buf, double threshold, int64_t* out, const char* who);
int chs_ch_hist(void* buf, int device, hipStream_t s, int32_t nbins, int64_t* out, const char* who);
void chs_ch_free(void** buf);
void chs_ch_forget(void* buf);   // the buffers stay, the last look goes

// ---- composition (chs_composition.hip) ----------------------------------------
// Range, sums, histogram and central moments of the values of E's field on stream `s` with the
// buffer set *buf (the handle's own, or the batch's one set), allocated here at the first look: iw[CHS_CMP_IWORDS],
// fw[CHS_CMP_FWORDS].  The histogram of the last look of a buffer set: chs_cmp_hist.  chs_cmp_select: exact order
// statistics, a look of its own with the same buffer set; it leaves the histogram alone.
int chs_cmp_look(Engine* E, hipStream_t s, void** buf, double threshold, int32_t nbins, double lo, double hi, int64_t* iw,
                 double* fw, const char* who);
int chs_cmp_hist(void* buf, int device, hipStream_t s, int32_t nbins, int64_t* out, const char* who);
int chs_cmp_select(Engine* E, hipStream_t s, void** buf, int32_t nq, const int64_t* ranks, double* values, const char* who);
int chs_cmp_last_ms(const void* h, const void* buf, double* ms, const char* what);
void chs_cmp_free(void** buf);
void chs_cmp_forget(void* buf);   // the buffers stay, the last look goes

// ---- two-point correlation (chs_two_point.hip) ---------------------------------
// The pair counts of both phases of E's field thresholded at `threshold` for every displacement up to rmax (DESIGN.md
// section 3i), on stream `s` with the buffer set *buf (the handle's own, or the batch's one set), allocated here at the
// first look: out[CHS_TP_WORDS].  The count table of the last look of a buffer set: chs_tp_counts.
int chs_tp_look(Engine* E, hipStream_t s, void** buf, double threshold, int32_t rmax, int64_t* out, const char* who);
int chs_tp_counts(void* buf, int device, hipStream_t s, int64_t n, int64_t* out, const char* who);
int chs_tp_last_ms(const void* h, const void* buf, double* ms, const char* what);
void chs_tp_free(void** buf);
void chs_tp_forget(void* buf);   // the buffers stay, the last look goes

// ---- contour (chs_contour.hip) -------------------------------------------------
// Length, orientation tensor and curvature of the level set U = threshold of E's field on stream
// `s` with the buffer set *buf (the handle's own, or the batch's one set), allocated here at the first look:
// words[CHS_CT_WORDS], sums[CHS_CT_SUMS].  Histograms and map of the last look of a buffer set: chs_ct_hist, chs_ct_map.
int chs_ct_look(Engine* E, hipStream_t s, void** buf, double threshold, int32_t bins, double kmax, int32_t want_map,
                int64_t* words, double* sums, const char* who);
int chs_ct_hist(void* buf, int device, hipStream_t s, int32_t bins, int64_t* out, const char* who);
int chs_ct_map(void* buf, int device, hipStream_t s, int64_t n, double* out, const char* who);
int chs_ct_last_ms(const void* h, const void* buf, double* ms, const char* what);
void chs_ct_free(void** buf);
void chs_ct_forget(void* buf);   // the buffers stay, the last look goes
