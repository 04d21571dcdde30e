// chs_batch.hip -- the batch of include/chs_hip.h: B ensemble members of one N, element type and device advance
// through their engine's step loop together, every step kernel launched ONCE for all of them.  A batch runs the engine
// a single handle of its members would run: the fast engine at N in {128 .. 2048} (everything below up to "A chirp
// batch"), the chirp engine at every other N it supports (the last paragraph).
//
// A member is an ordinary engine (chs_create: its own constants, state, field, transform scratch, partial sums and
// rows ring); the batch gives all of them one stream and keeps a device array of member records (BatchMember,
// chs_fast_kernels.h) that the batched kernels index by blockIdx.y.  Everything outside the step loop -- field
// up/downloads, prepare, the entry of a call (hat_U = dctn(U)), the state, the rebuild of U after a stop -- is
// the single handle's code, run member by member on the shared stream: once per call.  Inside the loop a step is
//   k_col, k_row_inv<fused>, k_step_tail_batch  [+ k_row_inv<last>, k_step_tail_batch<last> for the members whose
//   call ends with this step]
// in stream order: the tail of every member runs right behind its row kernel (no riding, no gate, no second hat_U
// buffer -- what those hide, the launch latency of one member's short kernels, is covered here by the other
// members' workgroups).  Every kernel body is the single handle's (the tail with the block size it has there).
//
// A batch whose members ALL adapt their time step (solver.py:177-193) runs the row kernel that also writes the partial
// column sums of the step-size integrand (k_row_inv<ADAPT>) and, between the row kernels and the tails,
//   k_colsum_slices_batch, k_colmin_slices_batch   (chs_pointwise.hip)
// which reduce every member's partial rows to its column minimum in the single handle's order; the tail of a member
// whose rule fires reads it (TailArgs::partColMin).  Whether the rule fires is each member's own affair, decided on
// the device from its own step counter; the host follows the counters (Engine::csHost) only to leave the reduction
// out on steps where it knows that no running member fires.  A configuration without the fused adaptive row kernel
// (N = 128: eight rows per workgroup) takes the sums from a sweep of U as its single handle does, member by member.
//
// The seat queue (chs_batch_step_n_queued): the same step kernels launched over a device array of `seats` records
// instead of over all members.  The batch's own array holds the records of the members in waiting; behind the tails
// k_seat_batch hands the seat of a member that has stopped or done its steps to the next one in member order, on the
// device.  The host never learns who sits where: it issues every step's kernels for every seat and follows the members
// through its polls of their states alone.
//
// Both entry points are "enter, own issue loop, finish" over one host record of the call (BatchCall): call_enter (the
// checks, the adaptive/fused decision, every member's entry and record), call_poll and call_take_rows (the state fetch
// behind a batch of steps and the rows that have completed) and call_finish (final states, the field of a member that
// stopped short, rows, status) exist once.  The row copy and the rebuild of a stopped member's field are the single
// handle's (chs_api.hip: chs_copy_rows_out, chs_stopped_short, chs_rebuild_stopped_u); the decisions that need no
// device -- the queue's step bound, its last-step bookkeeping, the plain batch's batch_rule_fires -- are in
// chs_batch_host.h, where a CPU test drives them.  The issue loops stay two: the plain batch knows who runs which step
// and leaves launches out, the queue does not and issues everything, so one loop would change what one of them launches.
//
// A chirp batch (Batch::chirp; N outside the fast batch's set, engine chirp or 'auto' where it resolves to chirp): the
// members are chirp engines, their records NatMember (chs_nat_batch.h) in Batch::dNat, and a step is the natural
// engines' unfused sequence of chs_api.hip (one_step) with every launch covering all members --
//   k_mu, k_pre, dct2d (k_chirp_lines, k_chirp_transpose, twice), k_spectral, dct2d, k_diag, k_fin: 13 launches --
// through the batched instantiations of the single handle's kernels (chs_pointwise.hip, chs_chirp_batch.hip).  A
// workgroup leaves at once when its member has halted or has no step left in the call; only k_fin advances the step
// counter, so the thirteen agree.  call_enter, call_poll, call_take_rows and call_finish are shared with the fast
// batch: the entry is every member's k_call_begin, the records, then hat_U = dctn(U) of all running members in four
// launches.  U is stored every step and a time-limit stop in k_pre leaves the previous U in place, as the reference
// does: there is no rebuild of U after a stop.  Outside a chirp batch's scope: the adaptive step (the natural path
// reduces partCol in chs_launch_pre, member by member; the batched reduction kernels are BatchMember's), the seat
// queue, jitter.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "chs_batch_host.h"
#include "chs_chirp_host.h"
#include "chs_fast_kernels.h"
#include "chs_nat_batch.h"

static_assert(CHS_BATCH_CHIRP_MIN_N == CHS_CHIRP_MIN_N && CHS_BATCH_CHIRP_MAX_N == CHS_CHIRP_MAX_N,
              "a chirp batch covers every N of the chirp engine (include/chs_hip.h)");

// The batch's per-step bookkeeping: one workgroup per member running the single handle's tail body (chs_tail.h) with
// the single handle's block size -- THREADS = that of the k_col the tail rides in there (LAST = false: the first step's
// time-step control with `pre_only`, the record + control of the next step otherwise), 1024 for the record of the
// call's last step (LAST, k_step_tail's) -- so that the sums are added up in the same order.  A member takes part when
// its running step (st->rows_written) is one of those.  (In a translation unit of its own: beside the k_col
// instantiations that share step_tail_body<THREADS> it would change how the compiler inlines it there.)
template <int THREADS, bool LAST>
__global__ __launch_bounds__(THREADS) void k_step_tail_batch(const BatchMember* __restrict__ mem, int pre_only) {
  __shared__ double red[TAIL_RED_DOUBLES(THREADS)];
  const BatchMember& m = mem[blockIdx.x];
  const long long done = m.st->rows_written, last = m.nsteps - 1;
  if ((LAST ? done != last : (pre_only ? done > last : done >= last)) || m.st->halt) return;
  step_tail_body<THREADS>(m.tail[LAST ? 2 : (pre_only ? 0 : 1)], m.st, red);
}

static int launch_tail(hipStream_t s, const BatchMember* mem, int B, int col_threads, bool last, int pre_only) {
  if (last) k_step_tail_batch<1024, true><<<B, 1024, 0, s>>>(mem, 0);
  else if (col_threads == 64) k_step_tail_batch<64, false><<<B, 64, 0, s>>>(mem, pre_only);
  else if (col_threads == 128) k_step_tail_batch<128, false><<<B, 128, 0, s>>>(mem, pre_only);
  else if (col_threads == 256) k_step_tail_batch<256, false><<<B, 256, 0, s>>>(mem, pre_only);
  else { chs_set_error("chs_batch_step_n: no batched tail for this block size"); return CHS_EINVAL; }
  CHS_HIP(hipGetLastError());
  return CHS_OK;
}

// The seat change of the queue.  `seat[seats]` are the records the step kernels of the coming launches index, `wait[R]`
// the records of all members of the call in member order, q[0] the number of the first member that has not been
// looked at yet and q[1 + m] the global step in front of which member m was seated (-1: not so far).  ONE wavefront
// walks the seats in ascending order, so who gets which seat is a function of the members' stop steps alone: a seat
// is free when its member has halted or has written the last record of its call (a vacant seat's record has
// nsteps = 0); it goes to the next waiting member that has steps to do and has not halted already (a time limit
// below the first step: its `pre_only` tail stopped it).  Lanes look at 64 seats / 64 waiting members at a time, the
// record is copied by all lanes in 8-byte words: plain vector loads and stores, nothing here is written by the
// scalar unit.  The step kernels read the records through the constant address space (scalar loads, batch_member):
// they see the new record because they are later launches of the same stream and a kernel's start invalidates the
// scalar cache -- what the hipMemcpyAsync of the records at the start of every call relies on already.
// Launched only in front of EVEN global steps (the host's choice, `step`): k_col walks its tiles in the direction the
// launch's step parity gives it, the partial sums of E2 land in block order and the tail adds them in that order -- a
// member seated in front of an odd step would get E2 of every step in the other summation order than the unqueued
// batch, where all members start at step 0.  A freed seat so idles one step at the most.
static_assert(sizeof(BatchMember) % 8 == 0 && alignof(BatchMember) == 8, "the seat kernel copies records in 8-byte words");
__global__ __launch_bounds__(64) void k_seat_batch(BatchMember* seat, int seats, const BatchMember* __restrict__ wait, int R,
                                                   long long* q, long long step) {
  const int lane = threadIdx.x;
  const long long head0 = q[0];
  long long head = head0;
  for (int s0 = 0; s0 < seats && head < R; s0 += 64) {
    const int j = s0 + lane;
    bool vacant = false;
    if (j < seats) {
      const DevState* st = seat[j].st;
      vacant = st->halt || st->rows_written >= seat[j].nsteps;
    }
    unsigned long long free_seats = __ballot(vacant);
    while (free_seats && head < R) {
      const int js = s0 + __ffsll(free_seats) - 1;
      int next = -1;
      while (head < R) {
        const long long c = head + lane;
        bool runs = false;
        if (c < R) runs = wait[c].nsteps > 0 && !wait[c].st->halt;
        const unsigned long long found = __ballot(runs);
        if (found) { next = (int)head + __ffsll(found) - 1; head = next + 1; break; }
        head += 64;
      }
      if (next < 0) break;
      free_seats &= free_seats - 1;
      const unsigned long long* src = reinterpret_cast<const unsigned long long*>(wait + next);
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(seat + js);
      for (int w = lane; w < (int)(sizeof(BatchMember) / 8); w += 64) dst[w] = src[w];
      if (lane == 0) q[1 + next] = step;
    }
  }
  if (lane == 0 && head != head0) q[0] = head < R ? head : R;
}

namespace {
struct Batch {
  int B = 0, N = 0, dtype = CHS_F64, device = 0;
  std::vector<Engine*> m;
  std::vector<hipStream_t> own;  // the members' own streams, handed back at chs_batch_destroy
  hipStream_t stream = nullptr;
  BatchMember* dMem = nullptr;
  std::vector<BatchMember> hMem;
  bool chirp = false;            // a batch of chirp engines: the records are NatMember, the step the natural sequence
  NatMember* dNat = nullptr;
  std::vector<NatMember> hNat;
  DevState* hPoll = nullptr;     // pinned [5][B]: slot 0 = the end of a call, 1..4 = the polls behind the step batches
  hipEvent_t evPoll[4] = {nullptr, nullptr, nullptr, nullptr};
  // the seat queue (chs_batch_step_n_queued; allocated at its first call)
  BatchMember* dSeat = nullptr;  // [seatCap] the records the step kernels index; dMem holds the waiting members' then
  int seatCap = 0;
  long long* dQueue = nullptr;   // [1 + B]: head of the queue, the members' seating steps (k_seat_batch)
  long long* hQueue = nullptr;   // pinned [5][1 + B], slots as in hPoll
  std::vector<BatchMember> hSeat;
  std::vector<long long> hQueue0;
  std::vector<std::vector<double>> qRows;  // the members' rows of the last queued call (chs_batch_member_rows)
  void* spec = nullptr;          // chs_batch_structure_factor of all members: its buffers (chs_spectrum.hip), at the first call
  void* morph = nullptr;         // chs_batch_morphology of all members: its buffers (chs_morphology.hip), at the first look
  void* cc = nullptr;            // chs_batch_components: the batch's one set of buffers (chs_components.hip), at the first look
  void* dt = nullptr;            // chs_batch_distance: the batch's one set of buffers (chs_distance.hip), at the first look
  void* ch = nullptr;            // chs_batch_chords: the batch's one set of buffers (chs_chords.hip), at the first look
  void* cmp = nullptr;           // chs_batch_composition: the batch's one set of buffers (chs_composition.hip), at the first look
  void* tp = nullptr;            // chs_batch_two_point: the batch's one set of buffers (chs_two_point.hip), at the first look
  void* ct = nullptr;            // chs_batch_contour: the batch's one set of buffers (chs_contour.hip), at the first look
  void* sh = nullptr;            // chs_batch_shapes: the batch's one set of buffers (chs_shapes.hip), at the first look
  void* tr = nullptr;            // chs_batch_track: the batch's one hash table and row list (chs_track.hip), at the first look;
                                 // the frames are the members' own (Engine::tr)
  void* th = nullptr;            // chs_batch_thickness: the batch's one set of buffers (chs_thickness.hip), at the first look
  void* geo = nullptr;           // chs_batch_geodesic: the batch's one set of buffers (chs_geodesic.hip), at the first look
  void* sk = nullptr;            // chs_batch_skeleton: the batch's one set of buffers (chs_skeleton.hip), at the first look
  void* trn = nullptr;           // chs_batch_transport: the batch's one set of buffers (chs_transport.hip), at the first look
};

bool batch_n_ok(int N) { return N == 128 || N == 256 || N == 512 || N == 1024 || N == 2048; }

int bad(const std::string& s) { chs_set_error(s); return CHS_EINVAL; }

void batch_free(Batch* b) {
  if (!b) return;
  hipSetDevice(b->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  for (size_t i = 0; i < b->m.size(); ++i) {
    if (!b->m[i]) continue;
    if (i < b->own.size() && b->own[i]) b->m[i]->stream = b->own[i];
    chs_destroy((chs_handle)b->m[i]);
  }
  chs_spectrum_free(&b->spec);
  chs_morph_free(&b->morph);
  chs_cc_free(&b->cc);
  chs_dt_free(&b->dt);
  chs_ch_free(&b->ch);
  chs_cmp_free(&b->cmp);
  chs_tp_free(&b->tp);
  chs_ct_free(&b->ct);
  chs_sh_free(&b->sh);
  chs_tr_free(&b->tr);
  chs_th_free(&b->th);
  chs_geo_free(&b->geo);
  chs_sk_free(&b->sk);
  chs_trn_free(&b->trn);
  if (b->dMem) hipFree(b->dMem);
  if (b->dNat) hipFree(b->dNat);
  if (b->dSeat) hipFree(b->dSeat);
  if (b->dQueue) hipFree(b->dQueue);
  if (b->hQueue) hipHostFree(b->hQueue);
  if (b->hPoll) hipHostFree(b->hPoll);
  for (auto e : b->evPoll) if (e) hipEventDestroy(e);
  if (b->stream) hipStreamDestroy(b->stream);
  delete b;
}

Batch* as_batch(chs_batch h) { return (Batch*)h; }
}  // namespace

extern "C" int chs_batch_create(const chs_consts* consts, int32_t B, const double* lambda, chs_batch* out) {
  if (!consts || !lambda || !out) return bad("chs_batch_create: null argument");
  *out = nullptr;
  if (B < 1) return bad("chs_batch_create: B must be >= 1");
  if (B > CHS_BATCH_MAX_MEMBERS)   // (the member is the grid's y or z dimension: 65535 at the most)
    return bad("chs_batch_create: B must be <= " + std::to_string(CHS_BATCH_MAX_MEMBERS));
  const chs_consts& c0 = consts[0];
  // the batch's engine is what a single handle of member 0 would run: the fast engine at the fast batch's sizes, the
  // chirp engine where it is asked for or where 'auto' resolves to it
  auto runs_chirp = [](const chs_consts& c) {   // (the engine a member resolves to, not how it is spelled)
    return c.engine == CHS_ENGINE_CHIRP ||
           (c.engine == CHS_ENGINE_AUTO && c.N >= CHS_CHIRP_AUTO_MIN_N && !chs_fast_supported(c.N, c.dtype));
  };
  const bool chirp = !batch_n_ok(c0.N) && chs_chirp_supported(c0.N) && runs_chirp(c0);
  for (int i = 0; i < B; ++i) {
    const chs_consts& c = consts[i];
    const std::string who = "chs_batch_create: member " + std::to_string(i) + ": ";
    if (c.N != c0.N || c.dtype != c0.dtype || c.device != c0.device)
      return bad(who + "every member needs the N, dtype and device of member 0");
    if (chirp) {
      if (!runs_chirp(c)) return bad(who + "engine differs from member 0's (a chirp batch: engine chirp, or auto where it resolves to chirp)");
      if (c.adaptive_time != 0)
        return bad(who + "adaptive_time: a chirp batch has no adaptive time step (the fast batch has)");
      continue;
    }
    if (c.engine == CHS_ENGINE_DIRECT) return bad(who + "a batch runs the fast or the chirp engine (engine=direct given)");
    if (batch_n_ok(c.N) && c.engine == CHS_ENGINE_CHIRP)
      return bad(who + "N=" + std::to_string(c.N) + " is a batch of the fast engine only (engine=chirp given)");
    if (!batch_n_ok(c.N))
      return bad(who + "a batch needs N in {128, 256, 512, 1024, 2048} for the fast engine, or the chirp engine (engine=chirp, or "
                       "auto from N=" + std::to_string(CHS_CHIRP_AUTO_MIN_N) + " where it resolves to chirp) at N in [8, 4096]");
    if (c.engine != CHS_ENGINE_AUTO && c.engine != CHS_ENGINE_FAST) return bad(who + "bad engine");
    if ((c.adaptive_time != 0) != (c0.adaptive_time != 0))
      return bad(who + "adaptive_time differs from member 0's (a batch adapts the step of all its members or of none)");
  }
  Batch* b = new (std::nothrow) Batch();
  if (!b) return bad("out of host memory");
  b->B = B; b->N = c0.N; b->dtype = c0.dtype; b->device = c0.device;
  auto fail = [&](int rc) { batch_free(b); return rc; };
  for (int i = 0; i < B; ++i) {
    chs_consts c = consts[i];
    c.engine = chirp ? CHS_ENGINE_CHIRP : CHS_ENGINE_FAST;
    chs_handle h = nullptr;
    const int rc = chs_create(&c, lambda, &h);
    if (rc) return fail(rc);
    b->m.push_back((Engine*)h);
  }
  b->chirp = chirp;
  FastPlan* P = chirp ? nullptr : (FastPlan*)b->m[0]->dTw;
  if (!chirp && (!P || !P->col_batch)) return fail(bad("chs_batch_create: no batched kernels for this configuration"));
#define TRY_HIP(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { chs_hip_fail(e__, #call, __FILE__, __LINE__); return fail(CHS_EHIP); } } while (0)
  TRY_HIP(hipSetDevice(b->device));
  int rc;
  if ((rc = chirp ? chs_chirp_batch_init(b->m[0]) : P->init_batch())) return fail(rc);
  TRY_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  for (Engine* E : b->m) {   // one stream for all members: their own launches and the batched ones stay in order
    TRY_HIP(hipStreamSynchronize(E->stream));
    b->own.push_back(E->stream);
    E->stream = b->stream;
  }
  if (chirp) TRY_HIP(hipMalloc(&b->dNat, sizeof(NatMember) * (size_t)B));
  else TRY_HIP(hipMalloc(&b->dMem, sizeof(BatchMember) * (size_t)B));
  TRY_HIP(hipHostMalloc((void**)&b->hPoll, sizeof(DevState) * 5 * (size_t)B, hipHostMallocDefault));
  for (auto& e : b->evPoll) TRY_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
#undef TRY_HIP
  if (chirp) b->hNat.resize((size_t)B);
  else b->hMem.resize((size_t)B);
  *out = (chs_batch)b;
  return CHS_OK;
}

extern "C" int chs_batch_engine(chs_batch h) {
  Batch* b = as_batch(h);
  if (!b || b->m.empty()) return CHS_EINVAL;
  for (const Engine* E : b->m)   // (what the members' handles report, chs_engine: one engine for all of them)
    if (E->engine != b->m[0]->engine) return CHS_EINVAL;
  return b->m[0]->engine;
}

extern "C" int chs_batch_destroy(chs_batch h) {
  batch_free(as_batch(h));
  return CHS_OK;
}

// member m, or every member for m = -1
template <class F>
static int each_member(Batch* b, int32_t member, const char* what, F&& f) {
  if (!b) { chs_set_error(std::string(what) + ": null handle"); return CHS_EINVAL; }
  if (member < -1 || member >= b->B) { chs_set_error(std::string(what) + ": no such member"); return CHS_EINVAL; }
  const int lo = member < 0 ? 0 : member, hi = member < 0 ? b->B : member + 1;
  for (int i = lo; i < hi; ++i) {
    const int rc = f(i, (chs_handle)b->m[i]);
    if (rc) return rc;
  }
  return CHS_OK;
}

extern "C" int chs_batch_set_U(chs_batch h, int32_t member, const double* host_U) {
  return each_member(as_batch(h), member, "chs_batch_set_U", [&](int, chs_handle e) { return chs_set_U(e, host_U); });
}

extern "C" int chs_batch_init_U_pcg64(chs_batch h, int32_t member, double base, double scale, const uint64_t state[2],
                                      const uint64_t inc[2]) {
  return each_member(as_batch(h), member, "chs_batch_init_U_pcg64",
                     [&](int, chs_handle e) { return chs_init_U_pcg64(e, base, scale, state, inc); });
}

extern "C" int chs_batch_get_U(chs_batch h, int32_t member, double* host_U) {
  if (member < 0) return bad("chs_batch_get_U: one member at a time");
  return each_member(as_batch(h), member, "chs_batch_get_U", [&](int, chs_handle e) { return chs_get_U(e, host_U); });
}

extern "C" int chs_batch_get_state(chs_batch h, int32_t member, chs_state* out) {
  if (member < 0) return bad("chs_batch_get_state: one member at a time");
  return each_member(as_batch(h), member, "chs_batch_get_state", [&](int, chs_handle e) { return chs_get_state(e, out); });
}

extern "C" int chs_batch_set_state(chs_batch h, int32_t member, const chs_state* in) {
  if (member < 0) return bad("chs_batch_set_state: one member at a time");
  return each_member(as_batch(h), member, "chs_batch_set_state", [&](int, chs_handle e) { return chs_set_state(e, in); });
}

// chs_prepare of every member; a member whose step-0 record is NaN does not keep the others from being prepared
extern "C" int chs_batch_prepare(chs_batch h, double* rows0) {
  if (!rows0) return bad("chs_batch_prepare: null argument");
  int nan = 0;
  const int rc = each_member(as_batch(h), -1, "chs_batch_prepare", [&](int i, chs_handle e) {
    const int r = chs_prepare(e, rows0 + 9 * (size_t)i);
    if (r == CHS_ENAN) { nan = 1; return CHS_OK; }
    return r;
  });
  if (rc) return rc;
  if (nan) { chs_set_error("chs_batch_prepare: NaN in a step-0 record (timedata.py:10)"); return CHS_ENAN; }
  return CHS_OK;
}

// the device and pinned arrays of the seat queue, at the first queued call (and when a call asks for more seats)
static int queue_buffers(Batch* b, int seats) {
  const size_t nq = 1 + (size_t)b->B;
  if (!b->dQueue) CHS_HIP(hipMalloc(&b->dQueue, sizeof(long long) * nq));
  if (!b->hQueue) CHS_HIP(hipHostMalloc((void**)&b->hQueue, sizeof(long long) * 5 * nq, hipHostMallocDefault));
  if (seats > b->seatCap) {
    if (b->dSeat) { CHS_HIP(hipStreamSynchronize(b->stream)); CHS_HIP(hipFree(b->dSeat)); b->dSeat = nullptr; b->seatCap = 0; }
    CHS_HIP(hipMalloc(&b->dSeat, sizeof(BatchMember) * (size_t)seats));
    b->seatCap = seats;
  }
  return CHS_OK;
}

// ---------------------------------------------------------------------------
// One call of the batch, plain or queued: what chs_batch_step_n and chs_batch_step_n_queued share.  Each of them is
// call_enter, its own issue loop with call_poll behind every batch of steps, call_finish.
// ---------------------------------------------------------------------------
namespace {
struct BatchCall {
  Batch* b;
  const char* who;            // the entry point's name, for the error texts
  const int64_t* nsteps;
  int64_t* steps_done;
  int32_t* status;
  double* rows;               // the plain batch: the caller's [B][maxn][9]; the queue's rows go to Batch::qRows
  bool queued;                // chs_batch_step_n_queued: the members take turns in ...
  int seats = 0;              // ... this many seats (min(seats asked for, B))
  int running = 0;            // members with steps to do
  int64_t maxn = 0;           // the longest call
  bool adaptive = false;      // an adaptive batch (all members or none: chs_batch_create)
  bool fused = true;          // ... whose row kernel adds up the step-size integrand
  int batch_steps = 1024;     // steps between two polls
  std::vector<long long> cs0; // the members' step counters at the entry, where the host knows them
  std::vector<int64_t> copied;  // rows of each member that its destination holds already
  int poll = 0;
};

// The checks of the arguments, then the entry of every member that runs -- re-armed loop, hat_U = dctn(U) and the first
// step's row transform of EnergieEut(U): the single handle's code on the shared stream -- and the members' records, on
// the device in Batch::dMem.  `seats`: what the caller of a queued call asked for.
int call_enter(BatchCall& c, int32_t flags, int32_t seats) {
  Batch* b = c.b;
  const std::string who = c.who;
  if (!b || !c.nsteps || !c.steps_done || !c.status) return bad(who + ": null argument");
  if (flags != 0) return bad(who + ": flags is reserved and must be 0");
  if (c.queued && b->chirp) return bad(who + ": a chirp batch has no seat queue (chs_batch_step_n runs it)");
  if (c.queued && seats < 1) return bad(who + ": seats must be >= 1");
  const int B = b->B;
  if (c.queued) c.seats = seats < B ? seats : B;
  for (int i = 0; i < B; ++i) {
    if (c.nsteps[i] > 0 && !b->m[i]->prepared) {
      chs_set_error(who + ": member " + std::to_string(i) + " not prepared (solver.py:139)");
      return CHS_ESTATE;
    }
    if (c.nsteps[i] > c.maxn) c.maxn = c.nsteps[i];
    c.running += c.nsteps[i] > 0;
  }
  if (!c.queued && c.maxn > 0 && !c.rows) return bad(who + ": rows is null");
  CHS_HIP(hipSetDevice(b->device));
  int rc;
  if (c.queued) {
    if ((rc = queue_buffers(b, c.seats))) return rc;
    b->qRows.assign((size_t)B, std::vector<double>());
  }
  for (int i = 0; i < B; ++i) {
    const Engine* E = b->m[i];
    c.adaptive |= E->dc.adaptive_time != 0;
    c.fused &= E->fusedAdapt && E->dPartColRows != nullptr;
  }
  c.fused &= c.adaptive;
  c.cs0.assign((size_t)B, -1);
  c.copied.assign((size_t)B, 0);
  for (int i = 0; b->chirp && i < B; ++i) {
    // a chirp member: the re-armed loop and its record; hat_U = dctn(U) follows for all members at once
    Engine* E = b->m[i];
    NatMember& r = b->hNat[(size_t)i];
    std::memset((void*)&r, 0, sizeof r);
    const int64_t n = c.nsteps[i] > 0 ? c.nsteps[i] : 0;
    r.nsteps = n;
    c.steps_done[i] = 0;
    c.status[i] = CHS_OK;
    r.st = E->dState;   // (rows_written >= nsteps = 0 keeps the member out of every launch)
    if (n == 0) continue;
    if (!E->dRows) return bad(who + ": member " + std::to_string(i) + " has no rows ring");
    E->stateCached = false; E->resident = false;
    c.cs0[(size_t)i] = E->csHost;
    if (chs_stop_armed(E)) c.batch_steps = E->batchSteps < c.batch_steps ? E->batchSteps : c.batch_steps;
    if ((rc = chs_launch_call_begin(E))) return rc;
    E->hat_valid = true;
    r.dc = E->dc;
    r.arr[NAT_U] = E->dU; r.arr[NAT_MU] = E->dMU; r.arr[NAT_T1] = E->dT1; r.arr[NAT_T2] = E->dT2; r.arr[NAT_HAT] = E->dHat;
    r.partMu = E->sums().mu; r.partDiag = E->sums().diag;
    r.rows = E->dRows; r.rowsCap = E->rowsCap;
  }
  for (int i = 0; !b->chirp && i < B; ++i) {
    Engine* E = b->m[i];
    BatchMember& r = b->hMem[(size_t)i];
    std::memset((void*)&r, 0, sizeof r);
    const int64_t n = c.nsteps[i] > 0 ? c.nsteps[i] : 0;
    r.nsteps = n;
    c.steps_done[i] = 0;
    c.status[i] = CHS_OK;
    r.st = E->dState;   // (read by every batched kernel: rows_written >= nsteps = 0 keeps the member out)
    if (n == 0) continue;   // sits the call out (a queue never seats it): state and field stay as they are
    E->stateCached = false; E->resident = false;
    c.cs0[(size_t)i] = E->csHost;
    if (chs_stop_armed(E)) c.batch_steps = E->batchSteps < c.batch_steps ? E->batchSteps : c.batch_steps;
    if ((rc = chs_launch_call_begin(E))) return rc;
    if ((rc = chs_fast_enter_fused(E))) return rc;
    E->hat_valid = true;
    r.dc = E->dc;
    r.T1 = E->dT1;
    r.T2 = E->dT1;
    r.hat = E->dHat;
    r.U = E->dU;
    const PartialSums& ps = E->sums();   // one set for the whole call: the batch's tail runs in stream order
    r.partDiag = ps.diag; r.partMu = ps.mu; r.partRa = ps.ra; r.partE2 = ps.e2;
    r.tail[0] = chs_tail_args(E, ps, 1);
    r.tail[0].pre_only = 1;
    r.tail[1] = chs_tail_args(E, ps, 1);
    r.tail[2] = chs_tail_args(E, ps, 0);
    if (c.adaptive) {
      // the first step's time-step control as the single handle runs it: the integrand's column sums from a sweep of
      // U (the rule looks at the counter as the previous call left it), then k_pre -- once per call
      if (c.fused && (rc = chs_colmin_batch_buffers(E, &r))) return rc;
      if ((rc = chs_launch_mu_colsums(E, 0))) return rc;
      if ((rc = chs_launch_pre(E))) return rc;
    }
  }
  if (const char* bs = getenv("CHS_BATCH_STEPS")) {   // (the test hook of chs_step_n: small batches exercise the polls)
    const long v = atol(bs);
    if (v >= 1 && v <= 8192) c.batch_steps = (int)v;
  }
  if (b->chirp) {
    CHS_HIP(hipMemcpyAsync(b->dNat, b->hNat.data(), sizeof(NatMember) * (size_t)B, hipMemcpyHostToDevice, b->stream));
    // hat_U = dctn(U) of every running member (solver.py:159), T1 the scratch as in the single handle's entry
    if (c.running > 0) return chs_chirp_batch_dct2d(b->m[0], b->stream, b->dNat, B, NAT_U, NAT_HAT, NAT_T1, false);
    return CHS_OK;
  }
  CHS_HIP(hipMemcpyAsync(b->dMem, b->hMem.data(), sizeof(BatchMember) * (size_t)B, hipMemcpyHostToDevice, b->stream));
  return CHS_OK;
}

// rows [copied, w) of member i out of its ring to where the call's rows go
int call_take_rows(BatchCall& c, int i, int64_t w) {
  int64_t& have = c.copied[(size_t)i];
  if (w <= have) return CHS_OK;
  double* dst;
  if (c.queued) {
    std::vector<double>& v = c.b->qRows[(size_t)i];
    v.resize((size_t)w * 9);
    dst = v.data();
  } else {
    dst = c.rows + (size_t)i * c.maxn * 9;
  }
  const int rc = chs_copy_rows_out(c.b->m[i], dst, have, w);
  have = w;
  return rc;
}

// Behind a batch of steps: the states of the members that `want` names are fetched into the pinned slot of this poll
// (and what `also` adds to it), and the poll before this one is waited for -- the device is busy with the steps just
// issued then, so it never idles.  *seen: the slot of that poll in hPoll (its members' rows that have completed are
// taken here), 0 while there is none; the caller draws its own conclusions from the states.
template <class Want, class Also>
int call_poll(BatchCall& c, Want&& want, Also&& also, int* seen) {
  Batch* b = c.b;
  const int B = b->B;
  const int slot = 1 + (c.poll & 3);
  for (int i = 0; i < B; ++i)
    if (want(i))
      CHS_HIP(hipMemcpyAsync(&b->hPoll[(size_t)slot * B + i], b->m[i]->dState, sizeof(DevState), hipMemcpyDeviceToHost, b->stream));
  int rc;
  if ((rc = also(slot))) return rc;
  CHS_HIP(hipEventRecord(b->evPoll[c.poll & 3], b->stream));
  *seen = 0;
  if (c.poll >= 1) {
    const int prev = (c.poll - 1) & 3;
    CHS_HIP(hipEventSynchronize(b->evPoll[prev]));
    *seen = 1 + prev;
  }
  ++c.poll;
  return CHS_OK;
}

// rows of member i that the state `ps` of a poll shows as completed
int call_take_polled(BatchCall& c, int i, const DevState& ps) {
  return call_take_rows(c, i, ps.rows_written < c.nsteps[i] ? ps.rows_written : c.nsteps[i]);
}

// The end of a call: the members' states, the field of a member that stopped before its last step, what the host keeps
// of the state, the remaining rows and the per-member status.
int call_finish(BatchCall& c) {
  Batch* b = c.b;
  const int B = b->B;
  int rc;
  for (int i = 0; i < B; ++i)
    if (c.nsteps[i] > 0)
      CHS_HIP(hipMemcpyAsync(&b->hPoll[i], b->m[i]->dState, sizeof(DevState), hipMemcpyDeviceToHost, b->stream));
  CHS_HIP(hipStreamSynchronize(b->stream));
  bool any_nan = false;
  for (int i = 0; i < B; ++i) {
    if (c.nsteps[i] <= 0) continue;
    Engine* E = b->m[i];
    const DevState s = b->hPoll[i];
    if (c.queued && !s.halt && s.rows_written < c.nsteps[i]) {   // (a queue's step bound or last-step pair went wrong)
      chs_set_error(std::string(c.who) + ": member " + std::to_string(i) + " was left with steps to do");
      return CHS_ESTATE;
    }
    // its row kernel has been keeping U in registers -- the member's own arrays, whoever has its seat by now -- unless
    // the step-size sums come from a sweep of U, which needs the field of every step (fused_row_mode)
    // (a chirp member stores U every step: what it holds after a stop is the field of its last completed step)
    if (!b->chirp && chs_stopped_short(s, c.nsteps[i], c.adaptive && !c.fused) && (rc = chs_rebuild_stopped_u(E, s))) return rc;
    if (s.halt) E->hat_valid = false;
    E->csHost = s.computed_steps;
    const int64_t done = s.rows_written < c.nsteps[i] ? s.rows_written : c.nsteps[i];
    c.steps_done[i] = done;
    if ((rc = call_take_rows(c, i, done))) return rc;
    double* mr = c.queued ? b->qRows[(size_t)i].data() : c.rows + (size_t)i * c.maxn * 9;
    // solver.py:230 `domtime = self.time_passed ** (1 / 3)` with the host libm
    for (int64_t k = 0; k < done; ++k) mr[k * 9 + 4] = pow(mr[k * 9 + 4], 1.0 / 3.0);
    if (s.nan_flag) { c.status[i] = CHS_ENAN; any_nan = true; }
  }
  if (any_nan) {
    chs_set_error("NaN in a recorded scalar (timedata.py:10) of a member: U left (0,1)");
    return CHS_ENAN;
  }
  return CHS_OK;
}
}  // namespace

// The issue loop of a chirp batch behind call_enter: the natural step's thirteen launches for all members while some
// member still has steps in the call; the kernels decide per member who takes part (nat_sits_out).  Polls and the end
// of the call are the fast batch's.
static int chirp_step_loop(BatchCall& c) {
  Batch* b = c.b;
  const int B = b->B;
  const int64_t maxn = c.maxn;
  const int64_t* nsteps = c.nsteps;
  Engine* E0 = b->m[0];
  const NatMember* mem = b->dNat;
  hipStream_t s = b->stream;
  int rc;
  int64_t issued = 0;
  bool stopped = false;
  while (issued < maxn && !stopped) {
    int64_t nb = maxn - issued;
    if (nb > c.batch_steps) nb = c.batch_steps;
    for (int64_t k = 0; k < nb; ++k) {
      if ((rc = chs_nat_batch_mu(E0, s, mem, B))) return rc;                                                   // 166-175
      if ((rc = chs_nat_batch_pre(E0, s, mem, B))) return rc;                                                  // 177-199, 225
      if ((rc = chs_chirp_batch_dct2d(E0, s, mem, B, NAT_MU, NAT_T2, NAT_T1, false))) return rc;               // 201
      if ((rc = chs_nat_batch_spectral(E0, s, mem, B))) return rc;                                             // 201-206
      if ((rc = chs_chirp_batch_dct2d(E0, s, mem, B, NAT_HAT, NAT_U, NAT_T1, true))) return rc;                // 208
      if ((rc = chs_nat_batch_diag(E0, s, mem, B))) return rc;                                                 // 213-228
      if ((rc = chs_nat_batch_fin(E0, s, mem, B))) return rc;                                                  // 230-249
    }
    issued += nb;
    if (issued < maxn) {
      int seen = 0;
      if ((rc = call_poll(c, [&](int i) { return nsteps[i] > 0; }, [](int) { return (int)CHS_OK; }, &seen))) return rc;
      if (seen) {
        const DevState* ps = &b->hPoll[(size_t)seen * B];
        bool all = true;
        for (int i = 0; i < B; ++i) {
          if (nsteps[i] <= 0) continue;
          if ((rc = call_take_polled(c, i, ps[i]))) return rc;
          if (!ps[i].halt && nsteps[i] > issued) all = false;   // (as in chs_batch_step_n below)
        }
        if (all) stopped = true;
      }
    }
  }
  return call_finish(c);
}

// chs_step_n of every member as a literal solve_or_resume call (hat_U = dctn(U) on entry, U stored at the end), the
// steps of all members issued together.  As in chs_step_n the steps go out in batches, and behind every batch the
// members' states are fetched; once every member that still has steps to do has halted nothing more is issued.
// The host knows who runs which step: it leaves out the launches that no member needs (`go_on`, `last`, batch_rule_fires).
extern "C" int chs_batch_step_n(chs_batch h, const int64_t* nsteps, int32_t flags, double* rows, int64_t* steps_done,
                                int32_t* status) {
  BatchCall c{as_batch(h), "chs_batch_step_n", nsteps, steps_done, status, rows, false};
  int rc;
  if ((rc = call_enter(c, flags, 0))) return rc;
  Batch* b = c.b;
  if (b->chirp) return chirp_step_loop(c);
  const int B = b->B;
  const int64_t maxn = c.maxn;
  const bool adaptive = c.adaptive, fused = c.fused;
  Engine* E0 = b->m[0];
  FastPlan* P = (FastPlan*)E0->dTw;
  if (maxn > 0 && !adaptive) {
    if ((rc = launch_tail(b->stream, b->dMem, B, P->col_threads, false, 1))) return rc;
  }
  const RowMode rm = fused_row_mode(adaptive, fused);
  int64_t issued = 0;
  bool stopped = false;
  while (issued < maxn && !stopped) {
    int64_t nb = maxn - issued;
    if (nb > c.batch_steps) nb = c.batch_steps;
    for (int64_t s = issued; s < issued + nb; ++s) {
      bool go_on = false, last = false;
      for (int i = 0; i < B; ++i) {
        go_on |= s < nsteps[i] - 1;
        last |= s == nsteps[i] - 1;
      }
      if ((rc = P->col_batch(E0, b->stream, b->dMem, B, (s & 1) ? 1 : 0))) return rc;
      if (go_on && (rc = P->row_inv_batch(E0, b->stream, b->dMem, B, rm.mode, rm.store_u))) return rc;
      if (last && (rc = P->row_inv_batch(E0, b->stream, b->dMem, B, ROW_INV_DIAG, 1))) return rc;
      if (adaptive && go_on) {
        // the column minimum of the coming step's integrand, for the members whose rule fires (the kernels check again)
        if (fused) {
          bool any = false;
          for (int i = 0; i < B; ++i) any |= batch_rule_fires(c.cs0[(size_t)i], nsteps[i], s);
          if (any && (rc = chs_launch_colmin_rows_batch(b->stream, b->dMem, B, b->N, b->dtype == CHS_F32))) return rc;
        } else {
          for (int i = 0; i < B; ++i)
            if (batch_rule_fires(c.cs0[(size_t)i], nsteps[i], s) && (rc = chs_launch_mu_colsums(b->m[i], 1))) return rc;
        }
      }
      // (the last-step records first: a member whose record the other launch writes moves on to its last step)
      if (last && (rc = launch_tail(b->stream, b->dMem, B, P->col_threads, true, 0))) return rc;
      if (go_on && (rc = launch_tail(b->stream, b->dMem, B, P->col_threads, false, 0))) return rc;
    }
    issued += nb;
    if (issued < maxn) {
      int seen = 0;
      if ((rc = call_poll(c, [&](int i) { return nsteps[i] > 0; }, [](int) { return (int)CHS_OK; }, &seen))) return rc;
      if (seen) {
        const DevState* ps = &b->hPoll[(size_t)seen * B];
        bool all = true;
        for (int i = 0; i < B; ++i) {
          if (nsteps[i] <= 0) continue;
          if ((rc = call_take_polled(c, i, ps[i]))) return rc;
          // (the poll is two batches behind: a member that was running then and has steps left now is still going)
          if (!ps[i].halt && nsteps[i] > issued) all = false;
        }
        if (all) stopped = true;
      }
    }
  }
  return call_finish(c);
}

// ---------------------------------------------------------------------------
// The seat queue: chs_batch_step_n over `seats` records that the members of the batch take turns in.
// ---------------------------------------------------------------------------

// chs_batch_step_n with the members taking turns in `seats` seats: the entry of every member up front (call_enter: the
// records are those of the waiting members), then every step kernel launched over the seats; k_seat_batch hands a seat
// on.  The host does not know who sits where, so it leaves nothing out that a seated member might need: the fused row
// kernel, the normal tail and (adaptive) the reduction go out on every step, the last-step pair from the first step on
// at which the call of some unfinished member may end (QueueMembers, chs_batch_host.h).  The kernels decide per member,
// as they always did.
extern "C" int chs_batch_step_n_queued(chs_batch h, int32_t seats, const int64_t* nsteps, int32_t flags,
                                       int64_t* steps_done, int32_t* status) {
  BatchCall c{as_batch(h), "chs_batch_step_n_queued", nsteps, steps_done, status, nullptr, true};
  int rc;
  if ((rc = call_enter(c, flags, seats))) return rc;
  Batch* b = c.b;
  const int R = b->B, S = c.seats, running = c.running;
  const bool adaptive = c.adaptive, fused = c.fused;
  // every seat vacant (no step in the call, somebody's state to look at); the queue at member 0, nobody seated
  b->hSeat.assign((size_t)S, BatchMember());
  for (BatchMember& v : b->hSeat) { std::memset((void*)&v, 0, sizeof v); v.st = b->m[0]->dState; }
  b->hQueue0.assign(1 + (size_t)R, -1);
  b->hQueue0[0] = 0;
  const size_t nq = 1 + (size_t)R;
  CHS_HIP(hipMemcpyAsync(b->dSeat, b->hSeat.data(), sizeof(BatchMember) * (size_t)S, hipMemcpyHostToDevice, b->stream));
  CHS_HIP(hipMemcpyAsync(b->dQueue, b->hQueue0.data(), sizeof(long long) * nq, hipMemcpyHostToDevice, b->stream));
  Engine* E0 = b->m[0];
  FastPlan* P = (FastPlan*)E0->dTw;
  // the first step's time-step control of ALL members, once: over the seats it would also run for members in mid-run
  if (running > 0 && !adaptive) {
    if ((rc = launch_tail(b->stream, b->dMem, R, P->col_threads, false, 1))) return rc;
  }
  const int64_t bound = queue_step_bound(nsteps, R, S);
  if (running > 0) {
    k_seat_batch<<<1, 64, 0, b->stream>>>(b->dSeat, S, b->dMem, R, b->dQueue, 0);
    CHS_HIP(hipGetLastError());
  }
  const RowMode rm = fused_row_mode(adaptive, fused);
  QueueMembers qm(nsteps, R, S);
  bool all_seated = running <= S;                 // nobody waits (any more): no seat changes hands
  int64_t issued = 0;
  int64_t poll_issued[4] = {0, 0, 0, 0};
  bool stopped = false;
  while (issued < bound && !stopped) {
    int64_t nb = bound - issued;
    if (nb > c.batch_steps) nb = c.batch_steps;
    for (int64_t s = issued; s < issued + nb; ++s) {
      const bool last = qm.last_pair(s);   // may the call of an unfinished member end with this step?
      if ((rc = P->col_batch(E0, b->stream, b->dSeat, S, (s & 1) ? 1 : 0))) return rc;
      if ((rc = P->row_inv_batch(E0, b->stream, b->dSeat, S, rm.mode, rm.store_u))) return rc;
      if (last && (rc = P->row_inv_batch(E0, b->stream, b->dSeat, S, ROW_INV_DIAG, 1))) return rc;
      if (adaptive) {
        if (fused) {
          if ((rc = chs_launch_colmin_rows_batch(b->stream, b->dSeat, S, b->N, b->dtype == CHS_F32))) return rc;
        } else {
          // (the sweep of U works on the member's own arrays, seated or not: what it leaves for a member in waiting is
          // written again behind that member's own row kernel before its tail reads it)
          for (int i = 0; i < R; ++i)
            if (!qm.finished[(size_t)i] && (rc = chs_launch_mu_colsums(b->m[i], 1))) return rc;
        }
      }
      // (the last-step records first, as in chs_batch_step_n)
      if (last && (rc = launch_tail(b->stream, b->dSeat, S, P->col_threads, true, 0))) return rc;
      if ((rc = launch_tail(b->stream, b->dSeat, S, P->col_threads, false, 0))) return rc;
      if (!all_seated && ((s + 1) & 1) == 0 && s + 1 < bound) {
        k_seat_batch<<<1, 64, 0, b->stream>>>(b->dSeat, S, b->dMem, R, b->dQueue, (long long)(s + 1));
        CHS_HIP(hipGetLastError());
      }
    }
    issued += nb;
    if (issued < bound) {
      poll_issued[c.poll & 3] = issued;
      int seen = 0;
      auto fetch_queue = [&](int slot) {
        CHS_HIP(hipMemcpyAsync(b->hQueue + (size_t)slot * nq, b->dQueue, sizeof(long long) * nq, hipMemcpyDeviceToHost, b->stream));
        return (int)CHS_OK;
      };
      if ((rc = call_poll(c, [&](int i) { return !qm.finished[(size_t)i]; }, fetch_queue, &seen))) return rc;
      if (seen) {
        const DevState* ps = &b->hPoll[(size_t)seen * R];
        const long long* pq = b->hQueue + (size_t)seen * nq;
        bool all = true;
        for (int i = 0; i < R; ++i) {
          if (qm.finished[(size_t)i]) continue;   // (its slot was not fetched; its rows were taken when it was found finished)
          if ((rc = call_take_polled(c, i, ps[i]))) return rc;
          if (qm.poll(i, ps[i].halt != 0, ps[i].rows_written, pq[1 + i], poll_issued[seen - 1])) all = false;
        }
        if (pq[0] >= R) all_seated = true;
        if (all) stopped = true;
      }
    }
  }
  return call_finish(c);
}

// rows of member `member` from the last chs_batch_step_n_queued: n = its steps_done
extern "C" int chs_batch_member_rows(chs_batch h, int32_t member, double* rows, int64_t n) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_member_rows: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_member_rows: no such member");
  const std::vector<double>* v = (size_t)member < b->qRows.size() ? &b->qRows[(size_t)member] : nullptr;
  const int64_t have = v ? (int64_t)(v->size() / 9) : 0;
  if (n < 0 || n > have) return bad("chs_batch_member_rows: member " + std::to_string(member) + " has " + std::to_string(have) + " rows");
  if (n > 0 && !rows) return bad("chs_batch_member_rows: rows is null");
  if (n > 0) std::memcpy(rows, v->data(), sizeof(double) * 9 * (size_t)n);
  return CHS_OK;
}

// The structure factor of one member -- the single handle's call on the batch's stream -- or of all of them at once.
extern "C" int chs_batch_structure_factor(chs_batch h, int32_t member, double* ssum, int32_t nbins) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_structure_factor: null handle");
  if (member < -1 || member >= b->B) return bad("chs_batch_structure_factor: no such member");
  if (member >= 0) return chs_spectrum_one(b->m[(size_t)member], ssum, nbins, "chs_batch_structure_factor");
  return chs_spectrum_all(b->m.data(), b->B, b->stream, b->chirp, &b->spec, ssum, nbins, "chs_batch_structure_factor");
}

// The morphology of one member -- the single handle's look on the batch's stream -- or of all of them at once.
extern "C" int chs_batch_morphology(chs_batch h, int32_t member, const double* threshold, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_morphology: null handle");
  if (member < -1 || member >= b->B) return bad("chs_batch_morphology: no such member");
  if (member >= 0) return chs_morph_one(b->m[(size_t)member], threshold, out, "chs_batch_morphology");
  return chs_morph_all(b->m.data(), b->B, b->stream, &b->morph, threshold, out, "chs_batch_morphology");
}

// The components of one member: the single handle's look on the batch's stream, with the batch's one set of buffers.
extern "C" int chs_batch_components(chs_batch h, int32_t member, double threshold, int32_t connectivity, int32_t side,
                                    int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_components: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_components: no such member");
  return chs_cc_look(b->m[(size_t)member], b->stream, &b->cc, threshold, connectivity, side, out, "chs_batch_components");
}

extern "C" int chs_batch_components_table(chs_batch h, int64_t rows, int32_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_components_table: null handle");
  return chs_cc_table(b->cc, b->m[0]->hc.device, b->stream, rows, out, "chs_batch_components_table");
}

extern "C" int chs_batch_components_labels(chs_batch h, int32_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_components_labels: null handle");
  return chs_cc_labels(b->cc, b->m[0]->hc.device, b->stream, out, "chs_batch_components_labels");
}

// The distance transform of one member: the single handle's look on the batch's stream, with the batch's one set of buffers.
extern "C" int chs_batch_distance(chs_batch h, int32_t member, double threshold, int32_t side, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_distance: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_distance: no such member");
  return chs_dt_look(b->m[(size_t)member], b->stream, &b->dt, threshold, side, out, "chs_batch_distance");
}

extern "C" int chs_batch_distance_hist(chs_batch h, int32_t nbins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_distance_hist: null handle");
  return chs_dt_hist(b->dt, b->m[0]->hc.device, b->stream, nbins, out, "chs_batch_distance_hist");
}

extern "C" int chs_batch_distance_map(chs_batch h, int32_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_distance_map: null handle");
  return chs_dt_map(b->dt, b->m[0]->hc.device, b->stream, out, "chs_batch_distance_map");
}

// The chord lengths of one member: the single handle's look on the batch's stream, with the batch's one set of buffers.
extern "C" int chs_batch_chords(chs_batch h, int32_t member, double threshold, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_chords: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_chords: no such member");
  return chs_ch_look(b->m[(size_t)member], b->stream, &b->ch, threshold, out, "chs_batch_chords");
}

extern "C" int chs_batch_chords_hist(chs_batch h, int32_t nbins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_chords_hist: null handle");
  return chs_ch_hist(b->ch, b->m[0]->hc.device, b->stream, nbins, out, "chs_batch_chords_hist");
}

// The composition of one member: the single handle's looks on the batch's stream, with the batch's one set of buffers.
extern "C" int chs_batch_composition(chs_batch h, int32_t member, double threshold, int32_t nbins, double lo, double hi,
                                     int64_t* iw, double* fw) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_composition: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_composition: no such member");
  return chs_cmp_look(b->m[(size_t)member], b->stream, &b->cmp, threshold, nbins, lo, hi, iw, fw, "chs_batch_composition");
}

extern "C" int chs_batch_composition_hist(chs_batch h, int32_t nbins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_composition_hist: null handle");
  return chs_cmp_hist(b->cmp, b->m[0]->hc.device, b->stream, nbins, out, "chs_batch_composition_hist");
}

extern "C" int chs_batch_composition_select(chs_batch h, int32_t member, int32_t nq, const int64_t* ranks, double* values) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_composition_select: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_composition_select: no such member");
  return chs_cmp_select(b->m[(size_t)member], b->stream, &b->cmp, nq, ranks, values, "chs_batch_composition_select");
}

extern "C" int chs_batch_composition_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_cmp_last_ms(b, b ? b->cmp : nullptr, ms, "chs_batch_composition");
}

// The two-point correlation of one member: the single handle's look on the batch's stream, with the batch's one set of
// buffers.
extern "C" int chs_batch_two_point(chs_batch h, int32_t member, double threshold, int32_t rmax, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_two_point: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_two_point: no such member");
  return chs_tp_look(b->m[(size_t)member], b->stream, &b->tp, threshold, rmax, out, "chs_batch_two_point");
}

extern "C" int chs_batch_two_point_counts(chs_batch h, int64_t n, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_two_point_counts: null handle");
  return chs_tp_counts(b->tp, b->m[0]->hc.device, b->stream, n, out, "chs_batch_two_point_counts");
}

extern "C" int chs_batch_two_point_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_tp_last_ms(b, b ? b->tp : nullptr, ms, "chs_batch_two_point");
}

// The contour of one member: the single handle's look on the batch's stream, with the batch's one set of buffers.
extern "C" int chs_batch_contour(chs_batch h, int32_t member, double threshold, int32_t bins, double kmax, int32_t want_map,
                                 int64_t* words, double* sums) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_contour: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_contour: no such member");
  return chs_ct_look(b->m[(size_t)member], b->stream, &b->ct, threshold, bins, kmax, want_map, words, sums, "chs_batch_contour");
}

extern "C" int chs_batch_contour_hist(chs_batch h, int32_t bins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_contour_hist: null handle");
  return chs_ct_hist(b->ct, b->m[0]->hc.device, b->stream, bins, out, "chs_batch_contour_hist");
}

extern "C" int chs_batch_contour_map(chs_batch h, int64_t n, double* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_contour_map: null handle");
  return chs_ct_map(b->ct, b->m[0]->hc.device, b->stream, n, out, "chs_batch_contour_map");
}

extern "C" int chs_batch_contour_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_ct_last_ms(b, b ? b->ct : nullptr, ms, "chs_batch_contour");
}

// The droplet shapes of one member: the single handle's look on the batch's stream, with the batch's one set of component
// buffers and one set of shape buffers.
extern "C" int chs_batch_shapes(chs_batch h, int32_t member, double threshold, int32_t connectivity, int32_t side,
                                int64_t out[CHS_SH_WORDS]) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_shapes: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_shapes: no such member");
  return chs_sh_look(b->m[(size_t)member], b->stream, &b->cc, &b->sh, threshold, connectivity, side, out, "chs_batch_shapes");
}

extern "C" int chs_batch_shapes_table(chs_batch h, int64_t rows, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_shapes_table: null handle");
  return chs_sh_table(b->sh, b->m[0]->hc.device, b->stream, rows, out, "chs_batch_shapes_table");
}

// The droplet tracking of one member: the single handle's look on the batch's stream.  The frame is the member's own (in
// its Engine, allocated at its first track look); the component and shape buffers, the hash table and the row list are
// the batch's one set.
extern "C" int chs_batch_track(chs_batch h, int32_t member, double threshold, int32_t connectivity, int32_t side, int32_t keep,
                               int64_t out[CHS_TR_WORDS]) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_track: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_track: no such member");
  Engine* E = b->m[(size_t)member];
  return chs_tr_look(E, b->stream, &b->cc, &b->sh, &E->tr, &b->tr, threshold, connectivity, side, keep, out, "chs_batch_track");
}

extern "C" int chs_batch_track_pairs(chs_batch h, int64_t rows, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_track_pairs: null handle");
  return chs_tr_pairs(b->tr, rows, out, "chs_batch_track_pairs");
}

extern "C" int chs_batch_track_reset(chs_batch h, int32_t member) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_track_reset: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_track_reset: no such member");
  chs_tr_reset(b->m[(size_t)member]->tr);
  return CHS_OK;
}

// The local thickness of one member: the single handle's look on the batch's stream, with the batch's one set of distance
// buffers and one set of thickness buffers.
extern "C" int chs_batch_thickness(chs_batch h, int32_t member, double threshold, int32_t side, int64_t max_work,
                                   int64_t out[CHS_TH_WORDS]) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_thickness: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_thickness: no such member");
  return chs_th_look(b->m[(size_t)member], b->stream, &b->dt, &b->th, threshold, side, max_work, out, "chs_batch_thickness");
}

extern "C" int chs_batch_thickness_hist(chs_batch h, int32_t nbins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_thickness_hist: null handle");
  return chs_th_hist(b->th, b->m[0]->hc.device, b->stream, nbins, out, "chs_batch_thickness_hist");
}

extern "C" int chs_batch_thickness_map(chs_batch h, int32_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_thickness_map: null handle");
  return chs_th_map(b->th, b->m[0]->hc.device, b->stream, out, "chs_batch_thickness_map");
}

extern "C" int chs_batch_thickness_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_th_last_ms(b, b ? b->th : nullptr, ms, "chs_batch_thickness");
}

// The geodesic look at one member: the single handle's look on the batch's stream, with the batch's one set of component
// buffers and one set of geodesic buffers.
extern "C" int chs_batch_geodesic(chs_batch h, int32_t member, double threshold, int32_t connectivity, int32_t side, int32_t source,
                                  int64_t max_rounds, int64_t out[CHS_GEO_WORDS]) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_geodesic: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_geodesic: no such member");
  return chs_geo_look(b->m[(size_t)member], b->stream, &b->cc, &b->geo, threshold, connectivity, side, source, max_rounds, out,
                      "chs_batch_geodesic");
}

extern "C" int chs_batch_geodesic_hist(chs_batch h, int32_t nbins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_geodesic_hist: null handle");
  return chs_geo_hist(b->geo, b->m[0]->hc.device, b->stream, nbins, out, "chs_batch_geodesic_hist");
}

extern "C" int chs_batch_geodesic_profile(chs_batch h, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_geodesic_profile: null handle");
  return chs_geo_profile(b->geo, b->m[0]->hc.device, b->stream, out, "chs_batch_geodesic_profile");
}

extern "C" int chs_batch_geodesic_map(chs_batch h, int32_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_geodesic_map: null handle");
  return chs_geo_map(b->geo, b->m[0]->hc.device, b->stream, out, "chs_batch_geodesic_map");
}

extern "C" int chs_batch_geodesic_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_geo_last_ms(b, b ? b->geo : nullptr, ms, "chs_batch_geodesic");
}

// The skeleton look at one member: the single handle's look on the batch's stream, with the batch's one set of distance
// buffers and one set of skeleton buffers.
extern "C" int chs_batch_skeleton(chs_batch h, int32_t member, double threshold, int32_t side, int64_t max_subiters,
                                  int64_t out[CHS_SK_WORDS]) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_skeleton: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_skeleton: no such member");
  return chs_sk_look(b->m[(size_t)member], b->stream, &b->dt, &b->sk, threshold, side, max_subiters, out, "chs_batch_skeleton");
}

extern "C" int chs_batch_skeleton_hist(chs_batch h, int32_t nbins, int64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_skeleton_hist: null handle");
  return chs_sk_hist(b->sk, b->m[0]->hc.device, b->stream, nbins, out, "chs_batch_skeleton_hist");
}

extern "C" int chs_batch_skeleton_plane(chs_batch h, uint64_t* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_skeleton_plane: null handle");
  return chs_sk_plane(b->sk, b->m[0]->hc.device, b->stream, out, "chs_batch_skeleton_plane");
}

extern "C" int chs_batch_skeleton_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_sk_last_ms(b, b ? b->sk : nullptr, ms, "chs_batch_skeleton");
}

extern "C" int chs_batch_skeleton_thin_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_sk_thin_ms(b, b ? b->sk : nullptr, ms, "chs_batch_skeleton");
}

// The transport look at one member: the single handle's look on the batch's stream, with the batch's one set of component
// buffers and one set of transport buffers.
extern "C" int chs_batch_transport(chs_batch h, int32_t member, double threshold, int32_t side, int32_t source, double tol,
                                   int64_t max_iters, int64_t words[CHS_TRN_WORDS], double vals[CHS_TRN_VALS]) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_transport: null handle");
  if (member < 0 || member >= b->B) return bad("chs_batch_transport: no such member");
  return chs_trn_look(b->m[(size_t)member], b->stream, &b->cc, &b->trn, threshold, side, source, tol, max_iters, words, vals,
                      "chs_batch_transport");
}

extern "C" int chs_batch_transport_profile(chs_batch h, double* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_transport_profile: null handle");
  return chs_trn_profile(b->trn, b->m[0]->hc.device, b->stream, out, "chs_batch_transport_profile");
}

extern "C" int chs_batch_transport_map(chs_batch h, double* out) {
  Batch* b = as_batch(h);
  if (!b) return bad("chs_batch_transport_map: null handle");
  return chs_trn_map(b->trn, b->m[0]->hc.device, b->stream, out, "chs_batch_transport_map");
}

extern "C" int chs_batch_transport_last_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_trn_last_ms(b, b ? b->trn : nullptr, ms, "chs_batch_transport");
}

extern "C" int chs_batch_transport_solve_ms(chs_batch h, double* ms) {
  Batch* b = as_batch(h);
  return chs_trn_solve_ms(b, b ? b->trn : nullptr, ms, "chs_batch_transport");
}
