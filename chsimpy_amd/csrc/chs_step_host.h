// chs_step_host.h -- the decisions of a call of the single handle that the host takes without looking at the device:
// how the call is entered (call_entry), what is constant over its steps (StepMode) and what one step of the fused
// pipeline issues (step_issue).  Plain C++, nothing of HIP: chs_api.hip and chs_fast.hip execute what these functions
// return, tests/step_issue_model.cpp checks them on a CPU against a model written from the launch sequences they
// replaced.  The device has its own copies of the firing rule (k_mu, k_pre, k_colsum_slices, k_colmin_slices,
// batch_member_fires, chs_tail.h): the kernels check again whatever the host decided.
#pragma once
#include <stdint.h>

// the row kernel of a step (FastPlan::row_inv, FastPlan::row_inv_batch)
enum { ROW_INV_PLAIN = 0, ROW_INV_DIAG = 1, ROW_INV_FUSED = 2, ROW_INV_FUSED_ADAPT = 3 };

// Stop rules on the small grids keep the tail deferred by alternating two hat_U buffers (StepMode::hatFlip).  The
// tiles of a small grid reach a gate before the riding tail has decided (N=512: 26.5 against 23.9 us/step); at N=4096
// the gate costs 1 % and a third 134 MB array would not fit beside T and hat_U in the Infinity Cache.
#ifndef CHS_HAT_FLIP_MAX_N
#define CHS_HAT_FLIP_MAX_N 2048
#endif

// The step-size rule looks at the counter behind a step's record: every second step beyond step 500 (solver.py:177).
inline bool rule_fires(long long cs) { return cs > 500 && (cs % 2) == 0; }

// Can the energy rule or the time limit end the run?  (Only NaN stops a run with neither.)
inline bool stop_armed(bool full_sim, double time_limit_s) { return !full_sim || time_limit_s > 0.0; }

// The fused row kernel of the steps inside a call and whether it stores U.  Between the steps of a call nothing reads U
// from HBM, so the kernel keeps it in registers -- unless the step-size integrand comes from a sweep of U (an adaptive
// run whose row kernel does not add it up itself: `fused_adaptive` false).  The single handle and both issue loops of
// the batch take it from here.
struct RowMode { int mode, store_u; };
inline RowMode fused_row_mode(bool adaptive, bool fused_adaptive) {
  return {fused_adaptive ? ROW_INV_FUSED_ADAPT : ROW_INV_FUSED, (adaptive && !fused_adaptive) ? 1 : 0};
}

// What a call finds and is asked for: the inputs of call_entry and step_mode, scalars only.
struct CallFacts {
  // the run's constants
  bool adaptive = false, full_sim = true;
  double time_limit_s = 0.0;
  int N = 0;
  // the engine: `fused` = the fast engine without jitter (the fused pipeline runs the steps); fusedAdapt, adaptSparse,
  // lamByColmin, gateEarly as chs_fast_rearm read them (CHS_ADAPT_SWEEP, CHS_ADAPT_SPARSE, CHS_LAM_BY_COLMIN,
  // CHS_GATE_EARLY); partRows / twoSets: the partial rows of the step-size integrand / the second set of partial sums exist
  bool fused = false, fusedAdapt = false, partRows = false, twoSets = false;
  bool adaptSparse = true, lamByColmin = true, gateEarly = false;
  // the call: profiling, CHS_STEP_CARRY_HAT, CHS_STEP_REDERIVE_HAT, CHS_STEP_KEEP_T1, CHS_STEP_LAST_CALL
  bool profile = false, carry_hat = false, rederive = false, keep_t1 = false, last_call = false;
  int64_t nsteps = 0;
  // what the previous call left (Engine::resident, Engine::hat_valid)
  bool resident = false, hat_valid = false;
};

// ---------------------------------------------------------------------------
// The entry of a call
// ---------------------------------------------------------------------------
// Fixed time step on the fused pipeline: the last step of a call leaves hat_U, the row transform of EnergieEut(U) and
// its sum of squares on the device, and a call that finds them continues the loop where it stopped (ENTRY_CONTINUE) --
// hat_U is the array the reference would recompute as dctn(idctn(hat_U)) (solver.py:159), equal up to rounding;
// CHS_STEP_REDERIVE_HAT asks for the literal recomputation.  Such a call gets hat_U = dctn(U) recomputed at every call;
// what it still takes over from its predecessor is the OTHER thing the last fused step leaves: T1 = the row transform
// of EnergieEut(U) and its sum of squares -- a function of the unchanged field U alone, which k_row_fwd2 would only
// compute again bit for bit -- when the caller allows it (ENTRY_HAT_ONLY; CHS_STEP_KEEP_T1, off by default: measured,
// it buys nothing at N=4096 -- the entry shrinks from 215 to 152 us, the call's last step, now the fused kernel, grows
// by as much: profiles/r04_ab_entry.txt).
enum {
  ENTRY_CONTINUE = 0,  // nothing to do: T1, partMu and hat_U are in place
  ENTRY_HAT_ONLY = 1,  // hat_U = dctn(U), literally; T1 and partMu are in place (chs_fast_enter_hat)
  ENTRY_FUSED = 2,     // hat_U = dctn(U) and the first step's row transform of EnergieEut(U) from one sweep of U
  ENTRY_PLAIN = 3      // hat_U = dctn(U) where `derive`, then the fused pipeline's prologue where `prologue`
};
struct CallEntry {
  int kind;
  bool derive, prologue;     // ENTRY_PLAIN alone
  bool resident, hat_valid;  // Engine::resident / hat_valid behind the entry (every entry leaves hat_U valid)
};
inline CallEntry call_entry(const CallFacts& f) {
  const bool steps = f.nsteps > 0;
  const bool warm = f.fused && f.resident && !f.profile && steps;
  const bool derive = !(f.carry_hat && f.hat_valid);
  CallEntry e = {ENTRY_PLAIN, false, false, f.resident && !steps, true};
  if (warm && f.hat_valid && !f.rederive) e.kind = ENTRY_CONTINUE;
  else if (warm && f.rederive && f.keep_t1) e.kind = ENTRY_HAT_ONLY;
  else if (derive && f.fused && steps) e.kind = ENTRY_FUSED;
  else { e.derive = derive; e.prologue = f.fused && steps; }
  return e;
}

// Two hat_U buffers alternated per ISSUED step (StepMode::hatFlip): the one that holds the state behind the steps that
// were COMPLETED is the call's first one (0) after an even number of them, the other one (1) after an odd number.
inline int hat_after_flip(int64_t completed_steps) { return (int)(completed_steps & 1); }

// ---------------------------------------------------------------------------
// What is constant over the steps of a call
// ---------------------------------------------------------------------------
struct StepMode {
  bool adaptive = false;
  // the fused row kernel adds up the step-size integrand per column itself (ROW_INV_FUSED_ADAPT); otherwise an
  // adaptive run sweeps U for it (chs_launch_mu_colsums) and the row kernel has to store U on every step
  bool fusedAdaptive = false;
  bool storesU = false;
  // the energy rule or the time limit can end the call early.  Then the tail runs in stream order behind the row
  // kernel or gates the next k_col: hat_U is still that of the last completed step when the run stops, and run_steps
  // rebuilds U = idctn(hat_U) once (chs_fast_recover_u) where the row kernel has not been storing it
  bool stopArmed = false;
  // Stop rules on the small grids (N <= CHS_HAT_FLIP_MAX_N, fixed time step): k_col reads hat_U from one buffer and
  // writes the other, alternating from step to step, so the tail can stay deferred -- when it stops the run, the
  // buffer the carrying k_col READ is the state of the last completed step (run_steps points dHat at it, hat_after_flip)
  bool hatFlip = false;
  // Fixed time step with nothing armed (or the hat flip): the tail of step s decides nothing the column pass of step
  // s+1 needs.  It is deferred and rides as one extra workgroup in k_col of step s+1 -- no launch of its own, nothing
  // waits for it.  Only NaN can stop such a run (one kernel later; the field is unspecified then anyway).  The partial
  // sums alternate between two sets.  The first step's time-step control rides in the same way in its own k_col.
  bool deferTail = false;
  // Every other run that is not being profiled (stop rules armed, or an adaptive time step): the bookkeeping still
  // rides in the next k_col, whose other workgroups wait for its decision in front of their first global write (gated
  // tail, gate_wait) -- no 14 us one-block launch per step.  A run being profiled keeps the separate launch.
  bool gateTail = false;
  bool profile = false;
  // Adaptive step with the host able to follow the step counter: only the steps whose rule fires need the column sums
  // reduced and the next k_col gated (its coefficients change).  On the others -- with nothing else armed that a tail
  // could decide -- the reduction launches are not issued at all (they used to return at once: two empty launches per
  // step) and the bookkeeping rides ungated.  (CHS_ADAPT_SPARSE=0: every step as if its rule fired.)
  bool adaptSparse = true;
  // A firing step with nothing else armed: the reduction's last block works out the coming step's coefficients itself
  // (k_colmin_slices, `decide`), so the next k_col needs no gate either -- its tiles read them from the state as ever
  bool lamByColmin = true;
  // ... or, gated, lets the tiles have their coefficients ahead of the record (chs_tail.h; CHS_GATE_EARLY=1: measured
  // equal -- what a gated k_col pays is its own check of the gate, not the wait for the decision -- an experiment switch)
  bool gateEarly = false;
  // the last step of the call leaves the field in HBM like ROW_INV_DIAG, and with it what the first column pass of a
  // following call needs (T1, sum(mu^2)): that call then starts without an entry pass (ENTRY_CONTINUE / _HAT_ONLY)
  bool keepResident = false;
};

inline StepMode step_mode(const CallFacts& f, int hat_flip_max_n = CHS_HAT_FLIP_MAX_N) {
  StepMode m;
  const bool rides = !f.profile && f.twoSets;   // the bookkeeping can ride in a k_col at all
  m.adaptive = f.adaptive;
  m.fusedAdaptive = f.adaptive && f.fusedAdapt && f.partRows;
  m.storesU = fused_row_mode(m.adaptive, m.fusedAdaptive).store_u != 0;
  m.stopArmed = stop_armed(f.full_sim, f.time_limit_s);
  m.hatFlip = f.fused && !f.adaptive && m.stopArmed && f.N <= hat_flip_max_n && rides;
  m.deferTail = !f.adaptive && (!m.stopArmed || m.hatFlip) && rides;
  m.gateTail = rides && !m.deferTail;
  m.profile = f.profile;
  m.adaptSparse = f.adaptSparse; m.lamByColmin = f.lamByColmin; m.gateEarly = f.gateEarly;
  m.keepResident = f.fused && !f.adaptive && !f.profile && !f.last_call && (!f.rederive || f.keep_t1);
  return m;
}

// ---------------------------------------------------------------------------
// One step of the fused pipeline
// ---------------------------------------------------------------------------
// The only thing one step hands to the next: its tail -- the record of the step and the time-step control of the next
// one -- still to run, as the extra workgroup of the next k_col.
struct PendingTail {
  bool any = false;
  bool gated = false;   // the other workgroups of that k_col wait for its decision
  bool early = false;   // ... and get the coefficients ahead of the record (StepMode::gateEarly)
  int set = 0;          // the set of partial sums it reads (the executing side fills it in: Engine::parity)
};
// What rides in a k_col<MODE_STEP> as its extra workgroup (FastPlan::col): nothing, the first step's time-step control
// alone, or the previous step's tail.
struct ColRider {
  bool pre_only = false;
  PendingTail tail;
};
inline ColRider no_rider() { return ColRider(); }
inline ColRider pre_rider() { ColRider r; r.pre_only = true; return r; }
inline ColRider tail_rider(const PendingTail& t) { ColRider r; r.tail = t; return r; }

enum { PRE_NONE = 0, PRE_LAUNCH = 1, PRE_RIDES = 2 };          // the first step's time-step control
enum { REDUCE_NONE = 0, REDUCE_COLMIN = 1, REDUCE_SWEEP = 2 };  // chs_launch_colmin_rows(E, 1, decide) / chs_launch_mu_colsums(E, 1)
struct StepIssue {
  // in front of k_col: the time-step control of the first step of the call (later steps get it from the tail), behind
  // the sweep chs_launch_mu_colsums(E, 0) of an adaptive run (the prologue wrote sum(mu^2) into the set that was
  // current then: folded in here)
  bool sweep0;
  int pre;
  bool flip;             // k_col writes the second hat_U buffer, the two change places
  int row_mode, store_u;
  // behind the row kernel: the column sums of the adaptive-step integrand of the NEXT step (solver.py:183); the record
  // of this step has not advanced computed_steps yet, hence the offset 1
  int reduce;
  bool decide;
  bool tail_now;         // chs_launch_step_tail(E, do_pre) ...
  int do_pre;
  PendingTail next;      // ... or the tail rides in the next k_col; the partial-set parity flips with it
  bool flips_parity() const { return next.any; }
};

// csHost: the device's computed_steps in front of this step as the host can follow it, < 0 = not known.
inline StepIssue step_issue(const StepMode& m, long long csHost, bool first, bool last) {
  StepIssue p = {};
  p.sweep0 = first && m.adaptive;
  p.pre = !first ? PRE_NONE : (m.deferTail ? PRE_RIDES : PRE_LAUNCH);
  p.flip = m.hatFlip;
  const bool fa = m.fusedAdaptive;
  // the counter behind this step's record is csHost + 1 (chs_tail.h: cs_next); an unknown counter fires
  const bool follows = m.adaptive && csHost >= 0 && m.adaptSparse;
  const bool fires = !follows || rule_fires(csHost + 1);
  const RowMode rm = fused_row_mode(m.adaptive, fa);
  p.row_mode = !last ? rm.mode : (m.keepResident ? ROW_INV_FUSED : ROW_INV_DIAG);
  p.store_u = last ? 1 : rm.store_u;
  p.decide = !last && fa && follows && fires && m.lamByColmin && !m.stopArmed && !m.profile;
  p.reduce = (last || !m.adaptive || (fa && !fires)) ? REDUCE_NONE : (fa ? REDUCE_COLMIN : REDUCE_SWEEP);
  p.tail_now = last || !(m.deferTail || m.gateTail);
  p.do_pre = last ? 0 : 1;
  if (p.tail_now) return p;
  // (an adaptive step whose rule does not fire, or whose reduction decides, leaves nothing for the next k_col to wait
  // for -- unless a stop rule is armed)
  const bool quiet = (!fires || p.decide) && fa && !m.stopArmed;
  p.next.any = true;
  p.next.gated = m.gateTail && !quiet;
  p.next.early = p.next.gated && fa && follows && fires && !m.stopArmed && m.gateEarly;
  return p;
}
