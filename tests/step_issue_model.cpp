// The host decisions of a call of the single handle (chsimpy_amd/csrc/chs_step_host.h: step_mode, step_issue,
// call_entry) against an independent model, on a CPU (tests/test_step_issue_host.py compiles and runs this).
//
// The model is NOT derived from the header.  It is the issue logic as chs_fast_step and run_steps had it before the
// header existed -- decisions computed between the launches from the engine's fields -- written down as one predicate
// per output over a plain record of those fields (`Parent`).  Every combination of the inputs is compared, then calls
// of 1, 2, 3 and 6 steps are walked through step_issue with the PendingTail carried from step to step, and the
// properties that make a call correct are asserted on the sequence.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chs_step_host.h"

namespace {
long long failures = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 40) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

const int FLIP_MAX = CHS_HAT_FLIP_MAX_N;

// the fields the old step function read: the run's constants, the engine's capabilities and switches, the call's flags
struct Parent {
  bool adaptive, fusedAdapt, partRows, full_sim, tl, profile, twoSets;   // tl: time_limit_s > 0; profile: timer.on
  bool adaptSparse, lamByColmin, gateEarly;
  bool fused, last_call, rederive, keep_t1;
  int N;
};

// ---- the old predicates, one per helper of chs_fast.hip -----------------------------------------------------------
bool hat_flip(const Parent& E) { return !E.adaptive && (!E.full_sim || E.tl) && E.N <= FLIP_MAX && !E.profile && E.twoSets; }
bool can_defer_tail(const Parent& E) { return !E.adaptive && ((!E.tl && E.full_sim) || hat_flip(E)) && !E.profile && E.twoSets; }
bool fused_adaptive(const Parent& E) { return E.adaptive && E.fusedAdapt && E.partRows; }
bool can_skip_u(const Parent& E) { return !E.adaptive || fused_adaptive(E); }
bool keep_resident(const Parent& E) { return E.fused && !E.adaptive && !E.profile && !E.last_call && (!E.rederive || E.keep_t1); }
bool fires(const Parent& E, long long cs) {   // cs: csHost in front of the step
  bool f = true;
  if (E.adaptive && cs >= 0 && E.adaptSparse) { const long long cs_next = cs + 1; f = (cs_next > 500 && (cs_next % 2) == 0); }
  return f;
}
// ---- ... and one per thing the step issued ------------------------------------------------------------------------
bool m_sweep0(const Parent& E, bool first) { return first && E.adaptive; }
int m_pre(const Parent& E, bool first) { return !first ? PRE_NONE : (can_defer_tail(E) ? PRE_RIDES : PRE_LAUNCH); }
int m_row_mode(const Parent& E, bool last) {
  if (last && keep_resident(E)) return ROW_INV_FUSED;
  return last ? ROW_INV_DIAG : (fused_adaptive(E) ? ROW_INV_FUSED_ADAPT : ROW_INV_FUSED);
}
int m_store_u(const Parent& E, bool last) {   // what the row kernel got; ROW_INV_DIAG always stores
  if (last) return 1;
  return can_skip_u(E) ? 0 : 1;
}
bool m_lam_by_colmin(const Parent& E, long long cs, bool last) {
  const long long after = cs >= 0 ? cs + 1 : cs;   // (csHost was incremented in front of the row kernel)
  return !last && fused_adaptive(E) && fires(E, cs) && after >= 0 && E.adaptSparse && E.lamByColmin && E.full_sim && !E.tl && !E.profile;
}
int m_reduce(const Parent& E, long long cs, bool last) {
  const bool fa = fused_adaptive(E);
  if (!last && E.adaptive && (fires(E, cs) || !fa)) return fa ? REDUCE_COLMIN : REDUCE_SWEEP;
  return REDUCE_NONE;
}
bool m_gate(const Parent& E) { return !can_defer_tail(E) && !E.profile && E.twoSets; }
bool m_tail_now(const Parent& E, bool last) { return last || (!can_defer_tail(E) && !m_gate(E)); }
bool m_quiet(const Parent& E, long long cs, bool last) {
  return (!fires(E, cs) || m_lam_by_colmin(E, cs, last)) && fused_adaptive(E) && E.full_sim && !E.tl;
}
bool m_gated(const Parent& E, long long cs, bool last) { return m_gate(E) && !m_quiet(E, cs, last); }
bool m_early(const Parent& E, long long cs, bool last) {
  const long long after = cs >= 0 ? cs + 1 : cs;
  return m_gated(E, cs, last) && fires(E, cs) && fused_adaptive(E) && E.full_sim && !E.tl && after >= 0 && E.adaptSparse && E.gateEarly;
}

CallFacts facts(const Parent& E) {
  CallFacts f;
  f.adaptive = E.adaptive; f.full_sim = E.full_sim; f.time_limit_s = E.tl ? 3600.0 : 0.0; f.N = E.N;
  f.fused = E.fused; f.fusedAdapt = E.fusedAdapt; f.partRows = E.partRows; f.twoSets = E.twoSets;
  f.adaptSparse = E.adaptSparse; f.lamByColmin = E.lamByColmin; f.gateEarly = E.gateEarly;
  f.profile = E.profile; f.rederive = E.rederive; f.keep_t1 = E.keep_t1; f.last_call = E.last_call;
  return f;
}

Parent parent_of(unsigned b) {   // 14 bits + N
  Parent E;
  E.adaptive = b & 1; E.fusedAdapt = b & 2; E.partRows = b & 4; E.full_sim = b & 8; E.tl = b & 16; E.profile = b & 32;
  E.twoSets = b & 64; E.adaptSparse = b & 128; E.lamByColmin = b & 256; E.gateEarly = b & 512;
  E.last_call = b & 1024; E.rederive = b & 2048; E.keep_t1 = b & 4096;
  E.N = (b & 8192) ? 2 * FLIP_MAX : FLIP_MAX;
  E.fused = true;   // (chs_fast_step runs on the fused pipeline alone)
  return E;
}
const unsigned PARENTS = 1u << 14;

void check_modes_and_steps() {
  const long long counters[5] = {-1, 499, 500, 501, 502};
  for (unsigned b = 0; b < PARENTS; ++b) {
    const Parent E = parent_of(b);
    const StepMode m = step_mode(facts(E), FLIP_MAX);
    // what run_steps reads of the mode
    CHECK(m.hatFlip == hat_flip(E), "b=%u", b);
    CHECK(m.keepResident == keep_resident(E), "b=%u", b);
    CHECK(m.storesU == !can_skip_u(E), "b=%u", b);
    CHECK(m.stopArmed == (!E.full_sim || E.tl), "b=%u", b);
    Parent J = E;
    J.fused = false;   // a jitter run or another engine: the step function never runs, nothing of it may show
    const StepMode mj = step_mode(facts(J), FLIP_MAX);
    CHECK(!mj.hatFlip && !mj.keepResident, "b=%u without the fused pipeline", b);
    for (int fl = 0; fl < 4; ++fl)
      for (long long cs : counters) {
        const bool first = fl & 1, last = fl & 2;
        const StepIssue p = step_issue(m, cs, first, last);
        ++cases;
        CHECK(p.sweep0 == m_sweep0(E, first), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        CHECK(p.pre == m_pre(E, first), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        CHECK(p.flip == hat_flip(E), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        CHECK(p.row_mode == m_row_mode(E, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        CHECK(p.store_u == m_store_u(E, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        CHECK(p.reduce == m_reduce(E, cs, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        if (p.reduce == REDUCE_COLMIN) CHECK(p.decide == m_lam_by_colmin(E, cs, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        else CHECK(!p.decide, "b=%u first=%d last=%d cs=%lld: decide without the reduction", b, first, last, cs);
        CHECK(p.tail_now == m_tail_now(E, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        CHECK(p.flips_parity() == !m_tail_now(E, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        if (p.tail_now) {
          CHECK(p.do_pre == (last ? 0 : 1), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
          CHECK(!p.next.any && !p.next.gated && !p.next.early, "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        } else {
          CHECK(p.next.any, "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
          CHECK(p.next.gated == m_gated(E, cs, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
          CHECK(p.next.early == m_early(E, cs, last), "b=%u first=%d last=%d cs=%lld", b, first, last, cs);
        }
      }
  }
}

// ---- the entry of a call: the old chain of run_steps --------------------------------------------------------------
struct OldEntry { int kind; bool entered, prologue, resident, hat_valid; };
OldEntry old_entry(bool fused, bool carry, bool rederive, bool keep_t1, bool profile, bool resident, bool hat_valid, int64_t nsteps) {
  OldEntry o = {-1, false, false, resident, hat_valid};
  const bool derive = !(carry && hat_valid);
  const bool cont = fused && resident && hat_valid && !rederive && !profile;
  const bool cont_t1 = fused && resident && rederive && keep_t1 && !profile;
  if (nsteps > 0) o.resident = false;
  if (cont && nsteps > 0) {
    o.kind = ENTRY_CONTINUE;
  } else if (cont_t1 && nsteps > 0) {
    o.kind = ENTRY_HAT_ONLY; o.hat_valid = true;
  } else if (derive && fused && nsteps > 0) {
    o.kind = ENTRY_FUSED; o.hat_valid = true;
  } else {
    o.kind = ENTRY_PLAIN;
    if (derive) o.entered = true;
    o.hat_valid = true;
    if (fused && nsteps > 0) o.prologue = true;
  }
  return o;
}

void check_entries() {
  const int64_t lengths[3] = {0, 1, 5};
  for (unsigned b = 0; b < 128; ++b)
    for (int64_t n : lengths) {
      CallFacts f;
      f.fused = b & 1; f.carry_hat = b & 2; f.rederive = b & 4; f.keep_t1 = b & 8; f.profile = b & 16;
      f.resident = b & 32; f.hat_valid = b & 64; f.nsteps = n;
      const CallEntry e = call_entry(f);
      const OldEntry o = old_entry(f.fused, f.carry_hat, f.rederive, f.keep_t1, f.profile, f.resident, f.hat_valid, n);
      ++cases;
      CHECK(e.kind == o.kind, "b=%u n=%lld: %d, the chain took %d", b, (long long)n, e.kind, o.kind);
      CHECK((e.kind == ENTRY_PLAIN && e.derive) == o.entered, "b=%u n=%lld", b, (long long)n);
      CHECK((e.kind == ENTRY_PLAIN && e.prologue) == o.prologue, "b=%u n=%lld", b, (long long)n);
      if (e.kind != ENTRY_PLAIN) CHECK(!e.derive && !e.prologue, "b=%u n=%lld", b, (long long)n);
      CHECK(e.resident == o.resident && e.hat_valid == o.hat_valid, "b=%u n=%lld", b, (long long)n);
    }
  // the buffer behind the completed steps: the call's first one after an even number of them
  for (int64_t done = 0; done < 9; ++done) CHECK((hat_after_flip(done) == 0) == ((done & 1) == 0), "done=%lld", (long long)done);
}

// ---- whole calls ---------------------------------------------------------------------------------------------------
void walk(unsigned b, const Parent& E, const StepMode& m, long long cs0, int n) {
  PendingTail pend;
  int parity = 0, pre_runs = 0;
  long long cs = cs0;
  std::vector<int> record((size_t)n, 0), control((size_t)n, 0);   // per step: its record, its time-step control
#define WHERE "b=%u cs0=%lld n=%d s=%d", b, cs0, n, s
  for (int s = 0; s < n; ++s) {
    const bool first = s == 0, last = s == n - 1;
    const StepIssue p = step_issue(m, cs, first, last);
    ++cases;
    if (p.pre != PRE_NONE) { ++pre_runs; ++control[(size_t)s]; CHECK(first, WHERE); }
    CHECK(!p.sweep0 || (first && p.pre != PRE_NONE), WHERE);
    // k_col of this step: one rider at most
    CHECK(!(p.pre == PRE_RIDES && pend.any), WHERE);
    if (pend.any) {
      ++record[(size_t)s - 1]; ++control[(size_t)s];    // (a riding tail always runs the next step's control: do_pre = 1)
      CHECK(pend.set != parity, WHERE);                  // this step's kernels do not write the sums the rider reads
      CHECK(!(pend.gated && p.flip), WHERE);             // the flip exists so that nothing waits
      CHECK(!pend.early || pend.gated, WHERE);
    }
    pend = PendingTail();
    if (cs >= 0) cs += 1;
    // U: a step that does not store it is followed by nothing that reads it from HBM -- no sweep of U behind it, a
    // next step in the same call (whose control comes from the tail, not from a sweep), and never the call's last step
    if (p.store_u == 0) CHECK(!last && p.reduce != REDUCE_SWEEP && (p.row_mode == ROW_INV_FUSED || p.row_mode == ROW_INV_FUSED_ADAPT), WHERE);
    if (last) CHECK(p.store_u == 1 && (p.row_mode == ROW_INV_DIAG || (p.row_mode == ROW_INV_FUSED && m.keepResident)), WHERE);
    CHECK((p.row_mode == ROW_INV_FUSED_ADAPT) == (!last && m.fusedAdaptive), WHERE);
    if (p.decide) CHECK(E.full_sim && !E.tl && !E.profile && cs0 >= 0 && p.reduce == REDUCE_COLMIN, WHERE);
    if (p.tail_now) {
      ++record[(size_t)s];
      if (p.do_pre) { CHECK(!last, WHERE); if (!last) ++control[(size_t)s + 1]; }
      else CHECK(last, WHERE);
      CHECK(!p.flips_parity(), WHERE);
    } else {
      CHECK(!last && p.next.any && p.flips_parity(), WHERE);
      pend = p.next;
      pend.set = parity;
      parity ^= 1;
    }
  }
  const int s = n;
  CHECK(!pend.any, WHERE);   // nothing is left behind the last step
  CHECK(pre_runs == 1, WHERE);
  for (int k = 0; k < n; ++k) CHECK(record[(size_t)k] == 1 && control[(size_t)k] == 1, "b=%u cs0=%lld n=%d step %d: record %d, control %d", b, cs0, n, k, record[(size_t)k], control[(size_t)k]);
#undef WHERE
}

void check_walks() {
  const long long starts[5] = {-1, 1, 497, 499, 600};
  const int lengths[4] = {1, 2, 3, 6};
  for (unsigned b = 0; b < PARENTS; ++b) {
    const Parent E = parent_of(b);
    const StepMode m = step_mode(facts(E), FLIP_MAX);
    for (long long cs0 : starts)
      for (int n : lengths) walk(b, E, m, cs0, n);
  }
}
}  // namespace

int main() {
  for (long long cs = -3; cs < 520; ++cs) CHECK(rule_fires(cs) == (cs > 500 && cs % 2 == 0), "cs=%lld", cs);
  CHECK(stop_armed(true, 0.0) == false && stop_armed(false, 0.0) && stop_armed(true, 1.0) && stop_armed(false, 1.0), "stop_armed");
  check_modes_and_steps();
  check_entries();
  check_walks();
  std::printf("%lld cases, %lld failures\n", cases, failures);
  return failures ? 1 : 0;
}
