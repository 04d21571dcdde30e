// The host decisions of the seat queue (chsimpy_amd/csrc/chs_batch_host.h) driven step by step against a plain C++
// model of the seat kernel's rule, on a CPU (tests/test_batch_queue_host.py compiles and runs this).  The loop below
// is the issue loop of chs_batch_step_n_queued with the launches replaced by the model: polls behind every
// `batch_steps` steps, each looked at two batches late.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chs_batch_host.h"

namespace {
int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Member { int64_t nsteps, rows = 0, halt_at, seat_step = -1; bool halt = false; };

// k_seat_batch's rule: the seats in ascending order; a seat is free when its member has halted or has written nsteps
// rows (a vacant seat: nobody there); it goes to the next member in order that has steps to do and has not halted.
void seat_kernel(std::vector<int>& seat, std::vector<Member>& m, std::vector<long long>& q, long long step) {
  const long long R = (long long)m.size();
  long long head = q[0];
  for (size_t j = 0; j < seat.size() && head < R; ++j) {
    if (seat[j] >= 0 && !m[(size_t)seat[j]].halt && m[(size_t)seat[j]].rows < m[(size_t)seat[j]].nsteps) continue;
    while (head < R && !(m[(size_t)head].nsteps > 0 && !m[(size_t)head].halt)) ++head;
    if (head >= R) break;
    seat[j] = (int)head;
    q[1 + (size_t)head] = step;
    m[(size_t)head].seat_step = step;
    ++head;
  }
  q[0] = head < R ? head : R;
}

// nsteps: the call lengths; halt_at[i] >= 0: member i halts when it has written that many rows (0: in front of its
// first step, the `pre_only` tail of the entry)
void run_case(const char* name, const std::vector<int64_t>& nsteps, const std::vector<int64_t>& halt_at, int seats,
              int batch_steps) {
  const int R = (int)nsteps.size();
  const int S = seats < R ? seats : R;
  std::vector<Member> m((size_t)R);
  int running = 0;
  bool early = false;
  for (int i = 0; i < R; ++i) {
    m[(size_t)i].nsteps = nsteps[(size_t)i] > 0 ? nsteps[(size_t)i] : 0;
    m[(size_t)i].halt_at = halt_at.empty() ? -1 : halt_at[(size_t)i];
    if (m[(size_t)i].nsteps > 0 && m[(size_t)i].halt_at >= 0 && m[(size_t)i].halt_at < m[(size_t)i].nsteps) early = true;
    if (m[(size_t)i].nsteps > 0 && m[(size_t)i].halt_at == 0) m[(size_t)i].halt = true;
    running += nsteps[(size_t)i] > 0;
  }
  std::vector<int> seat((size_t)S, -1);
  std::vector<long long> q(1 + (size_t)R, -1);
  q[0] = 0;
  const int64_t bound = queue_step_bound(nsteps.data(), R, S);
  if (running > 0) seat_kernel(seat, m, q, 0);
  QueueMembers qm(nsteps.data(), R, S);
  bool all_seated = running <= S;
  std::vector<char> pair_on((size_t)bound + 1, 0);
  // the pinned poll slots: the members' states and the queue as the fetch behind the batch finds them
  std::vector<std::vector<Member>> slot_m(4);
  std::vector<std::vector<long long>> slot_q(4);
  int64_t issued = 0, poll_issued[4] = {0, 0, 0, 0};
  int poll = 0;
  bool stopped = false;
  while (issued < bound && !stopped) {
    int64_t nb = bound - issued;
    if (nb > batch_steps) nb = batch_steps;
    for (int64_t s = issued; s < issued + nb; ++s) {
      const bool last = qm.last_pair(s);
      pair_on[(size_t)s] = last;
      for (int j : seat) {   // the step kernels, seat by seat
        if (j < 0) continue;
        Member& x = m[(size_t)j];
        if (x.halt || x.rows >= x.nsteps) continue;
        if (x.rows == x.nsteps - 1)
          CHECK(last, "member %d (seated at %lld, %lld steps) has its last step at %lld without the last-step pair", j,
                (long long)x.seat_step, (long long)x.nsteps, (long long)s);
        ++x.rows;
        if (x.rows == x.halt_at && x.rows < x.nsteps) x.halt = true;
      }
      if (!all_seated && ((s + 1) & 1) == 0 && s + 1 < bound) seat_kernel(seat, m, q, (long long)(s + 1));
    }
    issued += nb;
    if (issued < bound) {
      slot_m[(size_t)(poll & 3)] = m;
      slot_q[(size_t)(poll & 3)] = q;
      poll_issued[poll & 3] = issued;
      if (poll >= 1) {
        const int prev = (poll - 1) & 3;
        const std::vector<Member>& ps = slot_m[(size_t)prev];
        const std::vector<long long>& pq = slot_q[(size_t)prev];
        bool all = true;
        for (int i = 0; i < R; ++i) {
          if (qm.finished[(size_t)i]) continue;
          if (qm.poll(i, ps[(size_t)i].halt, ps[(size_t)i].rows, pq[1 + (size_t)i], poll_issued[prev])) all = false;
        }
        if (pq[0] >= R) all_seated = true;
        if (all) stopped = true;
      }
      ++poll;
    }
  }
  int64_t finish = 0;
  for (int i = 0; i < R; ++i) {
    const Member& x = m[(size_t)i];
    if (x.nsteps <= 0) { CHECK(x.seat_step < 0, "member %d has no step to do and was seated", i); continue; }
    CHECK(x.halt || x.rows >= x.nsteps, "member %d was left with steps to do: %lld of %lld after %lld issued (bound %lld)", i,
          (long long)x.rows, (long long)x.nsteps, (long long)issued, (long long)bound);
    if (x.seat_step < 0) continue;   // (halted in front of its first step: never seated)
    const bool whole = !x.halt;
    if (whole) {
      const int64_t at = x.seat_step + x.nsteps - 1;
      CHECK(at < bound && pair_on[(size_t)at], "member %d: no last-step pair on step %lld", i, (long long)at);
    }
    const int64_t end = x.seat_step + x.rows;
    if (end > finish) finish = end;
  }
  if (early) CHECK(bound >= finish, "bound %lld below the finishing step %lld", (long long)bound, (long long)finish);
  else CHECK(bound == finish, "bound %lld is not the finishing step %lld", (long long)bound, (long long)finish);
  if (seats >= running) {
    int64_t mx = 0;
    for (int64_t n : nsteps) if (n > mx) mx = n;
    CHECK(bound == mx, "a seat for everybody: bound %lld is not the longest call %lld", (long long)bound, (long long)mx);
  }
}

void fires_cases() {
  const char* name = "batch_rule_fires";
  CHECK(!batch_rule_fires(-1, 10, 9) && !batch_rule_fires(600, 10, 9) && !batch_rule_fires(600, 10, 12), "a step behind the last one");
  CHECK(batch_rule_fires(-1, 10, 0) && batch_rule_fires(-1, 10, 8), "an unknown counter fires");
  CHECK(!batch_rule_fires(1, 2000, 498) && !batch_rule_fires(1, 2000, 499), "cs_next = 500, 501");
  CHECK(batch_rule_fires(1, 2000, 500) && !batch_rule_fires(1, 2000, 501) && batch_rule_fires(1, 2000, 502), "cs_next = 502, 503, 504");
  CHECK(!batch_rule_fires(0, 2000, 400) && batch_rule_fires(700, 5, 1) && !batch_rule_fires(700, 5, 0), "parity follows the counter");
}
}  // namespace

int main() {
  const std::vector<int64_t> A = {5, 2, 9, 1, 4, 0, 3}, B = {2, 2, 0, 3, 1, 4, 2};
  const std::vector<int64_t> none;
  char name[96];
  int cases = 0;
  for (const std::vector<int64_t>* L : {&A, &B})
    for (int seats : {1, 2, 7, 16})
      for (int bs : {1, 4, 1024}) {
        std::snprintf(name, sizeof name, "lengths %c seats %d batch_steps %d", L == &A ? 'A' : 'B', seats, bs);
        run_case(name, *L, none, seats, bs);
        // members 1 and 3 halt early, at steps 1 and 2 (where their call is longer than that)
        std::vector<int64_t> h(L->size(), -1);
        h[1] = 1; h[3] = 2;
        std::snprintf(name, sizeof name, "lengths %c seats %d batch_steps %d, members 1 and 3 halt", L == &A ? 'A' : 'B', seats, bs);
        run_case(name, *L, h, seats, bs);
        cases += 2;
      }
  // longer calls, so that polls are looked at while members wait, run and change seats; a member stopped by the entry
  const std::vector<int64_t> Cn = {37, 12, 0, 25, 8, 40, 3, 19, 1, 22}, Ch = {-1, 1, -1, 2, 0, 13, -1, -1, -1, 21};
  for (int seats : {1, 2, 3, 7, 16})
    for (int bs : {1, 3, 4, 1024}) {
      std::snprintf(name, sizeof name, "lengths C seats %d batch_steps %d", seats, bs);
      run_case(name, Cn, none, seats, bs);
      std::snprintf(name, sizeof name, "lengths C seats %d batch_steps %d, early halts", seats, bs);
      run_case(name, Cn, Ch, seats, bs);
      cases += 2;
    }
  fires_cases();
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
