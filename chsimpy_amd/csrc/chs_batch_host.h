// chs_batch_host.h -- the decisions of a batched call that the host takes without looking at the device: how many
// steps a seat queue issues, on which steps the last-step kernel pair goes out while the host knows a member's seating
// step only as a lower bound, and whether a member's step-size rule can fire behind a step.  Plain C++, nothing of HIP:
// chs_batch.hip runs this code, tests/batch_queue_model.cpp drives it against a model of the seat kernel on a CPU.
#pragma once
#include <stdint.h>
#include <vector>

#include "chs_step_host.h"

// The global step count of a queued call when no member stops early: the members take the seats in member order, a
// seat changes hands in front of an even step (k_seat_batch).  A member that stops early only lets the ones behind it
// start sooner, so this bounds the steps to issue; with as many seats as members it is the largest nsteps.
inline int64_t queue_step_bound(const int64_t* nsteps, int R, int seats) {
  std::vector<int64_t> free_at((size_t)seats, 0);
  int64_t bound = 0;
  for (int i = 0; i < R; ++i) {
    if (nsteps[i] <= 0) continue;
    size_t k = 0;
    for (size_t j = 1; j < free_at.size(); ++j) if (free_at[j] < free_at[k]) k = j;
    const int64_t start = free_at[k] + (free_at[k] & 1);
    free_at[k] = start + nsteps[i];
    if (free_at[k] > bound) bound = free_at[k];
  }
  return bound;
}

// Does the step-size rule of a member fire behind step s of its call of n steps?  cs0 is its step counter at the entry
// (< 0: the host does not know it -- an unknown counter fires).  As far as the host can tell: the kernels check again.
inline bool batch_rule_fires(long long cs0, int64_t n, int64_t s) {
  if (s >= n - 1) return false;           // no step behind s: no time-step control
  if (cs0 < 0) return true;
  const long long cs_next = cs0 + s + 1;  // (chs_tail.h: cs_next; a halted member's kernels are no-ops)
  return rule_fires(cs_next);
}

// What the host of a queued call knows of its members, from the polls alone.  The last-step pair of member i belongs
// to step seated + nsteps[i] - 1 exactly: without it the member would stand at its last step while k_col goes on
// updating its hat_U.  While the seating step is not known, seated[i] is a lower bound of it (0, then what the polls
// show) and the pair goes out on EVERY step from seated[i] + nsteps[i] - 1 on; once a poll has shown the step
// (`known`), on that one step.  The first `seats` members that run are seated in front of step 0.
struct QueueMembers {
  const int64_t* nsteps;
  int R;
  std::vector<int64_t> seated;
  std::vector<char> known, served;
  std::vector<char> finished;   // (as far as the polls have shown)

  QueueMembers(const int64_t* nsteps_, int R_, int seats)
      : nsteps(nsteps_), R(R_), seated((size_t)R_, 0), known((size_t)R_, 0), served((size_t)R_, 0), finished((size_t)R_, 0) {
    for (int i = 0, k = 0; i < R; ++i) {
      finished[(size_t)i] = nsteps[i] <= 0;
      if (nsteps[i] > 0 && k++ < seats) known[(size_t)i] = 1;
    }
  }

  // may the call of an unfinished member end with step s?  (asked once per step, in ascending order)
  bool last_pair(int64_t s) {
    bool last = false;
    for (int i = 0; i < R; ++i) {
      if (finished[(size_t)i] || served[(size_t)i] || s < seated[(size_t)i] + nsteps[i] - 1) continue;
      last = true;
      served[(size_t)i] = known[(size_t)i];
    }
    return last;
  }

  // What the poll fetched behind `issued_then` steps shows of unfinished member i: its state and the step in front of
  // which it was seated (< 0: still waiting then, so it is not seated before the steps that had been issued).  True
  // while the member has steps to do.
  bool poll(int i, bool halt, int64_t rows_written, long long seated_at, int64_t issued_then) {
    if (halt || rows_written >= nsteps[i]) finished[(size_t)i] = 1;
    if (seated_at >= 0) { seated[(size_t)i] = (int64_t)seated_at; known[(size_t)i] = 1; }
    else if (!known[(size_t)i]) seated[(size_t)i] = issued_then;
    return !finished[(size_t)i];
  }
};
