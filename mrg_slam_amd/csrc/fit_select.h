// csrc/fit_select.h — the host side of bounded best-candidate selection (mrgfe_batch_align_best, loop_detector.cpp:126-145 and :156-160).
// Given a certified interval lower <= fitness <= upper per candidate, which candidates of a group must still be scored exactly, and which
// candidate the reference's sequential rule picks on the records that come back.  Plain C++: mrgfe_dbg_select_prune runs it without a GPU.
#pragma once
#include <cstdint>

namespace mrgfe {

enum : int32_t { kFitExact = 0, kFitPruned = 1, kFitAboveCap = 2, kFitSkipped = 3 };  // enum mrgfe_fit_state

// state[i] for every candidate.  group[i] = -1: EXACT.  Not converged: SKIPPED.  Otherwise, with U[g] the least `upper` among the converged
// candidates of the group: PRUNED when lower[i] > U[g] (strictly), else ABOVE_CAP when lower[i] > score_cap, else EXACT; a group holding a NaN
// bound is EXACT throughout (the rule lets a NaN score through and then accepts every later candidate).  The candidate that attains U[g] has
// lower <= upper = U[g] and is never pruned, so a pruned lower bound is strictly above an exact score of its own group.  A candidate without
// a certified upper bound passes upper = +inf (and lower = 0, or any lower bound): it is then never pruned and prunes nothing.
void fit_select_prune(int n, const double* lower, const double* upper, const int32_t* converged, const int32_t* group, int n_groups, double score_cap, int32_t* state);

// best[g] / best_score[g] from the records (fitness exact or a lower bound, per fit_select_prune): the rule of loop_detector.cpp:137-144
// (ties: the last candidate; +inf never matches), best[g] = a pair index or -1.  With score_cap < DBL_MAX, a group with a converged candidate
// whose best score exceeds the cap gets best[g] = -2 and best_score[g] = the least fitness of its converged candidates (> score_cap).
void fit_select_groups(int n, const double* fitness, const int32_t* converged, const int32_t* group, int n_groups, double score_cap, int32_t* best, double* best_score);

}  // namespace mrgfe
