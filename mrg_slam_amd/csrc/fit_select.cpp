// csrc/fit_select.cpp — see fit_select.h
#include "fit_select.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace mrgfe {

void fit_select_prune(int n, const double* lower, const double* upper, const int32_t* converged, const int32_t* group, int n_groups, double score_cap, int32_t* state)
{
    std::vector<double> U(static_cast<size_t>(n_groups > 0 ? n_groups : 0), INFINITY);
    std::vector<char>   has_nan(U.size(), 0);
    for (int i = 0; i < n; ++i) {
        const int g = group[i];
        if (g < 0 || !converged[i]) continue;
        if (std::isnan(lower[i]) || std::isnan(upper[i])) has_nan[g] = 1;
        else if (upper[i] < U[g]) U[g] = upper[i];
    }
    for (int i = 0; i < n; ++i) {
        const int g = group[i];
        if (g < 0) state[i] = kFitExact;
        else if (!converged[i]) state[i] = kFitSkipped;
        else if (has_nan[g]) state[i] = kFitExact;
        else if (lower[i] > U[g]) state[i] = kFitPruned;
        else if (lower[i] > score_cap) state[i] = kFitAboveCap;
        else state[i] = kFitExact;
    }
}

void fit_select_groups(int n, const double* fitness, const int32_t* converged, const int32_t* group, int n_groups, double score_cap, int32_t* best, double* best_score)
{
    std::vector<char>   any(static_cast<size_t>(n_groups > 0 ? n_groups : 0), 0);
    std::vector<double> least(any.size(), INFINITY);
    for (int g = 0; g < n_groups; ++g) { best[g] = -1; best_score[g] = DBL_MAX; }
    for (int i = 0; i < n; ++i) {  // pair-index order: the candidate order within every group
        const int g = group[i];
        if (g < 0 || !converged[i]) continue;
        const double score = fitness[i];
        any[g] = 1;
        if (score < least[g]) least[g] = score;
        if (score > best_score[g]) continue;  // loop_detector.cpp:137
        best_score[g] = score;
        best[g] = i;
    }
    for (int g = 0; g < n_groups; ++g)
        if (any[g] && best_score[g] > score_cap) {  // loop_detector.cpp:156-160: no loop from this group
            best[g] = -2;
            best_score[g] = least[g];
        }
}

}  // namespace mrgfe
