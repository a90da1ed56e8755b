// tests/sanitize/pclgicp_ctl_san.cpp — csrc/pclgicp_ctl.h on the CPU: pclgicp_align_host (the single registration's loop, BFGS<F> of bfgs.h calling
// its functor from inside the line search) against PclGicpController (the same loop as a resumable state machine, the batch's) over synthetic
// evaluators, each deterministic in (T of the last search, x).  Required equal, byte for byte: the sequence of requested (search, T, x), the number
// of evaluations, the outer iterations, the converged flag, the final matrix.  Built by tests/test_pclgicp_controller_cpu.py with
// g++ -fsanitize=address,undefined and run as a program.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pclgicp_ctl.h"

using namespace mrgfe;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

struct Entry {
    int    search;
    float  T[16];
    double x[6];
};

// the cost of the evaluators below is F(x0, x1, x2) with its gradient, handed over as the record a GPU evaluation would return for m correspondences:
// r[0] = m F, r[1..3] = (m / 2) dF/dt; a matrix dCost_dR_T makes a rotation gradient through computeRDerivative
struct Synthetic {
    int   kind = 0;
    int   n_search = 0;
    float T[16];
    std::vector<Entry> log;
    bool  pending = false;

    int search(const float t[16])
    {
        std::memcpy(T, t, sizeof(T));
        ++n_search;
        pending = true;
        return 0;
    }
    int evaluate(const double x[6], double r[kGicpStride])
    {
        Entry e;
        std::memset(&e, 0, sizeof(e));
        e.search = pending ? 1 : 0;
        pending = false;
        std::memcpy(e.T, T, sizeof(e.T));
        std::memcpy(e.x, x, sizeof(e.x));
        log.push_back(e);
        for (int k = 0; k < kGicpStride; ++k) r[k] = 0;
        double m = 100, F = 0, g[3] = {0, 0, 0}, dC[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        switch (kind) {
        case 0: {  // a coupled quadratic bowl whose centre moves with the searched T; the rotation enters through dCost_dR_T
            const double c[3] = {0.4 + 0.5 * T[3], -0.3 + 0.4 * T[7], 0.2 + 0.3 * T[11]};
            const double A[9] = {2.0, 0.6, 0.2, 0.6, 1.5, -0.4, 0.2, -0.4, 1.0};
            double d[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]}, Ad[3];
            for (int i = 0; i < 3; ++i) Ad[i] = A[i * 3] * d[0] + A[i * 3 + 1] * d[1] + A[i * 3 + 2] * d[2];
            F = 0.5 * (d[0] * Ad[0] + d[1] * Ad[1] + d[2] * Ad[2]) + 0.05 * (x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
            for (int i = 0; i < 3; ++i) g[i] = Ad[i];
            dC[1] = 0.02 * x[3] + 0.01 * d[0]; dC[5] = -0.03 * x[4]; dC[6] = 0.01 * x[5] + 0.02 * d[1]; dC[2] = 0.01;
            break;
        }
        case 1: {  // a narrow curved valley
            const double c = 0.2 * T[3];
            const double u = x[0] - c, v = x[1], w = x[2];
            F = (1 - u) * (1 - u) + 100 * (v - u * u) * (v - u * u) + 4 * (w - v * v) * (w - v * v);
            g[0] = -2 * (1 - u) - 400 * u * (v - u * u);
            g[1] = 200 * (v - u * u) - 16 * v * (w - v * v);
            g[2] = 8 * (w - v * v);
            break;
        }
        case 2: {  // kinks: the gradient never gets small, the sectioning ends in round-off
            const double u = x[0] - 0.3, v = x[1] + 0.2, w = x[2] - 0.05 * T[3];
            F = std::fabs(u) + 2 * std::fabs(v) + 0.5 * std::fabs(w);
            g[0] = u < 0 ? -1 : 1; g[1] = v < 0 ? -2 : 2; g[2] = w < 0 ? -0.5 : 0.5;
            break;
        }
        case 3: {  // a NaN slope behind the first trial steps
            F = std::exp(-x[0]) + x[1] * x[1] + x[2] * x[2];
            g[0] = x[0] > 0.004 ? std::numeric_limits<double>::quiet_NaN() : -std::exp(-x[0]);
            g[1] = 2 * x[1]; g[2] = 2 * x[2];
            break;
        }
        case 4:  // a zero gradient at the start
            F = x[0] * x[0] * x[0] * x[0] + x[1] * x[1] * x[1] * x[1];
            g[0] = 4 * x[0] * x[0] * x[0]; g[1] = 4 * x[1] * x[1] * x[1];
            break;
        case 5:  // fewer than four correspondences on the first evaluation
            m = 3; F = 1; g[0] = 1;
            break;
        case 6: {  // ... on a later outer iteration
            if (n_search >= 2) m = 2;
            const double d[3] = {x[0] - 0.5, x[1] + 0.25, x[2] - 0.125};
            F = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            for (int i = 0; i < 3; ++i) g[i] = 2 * d[i];
            break;
        }
        case 7:  // no correspondence at all: the all-zero record of an empty target
            m = 0;
            break;
        case 8:  // a slope that promises what no step keeps: the sectioning runs out of iterations, the step length stays 0 and updatePosition finds
                 // the slope in its cache but not the value (applyFDF's middle branch)
            F = std::fabs(x[0]) + std::fabs(x[1]) + std::fabs(x[2]);
            g[0] = -1e30;
            break;
        }
        r[28] = m;
        r[0] = m * F;
        for (int i = 0; i < 3; ++i) r[1 + i] = 0.5 * m * g[i];
        for (int i = 0; i < 9; ++i) r[4 + i] = 0.5 * m * dC[i];
        return 0;
    }
};

static unsigned g_visited = 0;

static void run_case(const char* name, int kind, PclGicpCtlParams prm, uint32_t n_src, uint32_t n_tgt, const float guess[16])
{
    Synthetic a, b;
    a.kind = b.kind = kind;
    pclgicp_identity(a.T);
    pclgicp_identity(b.T);
    PclGicpOutcome want;
    const int rc = pclgicp_align_host(prm, guess, n_src, a, want);
    CHECK(rc == 0, "%s: status %d", name, rc);
    PclGicpController ctl;
    ctl.start(prm, guess, n_src, n_tgt);
    int rounds = 0;
    while (!ctl.done() && rounds < 100000) {
        const PclGicpRequest& rq = ctl.request();
        double r[kGicpStride];
        if (rq.search) b.search(rq.T);
        b.evaluate(rq.x, r);
        ctl.on_result(r);
        ++rounds;
    }
    g_visited |= ctl.visited();
    CHECK(ctl.done(), "%s: the controller did not end", name);
    CHECK(a.log.size() == b.log.size(), "%s: %zu requests against %zu", name, a.log.size(), b.log.size());
    const size_t n = std::min(a.log.size(), b.log.size());
    size_t differ = n;
    for (size_t i = 0; i < n; ++i)
        if (std::memcmp(&a.log[i], &b.log[i], sizeof(Entry)) != 0) { differ = i; break; }
    CHECK(differ == n, "%s: request %zu differs", name, differ);
    CHECK(ctl.evaluations() == want.n_search + want.n_functor, "%s: evaluations %d against %d", name, ctl.evaluations(), want.n_search + want.n_functor);
    CHECK(ctl.iterations() == want.iterations, "%s: iterations %d against %d", name, ctl.iterations(), want.iterations);
    CHECK(ctl.converged() == want.converged, "%s: converged %d against %d", name, int(ctl.converged()), int(want.converged));
    CHECK(std::memcmp(ctl.final_transformation(), want.final_rm, sizeof(want.final_rm)) == 0, "%s: final matrix differs", name);
    std::printf("%-40s requests %4zu  evaluations %4d  iterations %2d  converged %d\n", name, a.log.size(), ctl.evaluations(), ctl.iterations(), int(ctl.converged()));
}

int main()
{
    float guess[16];
    pclgicp_identity(guess);
    guess[3] = 0.25f; guess[7] = -0.125f; guess[0] = 0.9980f; guess[1] = -0.0632f; guess[4] = 0.0632f; guess[5] = 0.9980f;
    const char* names[9] = {"bowl", "valley", "kinks", "nan slope", "zero gradient", "m < 4 first", "m < 4 later", "no correspondences", "false slope"};
    for (int whole = 0; whole < 2; ++whole) {
        for (int kind = 0; kind < 9; ++kind) {
            PclGicpCtlParams prm;
            prm.trans_eps = 0.01;
            prm.whole_gradient_norm = whole != 0;
            char name[96];
            std::snprintf(name, sizeof(name), "%s (%s)", names[kind], whole ? "whole norm" : "separate norms");
            run_case(name, kind, prm, 1000, kind == 7 ? 0 : 1000, guess);
            for (int inner = 1; inner <= 2; ++inner) {
                PclGicpCtlParams p2 = prm;
                p2.max_inner_iterations = inner;
                std::snprintf(name, sizeof(name), "%s, max_inner %d (%s)", names[kind], inner, whole ? "whole" : "separate");
                run_case(name, kind, p2, 1000, 1000, guess);
            }
            PclGicpCtlParams p3 = prm;
            p3.max_iterations = 1;
            std::snprintf(name, sizeof(name), "%s, max_iterations 1 (%s)", names[kind], whole ? "whole" : "separate");
            run_case(name, kind, p3, 1000, 1000, guess);
            p3.max_iterations = 3;  // the iteration limit on an alignment that would go on
            p3.trans_eps = 1e-9;
            p3.rot_eps = 1e-9;
            std::snprintf(name, sizeof(name), "%s, max_iterations 3, eps 1e-9 (%s)", names[kind], whole ? "whole" : "separate");
            run_case(name, kind, p3, 1000, 1000, guess);
        }
    }
    {  // an empty source: no iteration, final = guess
        PclGicpCtlParams prm;
        run_case("empty source", 0, prm, 0, 1000, guess);
    }
    // the evaluators reach every state of the machine, the round-off exit of the sectioning included
    for (int s = PclGicpController::kStepBegin; s <= PclGicpController::kStepDone; ++s) CHECK((g_visited >> s) & 1u, "state %d never reached", s);
    CHECK(g_visited & PclGicpController::kNoProgressBit, "the NoProgress exit was never reached");
    std::printf("%d checks\n%d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
