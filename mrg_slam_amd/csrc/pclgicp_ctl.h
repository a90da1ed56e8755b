// csrc/pclgicp_ctl.h — the host side of PCL_GICP_HIP / PCL_GICP_OMP_HIP (pcl::GeneralizedIterativeClosestPoint::computeTransformation +
// estimateRigidTransformationBFGS), without a line of HIP: what both drivers of the GPU sums share.
//   pclgicp_align_host<Evaluator>: the loop of a single registration (GicpEngine::align_pcl_gicp) — BFGS<F> of bfgs.h calling its functor from inside
//     its nested line-search loops, every call one evaluate() of the evaluator.
//   PclGicpController: the same decisions, in the same order and on the same doubles, as a resumable state machine — request() says where to
//     evaluate next, on_result() takes the 14-sum record.  GicpBatch::align_all_pcl drives one per pair, a round per request.
// tests/sanitize/pclgicp_ctl_san.cpp runs the two against each other over synthetic evaluators, bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "bfgs.h"

namespace mrgfe {

constexpr int kGicpStride = 32;  // partial record: err, b[6], H upper[21], n_corr, pad (PCL GICP: [0] cost sum, [1..3] sum of M d, [4..12] dCost_dR_T, [28] correspondences)

struct PclGicpCtlParams {
    int    max_iterations = 64;
    int    max_inner_iterations = 20;
    double trans_eps = 5e-4;
    double rot_eps = 2e-3;
    bool   whole_gradient_norm = false;  // pclomp::GICP
};

// GeneralizedIterativeClosestPoint::applyState: t.topLeftCorner<3,3>() = Rz(x5) Ry(x4) Rx(x3) t.topLeftCorner<3,3>(); t.col(3) += (x0, x1, x2, 0); all float,
// the rotations as Eigen::AngleAxisf::toRotationMatrix() builds them
inline void angle_axis_unit_f(float angle, int axis, float R[9])
{
    float ax[3] = {0, 0, 0};
    ax[axis] = 1.0f;
    const float sn = std::sin(angle), c = std::cos(angle);
    const float sin_axis[3] = {sn * ax[0], sn * ax[1], sn * ax[2]};
    const float cos1_axis[3] = {(1.0f - c) * ax[0], (1.0f - c) * ax[1], (1.0f - c) * ax[2]};
    float tmp;
    tmp = cos1_axis[0] * ax[1]; R[1] = tmp - sin_axis[2]; R[3] = tmp + sin_axis[2];
    tmp = cos1_axis[0] * ax[2]; R[2] = tmp + sin_axis[1]; R[6] = tmp - sin_axis[1];
    tmp = cos1_axis[1] * ax[2]; R[5] = tmp - sin_axis[0]; R[7] = tmp + sin_axis[0];
    R[0] = cos1_axis[0] * ax[0] + c; R[4] = cos1_axis[1] * ax[1] + c; R[8] = cos1_axis[2] * ax[2] + c;
}
inline void mul3f(const float a[9], const float b[9], float out[9])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const float p0 = a[r * 3 + 0] * b[0 * 3 + c], p1 = a[r * 3 + 1] * b[1 * 3 + c], p2 = a[r * 3 + 2] * b[2 * 3 + c];
            const float s = p0 + p1;
            out[r * 3 + c] = s + p2;
        }
}
inline void pclgicp_apply_state(float t[16], const double x[6])
{
    float Rx[9], Ry[9], Rz[9], Rzy[9], R[9], old[9], nw[9];
    angle_axis_unit_f(static_cast<float>(x[5]), 2, Rz);
    angle_axis_unit_f(static_cast<float>(x[4]), 1, Ry);
    angle_axis_unit_f(static_cast<float>(x[3]), 0, Rx);
    mul3f(Rz, Ry, Rzy);
    mul3f(Rzy, Rx, R);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) old[r * 3 + c] = t[r * 4 + c];
    mul3f(R, old, nw);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[r * 4 + c] = nw[r * 3 + c];
    for (int r = 0; r < 3; ++r) t[r * 4 + 3] += static_cast<float>(x[r]);
}
// computeRDerivative: g[3..5] = tr(dR/dphi dCost_dR_T), ... for R = Rz(psi) Ry(theta) Rx(phi)
inline void pclgicp_r_derivative(const double x[6], const double dC[9], double g[6])
{
    const double phi = x[3], theta = x[4], psi = x[5];
    const double cphi = std::cos(phi), sphi = std::sin(phi), ctheta = std::cos(theta), stheta = std::sin(theta), cpsi = std::cos(psi), spsi = std::sin(psi);
    const double dPhi[9] = {0, sphi * spsi + cphi * cpsi * stheta, cphi * spsi - cpsi * sphi * stheta, 0, -cpsi * sphi + cphi * spsi * stheta, -cphi * cpsi - sphi * spsi * stheta,
                            0, cphi * ctheta, -ctheta * sphi};
    const double dTheta[9] = {-cpsi * stheta, cpsi * ctheta * sphi, cphi * cpsi * ctheta, -spsi * stheta, ctheta * sphi * spsi, cphi * ctheta * spsi, -ctheta, -sphi * stheta, -cphi * stheta};
    const double dPsi[9] = {-ctheta * spsi, -cphi * cpsi - sphi * spsi * stheta, cpsi * sphi - cphi * spsi * stheta, cpsi * ctheta, -cphi * spsi + cpsi * sphi * stheta,
                            sphi * spsi + cphi * cpsi * stheta, 0, 0, 0};
    auto inner = [&](const double A[9]) {  // matricesInnerProd(A, dCost_dR_T) = sum_ij A(j, i) dC(i, j)
        double r = 0;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r += A[j * 3 + i] * dC[i * 3 + j];
        return r;
    };
    g[3] = inner(dPhi);
    g[4] = inner(dTheta);
    g[5] = inner(dPsi);
}

// the functor's values out of the raw record of one evaluation at x: f = r[0] / m, g_t = r[1..3] (2 / m), g_r = computeRDerivative(r[4..12] (2 / m));
// all zero without a correspondence
inline void pclgicp_normalise(const double r[kGicpStride], const double x[6], double* f, double g[6], int* n_corr)
{
    *f = 0;
    for (int k = 0; k < 6; ++k) g[k] = 0;
    const double m = r[28];
    *n_corr = static_cast<int>(m);
    if (m <= 0) return;
    *f = r[0] / m;
    for (int k = 0; k < 3; ++k) g[k] = r[1 + k] * (2.0 / m);
    double dC[9];
    for (int k = 0; k < 9; ++k) dC[k] = r[4 + k] * (2.0 / m);
    pclgicp_r_derivative(x, dC, g);
}
// the start of estimateRigidTransformationBFGS: x[3] = std::atan2(T(2,1), T(2,2)) and x[5] = std::atan2(T(1,0), T(0,0)) on floats, x[4] = asin(-T(2,0))
// through the C function (double)
inline void pclgicp_state_of(const float t[16], double x[6])
{
    x[0] = t[3]; x[1] = t[7]; x[2] = t[11];
    x[3] = static_cast<double>(std::atan2(t[9], t[10]));
    x[4] = std::asin(static_cast<double>(-t[8]));
    x[5] = static_cast<double>(std::atan2(t[4], t[0]));
}
// testGradient -> OptimizationFunctorWithIndices::checkGradient (PCL >= 1.11: translation and rotation parts apart; pclomp: the whole norm)
inline bool pclgicp_gradient_small(const PclGicpCtlParams& prm, const double gr[6])
{
    const double gt = std::sqrt(gr[0] * gr[0] + gr[1] * gr[1] + gr[2] * gr[2]), grn = std::sqrt(gr[3] * gr[3] + gr[4] * gr[4] + gr[5] * gr[5]);
    return prm.whole_gradient_norm ? std::sqrt(gt * gt + grn * grn) < 1e-2 : (gt < 1e-2 && grn < 1e-2);
}
// the convergence measure of computeTransformation: the largest entry change over rotation_epsilon_ (rotation block) / transformation_epsilon_
inline double pclgicp_outer_delta(const PclGicpCtlParams& prm, const float previous[16], const float transformation[16])
{
    double delta = 0;
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 4; ++l) {
            const double ratio = (k < 3 && l < 3) ? 1.0 / prm.rot_eps : 1.0 / prm.trans_eps;
            const double c_delta = ratio * std::fabs(static_cast<double>(previous[k * 4 + l] - transformation[k * 4 + l]));
            if (c_delta > delta) delta = c_delta;
        }
    return delta;
}
// final_transformation_ = previous_transformation_ * guess (float)
inline void pclgicp_final(const float previous[16], const float guess[16], float out[16])
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            float s = 0;
            for (int k = 0; k < 4; ++k) s += previous[r * 4 + k] * guess[k * 4 + c];
            out[r * 4 + c] = s;
        }
}
inline void pclgicp_identity(float t[16]) { for (int i = 0; i < 16; ++i) t[i] = (i % 5 == 0) ? 1.0f : 0.0f; }

struct PclGicpOutcome {
    float final_rm[16];
    bool  converged = false;
    int   iterations = 0;   // outer iterations
    int   n_search = 0;     // outer iterations whose BFGS ran to its end
    int   n_functor = 0;    // functor evaluations of those
};

// The loop of pcl::GICP::computeTransformation over an evaluator of the GPU sums:
//   int search(const float T_rowmajor[16])                         correspondences + Mahalanobis matrices at transformation_ = T
//   int evaluate(const double x[6], double r[kGicpStride])         the raw record of the functor at x over them
// both return 0 on success; any other status ends the loop and is returned.  n_src == 0: no iteration, final = guess.
template <class Evaluator>
int pclgicp_align_host(const PclGicpCtlParams& prm, const float guess[16], uint32_t n_src, Evaluator& ev, PclGicpOutcome& out)
{
    struct Functor {
        Evaluator* ev;
        int status = 0, evaluations = 0, m = 0;
        double operator()(const double x[6]) { double f = 0, g[6]; run(x, &f, g); return f; }
        void   df(const double x[6], double g[6]) { double f = 0; run(x, &f, g); }
        void   fdf(const double x[6], double& f, double g[6]) { run(x, &f, g); }
        void   run(const double x[6], double* f, double g[6])
        {
            ++evaluations;
            double r[kGicpStride];
            for (int k = 0; k < kGicpStride; ++k) r[k] = 0;
            const int rc = ev->evaluate(x, r);
            if (rc != 0 && status == 0) status = rc;
            pclgicp_normalise(r, x, f, g, &m);
        }
    };
    out = PclGicpOutcome();
    float transformation[16], previous[16];
    pclgicp_identity(transformation);
    pclgicp_identity(previous);
    pclgicp_identity(out.final_rm);
    while (!out.converged && n_src > 0) {
        const int rc = ev.search(transformation);  // the search loop of this iteration
        if (rc != 0) return rc;
        std::memcpy(previous, transformation, sizeof(previous));
        // ---- estimateRigidTransformationBFGS
        double x[6];
        pclgicp_state_of(transformation, x);
        Functor fn;
        fn.ev = &ev;
        // NotEnoughPointsException when fewer than four correspondences: known after the first evaluation (the count comes back with every record)
        BFGS<Functor> bfgs(fn);
        int inner = 0;
        BFGSSpace::Status result = bfgs.minimizeInit(x);
        if (fn.status != 0) return fn.status;
        if (fn.m < 4) break;
        result = BFGSSpace::Running;
        do {
            ++inner;
            result = bfgs.minimizeOneStep(x);
            if (fn.status != 0) return fn.status;
            if (result) break;
            result = pclgicp_gradient_small(prm, bfgs.gradient) ? BFGSSpace::Success : BFGSSpace::Running;
        } while (result == BFGSSpace::Running && inner < prm.max_inner_iterations);
        out.n_functor += fn.evaluations;
        out.n_search += 1;
        if (result == BFGSSpace::NoProgress || result == BFGSSpace::Success || inner == prm.max_inner_iterations) {
            pclgicp_identity(transformation);
            pclgicp_apply_state(transformation, x);
        } else {
            break;  // SolverDidntConvergeException
        }
        const double delta = pclgicp_outer_delta(prm, previous, transformation);
        ++out.iterations;
        if (out.iterations >= prm.max_iterations || delta < 1) {
            out.converged = true;
            std::memcpy(previous, transformation, sizeof(previous));
        }
    }
    pclgicp_final(previous, guess, out.final_rm);
    return 0;
}

struct PclGicpRequest {
    bool   search;  // first find the correspondences and Mahalanobis matrices at transformation_ = T ...
    float  T[16];   // (row-major)
    double x[6];    // ... then evaluate the functor at x over the stored correspondences
};

// pclgicp_align_host as an explicit state machine: every functor call of BFGS<F>::minimizeInit / minimizeOneStep / lineSearch is a point where the
// machine stops with a request and goes on in on_result().  The step-length caches of applyF / applyDF / applyFDF are kept as bfgs.h keeps them: a
// hit asks for nothing, f followed by df at the same step length are two requests.
class PclGicpController {
    struct NoFunctor {};

   public:
    void start(const PclGicpCtlParams& prm, const float guess_rowmajor[16], uint32_t n_src, uint32_t n_tgt)
    {
        prm_ = prm;
        std::memcpy(guess_, guess_rowmajor, sizeof(guess_));
        n_src_ = n_src;
        n_tgt_ = n_tgt;
        pclgicp_identity(transformation_);
        pclgicp_identity(previous_);
        pclgicp_identity(final_);
        converged_ = false;
        done_ = false;
        waiting_ = false;
        nr_iterations_ = n_search_ = n_functor_ = 0;
        visited_ = 0;
        std::memset(&req_, 0, sizeof(req_));
        if (n_src_ == 0) finish();
        else begin_outer();
    }
    bool done() const { return done_; }
    bool degenerate() const { return n_src_ == 0 || n_tgt_ == 0; }  // nothing to search: the caller hands on_result an all-zero record
    const PclGicpRequest& request() const { return req_; }
    void on_result(const double r[kGicpStride])
    {
        if (done_ || !waiting_) return;
        waiting_ = false;
        req_.search = false;
        double f, g[6];
        int    m = 0;
        pclgicp_normalise(r, req_.x, &f, g, &m);
        const double a = want_alpha_;
        switch (want_) {
        case kWantInit:  // the rest of minimizeInit
            f_ = f;
            copy(gradient_, g);
            copy(x0_, x_);
            copy(g0_, gradient_);
            g0norm_ = norm(g0_);
            for (int k = 0; k < 6; ++k) p_[k] = gradient_[k] * (-1 / g0norm_);
            pnorm_ = norm(p_);
            fp0_ = -g0norm_;
            copy(x_alpha_, x0_);
            x_cache_key_ = 0;
            f_alpha_ = f_;
            f_cache_key_ = 0;
            copy(g_alpha_, g0_);
            g_cache_key_ = 0;
            df_alpha_ = slope();
            df_cache_key_ = 0;
            if (m < 4) { finish(); return; }  // NotEnoughPointsException
            pc_ = kStepBegin;
            break;
        case kWantF:
            f_alpha_ = f;
            f_cache_key_ = a;
            break;
        case kWantDF:
            copy(g_alpha_, g);
            g_cache_key_ = a;
            df_alpha_ = slope();
            df_cache_key_ = a;
            break;
        case kWantFDF:
            f_alpha_ = f;
            copy(g_alpha_, g);
            f_cache_key_ = a;
            g_cache_key_ = a;
            df_alpha_ = slope();
            df_cache_key_ = a;
            break;
        }
        advance();
    }
    bool converged() const { return converged_; }
    int  iterations() const { return nr_iterations_; }
    int  evaluations() const { return n_search_ + n_functor_; }
    const float* final_transformation() const { return final_; }
    // bracket_iters + section_iters of bfgs.h: with max_iterations x (max_inner_iterations x this + 2) a caller bounds the requests of an alignment
    static int line_search_iterations() { const typename BFGS<NoFunctor>::Parameters p; return p.bracket_iters + p.section_iters; }
    // which states of the machine this alignment went through (bit = state; kNoProgressBit: the line search's round-off exit): tests
    enum Pc { kStepBegin, kFdfThenDF, kLsStart, kBracketTop, kBracketAfterF, kBracketAfterDF, kSectionTop, kSectionAfterF, kSectionAfterDF, kLsDone, kUpdDone, kStepDone };
    static constexpr unsigned kNoProgressBit = 1u << 30;
    unsigned visited() const { return visited_; }

   private:
    enum Want { kWantInit, kWantF, kWantDF, kWantFDF };

    PclGicpCtlParams prm_;
    typename BFGS<NoFunctor>::Parameters par_;  // the defaults of bfgs.h, which estimateRigidTransformationBFGS leaves alone
    PclGicpRequest   req_;
    float    guess_[16], transformation_[16], previous_[16], final_[16];
    uint32_t n_src_ = 0, n_tgt_ = 0;
    bool     done_ = true, converged_ = false, waiting_ = false;
    int      nr_iterations_ = 0, n_search_ = 0, n_functor_ = 0;
    int      inner_ = 0, fn_evals_ = 0;
    unsigned visited_ = 0;
    Pc       pc_ = kStepBegin, fdf_ret_ = kStepBegin;
    Want     want_ = kWantInit;
    double   want_alpha_ = 0, fdf_alpha_ = 0;
    // BFGS<F>
    double x_[6], f_ = 0, gradient_[6];
    double delta_f_ = 0, fp0_ = 0, g0norm_ = 0, pnorm_ = 0;
    double x0_[6], dx_[6], g0_[6], p_[6];
    double x_alpha_[6], g_alpha_[6], f_alpha_ = 0, df_alpha_ = 0;
    double x_cache_key_ = 0, f_cache_key_ = 0, g_cache_key_ = 0, df_cache_key_ = 0;
    // minimizeOneStep / lineSearch locals that live across requests
    BFGSSpace::Status step_status_ = BFGSSpace::Success, ls_status_ = BFGSSpace::Success;
    double step_f0_ = 0, alpha_new_ = 0;
    double ls_f0_ = 0, ls_fp0_ = 0, falpha_ = 0, falpha_prev_ = 0, fpalpha_ = 0, fpalpha_prev_ = 0, alpha_ = 0, alpha_prev_ = 0;
    double a_ = 0, b_ = 0, fa_ = 0, fb_ = 0, fpa_ = 0, fpb_ = 0;
    int    i_ = 0;

    static void   setZero(double v[6]) { for (int k = 0; k < 6; ++k) v[k] = 0; }
    static void   copy(double d[6], const double s[6]) { for (int k = 0; k < 6; ++k) d[k] = s[k]; }
    static double dot(const double a[6], const double b[6]) { double s = 0; for (int k = 0; k < 6; ++k) s += a[k] * b[k]; return s; }
    static double norm(const double a[6]) { return std::sqrt(dot(a, a)); }
    double slope() const { return dot(g_alpha_, p_); }
    void   moveTo(double alpha)
    {
        if (alpha == x_cache_key_) return;  // using previously cached position
        for (int k = 0; k < 6; ++k) x_alpha_[k] = x0_[k] + alpha * p_[k];
        x_cache_key_ = alpha;
    }

    void finish()
    {
        pclgicp_final(previous_, guess_, final_);
        done_ = true;
        waiting_ = false;
        req_.search = false;
    }
    void ask(Want w, double alpha, const double x[6])
    {
        want_ = w;
        want_alpha_ = alpha;
        copy(req_.x, x);
        ++fn_evals_;
        waiting_ = true;
    }
    // one outer iteration: the search at transformation_, then minimizeInit's fdf at the x of transformation_ — one request
    void begin_outer()
    {
        req_.search = true;
        std::memcpy(req_.T, transformation_, sizeof(req_.T));
        std::memcpy(previous_, transformation_, sizeof(previous_));
        pclgicp_state_of(transformation_, x_);
        fn_evals_ = 0;
        inner_ = 0;
        delta_f_ = 0;
        setZero(dx_);
        ask(kWantInit, 0.0, x_);
    }
    // applyF / applyDF / applyFDF: go on at `ret`, at once on a cache hit, after the record otherwise; the values are then f_alpha_ / df_alpha_
    void opF(double alpha, Pc ret)
    {
        pc_ = ret;
        if (alpha == f_cache_key_) return;
        moveTo(alpha);
        ask(kWantF, alpha, x_alpha_);
    }
    void opDF(double alpha, Pc ret)
    {
        pc_ = ret;
        if (alpha == df_cache_key_) return;
        moveTo(alpha);
        if (alpha != g_cache_key_) { ask(kWantDF, alpha, x_alpha_); return; }
        df_alpha_ = slope();
        df_cache_key_ = alpha;
    }
    void opFDF(double alpha, Pc ret)
    {
        if (alpha == f_cache_key_ && alpha == df_cache_key_) { pc_ = ret; return; }
        if (alpha == f_cache_key_ || alpha == g_cache_key_ || alpha == df_cache_key_) {  // fv = applyF(alpha); dfv = applyDF(alpha)
            fdf_alpha_ = alpha;
            fdf_ret_ = ret;
            opF(alpha, kFdfThenDF);
            return;
        }
        pc_ = ret;
        moveTo(alpha);
        ask(kWantFDF, alpha, x_alpha_);
    }

    // BFGS<F>::interpolate, restated: bfgs.h keeps its copy private and stays as it is
    static double interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax, int order)
    {
        double y, ymin = (xmin - a) / (b - a), ymax = (xmax - a) / (b - a);
        if (ymin > ymax) std::swap(ymin, ymax);  // ensure ymin <= ymax
        if (order > 2 && !(fpb != fpb) && fpb != std::numeric_limits<double>::infinity() && fpb != -std::numeric_limits<double>::infinity()) {
            fpa = fpa * (b - a);
            fpb = fpb * (b - a);
            const double eta = 3 * (fb - fa) - 2 * fpa - fpb, xi = fpa + fpb - 2 * (fb - fa);
            const double c0 = fa, c1 = fpa, c2 = eta, c3 = xi;
            auto cubic = [&](double z) { return c0 + z * (c1 + z * (c2 + z * c3)); };
            double zmin = ymin, fmin = cubic(ymin);
            auto checkExtremum = [&](double z) { const double v = cubic(z); if (v < fmin) { zmin = z; fmin = v; } };
            checkExtremum(ymax);
            // roots of the derivative 3 c3 z^2 + 2 c2 z + c1
            const double qa = 3 * c3, qb = 2 * c2, qc = c1;
            double z0 = 0, z1 = 0;
            int    n = 0;
            if (qa == 0) {
                if (qb != 0) { z0 = -qc / qb; n = 1; }
            } else {
                const double disc = qb * qb - 4 * qa * qc;
                if (disc > 0) {
                    if (qb == 0) { const double r = std::sqrt(-qc / qa); z0 = -r; z1 = r; }
                    else {
                        const double sgnb = (qb > 0 ? 1 : -1), temp = -0.5 * (qb + sgnb * std::sqrt(disc)), r1 = temp / qa, r2 = qc / temp;
                        if (r1 < r2) { z0 = r1; z1 = r2; } else { z0 = r2; z1 = r1; }
                    }
                    n = 2;
                } else if (disc == 0) { z0 = -0.5 * qb / qa; z1 = -0.5 * qb / qa; n = 2; }
            }
            if (n == 2) {
                if (z0 > ymin && z0 < ymax) checkExtremum(z0);
                if (z1 > ymin && z1 < ymax) checkExtremum(z1);
            } else if (n == 1) {
                if (z0 > ymin && z0 < ymax) checkExtremum(z0);
            }
            y = zmin;
        } else {
            fpa = fpa * (b - a);
            const double fl = fa + ymin * (fpa + ymin * (fb - fa - fpa)), fh = fa + ymax * (fpa + ymax * (fb - fa - fpa));
            const double c = 2 * (fb - fa - fpa);  // curvature
            double zmin = ymin, fmin = fl;
            if (fh < fmin) { zmin = ymax; fmin = fh; }
            if (c > 0) {  // positive curvature required for a minimum
                const double z = -fpa / c;
                if (z > ymin && z < ymax) {
                    const double fz = fa + z * (fpa + z * (fb - fa - fpa));
                    if (fz < fmin) { zmin = z; fmin = fz; }
                }
            }
            y = zmin;
        }
        return a + y * (b - a);
    }

    // runs the machine until it needs a record or the alignment is over
    void advance()
    {
        const double NaN = std::numeric_limits<double>::quiet_NaN();
        while (!done_ && !waiting_) {
            visited_ |= 1u << pc_;
            switch (pc_) {
            case kStepBegin: {  // minimizeOneStep up to the line search's first call
                ++inner_;
                alpha_new_ = 0.0;
                step_f0_ = f_;
                if (pnorm_ == 0.0 || g0norm_ == 0.0 || fp0_ == 0) {
                    setZero(dx_);
                    step_status_ = BFGSSpace::NoProgress;
                    pc_ = kStepDone;
                    break;
                }
                double alpha1;
                if (delta_f_ < 0) {
                    const double del = std::max(-delta_f_, 10 * std::numeric_limits<double>::epsilon() * std::fabs(step_f0_));
                    alpha1 = std::min(1.0, 2.0 * del / (-fp0_));
                } else {
                    alpha1 = std::fabs(par_.step_size);
                }
                alpha_ = alpha1;
                alpha_prev_ = 0.0;
                i_ = 0;
                opFDF(0.0, kLsStart);
                break;
            }
            case kFdfThenDF:
                opDF(fdf_alpha_, fdf_ret_);
                break;
            case kLsStart:
                ls_f0_ = f_alpha_;
                ls_fp0_ = df_alpha_;
                falpha_prev_ = ls_f0_;
                fpalpha_prev_ = ls_fp0_;
                a_ = 0.0; b_ = alpha_; fa_ = ls_f0_; fb_ = 0.0; fpa_ = ls_fp0_; fpb_ = 0.0;
                pc_ = kBracketTop;
                break;
            case kBracketTop:  // begin bracketing
                if (i_++ < par_.bracket_iters) opF(alpha_, kBracketAfterF);
                else pc_ = kSectionTop;
                break;
            case kBracketAfterF:
                falpha_ = f_alpha_;
                if (falpha_ > ls_f0_ + alpha_ * par_.rho * ls_fp0_ || falpha_ >= falpha_prev_) {  // Fletcher's rho test
                    a_ = alpha_prev_; fa_ = falpha_prev_; fpa_ = fpalpha_prev_;
                    b_ = alpha_; fb_ = falpha_; fpb_ = NaN;
                    pc_ = kSectionTop;
                    break;
                }
                opDF(alpha_, kBracketAfterDF);
                break;
            case kBracketAfterDF: {
                fpalpha_ = df_alpha_;
                if (std::fabs(fpalpha_) <= -par_.sigma * ls_fp0_) { alpha_new_ = alpha_; ls_status_ = BFGSSpace::Success; pc_ = kLsDone; break; }  // Fletcher's sigma test
                if (fpalpha_ >= 0) {
                    a_ = alpha_; fa_ = falpha_; fpa_ = fpalpha_;
                    b_ = alpha_prev_; fb_ = falpha_prev_; fpb_ = fpalpha_prev_;
                    pc_ = kSectionTop;
                    break;
                }
                const double delta = alpha_ - alpha_prev_;
                const double alpha_next = interpolate(alpha_prev_, falpha_prev_, fpalpha_prev_, alpha_, falpha_, fpalpha_, alpha_ + delta, alpha_ + par_.tau1 * delta, par_.order);
                alpha_prev_ = alpha_;
                falpha_prev_ = falpha_;
                fpalpha_prev_ = fpalpha_;
                alpha_ = alpha_next;
                pc_ = kBracketTop;
                break;
            }
            case kSectionTop: {  // sectioning of bracket [a, b]
                if (!(i_++ < par_.section_iters)) { ls_status_ = BFGSSpace::Success; pc_ = kLsDone; break; }
                const double delta = b_ - a_;
                alpha_ = interpolate(a_, fa_, fpa_, b_, fb_, fpb_, a_ + par_.tau2 * delta, b_ - par_.tau3 * delta, par_.order);
                opF(alpha_, kSectionAfterF);
                break;
            }
            case kSectionAfterF:
                falpha_ = f_alpha_;
                if ((a_ - alpha_) * fpa_ <= std::numeric_limits<double>::epsilon()) { ls_status_ = BFGSSpace::NoProgress; visited_ |= kNoProgressBit; pc_ = kLsDone; break; }  // roundoff prevents progress
                if (falpha_ > ls_f0_ + par_.rho * alpha_ * ls_fp0_ || falpha_ >= fa_) {
                    b_ = alpha_; fb_ = falpha_; fpb_ = NaN;  // a_next = a
                    pc_ = kSectionTop;
                    break;
                }
                opDF(alpha_, kSectionAfterDF);
                break;
            case kSectionAfterDF:
                fpalpha_ = df_alpha_;
                if (std::fabs(fpalpha_) <= -par_.sigma * ls_fp0_) { alpha_new_ = alpha_; ls_status_ = BFGSSpace::Success; pc_ = kLsDone; break; }  // terminate
                if (((b_ - a_) >= 0 && fpalpha_ >= 0) || ((b_ - a_) <= 0 && fpalpha_ <= 0)) { b_ = a_; fb_ = fa_; fpb_ = fpa_; a_ = alpha_; fa_ = falpha_; fpa_ = fpalpha_; }
                else { a_ = alpha_; fa_ = falpha_; fpa_ = fpalpha_; }
                pc_ = kSectionTop;
                break;
            case kLsDone:
                if (ls_status_ != BFGSSpace::Success) { step_status_ = ls_status_; pc_ = kStepDone; break; }
                opFDF(alpha_new_, kUpdDone);  // updatePosition
                break;
            case kUpdDone: {  // the rest of minimizeOneStep
                f_ = f_alpha_;
                copy(x_, x_alpha_);
                copy(gradient_, g_alpha_);
                delta_f_ = f_ - step_f0_;
                // choose a new direction for the next step: p' = g1 - A dx - B dg, A = -(1 + dg.dg / dx.dg) B + dg.g / dx.dg, B = dx.g / dx.dg
                {
                    double dx0[6], dg0[6];
                    for (int k = 0; k < 6; ++k) { dx0[k] = x_[k] - x0_[k]; dx_[k] = dx0[k]; dg0[k] = gradient_[k] - g0_[k]; }
                    const double dxg = dot(dx0, gradient_), dgg = dot(dg0, gradient_), dxdg = dot(dx0, dg0), dgnorm = norm(dg0);
                    double A, B;
                    if (dxdg != 0) { B = dxg / dxdg; A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg; }
                    else { B = 0; A = 0; }
                    for (int k = 0; k < 6; ++k) { p_[k] = -A * dx0[k]; p_[k] += gradient_[k]; p_[k] += -B * dg0[k]; }
                }
                copy(g0_, gradient_);
                copy(x0_, x_);
                g0norm_ = norm(g0_);
                pnorm_ = norm(p_);
                const double dir = (dot(p_, gradient_) > 0) ? -1.0 : 1.0;  // update direction and fp0
                for (int k = 0; k < 6; ++k) p_[k] *= dir / pnorm_;
                pnorm_ = norm(p_);
                fp0_ = dot(p_, g0_);
                // changeDirection
                copy(x_alpha_, x0_);
                x_cache_key_ = 0.0;
                f_cache_key_ = 0.0;
                copy(g_alpha_, g0_);
                g_cache_key_ = 0.0;
                df_alpha_ = slope();
                df_cache_key_ = 0.0;
                step_status_ = BFGSSpace::Success;
                pc_ = kStepDone;
                break;
            }
            case kStepDone: {  // the body of estimateRigidTransformationBFGS's do-while behind minimizeOneStep, and what follows the loop
                BFGSSpace::Status result = step_status_;
                if (!result) result = pclgicp_gradient_small(prm_, gradient_) ? BFGSSpace::Success : BFGSSpace::Running;
                if (result == BFGSSpace::Running && inner_ < prm_.max_inner_iterations) { pc_ = kStepBegin; break; }
                n_functor_ += fn_evals_;
                n_search_ += 1;
                if (result == BFGSSpace::NoProgress || result == BFGSSpace::Success || inner_ == prm_.max_inner_iterations) {
                    pclgicp_identity(transformation_);
                    pclgicp_apply_state(transformation_, x_);
                } else {
                    finish();  // SolverDidntConvergeException
                    break;
                }
                const double delta = pclgicp_outer_delta(prm_, previous_, transformation_);
                ++nr_iterations_;
                if (nr_iterations_ >= prm_.max_iterations || delta < 1) {
                    converged_ = true;
                    std::memcpy(previous_, transformation_, sizeof(previous_));
                }
                if (converged_) finish();
                else begin_outer();
                break;
            }
            }
        }
    }
};

}  // namespace mrgfe
