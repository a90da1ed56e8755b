// csrc/api.cpp — the extern "C" surface declared in include/mrgfe.h, all but the batch (batch.cpp).  Thin: argument checks, column-major <-> row-major
// conversion, and dispatch into the engines and device passes; the handles here (mrgfe_reg, mrgfe_map_store) hold state and no algorithm.  Failures set
// the thread-local message and return a code.  No exception crosses the C boundary: the entry points that construct engines, grow host containers or start
// threads run inside abi_guard (common.h), which turns one into MRGFE_ERR_INVALID and a message.
// The handles own their engines, grids and buffers: a *_destroy takes the context lock, binds the device and deletes.
#include <algorithm>
#include <cfloat>
#include <memory>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "cellsort.h"
#include "common.h"
#include "glibc_exp.h"
#include "filters.h"
#include "floor.h"
#include "ground_fill.h"
#include "mapcloud.h"
#include "gicp_engine.h"
#include "ingest.h"
#include "ndt_derivatives.h"
#include "ndt_engine.h"
#include "nn_grid.h"
#include "scan_point.h"
#include "fit_select.h"
#include "api_internal.h"

using namespace mrgfe;

// (struct mrgfe_reg: api_internal.h — the odometry frame of odometry.cpp works on it too)

extern "C" {

void mrgfe_reg_default_params(int method, mrgfe_reg_params* out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->method = method;
    out->num_threads = 0;                       // registrations.cpp:35
    out->transformation_epsilon = 0.01;         // :36
    out->maximum_iterations = 64;               // :37
    out->max_correspondence_distance = 2.0;     // :38
    out->max_optimizer_iterations = 20;         // :39
    out->use_reciprocal_correspondences = 0;    // :40
    out->correspondence_randomness = 20;        // :41
    out->resolution = 1.0;                      // :42
    out->nn_search_method = MRGFE_DIRECT7;      // :43
    out->step_size = 0.1;
    out->outlier_ratio = 0.55;
    out->rotation_epsilon = 2e-3;
}

int mrgfe_reg_create(mrgfe_ctx* ctx, const mrgfe_reg_params* params, mrgfe_reg** out)
{
    return abi_guard("mrgfe_reg_create", [&]() -> int {
        if (!ctx || !out) { set_error("mrgfe_reg_create: NULL argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        MRGFE_TRY(check_params(params));
        std::unique_ptr<mrgfe_reg> r(new (std::nothrow) mrgfe_reg(ctx));
        if (!r) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        r->params = *params;
        if (is_ndt(params->method)) {
            r->ndt = std::make_unique<NdtEngine>(ctx, ndt_params_from(*params), &r->book);
            if (const char* e = std::getenv("MRGFE_FORCE_HASH")) r->ndt->set_force_hash(e[0] == '1');
        } else {
            r->gicp = std::make_unique<GicpEngine>(ctx, gicp_params_from(*params));
        }
        for (int i = 0; i < 16; ++i) r->final_rm[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        for (int i = 0; i < 36; ++i) r->hessian[i] = 0;
        *out = r.release();
        return MRGFE_OK;
    });
}

void mrgfe_reg_destroy(mrgfe_reg* reg)
{
    if (!reg) return;
    MRGFE_LOCK(reg->ctx);
    (void)hipSetDevice(reg->ctx->device);
    delete reg;
}

static int reg_target_changed(mrgfe_reg* reg)
{
    reg->has_target = true;
    reg->nn_valid = false;
    if (reg->ndt) {
        reg->book.clear();
        reg->ndt->clear();
        int ti = reg->book.add_target_device(reg->d_tgt, reg->n_tgt);
        if (ti < 0) return ti;
        MRGFE_TRY(reg->ndt->build_targets());
        reg->target_status = reg->ndt->target(0).status;
        if (reg->target_status == MRGFE_ERR_OVERFLOW) set_error("[NDT_HIP::setInputTarget] Leaf size is too small for the input dataset. Integer indices would overflow.");
        if (reg->target_status == MRGFE_ERR_EMPTY) { set_error("setInputTarget: cloud has no finite point"); }
        return reg->target_status;
    }
    MRGFE_TRY(reg->gicp->set_target(reg->d_tgt, reg->n_tgt));
    reg->target_status = MRGFE_OK;
    return MRGFE_OK;
}

int mrgfe_reg_set_target(mrgfe_reg* reg, const float* xyzi, size_t n, size_t stride_bytes)
{
    return abi_guard("mrgfe_reg_set_target", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_reg_set_target"));
        if (!reg || (n && !xyzi)) { set_error("mrgfe_reg_set_target: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        // after source_becomes_target the source lives in reg->tgt: give that buffer back to the source (reg->d_src and the GICP engine's d_src_ keep
        // pointing at it) and upload into the spare one, the only buffer that may be freed and regrown here
        if (reg->d_src == reg->tgt.p && reg->tgt.p != nullptr) std::swap(reg->src, reg->tgt);
        MRGFE_TRY(reg->tgt.ensure(std::max<size_t>(n, 1) * 16));
        MRGFE_TRY(upload_cloud(reg->ctx, xyzi, n, stride_bytes, reg->tgt.p));
        reg->d_tgt = reg->tgt.p;
        reg->n_tgt = n;
        TraceRange tr("mrgfe_reg_set_target");
        return reg_target_changed(reg);
    });
}

int mrgfe_reg_set_target_device(mrgfe_reg* reg, const void* d_xyzi, size_t n)
{
    return abi_guard("mrgfe_reg_set_target_device", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_reg_set_target_device"));
        if (!reg || (n && !d_xyzi)) { set_error("mrgfe_reg_set_target_device: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        reg->d_tgt = d_xyzi;
        reg->n_tgt = n;
        return reg_target_changed(reg);
    });
}

int mrgfe_reg_set_source(mrgfe_reg* reg, const float* xyzi, size_t n, size_t stride_bytes)
{
    return abi_guard("mrgfe_reg_set_source", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_reg_set_source"));
        if (!reg || (n && !xyzi)) { set_error("mrgfe_reg_set_source: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        MRGFE_TRY(reg->src.ensure(std::max<size_t>(n, 1) * 16));
        MRGFE_TRY(upload_cloud(reg->ctx, xyzi, n, stride_bytes, reg->src.p));
        reg->d_src = reg->src.p;
        reg->n_src = n;
        reg->has_source = true;
        if (reg->gicp) MRGFE_TRY(reg->gicp->set_source(reg->d_src, reg->n_src));
        return MRGFE_OK;
    });
}

int mrgfe_reg_set_source_device(mrgfe_reg* reg, const void* d_xyzi, size_t n)
{
    return abi_guard("mrgfe_reg_set_source_device", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_reg_set_source_device"));
        if (!reg || (n && !d_xyzi)) { set_error("mrgfe_reg_set_source_device: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        reg->d_src = d_xyzi;
        reg->n_src = n;
        reg->has_source = true;
        if (reg->gicp) MRGFE_TRY(reg->gicp->set_source(reg->d_src, reg->n_src));
        return MRGFE_OK;
    });
}

int mrgfe_reg_set_source_from_prefilter(mrgfe_reg* reg, const void* d_xyzi, size_t n)
{
    return abi_guard("mrgfe_reg_set_source_from_prefilter", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_reg_set_source_from_prefilter"));
        if (!reg || (n && !d_xyzi)) { set_error("mrgfe_reg_set_source_from_prefilter: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        reg->d_src = d_xyzi;
        reg->n_src = n;
        reg->has_source = true;
        const mrgfe_ctx* c = reg->ctx;
        const bool boxed = c->pf_out_valid && c->pf_out_ptr == d_xyzi && c->pf_out_n == n && n > 0;
        if (reg->gicp) MRGFE_TRY(reg->gicp->set_source(reg->d_src, reg->n_src, boxed ? c->pf_out_box : nullptr));
        return MRGFE_OK;
    });
}

int mrgfe_reg_source_becomes_target(mrgfe_reg* reg)
{
    return abi_guard("mrgfe_reg_source_becomes_target", [&]() -> int {
        if (!reg) { set_error("mrgfe_reg_source_becomes_target: NULL argument"); return MRGFE_ERR_INVALID; }
        if (!reg->has_source) { set_error("mrgfe_reg_source_becomes_target: setInputSource first"); return MRGFE_ERR_STATE; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        TraceRange tr("mrgfe_reg_source_becomes_target");
        // a cloud the library uploaded lives in reg->src: that buffer becomes the target's, the old target's takes the next source
        if (reg->d_src == reg->src.p && reg->src.p != nullptr) std::swap(reg->src, reg->tgt);
        reg->d_tgt = reg->d_src;
        reg->n_tgt = reg->n_src;
        if (reg->gicp) {
            reg->has_target = true;
            reg->nn_valid = false;
            MRGFE_TRY(reg->gicp->source_becomes_target());
            reg->target_status = MRGFE_OK;
            return MRGFE_OK;
        }
        return reg_target_changed(reg);  // NDT: the voxel grid of the new target (a source has nothing to hand over)
    });
}

int mrgfe_reg_align(mrgfe_reg* reg, const float guess[16], float* aligned_xyzi)
{
    return abi_guard("mrgfe_reg_align", [&]() -> int {
        if (!reg || !guess) { set_error("mrgfe_reg_align: NULL argument"); return MRGFE_ERR_INVALID; }
        if (!reg->has_target || !reg->has_source) { set_error("align: setInputTarget / setInputSource first"); return MRGFE_ERR_STATE; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        TraceRange tr("mrgfe_reg_align");
        float g[16];
        col2row(guess, g);
        if (reg->ndt) {
            NdtEngine& e = *reg->ndt;
            reg->book.clear_pairs();
            int pi = reg->book.add_pair_device(0, reg->d_src, reg->n_src, g);
            if (pi < 0) return pi;
            MRGFE_TRY(e.align_all());
            const NdtController& c = e.ctl(0);
            std::memcpy(reg->final_rm, c.final_transformation(), sizeof(reg->final_rm));
            reg->converged = c.converged();
            reg->iterations = c.iterations();
            reg->evaluations = c.evaluations();
            reg->trans_probability = c.trans_probability();
            std::memcpy(reg->hessian, c.hessian(), sizeof(reg->hessian));
            reg->mean_neighbours = c.evaluations() ? c.neighbours_sum() / c.evaluations() : 0.0;
            if (aligned_xyzi) MRGFE_TRY(e.aligned_cloud(0, aligned_xyzi));
        } else {
            GicpEngine& e = *reg->gicp;
            MRGFE_TRY(e.align(g));
            std::memcpy(reg->final_rm, e.final_transformation(), sizeof(reg->final_rm));
            reg->converged = e.converged();
            reg->iterations = e.iterations();
            reg->evaluations = e.evaluations();
            reg->trans_probability = 0;
            std::memcpy(reg->hessian, e.hessian(), sizeof(reg->hessian));
            if (aligned_xyzi) MRGFE_TRY(e.aligned_cloud(aligned_xyzi));
        }
        reg->aligned_once = true;
        return MRGFE_OK;
    });
}

int mrgfe_reg_has_converged(const mrgfe_reg* reg) { return reg && reg->converged ? 1 : 0; }

int mrgfe_reg_final_transformation(const mrgfe_reg* reg, float out[16])
{
    if (!reg || !out) { set_error("mrgfe_reg_final_transformation: NULL argument"); return MRGFE_ERR_INVALID; }
    row2col(reg->final_rm, out);
    return MRGFE_OK;
}

static int reg_ensure_nn(mrgfe_reg* reg)
{
    if (!reg->has_target) { set_error("no target set"); return MRGFE_ERR_STATE; }
    if (!reg->nn_valid) {
        MRGFE_TRY(reg->nn.build(reg->ctx, static_cast<const float4*>(reg->d_tgt), reg->n_tgt, 1.0f, NnGrid::kCrowding1nn, 1));
        reg->nn_valid = true;
    }
    return MRGFE_OK;
}

int mrgfe_reg_fitness(mrgfe_reg* reg, double max_range, double* out)
{
    TraceRange tr("mrgfe_reg_fitness");
    if (!reg || !out) { set_error("mrgfe_reg_fitness: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!reg->has_target || !reg->has_source) { set_error("getFitnessScore: target / source not set"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    MRGFE_TRY(reg->ctx->bind());
    if (reg->n_tgt == 0 || reg->n_src == 0) { *out = DBL_MAX; return MRGFE_OK; }
    MRGFE_TRY(reg_ensure_nn(reg));
    return reg->nn.fitness(reg->ctx, static_cast<const float4*>(reg->d_src), reg->n_src, reg->final_rm, max_range, out);
}

int mrgfe_reg_nn1_target(mrgfe_reg* reg, const float* q, size_t n, size_t stride_bytes, int32_t* idx, float* sqd)
{
    MRGFE_TRY(check_count(n, "mrgfe_reg_nn1_target"));
    if (!reg || (n && (!q || !idx || !sqd))) { set_error("mrgfe_reg_nn1_target: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(reg->ctx);
    MRGFE_TRY(reg->ctx->bind());
    MRGFE_TRY(reg_ensure_nn(reg));
    return reg->nn.nearest_host(reg->ctx, q, n, stride_bytes, idx, sqd);
}

// ---- scan-matching status (ScanMatchingOdometryComponent::publish_scan_matching_status, apps/scan_matching_odometry_component.cpp:391-431) ----
// isometry2pose (src/ros_utils.cpp:52-66) of a double isometry given as rotation R (row-major) and translation t: position, then Eigen::Quaterniond(R) as
// x y z w.  [UPSTREAM-RECALL] Eigen 3.3 Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>: the algorithm odometry.quat_w restates in float,
// here in double and for all four components; the trace is summed (m00 + m11) + m22 as there.
static void isometry2pose(const double R[3][3], const double t[3], double pose[7])
{
    double q[4];  // x y z w
    double tr = (R[0][0] + R[1][1]) + R[2][2];
    if (tr > 0.0) {
        tr = std::sqrt(tr + 1.0);
        q[3] = 0.5 * tr;
        tr = 0.5 / tr;
        q[0] = (R[2][1] - R[1][2]) * tr;
        q[1] = (R[0][2] - R[2][0]) * tr;
        q[2] = (R[1][0] - R[0][1]) * tr;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        tr = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
        q[i] = 0.5 * tr;
        tr = 0.5 / tr;
        q[3] = (R[k][j] - R[j][k]) * tr;
        q[j] = (R[j][i] + R[i][j]) * tr;
        q[k] = (R[k][i] + R[i][k]) * tr;
    }
    pose[0] = t[0]; pose[1] = t[1]; pose[2] = t[2];
    pose[3] = q[0]; pose[4] = q[1]; pose[5] = q[2]; pose[6] = q[3];
}

int mrgfe_status_poses(const float final_transformation[16], const float* msf_delta, double relative_pose[7], double prediction_error[7])
{
    if (!final_transformation || !relative_pose || (msf_delta && !prediction_error)) { set_error("mrgfe_status_poses: NULL argument"); return MRGFE_ERR_INVALID; }
    const float* F = final_transformation;  // column-major: element (r, c) at [4 c + r]
    double R[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[r][c] = static_cast<double>(F[4 * c + r]);  // Isometry3f(final).cast<double>(): floats widened exactly (:419)
        t[r] = static_cast<double>(F[12 + r]);
    }
    isometry2pose(R, t, relative_pose);
    if (!msf_delta) return MRGFE_OK;
    // Isometry3f(final).inverse() * msf_delta (:426), all in float.  [UPSTREAM-RECALL] Eigen 3.3 Geometry/Transform.h: the inverse of an Isometry is
    // (R^T, -R^T t); the product of two isometries is (R1 R2, R1 t2 + t1); three-term sums left to right.
    const float* D = msf_delta;
    float Ri[3][3], ti[3], Re[3][3], te[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ri[r][c] = F[4 * r + c];
    for (int r = 0; r < 3; ++r) ti[r] = ((-Ri[r][0]) * F[12] + (-Ri[r][1]) * F[13]) + (-Ri[r][2]) * F[14];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Re[r][c] = (Ri[r][0] * D[4 * c] + Ri[r][1] * D[4 * c + 1]) + Ri[r][2] * D[4 * c + 2];
        te[r] = ((Ri[r][0] * D[12] + Ri[r][1] * D[13]) + Ri[r][2] * D[14]) + ti[r];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[r][c] = static_cast<double>(Re[r][c]);
        t[r] = static_cast<double>(te[r]);
    }
    isometry2pose(R, t, prediction_error);  // error.cast<double>() (:427)
    return MRGFE_OK;
}

size_t mrgfe_matching_status_size(void) { return sizeof(mrgfe_matching_status); }

int mrgfe_reg_matching_status(mrgfe_reg* reg, double max_correspondence_dist, const float* msf_delta, mrgfe_matching_status* out)
{
    return abi_guard("mrgfe_reg_matching_status", [&]() -> int {
        if (!reg || !out) { set_error("mrgfe_reg_matching_status: NULL argument"); return MRGFE_ERR_INVALID; }
        if (!reg->has_target || !reg->has_source) { set_error("matching status: target / source not set"); return MRGFE_ERR_STATE; }
        MRGFE_LOCK(reg->ctx);
        MRGFE_TRY(reg->ctx->bind());
        TraceRange tr("mrgfe_reg_matching_status");
        double res[3] = {DBL_MAX, 0.0, 0.0};
        if (reg->n_tgt > 0 && reg->n_src > 0) MRGFE_TRY(reg_ensure_nn(reg));
        if (reg->n_tgt > 0 && reg->n_src > 0 && reg->nn.dev().n > 0) {  // (a target without a finite point: nothing to match, as NnGrid::fitness)
            const NnFitnessJob job = reg->nn.make_fitness_job(static_cast<const float4*>(reg->d_src), reg->n_src, reg->final_rm);
            MRGFE_TRY(nn_status_batch(reg->ctx, &job, 1, max_correspondence_dist * max_correspondence_dist, res));  // :413
        }
        mrgfe_matching_status s{};
        s.has_converged = reg->converged ? 1 : 0;
        s.n_points = static_cast<uint32_t>(reg->n_src);
        s.num_inliers = static_cast<uint32_t>(res[2]);
        s.inlier_fraction = static_cast<float>(s.num_inliers) / static_cast<float>(reg->n_src);  // :417 (float / size_t: the size converts to float)
        s.matching_error = res[0];
        float final_cm[16];
        row2col(reg->final_rm, final_cm);
        s.has_prediction = msf_delta ? 1 : 0;
        MRGFE_TRY(mrgfe_status_poses(final_cm, msf_delta, s.relative_pose, s.prediction_error));
        *out = s;
        return MRGFE_OK;
    });
}

int    mrgfe_reg_iterations(const mrgfe_reg* reg) { return reg ? reg->iterations : 0; }
int    mrgfe_reg_evaluations(const mrgfe_reg* reg) { return reg ? reg->evaluations : 0; }
double mrgfe_reg_trans_probability(const mrgfe_reg* reg) { return reg ? reg->trans_probability : 0.0; }
int    mrgfe_reg_hessian(const mrgfe_reg* reg, double out[36])
{
    if (!reg || !out) { set_error("mrgfe_reg_hessian: NULL argument"); return MRGFE_ERR_INVALID; }
    std::memcpy(out, reg->hessian, sizeof(reg->hessian));
    return MRGFE_OK;
}

// ---- NDT internals --------------------------------------------------------------------------------------------
static int ndt_evaluate_ppt(mrgfe_reg* reg, const float T[16], const double p[6], int mode, int ppt, double* score, double grad[6], double hess[36])
{
    if (!reg || !reg->ndt || !T || !p || !score || !grad || !hess) { set_error("mrgfe_ndt_evaluate: needs an NDT registration and non-NULL arguments"); return MRGFE_ERR_INVALID; }
    if (!reg->has_target || !reg->has_source) { set_error("evaluate: target / source not set"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    float Tr[16];
    col2row(T, Tr);
    NdtEngine& e = *reg->ndt;
    reg->book.clear_pairs();
    float ident[16];
    for (int i = 0; i < 16; ++i) ident[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    int pi = reg->book.add_pair_device(0, reg->d_src, reg->n_src, ident);
    if (pi < 0) return pi;
    return e.evaluate(0, Tr, p, mode, score, grad, hess, ppt);
}
int mrgfe_ndt_evaluate(mrgfe_reg* reg, const float T[16], const double p[6], int mode, double* score, double grad[6], double hess[36])
{
    return ndt_evaluate_ppt(reg, T, p, mode, 1, score, grad, hess);
}
int mrgfe_dbg_ndt_evaluate_ppt(mrgfe_reg* reg, const float T[16], const double p[6], int mode, int ppt, double* score, double grad[6], double hess[36])
{
    return ndt_evaluate_ppt(reg, T, p, mode, ppt, score, grad, hess);
}
int mrgfe_dbg_ndt_eval_neighbours(const mrgfe_reg* reg, double* neighbours)
{
    if (!reg || !reg->ndt || !neighbours) { set_error("mrgfe_dbg_ndt_eval_neighbours: needs an NDT registration and a non-NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(reg->ctx);
    *neighbours = reg->ndt->last_eval_neighbours();
    return MRGFE_OK;
}
int mrgfe_dbg_reg_ndt_rounds(const mrgfe_reg* reg, int cap, uint32_t* n_pairs, uint32_t* n_items)
{
    if (!reg || !reg->ndt || cap < 0) { set_error("mrgfe_dbg_reg_ndt_rounds: needs an NDT registration"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(reg->ctx);
    return reg->ndt->round_info(cap, n_pairs, n_items);
}

int mrgfe_knn(mrgfe_ctx* ctx, const float* cloud, size_t n, const float* query, size_t nq, size_t stride, int k, int32_t* idx, float* sqd)
{
    MRGFE_TRY(check_count(n, "mrgfe_knn"));
    MRGFE_TRY(check_count(nq, "mrgfe_knn"));
    if (!ctx || (n && !cloud) || (nq && (!query || !idx || !sqd))) { set_error("mrgfe_knn: NULL argument"); return MRGFE_ERR_INVALID; }
    if (k < 1 || k > 256) { set_error("mrgfe_knn: k must be in [1, 256]"); return MRGFE_ERR_INVALID; }
    if (nq == 0) return MRGFE_OK;
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf dd, di, dq, dc;  // (freed at the return in reverse order, the grid first)
    NnGrid grid;
    MRGFE_TRY(dc.ensure(std::max<size_t>(n, 1) * 16));
    MRGFE_TRY(dq.ensure(nq * 16));
    MRGFE_TRY(di.ensure(nq * k * 4));
    MRGFE_TRY(dd.ensure(nq * k * 4));
    if (n) MRGFE_TRY(upload_cloud(ctx, cloud, n, stride, dc.p));
    MRGFE_TRY(upload_cloud(ctx, query, nq, stride, dq.p));
    MRGFE_TRY(grid.build(ctx, dc.as<float4>(), n, 1.0f, NnGrid::kCrowdingKnn));
    MRGFE_TRY(grid.knn_device(ctx, dq.as<float4>(), nq, k, di.as<int32_t>(), dd.as<float>()));
    if (hipMemcpyAsync(idx, di.p, nq * k * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(sqd, dd.p, nq * k * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_error("mrgfe_knn: device to host copy failed");
        return MRGFE_ERR_HIP;
    }
    return MRGFE_OK;
}

int mrgfe_dbg_set_gicp_corr_passes(int mode) { return gicp_set_corr_passes(mode); }

int mrgfe_dbg_grid_set_query(mrgfe_ctx* ctx, const float* const* clouds, const size_t* n, int count, const float* query, size_t nq, int k, int rounds, int32_t* idx, float* sqd)
{
    if (!ctx || count < 1 || !clouds || !n || !query || !idx || !sqd || nq == 0) { set_error("mrgfe_dbg_grid_set_query: bad argument"); return MRGFE_ERR_INVALID; }
    if (k < 1 || k > 256) { set_error("mrgfe_dbg_grid_set_query: k must be in [1, 256]"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf     dd, di, dq;  // (freed in reverse order of declaration: the set, the clouds, then these)
    std::vector<DevBuf>        dc(count);
    std::vector<NnGrid>        grids(count);
    std::vector<NnGrid*>       gp(count);
    std::vector<const float4*> cp(count);
    std::vector<uint32_t>      nn(count);
    NnGridSet  set;
    int rc = dq.ensure(nq * 16);
    if (rc == MRGFE_OK) rc = di.ensure(nq * k * 4);
    if (rc == MRGFE_OK) rc = dd.ensure(nq * k * 4);
    if (rc == MRGFE_OK) rc = upload_cloud(ctx, query, nq, 16, dq.p);
    for (int m = 0; m < count && rc == MRGFE_OK; ++m) {
        rc = dc[m].ensure(std::max<size_t>(n[m], 1) * 16);
        if (rc == MRGFE_OK && n[m]) rc = upload_cloud(ctx, clouds[m], n[m], 16, dc[m].p);
        cp[m] = dc[m].as<float4>();
        nn[m] = static_cast<uint32_t>(n[m]);
        gp[m] = &grids[m];
    }
    // (built `rounds` times: the second and later builds start from the first one's cell edges)
    for (int r = 0; r < std::max(1, rounds) && rc == MRGFE_OK; ++r)
        rc = k == 1 ? set.build(ctx, cp.data(), nn.data(), count, 1.0f, NnGrid::kCrowding1nn, 1, gp.data()) : set.build(ctx, cp.data(), nn.data(), count, 1.0f, NnGrid::kCrowdingKnn, kNnMaxLevels, gp.data());
    for (int m = 0; m < count && rc == MRGFE_OK; ++m) {
        rc = k == 1 ? grids[m].nearest_device(ctx, dq.as<float4>(), nq, nullptr, di.as<int32_t>(), dd.as<float>()) : grids[m].knn_device(ctx, dq.as<float4>(), nq, k, di.as<int32_t>(), dd.as<float>());
        if (rc == MRGFE_OK && (hipMemcpyAsync(idx + size_t(m) * nq * k, di.p, nq * k * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                               hipMemcpyAsync(sqd + size_t(m) * nq * k, dd.p, nq * k * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)) {
            set_error("mrgfe_dbg_grid_set_query: device to host copy failed");
            rc = MRGFE_ERR_HIP;
        }
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == MRGFE_OK) rc = MRGFE_ERR_HIP;
    return rc;  // (every path waits for the stream above before the buffers go)
}

int mrgfe_gicp_linearize(mrgfe_reg* reg, const double T[16], double H[36], double b[6], double* sum_errors, int* n_correspondences)
{
    if (!reg || !reg->gicp || !T || !H || !b || !sum_errors || !n_correspondences) { set_error("mrgfe_gicp_linearize: needs a GICP registration and non-NULL arguments"); return MRGFE_ERR_INVALID; }
    if (reg->params.method == MRGFE_ICP_HIP) { set_error("mrgfe_gicp_linearize: ICP_HIP has no linearised cost"); return MRGFE_ERR_INVALID; }
    if (reg->params.method == MRGFE_PCL_GICP_HIP || reg->params.method == MRGFE_PCL_GICP_OMP_HIP) { set_error("mrgfe_gicp_linearize: PCL_GICP_HIP minimises with BFGS (mrgfe_pclgicp_evaluate)"); return MRGFE_ERR_INVALID; }
    if (!reg->has_target || !reg->has_source) { set_error("linearize: target / source not set"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    MRGFE_TRY(reg->ctx->bind());
    double Tr[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tr[r * 4 + c] = T[c * 4 + r];
    return reg->gicp->linearize(Tr, H, b, sum_errors, n_correspondences);
}

int mrgfe_gicp_error(mrgfe_reg* reg, const double T[16], double* sum_errors, int* n_terms)
{
    if (!reg || !reg->gicp || !T || !sum_errors || !n_terms) { set_error("mrgfe_gicp_error: needs a GICP registration and non-NULL arguments"); return MRGFE_ERR_INVALID; }
    if (reg->params.method == MRGFE_ICP_HIP) { set_error("mrgfe_gicp_error: ICP_HIP has no linearised cost"); return MRGFE_ERR_INVALID; }
    if (reg->params.method == MRGFE_PCL_GICP_HIP || reg->params.method == MRGFE_PCL_GICP_OMP_HIP) { set_error("mrgfe_gicp_error: PCL_GICP_HIP minimises with BFGS (mrgfe_pclgicp_evaluate)"); return MRGFE_ERR_INVALID; }
    if (!reg->has_target || !reg->has_source) { set_error("error: target / source not set"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    MRGFE_TRY(reg->ctx->bind());
    double Tr[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tr[r * 4 + c] = T[c * 4 + r];
    return reg->gicp->error(Tr, sum_errors, n_terms);
}

int mrgfe_pclgicp_evaluate(mrgfe_reg* reg, const float T[16], const double x[6], double* f, double grad[6], int* n_correspondences)
{
    if (!reg || !reg->gicp || !T || !x || !f || !grad || !n_correspondences) { set_error("mrgfe_pclgicp_evaluate: NULL argument"); return MRGFE_ERR_INVALID; }
    if (reg->params.method != MRGFE_PCL_GICP_HIP && reg->params.method != MRGFE_PCL_GICP_OMP_HIP) { set_error("mrgfe_pclgicp_evaluate: needs a PCL_GICP_HIP registration"); return MRGFE_ERR_INVALID; }
    if (!reg->has_target || !reg->has_source) { set_error("evaluate: target / source not set"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    MRGFE_TRY(reg->ctx->bind());
    float Tr[16], eye[16];
    col2row(T, Tr);
    for (int i = 0; i < 16; ++i) eye[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    MRGFE_TRY(reg->gicp->covariances(0, nullptr));  // covariances, target grid and work buffers in place
    return reg->gicp->pcl_evaluate(Tr, eye, reg->gicp->source_points(), true, x, f, grad, n_correspondences);
}

int mrgfe_gicp_covariances(mrgfe_reg* reg, int which, double* cov9_per_point)
{
    if (!reg || !reg->gicp || !cov9_per_point || which < 0 || which > 1) { set_error("mrgfe_gicp_covariances: needs a GICP registration, which in {0, 1} and an output buffer"); return MRGFE_ERR_INVALID; }
    if (reg->params.method == MRGFE_ICP_HIP) { set_error("mrgfe_gicp_covariances: ICP_HIP has no covariances"); return MRGFE_ERR_INVALID; }
    if ((which == 0 && !reg->has_source) || (which == 1 && !reg->has_target)) { set_error("covariances: cloud not set"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    MRGFE_TRY(reg->ctx->bind());
    return reg->gicp->covariances(which, cov9_per_point);
}

int mrgfe_ndt_num_leaves(const mrgfe_reg* reg) { return (reg && reg->ndt && reg->ndt->n_targets() > 0) ? static_cast<int>(reg->ndt->target(0).n_leaves) : 0; }

int mrgfe_ndt_grid(const mrgfe_reg* reg, int32_t min_b[3], int32_t max_b[3], int32_t div_b[3])
{
    if (!reg || !reg->ndt || reg->ndt->n_targets() == 0) { set_error("mrgfe_ndt_grid: no NDT target"); return MRGFE_ERR_STATE; }
    const NdtTargetInfo& t = reg->ndt->target(0);
    for (int a = 0; a < 3; ++a) { min_b[a] = t.min_b[a]; max_b[a] = t.max_b[a]; div_b[a] = t.div_b[a]; }
    return MRGFE_OK;
}

int mrgfe_ndt_leaves(mrgfe_reg* reg, int32_t* keys, int32_t* nr_points, double* mean3, double* icov9)
{
    if (!reg || !reg->ndt || reg->ndt->n_targets() == 0) { set_error("mrgfe_ndt_leaves: no NDT target"); return MRGFE_ERR_STATE; }
    MRGFE_LOCK(reg->ctx);
    return reg->ndt->read_leaves(0, keys, nr_points, mean3, icov9);
}

double mrgfe_ndt_mean_neighbours(const mrgfe_reg* reg) { return reg ? reg->mean_neighbours : 0.0; }

int mrgfe_reg_kernel_stats(const mrgfe_reg* reg, int mode, double* ms, int64_t* launches, double* bytes)
{
    if (!reg) { set_error("NULL registration"); return MRGFE_ERR_INVALID; }
    double m = 0, b = 0;
    int64_t l = 0;
    if (reg->ndt) reg->ndt->kernel_stats(mode, &m, &l, &b);
    if (reg->gicp) { m = reg->gicp->kernel_ms; l = reg->gicp->kernel_launches; b = reg->gicp->kernel_alg_bytes; }
    if (ms) *ms = m;
    if (launches) *launches = l;
    if (bytes) *bytes = b;
    return MRGFE_OK;
}

// ---- prefilters -----------------------------------------------------------------------------------------------
int mrgfe_distance_filter(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double near_thresh, double far_thresh, float* out, size_t* out_n)
{
    MRGFE_TRY(check_count(n, "mrgfe_distance_filter"));
    if (!ctx || !out_n || (n && (!xyzi || !out))) { set_error("mrgfe_distance_filter: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return filter_distance(ctx, xyzi, n, stride, near_thresh, far_thresh, out, out_n);
}
int mrgfe_approx_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float leaf, float* out, size_t* out_n)
{
    MRGFE_TRY(check_count(n, "mrgfe_approx_voxelgrid"));
    if (!ctx || !out_n || (n && (!xyzi || !out))) { set_error("mrgfe_approx_voxelgrid: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!(leaf > 0)) { set_error("mrgfe_approx_voxelgrid: leaf size must be > 0"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return filter_approx_voxelgrid(ctx, xyzi, n, stride, leaf, out, out_n);
}
int mrgfe_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float leaf, int min_pts, float* out, size_t* out_n, int* overflow)
{
    MRGFE_TRY(check_count(n, "mrgfe_voxelgrid"));
    if (!ctx || !out_n || (n && (!xyzi || !out))) { set_error("mrgfe_voxelgrid: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!(leaf > 0)) { set_error("mrgfe_voxelgrid: leaf size must be > 0"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return filter_voxelgrid(ctx, xyzi, n, stride, leaf, min_pts, out, out_n, overflow);
}
int mrgfe_radius_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double radius, int min_neighbors, float* out, size_t* out_n)
{
    MRGFE_TRY(check_count(n, "mrgfe_radius_outlier"));
    if (!ctx || !out_n || (n && (!xyzi || !out))) { set_error("mrgfe_radius_outlier: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!(radius > 0)) { set_error("mrgfe_radius_outlier: radius must be > 0"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return filter_radius_outlier(ctx, xyzi, n, stride, radius, min_neighbors, out, out_n);
}
int mrgfe_statistical_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, int mean_k, double stddev_mul, float* out, size_t* out_n)
{
    MRGFE_TRY(check_count(n, "mrgfe_statistical_outlier"));
    if (!ctx || !out_n || (n && (!xyzi || !out))) { set_error("mrgfe_statistical_outlier: NULL argument"); return MRGFE_ERR_INVALID; }
    if (mean_k < 1 || mean_k > 255) { set_error("mrgfe_statistical_outlier: mean_k must be in [1, 255]"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return filter_statistical_outlier(ctx, xyzi, n, stride, mean_k, stddev_mul, out, out_n);
}
void mrgfe_prefilter_default_params(mrgfe_prefilter_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->enable_distance_filter = 1;           // config/mrg_slam.yaml:62-64
    p->distance_near_thresh = 0.1;
    p->distance_far_thresh = 35.0;
    p->downsample_method = 1;                // :48-50
    p->downsample_resolution = 0.1;
    p->downsample_min_points_per_voxel = 1;
    p->outlier_removal_method = 1;           // :53-59
    p->radius_radius = 0.5;
    p->radius_min_neighbors = 2;
    p->statistical_mean_k = 30;
    p->statistical_stddev = 1.2;
}
static int prefilter_impl(mrgfe_ctx* ctx, const mrgfe_prefilter_params* p, const float* xyzi, size_t n, size_t stride, void* out, size_t* out_n, bool on_device,
                          const RecordSink* rec = nullptr);
int mrgfe_prefilter(mrgfe_ctx* ctx, const mrgfe_prefilter_params* p, const float* xyzi, size_t n, size_t stride, float* out, size_t* out_n)
{
    MRGFE_TRY(check_count(n, "mrgfe_prefilter"));
    return prefilter_impl(ctx, p, xyzi, n, stride, out, out_n, false);
}
int mrgfe_prefilter_device(mrgfe_ctx* ctx, const mrgfe_prefilter_params* p, const float* xyzi, size_t n, size_t stride, void* d_out, size_t* out_n)
{
    MRGFE_TRY(check_count(n, "mrgfe_prefilter_device"));
    return prefilter_impl(ctx, p, xyzi, n, stride, d_out, out_n, true);
}
// the ROS parameters -> the chain's switches; MRGFE_ERR_INVALID (message set, `fn` named) for what the component's constructor would not accept
static int chain_from_params(const char* fn, const mrgfe_prefilter_params* p, PrefilterChain* out)
{
    if (p->downsample_method < 0 || p->downsample_method > 2 || p->outlier_removal_method < 0 || p->outlier_removal_method > 2) { set_error("%s: unknown method", fn); return MRGFE_ERR_INVALID; }
    if (p->downsample_method >= 1 && !(p->downsample_resolution > 0)) { set_error("%s: downsample_resolution must be > 0", fn); return MRGFE_ERR_INVALID; }
    // (mean_k + 1 entries must fit the widest neighbour list, NnGrid::knn_device's 256)
    if (p->outlier_removal_method == 2 && p->statistical_mean_k > 255) { set_error("%s: statistical_mean_k must be in [1, 255]", fn); return MRGFE_ERR_INVALID; }
    PrefilterChain ch;
    ch.distance = p->enable_distance_filter != 0;
    ch.near_t = p->distance_near_thresh;
    ch.far_t = p->distance_far_thresh;
    ch.voxelgrid = p->downsample_method == 1;
    ch.approx_voxelgrid = p->downsample_method == 2;
    ch.leaf = static_cast<float>(p->downsample_resolution);
    ch.min_pts = p->downsample_min_points_per_voxel;
    ch.outlier = p->outlier_removal_method;
    ch.radius = p->radius_radius;
    ch.radius_min_neighbors = p->radius_min_neighbors;
    ch.mean_k = p->statistical_mean_k;
    ch.stddev_mul = p->statistical_stddev;
    *out = ch;
    return MRGFE_OK;
}
static int prefilter_impl(mrgfe_ctx* ctx, const mrgfe_prefilter_params* p, const float* xyzi, size_t n, size_t stride, void* out, size_t* out_n, bool on_device, const RecordSink* rec)
{
    if (!ctx || !p || !out_n || (n && (!xyzi || (!out && !rec)))) { set_error("mrgfe_prefilter: NULL argument"); return MRGFE_ERR_INVALID; }
    PrefilterChain ch;
    MRGFE_TRY(chain_from_params("mrgfe_prefilter", p, &ch));
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return filter_chain(ctx, ch, xyzi, n, stride, out, out_n, on_device, rec);
}
// What the record calls refuse before anything of the context is touched (mrgfe_scan_callback_records, mrgfe_prefilter_records,
// mrgfe_cloud_records_device): a NULL destination, a point_step other than the two of record_store.h, no room for one record per input point
static int check_record_sink(const char* fn, int point_step, void* records, size_t capacity_bytes, size_t n_in, RecordSink* sink)
{
    if (!records) { set_error("%s: NULL records", fn); return MRGFE_ERR_INVALID; }
    if (point_step != 16 && point_step != 32) { set_error("%s: point_step %d (16: x y z intensity, 32: pcl::PointXYZI)", fn, point_step); return MRGFE_ERR_INVALID; }
    if (capacity_bytes / size_t(point_step) < n_in) {
        set_error("%s: capacity_bytes %zu, %zu input points of %d bytes need room", fn, capacity_bytes, n_in, point_step);
        return MRGFE_ERR_INVALID;
    }
    sink->point_step = point_step;
    sink->records = records;
    sink->capacity = capacity_bytes;
    return MRGFE_OK;
}
int mrgfe_prefilter_records(mrgfe_ctx* ctx, const mrgfe_prefilter_params* p, const float* xyzi, size_t n, size_t stride, int point_step, void* records, size_t capacity_bytes,
                            void* d_out_xyzi, size_t* out_n)
{
    static const char* fn = "mrgfe_prefilter_records";
    return abi_guard(fn, [&]() -> int {
        MRGFE_TRY(check_count(n, fn));
        RecordSink sink;
        MRGFE_TRY(check_record_sink(fn, point_step, records, capacity_bytes, n, &sink));
        return prefilter_impl(ctx, p, xyzi, n, stride, d_out_xyzi, out_n, d_out_xyzi != nullptr, &sink);
    });
}

// ---- the scan callback: PointCloud2 bytes -> filtered scan (PrefilteringComponent::cloud_callback :116-156 in one call) -----------------------------
static_assert(sizeof(mrgfe_scan_params) == 200 && offsetof(mrgfe_scan_params, filters) == 128, "mrgfe_scan_params: the layout the bindings mirror");
size_t mrgfe_scan_params_size(void) { return sizeof(mrgfe_scan_params); }
void mrgfe_scan_default_params(mrgfe_scan_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->height = 1;  // (width: the caller's point count)
    p->point_step = 16;  // the replay scripts' layout: python_scripts/kitti_singlerobot_processor.py:164-185
    p->off_x = 0; p->off_y = 4; p->off_z = 8; p->off_intensity = 12;
    p->scan_period = 0.1;  // config/mrg_slam.yaml:45
    p->T[0] = p->T[5] = p->T[10] = p->T[15] = 1.0f;
    mrgfe_prefilter_default_params(&p->filters);
}
// rec_step != 0: the record form — `records` / `capacity_bytes` are checked (check_record_sink) and `out` is the caller's device buffer or NULL
// colored != NULL (mrgfe_scan_callback_outputs): the coloured cloud's 32-byte records beside whatever else the call makes; then `out` and `records` may both be
// NULL (no chain runs) and *out_n_colored receives width * height
static int scan_callback_impl(const char* fn, mrgfe_ctx* ctx, const mrgfe_scan_params* p, const uint8_t* data, void* out, size_t* out_n, bool on_device, bool as_records = false,
                              int rec_step = 0, void* records = nullptr, size_t capacity_bytes = 0, void* colored = nullptr, size_t colored_capacity_bytes = 0,
                              size_t* out_n_colored = nullptr)
{
    return abi_guard(fn, [&]() -> int {
        if (!ctx || !p || !out_n) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *out_n = 0;
        RecordSink sink, colored_sink;
        if (as_records) MRGFE_TRY(check_record_sink(fn, rec_step, records, capacity_bytes, size_t(p->width) * p->height, &sink));
        if (colored) MRGFE_TRY(check_record_sink(fn, 32, colored, colored_capacity_bytes, size_t(p->width) * p->height, &colored_sink));
        const RecordSink* rec = as_records ? &sink : nullptr;
        const RecordSink* col = colored ? &colored_sink : nullptr;
        PrefilterChain ch;
        MRGFE_TRY(chain_from_params(fn, &p->filters, &ch));
        if (size_t(p->width) * p->height == 0) return MRGFE_OK;  // where the reference returns early (:121-123)
        if (!data || (!out && !rec && !col)) { set_error("%s: NULL data / output", fn); return MRGFE_ERR_INVALID; }
        ScanHead h;
        h.data = data;
        h.width = p->width; h.height = p->height; h.point_step = p->point_step; h.row_step = p->row_step;
        h.off_x = p->off_x; h.off_y = p->off_y; h.off_z = p->off_z; h.off_intensity = p->off_intensity;
        MRGFE_TRY(check_pointcloud2_layout(ctx, fn, h.width, h.height, h.point_step, &h.row_step, h.off_x, h.off_y, h.off_z, h.off_intensity));
        h.deskew = p->deskew != 0;
        for (int k = 0; k < 3; ++k) h.ang_v[k] = p->ang_v[k];
        h.scan_period = p->scan_period;
        h.transform = p->transform != 0;
        float Tr[16];
        col2row(p->T, Tr);
        std::memcpy(h.T, Tr, sizeof(h.T));
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        if (!out && !rec) MRGFE_TRY(scan_colored_records(ctx, h, *col));  // (the coloured cloud alone: no chain)
        else MRGFE_TRY(scan_chain(ctx, ch, h, out, out_n, on_device, rec, col));
        if (col) *out_n_colored = size_t(h.width) * h.height;
        return MRGFE_OK;
    });
}
int mrgfe_scan_callback(mrgfe_ctx* ctx, const mrgfe_scan_params* p, const uint8_t* data, float* out_xyzi, size_t* out_n)
{
    return scan_callback_impl("mrgfe_scan_callback", ctx, p, data, out_xyzi, out_n, false);
}
int mrgfe_scan_callback_device(mrgfe_ctx* ctx, const mrgfe_scan_params* p, const uint8_t* data, void* d_out_xyzi, size_t* out_n)
{
    return scan_callback_impl("mrgfe_scan_callback_device", ctx, p, data, d_out_xyzi, out_n, true);
}
int mrgfe_scan_callback_records(mrgfe_ctx* ctx, const mrgfe_scan_params* p, const uint8_t* data, int point_step, void* records, size_t capacity_bytes, void* d_out_xyzi, size_t* out_n)
{
    return scan_callback_impl("mrgfe_scan_callback_records", ctx, p, data, d_out_xyzi, out_n, d_out_xyzi != nullptr, true, point_step, records, capacity_bytes);
}
size_t mrgfe_scan_outputs_size(void) { return sizeof(mrgfe_scan_outputs); }
int mrgfe_scan_callback_outputs(mrgfe_ctx* ctx, const mrgfe_scan_params* p, const uint8_t* data, const mrgfe_scan_outputs* o, size_t* out_n, size_t* out_n_colored)
{
    static const char* fn = "mrgfe_scan_callback_outputs";
    if (!o || !out_n_colored) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
    *out_n_colored = 0;
    if (!o->colored_records) {  // the call is mrgfe_scan_callback_records (which refuses NULL records)
        return scan_callback_impl(fn, ctx, p, data, o->d_out_xyzi, out_n, o->d_out_xyzi != nullptr, true, o->point_step, o->records, o->capacity_bytes);
    }
    return scan_callback_impl(fn, ctx, p, data, o->d_out_xyzi, out_n, o->d_out_xyzi != nullptr, o->records != nullptr, o->point_step, o->records, o->capacity_bytes,
                              o->colored_records, o->colored_capacity_bytes, out_n_colored);
}
int mrgfe_calc_fitness_score(mrgfe_ctx* ctx, const float* cloud1, size_t n1, const float* cloud2, size_t n2, size_t stride, const double relpose[16], double max_range, double* out)
{
    MRGFE_TRY(check_count(n1, "mrgfe_calc_fitness_score"));
    MRGFE_TRY(check_count(n2, "mrgfe_calc_fitness_score"));
    if (!ctx || !out || !relpose || (n1 && !cloud1) || (n2 && !cloud2)) { set_error("mrgfe_calc_fitness_score: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    if (n1 == 0 || n2 == 0) { *out = DBL_MAX; return MRGFE_OK; }
    DevBuf &d1 = ctx->scratch[10], &d2 = ctx->scratch[11];
    MRGFE_TRY(d1.ensure(n1 * 16));
    MRGFE_TRY(d2.ensure(n2 * 16));
    MRGFE_TRY(upload_cloud(ctx, cloud1, n1, stride, d1.p));
    MRGFE_TRY(upload_cloud(ctx, cloud2, n2, stride, d2.p));
    NnGrid& g = ctx_tmp_grid(ctx);
    int st = g.build(ctx, d1.as<float4>(), n1, 1.0f, NnGrid::kCrowding1nn, 1);
    if (st == MRGFE_OK) {
        float T[16];  // relpose.cast<float>(), row-major
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T[r * 4 + c] = static_cast<float>(relpose[c * 4 + r]);
        st = g.fitness(ctx, d2.as<float4>(), n2, T, max_range, out);
    }
    return st;
}

// ---- InformationMatrixCalculator (src/mrg_slam/information_matrix_calculator.cpp) ------------------------------------------
void mrgfe_inf_default_params(mrgfe_inf_params* p)
{
    if (!p) return;
    p->use_const_inf_matrix = 0;   // config/mrg_slam.yaml:216
    p->const_stddev_x = 0.5;       // :217
    p->const_stddev_q = 0.1;       // :218
    p->var_gain_a = 2.0;           // :219
    p->min_stddev_x = 0.1;         // :220
    p->max_stddev_x = 0.75;        // :221
    p->min_stddev_q = 0.05;        // :222
    p->max_stddev_q = 0.2;         // :223
    p->fitness_score_thresh = 1.25;  // :173
}
double mrgfe_inf_weight(double a, double max_x, double min_y, double max_y, double x)
{
    const double y = (1.0 - std::exp(-a * x)) / (1.0 - std::exp(-a * max_x));  // information_matrix_calculator.cpp:86
    return min_y + (max_y - min_y) * y;
}
int mrgfe_inf_matrix_from_fitness(const mrgfe_inf_params* p, double fitness_score, double inf[36])
{
    if (!p || !inf) { set_error("mrgfe_inf_matrix_from_fitness: NULL argument"); return MRGFE_ERR_INVALID; }
    double dx, dq;  // divisors of the two diagonal blocks
    if (p->use_const_inf_matrix) {  // :19-24 (divides by the standard deviation itself, as the reference does)
        dx = p->const_stddev_x;
        dq = p->const_stddev_q;
    } else {                        // :30-43
        const double min_var_x = std::pow(p->min_stddev_x, 2), max_var_x = std::pow(p->max_stddev_x, 2);
        const double min_var_q = std::pow(p->min_stddev_q, 2), max_var_q = std::pow(p->max_stddev_q, 2);
        dx = mrgfe_inf_weight(p->var_gain_a, p->fitness_score_thresh, min_var_x, max_var_x, fitness_score);
        dq = mrgfe_inf_weight(p->var_gain_a, p->fitness_score_thresh, min_var_q, max_var_q, fitness_score);
    }
    for (int k = 0; k < 36; ++k) inf[k] = 0.0;
    for (int k = 0; k < 3; ++k) { inf[k * 7] = 1.0 / dx; inf[(k + 3) * 7] = 1.0 / dq; }
    return MRGFE_OK;
}
int mrgfe_calc_information_matrix(mrgfe_ctx* ctx, const mrgfe_inf_params* p, const float* cloud1, size_t n1, const float* cloud2, size_t n2, size_t stride,
                                  const double relpose[16], double inf[36], double* fitness_out)
{
    MRGFE_TRY(check_count(n1, "mrgfe_calc_information_matrix"));
    MRGFE_TRY(check_count(n2, "mrgfe_calc_information_matrix"));
    if (!p || !inf) { set_error("mrgfe_calc_information_matrix: NULL argument"); return MRGFE_ERR_INVALID; }
    double fit = 0.0;
    if (!p->use_const_inf_matrix) MRGFE_TRY(mrgfe_calc_fitness_score(ctx, cloud1, n1, cloud2, n2, stride, relpose, DBL_MAX, &fit));  // the header's default max_range
    if (fitness_out) *fitness_out = fit;
    return mrgfe_inf_matrix_from_fitness(p, fit, inf);
}

// ---- map cloud, other-robot removal, deskewing --------------------------------------------------------------------
// shared tail of the two map-cloud entry points: run the device pass over `total` points (d_cat, or the per-keyframe
// pointers kf_ptrs), apply the reference's emptiness / capacity rules and bring the result down
static int map_cloud_finish(mrgfe_ctx* ctx, int K_all, const float4* d_cat, const float4* const* kf_ptrs, const std::vector<uint32_t>& off, const std::vector<float>& pose_f,
                            float resolution, int min_points_per_voxel, float distance_far_thresh, float* out, size_t capacity, size_t* out_n)
{
    const uint64_t total = off.back();
    size_t m = 0, unfiltered = 0;
    DevBuf dout;  // (a fresh buffer per call, freed at the return: after the download)
    if (total) {
        MRGFE_TRY(dout.ensure(total * 16));
        MRGFE_TRY(map_cloud_device(ctx, d_cat, off.data(), pose_f.data(), static_cast<int>(off.size()) - 1, resolution, min_points_per_voxel, distance_far_thresh, dout.as<float4>(), &m,
                                   &unfiltered, kf_ptrs));
    }
    // :57-60: the cloud BEFORE the voxel filter decides
    if (unfiltered == 0 && K_all > 1) { set_error("cloud is empty after processing keyframes"); return MRGFE_ERR_EMPTY; }
    if (m > capacity) { *out_n = m; set_error("map cloud: output needs %zu points, capacity is %zu", m, capacity); return MRGFE_ERR_INVALID; }
    if (m) {
        if (!out) { set_error("map cloud: NULL output"); return MRGFE_ERR_INVALID; }
        if (hipMemcpyAsync(out, dout.p, m * 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            set_error("map cloud: device to host copy failed");
            return MRGFE_ERR_HIP;
        }
    }
    *out_n = m;
    return MRGFE_OK;
}

int mrgfe_map_cloud_generate(mrgfe_ctx* ctx, int K, const float* const* clouds, const size_t* n_points, size_t stride, const double* poses, const uint8_t* first_keyframe,
                             float resolution, int min_points_per_voxel, float distance_far_thresh, int skip_first_cloud, float* out, size_t capacity, size_t* out_n)
{
    return abi_guard("mrgfe_map_cloud_generate", [&]() -> int {
        if (!ctx || !out_n || (K > 0 && (!clouds || !n_points || !poses))) { set_error("mrgfe_map_cloud_generate: NULL argument"); return MRGFE_ERR_INVALID; }
        *out_n = 0;
        if (K <= 0) { set_error("keyframes are empty, cannot generate map cloud"); return MRGFE_ERR_EMPTY; }  // map_cloud_generator.cpp:19-22
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        std::vector<uint32_t> off(1, 0u);
        std::vector<float>    pose_f;
        std::vector<int>      used;
        uint64_t total = 0;
        for (int k = 0; k < K; ++k) {
            if (first_keyframe && first_keyframe[k] && skip_first_cloud) continue;  // :32-34
            if (n_points[k] && !clouds[k]) { set_error("mrgfe_map_cloud_generate: NULL cloud %d", k); return MRGFE_ERR_INVALID; }
            total += n_points[k];
            if (total > 0x7fffffffu) { set_error("mrgfe_map_cloud_generate: more than 2^31 points"); return MRGFE_ERR_INVALID; }
            used.push_back(k);
            off.push_back(static_cast<uint32_t>(total));
            for (int t = 0; t < 16; ++t) pose_f.push_back(static_cast<float>(poses[16 * k + t]));  // pose.matrix().cast<float>()
        }
        DevBuf dcat;  // (a fresh buffer per call, freed at the return: after map_cloud_finish has freed its own and the download is done)
        if (total) {
            MRGFE_TRY(dcat.ensure(total * 16));
            for (size_t u = 0; u < used.size(); ++u)
                if (n_points[used[u]]) MRGFE_TRY(upload_cloud(ctx, clouds[used[u]], n_points[used[u]], stride, dcat.as<char>() + size_t(off[u]) * 16));
        }
        return map_cloud_finish(ctx, K, dcat.as<float4>(), nullptr, off, pose_f, resolution, min_points_per_voxel, distance_far_thresh, out, capacity, out_n);
    });
}

// ---- map store: keyframe clouds resident in HBM (include/mrgfe.h; struct mrgfe_map_store: api_internal.h) --------------------------------
int mrgfe_map_store_create(mrgfe_ctx* ctx, mrgfe_map_store** out)
{
    return abi_guard("mrgfe_map_store_create", [&]() -> int {
        if (!ctx || !out) { set_error("mrgfe_map_store_create: NULL argument"); return MRGFE_ERR_INVALID; }
        mrgfe_map_store* s = new (std::nothrow) mrgfe_map_store();
        if (!s) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        s->ctx = ctx;
        *out = s;
        return MRGFE_OK;
    });
}
void mrgfe_map_store_destroy(mrgfe_map_store* s)
{
    if (!s) return;
    MRGFE_LOCK(s->ctx);
    (void)s->ctx->bind();
    delete s;
}
int mrgfe_map_store_add(mrgfe_map_store* s, uint64_t key, const float* xyzi, size_t n, size_t stride)
{
    return abi_guard("mrgfe_map_store_add", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_map_store_add"));
        if (!s || key == 0 || (n && !xyzi)) { set_error("mrgfe_map_store_add: NULL store / cloud or key 0"); return MRGFE_ERR_INVALID; }
        if (n > 0x7fffffffu) { set_error("cloud too large"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        auto it = s->clouds.find(key);
        if (it != s->clouds.end()) {
            if (it->second.n == n) return MRGFE_OK;
            set_error("mrgfe_map_store_add: keyframe %llu is stored with %u points, not %zu", static_cast<unsigned long long>(key), it->second.n, n);
            return MRGFE_ERR_INVALID;
        }
        void* p = nullptr;
        if (n) {
            MRGFE_TRY(s->arena.alloc(n * 16, &p));
            MRGFE_TRY(upload_cloud(s->ctx, xyzi, n, stride, p));
        }
        s->clouds[key] = {static_cast<const float4*>(p), static_cast<uint32_t>(n)};
        s->bytes += n * 16;
        return MRGFE_OK;
    });
}
int mrgfe_map_store_has(const mrgfe_map_store* s, uint64_t key, size_t* n)
{
    if (!s) return 0;
    MRGFE_LOCK(s->ctx);
    auto it = s->clouds.find(key);
    if (it == s->clouds.end()) return 0;
    if (n) *n = it->second.n;
    return 1;
}
size_t mrgfe_map_store_bytes(const mrgfe_map_store* s)
{
    if (!s) return 0;
    MRGFE_LOCK(s->ctx);
    return s->bytes;
}
int mrgfe_map_store_generate(mrgfe_map_store* s, int K, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe, float resolution, int min_points_per_voxel,
                             float distance_far_thresh, int skip_first_cloud, float* out, size_t capacity, size_t* out_n)
{
    return abi_guard("mrgfe_map_store_generate", [&]() -> int {
        if (!s || !out_n || (K > 0 && (!keys || !poses))) { set_error("mrgfe_map_store_generate: NULL argument"); return MRGFE_ERR_INVALID; }
        *out_n = 0;
        if (K <= 0) { set_error("keyframes are empty, cannot generate map cloud"); return MRGFE_ERR_EMPTY; }  // map_cloud_generator.cpp:19-22
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        std::vector<uint32_t>      off(1, 0u);
        std::vector<float>         pose_f;
        std::vector<const float4*> ptrs;
        uint64_t total = 0;
        for (int k = 0; k < K; ++k) {
            if (first_keyframe && first_keyframe[k] && skip_first_cloud) continue;  // :32-34
            auto it = s->clouds.find(keys[k]);
            if (it == s->clouds.end()) { set_error("mrgfe_map_store_generate: keyframe %llu is not in the store", static_cast<unsigned long long>(keys[k])); return MRGFE_ERR_INVALID; }
            total += it->second.n;
            if (total > 0x7fffffffu) { set_error("mrgfe_map_store_generate: more than 2^31 points"); return MRGFE_ERR_INVALID; }
            ptrs.push_back(it->second.p);
            off.push_back(static_cast<uint32_t>(total));
            for (int t = 0; t < 16; ++t) pose_f.push_back(static_cast<float>(poses[16 * k + t]));
        }
        MRGFE_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));  // clouds added just before are still on their way up
        return map_cloud_finish(s->ctx, K, nullptr, ptrs.data(), off, pose_f, resolution, min_points_per_voxel, distance_far_thresh, out, capacity, out_n);
    });
}

// ---- egress: the map as wire records, stored keyframes read back (include/mrgfe.h) -----------------------------------------------------
static_assert(sizeof(mrgfe_map_publish_params) == 48, "mrgfe_map_publish_params: the layout the bindings mirror");
static_assert(sizeof(mrgfe_map_publish_result) == 32, "mrgfe_map_publish_result: the layout the bindings mirror");
size_t mrgfe_map_publish_params_size(void) { return sizeof(mrgfe_map_publish_params); }
size_t mrgfe_map_publish_result_size(void) { return sizeof(mrgfe_map_publish_result); }
void mrgfe_map_publish_default_params(mrgfe_map_publish_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->resolution = 0.1f;              // config/mrg_slam.yaml:235
    p->min_points_per_voxel = 1;       // :236
    p->distance_far_thresh = 10000.0f; // :237
    p->point_step = 32;
}
// One publish / read past its argument checks: the store's statistics start over, and what the workspace grew by is known when the call ends
struct EgressCall {
    mrgfe_map_store* s;
    size_t           before;
    explicit EgressCall(mrgfe_map_store* st) : s(st), before(st->egress.footprint(st->ctx)) { s->egress_stats = EgressStats(); }
    ~EgressCall() { s->egress_stats.grown = static_cast<int64_t>(s->egress.footprint(s->ctx) - before); }
};
// both forms behind their NULL checks; to_host: the records come down into `data` (capacity_bytes), else they stay in the workspace and *d_data receives their address
static int map_publish_locked(const char* fn, mrgfe_map_store* s, int K, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe, const mrgfe_map_publish_params* p,
                              bool to_host, void* data, size_t capacity_bytes, const void** d_data, mrgfe_map_publish_result* out)
{
    std::memset(out, 0, sizeof(*out));
    if (p->point_step != 16 && p->point_step != 32) { set_error("%s: point_step %d (32: pcl::PointXYZI records, 16: packed points)", fn, p->point_step); return MRGFE_ERR_INVALID; }
    if (p->n_offsets < 0 || p->n_offsets > 2) { set_error("%s: %d offsets (0 to 2)", fn, p->n_offsets); return MRGFE_ERR_INVALID; }
    out->point_step = p->point_step;
    out->off_intensity = p->point_step == 32 ? 16 : 12;
    if (K <= 0) { set_error("keyframes are empty, cannot generate map cloud"); return MRGFE_ERR_EMPTY; }  // map_cloud_generator.cpp:19-22
    MRGFE_LOCK(s->ctx);
    MRGFE_TRY(s->ctx->bind());
    std::vector<uint32_t>      off(1, 0u);
    std::vector<float>         pose_f;
    std::vector<const float4*> ptrs;
    uint64_t total = 0;
    for (int k = 0; k < K; ++k) {  // (as mrgfe_map_store_generate walks them: every key is looked up before anything is launched)
        if (first_keyframe && first_keyframe[k] && p->skip_first_cloud) continue;  // :32-34
        auto it = s->clouds.find(keys[k]);
        if (it == s->clouds.end()) { set_error("%s: keyframe %llu is not in the store", fn, static_cast<unsigned long long>(keys[k])); return MRGFE_ERR_INVALID; }
        total += it->second.n;
        if (total > 0x7fffffffu) { set_error("%s: more than 2^31 points", fn); return MRGFE_ERR_INVALID; }
        ptrs.push_back(it->second.p);
        off.push_back(static_cast<uint32_t>(total));
        for (int t = 0; t < 16; ++t) pose_f.push_back(static_cast<float>(poses[16 * k + t]));
    }
    EgressCall  call(s);
    EgressStats& st = s->egress_stats;
    MRGFE_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));  // clouds added just before are still on their way up
    st.waits += 1;
    EgressFormat f{p->point_step, p->n_offsets, {0, 0, 0, 0, 0, 0}};
    for (int t = 0; t < 3 * p->n_offsets; ++t) f.offsets[t] = p->offsets[t];
    size_t m = 0, unfiltered = 0;
    bool   complete = true;
    if (total) MRGFE_TRY(map_publish_device(s->ctx, s->egress, off.data(), pose_f.data(), static_cast<int>(ptrs.size()), ptrs.data(), p->resolution, p->min_points_per_voxel,
                                            p->distance_far_thresh, f, &m, &unfiltered, &complete, &st));
    // :57-60: the cloud BEFORE the voxel filter decides
    if (unfiltered == 0 && K > 1) { set_error("cloud is empty after processing keyframes"); return MRGFE_ERR_EMPTY; }
    out->n_points = m;
    out->n_unfiltered = unfiltered;
    out->data_bytes = uint64_t(m) * p->point_step;
    if (!to_host) {
        if (m && !complete) {  // the hand-over rule of the `_device` producers: the records are complete when the call returns, for readers on any stream
            MRGFE_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
            st.waits += 1;
        }
        *d_data = m ? s->egress.rec.p : nullptr;
        return MRGFE_OK;
    }
    if (out->data_bytes > capacity_bytes) { set_error("%s: the records need %llu bytes, capacity is %zu", fn, static_cast<unsigned long long>(out->data_bytes), capacity_bytes); return MRGFE_ERR_INVALID; }
    if (m) {
        if (!data) { set_error("%s: NULL data", fn); return MRGFE_ERR_INVALID; }
        MRGFE_HIP_CHECK(hipMemcpyAsync(data, s->egress.rec.p, out->data_bytes, hipMemcpyDeviceToHost, s->ctx->stream));
        MRGFE_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
        st.waits += 1;
        st.bytes_down = static_cast<int64_t>(out->data_bytes);
    }
    return MRGFE_OK;
}
int mrgfe_map_store_publish(mrgfe_map_store* s, int K, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe, const mrgfe_map_publish_params* p, void* data,
                            size_t capacity_bytes, mrgfe_map_publish_result* out)
{
    static const char* fn = "mrgfe_map_store_publish";
    return abi_guard(fn, [&]() -> int {
        if (!s || !p || !out || (K > 0 && (!keys || !poses))) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        return map_publish_locked(fn, s, K, keys, poses, first_keyframe, p, true, data, capacity_bytes, nullptr, out);
    });
}
int mrgfe_map_store_publish_device(mrgfe_map_store* s, int K, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe, const mrgfe_map_publish_params* p,
                                   const void** d_data, mrgfe_map_publish_result* out)
{
    static const char* fn = "mrgfe_map_store_publish_device";
    return abi_guard(fn, [&]() -> int {
        if (!s || !p || !out || !d_data || (K > 0 && (!keys || !poses))) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *d_data = nullptr;
        return map_publish_locked(fn, s, K, keys, poses, first_keyframe, p, false, nullptr, 0, d_data, out);
    });
}
int mrgfe_map_store_read(mrgfe_map_store* s, int n_keys, const uint64_t* keys, int point_step, void* data, size_t capacity_bytes, uint64_t* offsets_bytes)
{
    static const char* fn = "mrgfe_map_store_read";
    return abi_guard(fn, [&]() -> int {
        if (!s || n_keys < 0 || !offsets_bytes || (n_keys > 0 && !keys)) { set_error("%s: NULL argument or a negative count", fn); return MRGFE_ERR_INVALID; }
        if (point_step != 16 && point_step != 32) { set_error("%s: point_step %d (32: pcl::PointXYZI records, 16: packed points)", fn, point_step); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        std::vector<KeyframeRecordItem> items;
        uint64_t points = 0;
        for (int i = 0; i < n_keys; ++i) {  // every key is looked up before anything is written
            auto it = s->clouds.find(keys[i]);
            if (it == s->clouds.end()) { set_error("%s: keyframe %llu is not in the store", fn, static_cast<unsigned long long>(keys[i])); return MRGFE_ERR_INVALID; }
            items.push_back({it->second.p, it->second.n, points});
            points += it->second.n;
        }
        if (points > kMaxPoints) { set_error("%s: more than 2^31 - 1 points", fn); return MRGFE_ERR_INVALID; }
        for (int i = 0; i < n_keys; ++i) offsets_bytes[i] = items[i].first_record * uint64_t(point_step);
        offsets_bytes[n_keys] = points * uint64_t(point_step);
        const uint64_t bytes = offsets_bytes[n_keys];
        if (bytes > capacity_bytes) { set_error("%s: the records need %llu bytes, capacity is %zu", fn, static_cast<unsigned long long>(bytes), capacity_bytes); return MRGFE_ERR_INVALID; }
        EgressCall  call(s);
        EgressStats& st = s->egress_stats;
        if (!points) return MRGFE_OK;
        if (!data) { set_error("%s: NULL data", fn); return MRGFE_ERR_INVALID; }
        mrgfe_ctx* ctx = s->ctx;
        if (point_step == 16) {  // the stored clouds are the records: copies out of the arena, behind whatever is still filling it on the stream
            for (const KeyframeRecordItem& it : items)
                if (it.n) MRGFE_HIP_CHECK(hipMemcpyAsync(static_cast<char*>(data) + it.first_record * 16, it.d_cloud, size_t(it.n) * 16, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            MRGFE_TRY(s->egress.rec.ensure(bytes));
            MRGFE_TRY(keyframe_records_many_device(ctx, items.data(), items.size(), s->egress.rec.p));
            st.launches += 1;
            MRGFE_HIP_CHECK(hipMemcpyAsync(data, s->egress.rec.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the only wait
        st.waits += 1;
        st.bytes_down = static_cast<int64_t>(bytes);
        return MRGFE_OK;
    });
}
int mrgfe_map_store_egress_stats(const mrgfe_map_store* s, int64_t out[4])
{
    if (!s || !out) { set_error("mrgfe_map_store_egress_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(s->ctx);
    out[0] = s->egress_stats.launches; out[1] = s->egress_stats.waits; out[2] = s->egress_stats.bytes_down; out[3] = s->egress_stats.grown;
    return MRGFE_OK;
}

int mrgfe_map_store_fitness(mrgfe_map_store* s, uint64_t key1, uint64_t key2, const double relpose[16], double max_range, double* out)
{
    return abi_guard("mrgfe_map_store_fitness", [&]() -> int {
        if (!s || !relpose || !out) { set_error("mrgfe_map_store_fitness: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        auto i1 = s->clouds.find(key1), i2 = s->clouds.find(key2);
        if (i1 == s->clouds.end() || i2 == s->clouds.end()) {
            set_error("mrgfe_map_store_fitness: keyframe %llu is not in the store", static_cast<unsigned long long>(i1 == s->clouds.end() ? key1 : key2));
            return MRGFE_ERR_INVALID;
        }
        if (i1->second.n == 0 || i2->second.n == 0) { *out = DBL_MAX; return MRGFE_OK; }
        mrgfe_map_store::CachedGrid* g = nullptr;
        for (auto& c : s->grids) if (c->key == key1) g = c.get();
        if (!g) {
            if (s->grids.size() < s->max_grids) { s->grids.push_back(std::make_unique<mrgfe_map_store::CachedGrid>()); g = s->grids.back().get(); }
            else { g = s->grids[0].get(); for (auto& c : s->grids) if (c->tick < g->tick) g = c.get(); }
            g->key = 0;
            MRGFE_TRY(g->grid.build(s->ctx, i1->second.p, i1->second.n, 1.0f, NnGrid::kCrowding1nn, 1));
            g->key = key1;
        }
        g->tick = ++s->tick;
        float T[16];  // relpose.cast<float>(), row-major
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T[r * 4 + c] = static_cast<float>(relpose[c * 4 + r]);
        return g->grid.fitness(s->ctx, i2->second.p, i2->second.n, T, max_range, out);
    });
}
int mrgfe_map_store_information_matrix(mrgfe_map_store* s, const mrgfe_inf_params* p, uint64_t key1, uint64_t key2, const double relpose[16], double inf[36], double* fitness_out)
{
    if (!p || !inf) { set_error("mrgfe_map_store_information_matrix: NULL argument"); return MRGFE_ERR_INVALID; }
    double fit = 0.0;
    if (!p->use_const_inf_matrix) MRGFE_TRY(mrgfe_map_store_fitness(s, key1, key2, relpose, DBL_MAX, &fit));
    if (fitness_out) *fitness_out = fit;
    return mrgfe_inf_matrix_from_fitness(p, fit, inf);
}

// ---- the keyframe callback: PointCloud2 bytes -> keyframe `key` of the store (MrgSlamComponent::cloud_callback :372-446 in one call) ----------------
static_assert(sizeof(mrgfe_keyframe_params) == 32, "mrgfe_keyframe_params: the layout the bindings mirror");
size_t mrgfe_keyframe_params_size(void) { return sizeof(mrgfe_keyframe_params); }
void mrgfe_keyframe_default_params(mrgfe_keyframe_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->height = 1;  // (width: the caller's point count)
    p->point_step = 16;  // the replay scripts' layout: python_scripts/kitti_singlerobot_processor.py:164-185
    p->off_x = 0; p->off_y = 4; p->off_z = 8; p->off_intensity = 12;
}
// The callback behind its argument checks, for both forms (the caller holds the context's lock and has bound its device; `l` has passed
// check_pointcloud2_layout): `d_records` NULL: `raw_bytes` of `data` go up through the raw staging path first; else the records are read where they are.
static int keyframe_callback_locked(const char* fn, mrgfe_map_store* s, uint64_t key, const KeyframeLayout& l, const void* data, size_t raw_bytes, const void* d_records,
                                    const float* centres, int n_centres, float radius_sqr, float* kept, size_t* n_kept, float* removed, size_t* n_removed,
                                    bool as_records = false, const RecordSink* kept_rec = nullptr, const RecordSink* removed_rec = nullptr)
{
    const size_t n = size_t(l.width) * l.height;
    if (s->clouds.count(key)) { set_error("%s: keyframe %llu is already stored", fn, static_cast<unsigned long long>(key)); return MRGFE_ERR_STATE; }
    size_t nk = 0, nr = 0;
    void*  p = nullptr;
    if (n) {
        mrgfe_ctx* ctx = s->ctx;
        MRGFE_TRY(s->arena.alloc(n * 16, &p));  // room for every point; what the removal does not keep is handed back below
        DevBuf& drem = ctx->scratch[2];
        auto run = [&]() -> int {
            const void* d_raw = d_records;
            if (!d_raw) MRGFE_TRY(upload_raw_records(ctx, data, raw_bytes, &d_raw));
            if (as_records) {
                // the record form (mrgfe_keyframe_callback_records): the same gather or split, then ONE record launch over the stored cloud and the removed
                // points and the wait behind it — without centres the call's only one, else its second
                if (n_centres == 0) {
                    MRGFE_TRY(keyframe_gather_device(ctx, d_raw, l, static_cast<float4*>(p)));
                    nk = n;
                } else {
                    if (removed_rec) MRGFE_TRY(drem.ensure(n * 16));
                    MRGFE_TRY(keyframe_split_device(ctx, d_raw, l, centres, n_centres, radius_sqr, static_cast<float4*>(p), &nk, removed_rec ? drem.as<float4>() : nullptr, &nr));  // (the first wait)
                }
                if ((kept_rec && nk) || (removed_rec && nr)) return cloud_pair_records_device(ctx, static_cast<const float4*>(p), nk, kept_rec, drem.as<float4>(), nr, removed_rec);
                if (n_centres == 0) MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (no record is wanted: the gather is still waited for)
                return MRGFE_OK;
            }
            if (n_centres == 0) {
                MRGFE_TRY(keyframe_gather_device(ctx, d_raw, l, static_cast<float4*>(p)));
                nk = n;
            } else {
                if (removed) MRGFE_TRY(drem.ensure(n * 16));
                MRGFE_TRY(keyframe_split_device(ctx, d_raw, l, centres, n_centres, radius_sqr, static_cast<float4*>(p), &nk, removed ? drem.as<float4>() : nullptr, &nr));  // (the first wait)
                if (!((kept && nk) || (removed && nr))) return MRGFE_OK;  // nothing to bring down: the stream is idle
            }
            if (kept && nk) MRGFE_HIP_CHECK(hipMemcpyAsync(kept, p, nk * 16, hipMemcpyDeviceToHost, ctx->stream));
            if (removed && nr) MRGFE_HIP_CHECK(hipMemcpyAsync(removed, drem.p, nr * 16, hipMemcpyDeviceToHost, ctx->stream));
            MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // without centres the only wait, else the second
            return MRGFE_OK;
        };
        const int rc = run();
        if (rc != MRGFE_OK) {
            (void)hipStreamSynchronize(ctx->stream);  // nothing is in flight when the room goes back
            s->arena.shrink_last(p, n * 16, 0);
            return rc;
        }
        s->arena.shrink_last(p, n * 16, nk * 16);
        if (nk == 0) p = nullptr;
    }
    s->clouds[key] = {static_cast<const float4*>(p), static_cast<uint32_t>(nk)};
    s->bytes += nk * 16;
    *n_kept = nk;
    if (n_removed) *n_removed = nr;
    return MRGFE_OK;
}
// what both forms refuse before they look at the cloud
static int keyframe_callback_check(const char* fn, uint64_t key, const float* centres, int n_centres)
{
    if (key == 0) { set_error("%s: key 0", fn); return MRGFE_ERR_INVALID; }
    if (n_centres < 0 || n_centres > kMaxCentres || (n_centres > 0 && !centres)) { set_error("%s: %d centres (0 to %d, and their positions)", fn, n_centres, kMaxCentres); return MRGFE_ERR_INVALID; }
    return MRGFE_OK;
}
int mrgfe_keyframe_callback(mrgfe_map_store* s, uint64_t key, const mrgfe_keyframe_params* lay, const void* data, size_t data_bytes, const float* centres, int n_centres,
                            float radius_sqr, float* kept, size_t* n_kept, float* removed, size_t* n_removed)
{
    static const char* fn = "mrgfe_keyframe_callback";
    return abi_guard(fn, [&]() -> int {
        if (!s || !lay || !n_kept) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *n_kept = 0;
        if (n_removed) *n_removed = 0;
        MRGFE_TRY(keyframe_callback_check(fn, key, centres, n_centres));
        KeyframeLayout l{lay->width, lay->height, lay->point_step, lay->row_step, lay->off_x, lay->off_y, lay->off_z, lay->off_intensity};
        MRGFE_TRY(check_pointcloud2_layout(s->ctx, fn, l.width, l.height, l.point_step, &l.row_step, l.off_x, l.off_y, l.off_z, l.off_intensity));
        const size_t n = size_t(l.width) * l.height;
        const size_t raw_bytes = n ? size_t(l.height - 1) * l.row_step + size_t(l.width) * l.point_step : 0;
        if (n && !data) { set_error("%s: NULL data", fn); return MRGFE_ERR_INVALID; }
        if (data_bytes < raw_bytes) { set_error("%s: the payload has %zu bytes, the layout needs %zu", fn, data_bytes, raw_bytes); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        return keyframe_callback_locked(fn, s, key, l, data, raw_bytes, nullptr, centres, n_centres, radius_sqr, kept, n_kept, removed, n_removed);
    });
}
// MRGFE_OK when the n packed points at `d` are device memory of the context's GPU (both ends of the cloud are asked about: hipPointerGetAttributes);
// anything else — host memory, managed memory, another GPU's, a pointer the runtime does not know — is refused unread
static int check_device_cloud(const mrgfe_ctx* ctx, const char* fn, const void* d, size_t n)
{
    const char* ends[2] = {static_cast<const char*>(d), static_cast<const char*>(d) + n * 16 - 1};
    for (const char* e : ends) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, e) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != ctx->device) {
            (void)hipGetLastError();  // (a pointer the runtime does not know is an error to the query, not a failure of the device)
            set_error("%s: the cloud is not in the memory of device %d", fn, ctx->device);
            return MRGFE_ERR_INVALID;
        }
    }
    return MRGFE_OK;
}
int mrgfe_cloud_records_device(mrgfe_ctx* ctx, const void* d_xyzi, size_t n, int point_step, void* records, size_t capacity_bytes)
{
    static const char* fn = "mrgfe_cloud_records_device";
    return abi_guard(fn, [&]() -> int {
        MRGFE_TRY(check_count(n, fn));
        if (!ctx || (n && !d_xyzi)) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        RecordSink sink;
        MRGFE_TRY(check_record_sink(fn, point_step, records, capacity_bytes, n, &sink));
        if (n == 0) return MRGFE_OK;  // (nothing to ask of the device, as for an empty message)
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        MRGFE_TRY(check_device_cloud(ctx, fn, d_xyzi, n));
        return cloud_records_device(ctx, static_cast<const float4*>(d_xyzi), n, sink);
    });
}
int mrgfe_keyframe_callback_device(mrgfe_map_store* s, uint64_t key, const void* d_xyzi, size_t n, const float* centres, int n_centres, float radius_sqr, float* kept,
                                   size_t* n_kept, float* removed, size_t* n_removed)
{
    static const char* fn = "mrgfe_keyframe_callback_device";
    return abi_guard(fn, [&]() -> int {
        if (!n_kept) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *n_kept = 0;
        if (n_removed) *n_removed = 0;
        // (what can be refused without the store is refused first)
        MRGFE_TRY(keyframe_callback_check(fn, key, centres, n_centres));
        MRGFE_TRY(check_count(n, fn));
        if (n && !d_xyzi) { set_error("%s: NULL cloud", fn); return MRGFE_ERR_INVALID; }
        if (!s) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        // a packed device cloud is a PointCloud2 payload with point_step 16 that already sits where the head kernel reads it (one row: its row_step, which
        // past 2^28 points no longer fits the field, is never multiplied)
        const KeyframeLayout l{static_cast<uint32_t>(n), 1, 16, static_cast<uint32_t>(n * 16), 0, 4, 8, 12};
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        if (n) MRGFE_TRY(check_device_cloud(s->ctx, fn, d_xyzi, n));
        return keyframe_callback_locked(fn, s, key, l, nullptr, 0, n ? d_xyzi : nullptr, centres, n_centres, radius_sqr, kept, n_kept, removed, n_removed);
    });
}
// the two sinks of the record forms: each one that is given is checked as every record sink is (check_record_sink), a NULL one stays NULL
static int keyframe_record_sinks(const char* fn, int point_step, size_t n, void* kept_records, size_t kept_capacity, void* removed_records, size_t removed_capacity,
                                 RecordSink* kept, RecordSink* removed, const RecordSink** kept_rec, const RecordSink** removed_rec)
{
    *kept_rec = *removed_rec = nullptr;
    if (kept_records) { MRGFE_TRY(check_record_sink(fn, point_step, kept_records, kept_capacity, n, kept)); *kept_rec = kept; }
    if (removed_records) { MRGFE_TRY(check_record_sink(fn, point_step, removed_records, removed_capacity, n, removed)); *removed_rec = removed; }
    return MRGFE_OK;
}
int mrgfe_keyframe_callback_records(mrgfe_map_store* s, uint64_t key, const mrgfe_keyframe_params* lay, const void* data, size_t data_bytes, const float* centres, int n_centres,
                                    float radius_sqr, int point_step, void* kept_records, size_t kept_capacity_bytes, size_t* n_kept, void* removed_records,
                                    size_t removed_capacity_bytes, size_t* n_removed)
{
    static const char* fn = "mrgfe_keyframe_callback_records";
    return abi_guard(fn, [&]() -> int {
        if (!s || !lay || !n_kept) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *n_kept = 0;
        if (n_removed) *n_removed = 0;
        MRGFE_TRY(keyframe_callback_check(fn, key, centres, n_centres));
        KeyframeLayout l{lay->width, lay->height, lay->point_step, lay->row_step, lay->off_x, lay->off_y, lay->off_z, lay->off_intensity};
        MRGFE_TRY(check_pointcloud2_layout(s->ctx, fn, l.width, l.height, l.point_step, &l.row_step, l.off_x, l.off_y, l.off_z, l.off_intensity));
        const size_t n = size_t(l.width) * l.height;
        const size_t raw_bytes = n ? size_t(l.height - 1) * l.row_step + size_t(l.width) * l.point_step : 0;
        if (n && !data) { set_error("%s: NULL data", fn); return MRGFE_ERR_INVALID; }
        if (data_bytes < raw_bytes) { set_error("%s: the payload has %zu bytes, the layout needs %zu", fn, data_bytes, raw_bytes); return MRGFE_ERR_INVALID; }
        RecordSink        kept, removed;
        const RecordSink *kept_rec, *removed_rec;
        MRGFE_TRY(keyframe_record_sinks(fn, point_step, n, kept_records, kept_capacity_bytes, removed_records, removed_capacity_bytes, &kept, &removed, &kept_rec, &removed_rec));
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        return keyframe_callback_locked(fn, s, key, l, data, raw_bytes, nullptr, centres, n_centres, radius_sqr, nullptr, n_kept, nullptr, n_removed, true, kept_rec, removed_rec);
    });
}
int mrgfe_keyframe_callback_records_device(mrgfe_map_store* s, uint64_t key, const void* d_xyzi, size_t n, const float* centres, int n_centres, float radius_sqr, int point_step,
                                           void* kept_records, size_t kept_capacity_bytes, size_t* n_kept, void* removed_records, size_t removed_capacity_bytes, size_t* n_removed)
{
    static const char* fn = "mrgfe_keyframe_callback_records_device";
    return abi_guard(fn, [&]() -> int {
        if (!n_kept) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *n_kept = 0;
        if (n_removed) *n_removed = 0;
        MRGFE_TRY(keyframe_callback_check(fn, key, centres, n_centres));
        MRGFE_TRY(check_count(n, fn));
        if (n && !d_xyzi) { set_error("%s: NULL cloud", fn); return MRGFE_ERR_INVALID; }
        if (!s) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        RecordSink        kept, removed;
        const RecordSink *kept_rec, *removed_rec;
        MRGFE_TRY(keyframe_record_sinks(fn, point_step, n, kept_records, kept_capacity_bytes, removed_records, removed_capacity_bytes, &kept, &removed, &kept_rec, &removed_rec));
        const KeyframeLayout l{static_cast<uint32_t>(n), 1, 16, static_cast<uint32_t>(n * 16), 0, 4, 8, 12};  // (as mrgfe_keyframe_callback_device)
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        if (n) MRGFE_TRY(check_device_cloud(s->ctx, fn, d_xyzi, n));
        return keyframe_callback_locked(fn, s, key, l, nullptr, 0, n ? d_xyzi : nullptr, centres, n_centres, radius_sqr, nullptr, n_kept, nullptr, n_removed, true, kept_rec, removed_rec);
    });
}

// ---- the graph database's loops in one call each: many keyframe messages into the store, many edges scored (include/mrgfe.h) -----------------------
static_assert(sizeof(mrgfe_keyframe_msg) == 56, "mrgfe_keyframe_msg: the layout the bindings mirror");
static_assert(sizeof(mrgfe_graph_edge) == 144, "mrgfe_graph_edge: the layout the bindings mirror");
size_t mrgfe_keyframe_msg_size(void) { return sizeof(mrgfe_keyframe_msg); }
size_t mrgfe_graph_edge_size(void) { return sizeof(mrgfe_graph_edge); }

int mrgfe_map_store_add_keyframes(mrgfe_map_store* s, int n, const mrgfe_keyframe_msg* msgs, uint8_t* added)
{
    static const char* fn = "mrgfe_map_store_add_keyframes";
    return abi_guard(fn, [&]() -> int {
        if (added && n > 0) std::memset(added, 0, size_t(n));
        if (!s || n < 0 || (n > 0 && !msgs)) { set_error("%s: NULL argument or a negative count", fn); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        // 1. every message is checked before anything is allocated or sent
        struct New { int msg; KeyframeLayout lay; size_t n, raw_bytes, raw_at, cloud_at; };
        std::vector<New> fresh;
        std::unordered_map<uint64_t, size_t> in_call;  // keys this call adds -> their point count
        size_t raw_total = 0, block = 0, points = 0;
        for (int i = 0; i < n; ++i) {
            const mrgfe_keyframe_msg& m = msgs[i];
            const unsigned long long  key = static_cast<unsigned long long>(m.key);
            if (m.key == 0) { set_error("%s: message %d: key 0", fn, i); return MRGFE_ERR_INVALID; }
            KeyframeLayout l{m.layout.width, m.layout.height, m.layout.point_step, m.layout.row_step, m.layout.off_x, m.layout.off_y, m.layout.off_z, m.layout.off_intensity};
            MRGFE_TRY(check_pointcloud2_layout(s->ctx, fn, l.width, l.height, l.point_step, &l.row_step, l.off_x, l.off_y, l.off_z, l.off_intensity));
            const size_t np = size_t(l.width) * l.height;
            const size_t raw_bytes = np ? size_t(l.height - 1) * l.row_step + size_t(l.width) * l.point_step : 0;
            if (np && !m.data) { set_error("%s: message %d (keyframe %llu): NULL data", fn, i, key); return MRGFE_ERR_INVALID; }
            if (m.data_bytes < raw_bytes) { set_error("%s: message %d (keyframe %llu): the payload has %zu bytes, the layout needs %zu", fn, i, key, m.data_bytes, raw_bytes); return MRGFE_ERR_INVALID; }
            size_t have = 0;
            bool   known = false;
            auto it = s->clouds.find(m.key);
            if (it != s->clouds.end()) { known = true; have = it->second.n; }
            else { auto jt = in_call.find(m.key); if (jt != in_call.end()) { known = true; have = jt->second; } }
            if (known) {
                if (have == np) continue;  // graph_database.cpp:173-178, :272-274: already in the graph or in the queue
                set_error("%s: message %d: keyframe %llu is stored with %zu points, not %zu", fn, i, key, have, np);
                return MRGFE_ERR_STATE;
            }
            in_call[m.key] = np;
            fresh.push_back({i, l, np, raw_bytes, raw_total, block});
            raw_total += (raw_bytes + 255) & ~size_t(255);
            block += (np * 16 + 255) & ~size_t(255);  // every cloud starts on a 256-byte line, as the clouds of mrgfe_map_store_add do
            points += np;
        }
        s->clouds.reserve(s->clouds.size() + fresh.size());
        // 2. one block, the payloads behind one another, one launch, one wait
        char* base = nullptr;
        if (points) {
            mrgfe_ctx* ctx = s->ctx;
            void* p = nullptr;
            MRGFE_TRY(s->arena.alloc(block, &p));
            base = static_cast<char*>(p);
            auto run = [&]() -> int {
                MRGFE_TRY(ctx->up_raw.ensure(raw_total));  // (grown BEFORE the first copy: stream order keeps the earlier readers of the old buffer safe)
                std::vector<KeyframeGatherItem> items;
                for (const New& f : fresh) {
                    if (!f.n) continue;
                    char* d_raw = ctx->up_raw.as<char>() + f.raw_at;
                    MRGFE_TRY(upload_raw_records_to(ctx, msgs[f.msg].data, f.raw_bytes, d_raw));
                    items.push_back({d_raw, f.lay, reinterpret_cast<float4*>(base + f.cloud_at)});
                }
                MRGFE_TRY(keyframe_gather_many_device(ctx, items.data(), items.size()));
                MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the only wait
                return MRGFE_OK;
            };
            const int rc = run();
            if (rc != MRGFE_OK) {
                (void)hipStreamSynchronize(ctx->stream);  // nothing is in flight when the block goes back
                s->arena.shrink_last(p, block, 0);
                return rc;
            }
        }
        for (const New& f : fresh) {
            s->clouds[msgs[f.msg].key] = {f.n ? reinterpret_cast<const float4*>(base + f.cloud_at) : nullptr, static_cast<uint32_t>(f.n)};
            s->bytes += f.n * 16;
            if (added) added[f.msg] = 1;
        }
        return MRGFE_OK;
    });
}

int mrgfe_map_store_edges(mrgfe_map_store* s, const mrgfe_inf_params* p, int n_edges, const mrgfe_graph_edge* edges, double* inf, double* fitness)
{
    static const char* fn = "mrgfe_map_store_edges";
    return abi_guard(fn, [&]() -> int {
        if (!p || n_edges < 0 || (n_edges > 0 && (!edges || !inf))) { set_error("%s: NULL argument or a negative count", fn); return MRGFE_ERR_INVALID; }
        const size_t E = static_cast<size_t>(n_edges);
        std::vector<double> fit(E, 0.0), mats(36 * E);
        if (!p->use_const_inf_matrix && E) {
            if (!s) { set_error("%s: NULL store", fn); return MRGFE_ERR_INVALID; }
            MRGFE_LOCK(s->ctx);
            MRGFE_TRY(s->ctx->bind());
            struct Side { const float4* p; uint32_t n; };
            std::vector<Side> c1(E), c2(E);
            for (size_t e = 0; e < E; ++e) {
                auto i1 = s->clouds.find(edges[e].key1), i2 = s->clouds.find(edges[e].key2);
                if (i1 == s->clouds.end() || i2 == s->clouds.end()) {
                    set_error("%s: edge %zu: keyframe %llu is not in the store", fn, e, static_cast<unsigned long long>(i1 == s->clouds.end() ? edges[e].key1 : edges[e].key2));
                    return MRGFE_ERR_INVALID;
                }
                c1[e] = {i1->second.p, i1->second.n};
                c2[e] = {i2->second.p, i2->second.n};
            }
            // the grid of every distinct key1 that has points on both sides of one of its edges: the single calls' cache, the last set, or a new set
            std::unordered_map<uint64_t, const NnGrid*> grid_of;
            std::vector<uint64_t>      set_keys;  // key1s the cache does not hold, in order of appearance
            std::vector<const float4*> set_p;
            std::vector<uint32_t>      set_n;
            for (size_t e = 0; e < E; ++e) {
                const uint64_t k = edges[e].key1;
                if (c1[e].n == 0 || c2[e].n == 0 || grid_of.count(k)) continue;
                const NnGrid* g = nullptr;
                for (auto& c : s->grids)
                    if (c->key == k) { g = &c->grid; c->tick = ++s->tick; }
                grid_of[k] = g;
                if (!g) { set_keys.push_back(k); set_p.push_back(c1[e].p); set_n.push_back(c1[e].n); }
            }
            bool build = false;
            for (uint64_t k : set_keys) build = build || std::find(s->edge_keys.begin(), s->edge_keys.end(), k) == s->edge_keys.end();
            if (build) {
                s->edge_keys.clear();  // (a failed build leaves no view behind)
                s->edge_views.clear();
                s->edge_views.resize(set_keys.size());
                std::vector<NnGrid*> out(set_keys.size());
                for (size_t m = 0; m < out.size(); ++m) out[m] = &s->edge_views[m];
                MRGFE_TRY(s->edge_set.build(s->ctx, set_p.data(), set_n.data(), static_cast<int>(set_keys.size()), 1.0f, NnGrid::kCrowding1nn, 1, out.data()));  // as mrgfe_map_store_fitness builds one
                s->edge_keys = set_keys;
            }
            for (uint64_t k : set_keys) grid_of[k] = &s->edge_views[static_cast<size_t>(std::find(s->edge_keys.begin(), s->edge_keys.end(), k) - s->edge_keys.begin())];
            std::vector<NnFitnessJob> jobs;
            std::vector<size_t>       job_edge;
            for (size_t e = 0; e < E; ++e) {
                fit[e] = DBL_MAX;  // an empty cloud on either side (NnGrid::fitness: ... or no finite point in cloud1)
                if (c1[e].n == 0 || c2[e].n == 0) continue;
                const NnGrid* g = grid_of[edges[e].key1];
                if (g->dev().n == 0) continue;
                float T[16];  // relpose.cast<float>(), row-major
                for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T[r * 4 + c] = static_cast<float>(edges[e].relpose[c * 4 + r]);
                jobs.push_back(g->make_fitness_job(c2[e].p, c2[e].n, T));
                job_edge.push_back(e);
            }
            if (!jobs.empty()) {
                std::vector<double> out(jobs.size());
                MRGFE_TRY(nn_fitness_batch(s->ctx, jobs.data(), jobs.size(), DBL_MAX, out.data()));
                for (size_t j = 0; j < jobs.size(); ++j) fit[job_edge[j]] = out[j];
            }
        }
        for (size_t e = 0; e < E; ++e) MRGFE_TRY(mrgfe_inf_matrix_from_fitness(p, fit[e], &mats[36 * e]));
        if (E) std::memcpy(inf, mats.data(), sizeof(double) * 36 * E);
        if (fitness && E) std::memcpy(fitness, fit.data(), sizeof(double) * E);
        return MRGFE_OK;
    });
}

int mrgfe_remove_points_near(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, const float* centres, int n_centres, float radius_sqr, float* kept, size_t* n_kept,
                             float* removed, size_t* n_removed)
{
    MRGFE_TRY(check_count(n, "mrgfe_remove_points_near"));
    if (!ctx || !n_kept || (n && (!xyzi || !kept)) || (n_centres > 0 && !centres) || n_centres < 0) { set_error("mrgfe_remove_points_near: bad argument"); return MRGFE_ERR_INVALID; }
    *n_kept = 0;
    if (n_removed) *n_removed = 0;
    if (n == 0) return MRGFE_OK;
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf dr, dk, din;  // (freed at the return, `din` first)
    size_t nk = 0, nr = 0;
    auto run = [&]() -> int {
        MRGFE_TRY(din.ensure(n * 16));
        MRGFE_TRY(dk.ensure(n * 16));
        if (removed) MRGFE_TRY(dr.ensure(n * 16));
        MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
        MRGFE_TRY(remove_points_near_device(ctx, din.as<float4>(), n, centres, n_centres, radius_sqr, dk.as<float4>(), &nk, removed ? dr.as<float4>() : nullptr, &nr));
        if (nk && hipMemcpyAsync(kept, dk.p, nk * 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return MRGFE_ERR_HIP;
        if (removed && nr && hipMemcpyAsync(removed, dr.p, nr * 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return MRGFE_ERR_HIP;
        return MRGFE_OK;
    };
    int rc = run();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == MRGFE_OK) rc = MRGFE_ERR_HIP;  // (also on failure: nothing is in flight when the buffers go)
    if (rc == MRGFE_ERR_HIP) set_error("mrgfe_remove_points_near: device to host copy failed");
    if (rc != MRGFE_OK) return rc;
    *n_kept = nk;
    if (n_removed) *n_removed = nr;
    return MRGFE_OK;
}

int mrgfe_deskew(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, const float ang_v[3], double scan_period, float* out)
{
    MRGFE_TRY(check_count(n, "mrgfe_deskew"));
    if (!ctx || !ang_v || (n && (!xyzi || !out))) { set_error("mrgfe_deskew: NULL argument"); return MRGFE_ERR_INVALID; }
    if (n == 0) return MRGFE_OK;
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf dout, din;  // (a fresh pair per call, freed at the return, `din` first)
    MRGFE_TRY(din.ensure(n * 16));
    MRGFE_TRY(dout.ensure(n * 16));
    MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
    MRGFE_TRY(deskew_device(ctx, din.as<float4>(), n, ang_v, scan_period, dout.as<float4>()));
    if (hipMemcpyAsync(out, dout.p, n * 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_error("mrgfe_deskew: device to host copy failed");
        return MRGFE_ERR_HIP;
    }
    return MRGFE_OK;
}

int mrgfe_transform_cloud(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, const float T[16], float* out)
{
    MRGFE_TRY(check_count(n, "mrgfe_transform_cloud"));
    if (!ctx || !T || (n && (!xyzi || !out))) { set_error("mrgfe_transform_cloud: NULL argument"); return MRGFE_ERR_INVALID; }
    if (n == 0) return MRGFE_OK;
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    float Tr[16];
    col2row(T, Tr);
    DevBuf dout, din;  // (a fresh pair per call, freed at the return, `din` first)
    MRGFE_TRY(din.ensure(n * 16));
    MRGFE_TRY(dout.ensure(n * 16));
    MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
    MRGFE_TRY(transform_cloud_device(ctx, din.as<float4>(), n, Tr, dout.as<float4>()));
    if (hipMemcpyAsync(out, dout.p, n * 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_error("mrgfe_transform_cloud: device to host copy failed");
        return MRGFE_ERR_HIP;
    }
    return MRGFE_OK;
}

int mrgfe_dbg_select_prune(int n_pairs, const double* lower, const double* upper, const int32_t* converged, const int32_t* group, int n_groups, double score_cap, int32_t* state)
{
    if (n_pairs < 0 || n_groups < 0 || (n_pairs > 0 && (!lower || !upper || !converged || !group || !state))) { set_error("mrgfe_dbg_select_prune: bad argument"); return MRGFE_ERR_INVALID; }
    if (std::isnan(score_cap)) { set_error("mrgfe_dbg_select_prune: score_cap is NaN"); return MRGFE_ERR_INVALID; }
    for (int i = 0; i < n_pairs; ++i)
        if (group[i] < -1 || group[i] >= n_groups) { set_error("mrgfe_dbg_select_prune: group[%d] = %d is not -1 or in [0, %d)", i, group[i], n_groups); return MRGFE_ERR_INVALID; }
    fit_select_prune(n_pairs, lower, upper, converged, group, n_groups, score_cap, state);
    return MRGFE_OK;
}
int mrgfe_dbg_set_prefilter_device_driven(int mode) { return prefilter_set_device_driven(mode); }
int mrgfe_dbg_set_sor_grid_rule(float start_edge, double crowding_target, int max_halvings)
{
    prefilter_set_sor_grid_rule(start_edge, crowding_target, max_halvings);
    return MRGFE_OK;
}

int mrgfe_dbg_prefilter_output(mrgfe_ctx* ctx, int* remembered, size_t* n, float box[6])
{
    if (!ctx || !remembered) { set_error("mrgfe_dbg_prefilter_output: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    *remembered = ctx->pf_out_valid ? 1 : 0;
    if (n) *n = ctx->pf_out_valid ? ctx->pf_out_n : 0;
    if (box && ctx->pf_out_valid) std::memcpy(box, ctx->pf_out_box, sizeof(ctx->pf_out_box));
    return MRGFE_OK;
}

int mrgfe_dbg_sor_threshold(mrgfe_ctx* ctx, const float* dist, const uint32_t* valid, size_t n, double stddev_mul, int on_device, double out[6])
{
    if (!out || (n && (!dist || !valid)) || (on_device && !ctx)) { set_error("mrgfe_dbg_sor_threshold: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!on_device) return sor_threshold_debug(nullptr, dist, valid, n, stddev_mul, 0, out);
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    return sor_threshold_debug(ctx, dist, valid, n, stddev_mul, 1, out);
}
int mrgfe_dbg_set_pclgicp_reference_order(int mode) { return gicp_set_pcl_reference_order(mode); }

// ---- diagnostics ----------------------------------------------------------------------------------------------
int mrgfe_dbg_sort_pairs(mrgfe_ctx* ctx, const uint32_t* keys, const uint32_t* vals, size_t n, int key_bits, uint32_t* out_keys, uint32_t* out_vals)
{
    MRGFE_TRY(check_count(n, "mrgfe_dbg_sort_pairs"));
    if (!ctx || (n && (!keys || !vals || !out_keys || !out_vals))) { set_error("mrgfe_dbg_sort_pairs: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    if (n == 0) return MRGFE_OK;
    uint32_t  nn = static_cast<uint32_t>(n);
    SliceTable tab;
    tab.build(&nn, 1);
    DevBuf &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6], &ds = ctx->scratch[0];
    MRGFE_TRY(dk.ensure(n * 4)); MRGFE_TRY(dv.ensure(n * 4)); MRGFE_TRY(dkt.ensure(n * 4)); MRGFE_TRY(dvt.ensure(n * 4));
    MRGFE_TRY(dh.ensure(sizeof(uint32_t) * 256 * (tab.total_blks + 1)));
    MRGFE_TRY(ds.ensure(sizeof(Slice)));
    MRGFE_HIP_CHECK(hipMemcpy(ds.p, tab.h.data(), sizeof(Slice), hipMemcpyHostToDevice));
    MRGFE_HIP_CHECK(hipMemcpy(dk.p, keys, n * 4, hipMemcpyHostToDevice));
    MRGFE_HIP_CHECK(hipMemcpy(dv.p, vals, n * 4, hipMemcpyHostToDevice));
    uint32_t *sk, *sv;
    MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), ds.as<Slice>(), tab, key_bits, dh.as<uint32_t>(), &sk, &sv));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MRGFE_HIP_CHECK(hipMemcpy(out_keys, sk, n * 4, hipMemcpyDeviceToHost));
    MRGFE_HIP_CHECK(hipMemcpy(out_vals, sv, n * 4, hipMemcpyDeviceToHost));
    return MRGFE_OK;
}

int mrgfe_dbg_wave_sums(mrgfe_ctx* ctx, int n_vals, const double* in, int cases, double* out_fold, double* out_plain)
{
    if (!ctx || !in || !out_fold || !out_plain || cases < 0) { set_error("mrgfe_dbg_wave_sums: bad argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    const size_t n_in = size_t(cases) * 64 * n_vals, n_out = size_t(cases) * n_vals;
    DevBuf &di = ctx->scratch[0], &df = ctx->scratch[1], &dp = ctx->scratch[2];
    MRGFE_TRY(di.ensure(std::max<size_t>(n_in, 1) * 8)); MRGFE_TRY(df.ensure(std::max<size_t>(n_out, 1) * 8)); MRGFE_TRY(dp.ensure(std::max<size_t>(n_out, 1) * 8));
    MRGFE_HIP_CHECK(hipMemcpyAsync(di.p, in, n_in * 8, hipMemcpyHostToDevice, ctx->stream));
    MRGFE_TRY(wave_fold_check_device(ctx, n_vals, di.as<double>(), cases, df.as<double>(), dp.as<double>()));
    MRGFE_HIP_CHECK(hipMemcpyAsync(out_fold, df.p, n_out * 8, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipMemcpyAsync(out_plain, dp.p, n_out * 8, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MRGFE_OK;
}

int mrgfe_dbg_exclusive_scan(mrgfe_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out, uint32_t* total)
{
    MRGFE_TRY(check_count(n, "mrgfe_dbg_exclusive_scan"));
    if (!ctx || !total || (n && (!in || !out))) { set_error("mrgfe_dbg_exclusive_scan: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    uint32_t  nn = static_cast<uint32_t>(n);
    SliceTable tab;
    tab.build(&nn, 1);
    DevBuf &di = ctx->scratch[2], &dout = ctx->scratch[3], &db = ctx->scratch[8], &ds = ctx->scratch[0];
    MRGFE_TRY(di.ensure(std::max<size_t>(n, 1) * 4)); MRGFE_TRY(dout.ensure(std::max<size_t>(n, 1) * 4));
    MRGFE_TRY(db.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    MRGFE_TRY(ds.ensure(sizeof(Slice)));
    MRGFE_HIP_CHECK(hipMemcpy(ds.p, tab.h.data(), sizeof(Slice), hipMemcpyHostToDevice));
    if (n) MRGFE_HIP_CHECK(hipMemcpy(di.p, in, n * 4, hipMemcpyHostToDevice));
    uint32_t* d_tot = db.as<uint32_t>() + tab.total_blks;
    MRGFE_TRY(exclusive_scan(ctx, di.as<uint32_t>(), dout.as<uint32_t>(), ds.as<Slice>(), tab, db.as<uint32_t>(), d_tot));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (n) MRGFE_HIP_CHECK(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    MRGFE_HIP_CHECK(hipMemcpy(total, d_tot, 4, hipMemcpyDeviceToHost));
    return MRGFE_OK;
}

int mrgfe_dbg_minmax(mrgfe_ctx* ctx, const float* xyzi, size_t n, float min3[3], float max3[3], uint32_t* n_finite)
{
    MRGFE_TRY(check_count(n, "mrgfe_dbg_minmax"));
    if (!ctx || !min3 || !max3 || !n_finite || (n && !xyzi)) { set_error("mrgfe_dbg_minmax: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    uint32_t  nn = static_cast<uint32_t>(n);
    SliceTable tab;
    tab.build(&nn, 1);
    DevBuf &dp = ctx->scratch[10], &dbb = ctx->scratch[1], &ds = ctx->scratch[0];
    MRGFE_TRY(dp.ensure(std::max<size_t>(n, 1) * 16));
    MRGFE_TRY(dbb.ensure(sizeof(BBox) * (tab.total_blks + 1)));
    MRGFE_TRY(ds.ensure(sizeof(Slice) + sizeof(void*)));
    MRGFE_TRY(upload_cloud(ctx, xyzi, n, 16, dp.p));
    const void* cp = dp.p;
    MRGFE_HIP_CHECK(hipMemcpy(ds.p, tab.h.data(), sizeof(Slice), hipMemcpyHostToDevice));
    MRGFE_HIP_CHECK(hipMemcpy(ds.as<char>() + sizeof(Slice), &cp, sizeof(void*), hipMemcpyHostToDevice));
    BBox* d_part = dbb.as<BBox>();
    BBox* d_out = d_part + tab.total_blks;
    MRGFE_TRY(bounding_boxes(ctx, reinterpret_cast<const float4* const*>(ds.as<char>() + sizeof(Slice)), ds.as<Slice>(), tab, d_part, d_out));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    BBox bb;
    MRGFE_HIP_CHECK(hipMemcpy(&bb, d_out, sizeof(BBox), hipMemcpyDeviceToHost));
    for (int a = 0; a < 3; ++a) { min3[a] = bb.mn[a]; max3[a] = bb.mx[a]; }
    *n_finite = bb.n_finite;
    return MRGFE_OK;
}

// ---- the NDT optimiser state machine stepped by hand (no GPU involved): tests/test_controller_cpu.py feeds it the CPU oracle's
// derivative evaluations and must end where the oracle's own computeTransformation ends -------------------------------------
struct mrgfe_dbg_ctl { NdtController c; };

int mrgfe_dbg_set_host_control(int mode)
{
    ndt_set_host_control(mode);
    return MRGFE_OK;
}
int mrgfe_dbg_set_fused_launch(int mode) { return ndt_set_fused_launch(mode); }
int mrgfe_dbg_set_ndt_reference_order(int mode) { return ndt_set_reference_order(mode); }
int mrgfe_dbg_set_ndt_round_shape(int wg_target, int max_ppt)
{
    if (wg_target < 0 || max_ppt < 0 || max_ppt > 64) { set_error("mrgfe_dbg_set_ndt_round_shape: wg_target >= 0, max_ppt 0..64"); return MRGFE_ERR_INVALID; }
    ndt_set_round_shape(static_cast<uint32_t>(wg_target), static_cast<uint32_t>(max_ppt));
    return MRGFE_OK;
}
int mrgfe_dbg_set_fit_sweep(int mode) { return nn_set_fit_sweep(mode); }
int mrgfe_dbg_set_fit_stats(int mode) { return nn_set_fit_stats(mode); }
void mrgfe_dbg_sincosf(const float* x, size_t n, float* sin_out, float* cos_out)
{
    for (size_t i = 0; i < n; ++i) { sin_out[i] = ctl::sin_f(x[i]); cos_out[i] = ctl::cos_f(x[i]); }
}
int mrgfe_dbg_exp(mrgfe_ctx* ctx, const double* x, size_t n, int on_device, double* out)
{
    if ((n && (!x || !out)) || (on_device && !ctx)) { set_error("mrgfe_dbg_exp: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!on_device) {
        for (size_t i = 0; i < n; ++i) out[i] = glibc_exp(x[i]);
        return MRGFE_OK;
    }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf dout, dx;  // (freed at the return, `dx` first)
    MRGFE_TRY(dx.ensure(std::max<size_t>(n, 1) * 8));
    int st = dout.ensure(std::max<size_t>(n, 1) * 8);
    if (st == MRGFE_OK && n) {
        if (hipMemcpyAsync(dx.p, x, n * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) st = MRGFE_ERR_HIP;
        if (st == MRGFE_OK) st = glibc_exp_device(ctx, dx.as<double>(), n, dout.as<double>());
        if (st == MRGFE_OK && hipMemcpyAsync(out, dout.p, n * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = MRGFE_ERR_HIP;
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == MRGFE_OK) st = MRGFE_ERR_HIP;
        if (st == MRGFE_ERR_HIP) set_error("mrgfe_dbg_exp: a HIP call failed");
    }
    return st;
}

int mrgfe_dbg_exp_float_args(mrgfe_ctx* ctx, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad, uint64_t classes[4])
{
    if (!ctx || !mismatches || !first_bad || count > (1ull << 32)) { set_error("mrgfe_dbg_exp_float_args: NULL argument or more than 2^32 patterns"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    unsigned long long h[6] = {0, ~0ull, 0, 0, 0, 0};
    DevBuf dout;  // (freed at the return)
    MRGFE_TRY(dout.ensure(sizeof(h)));
    int st = MRGFE_OK;
    if (hipMemcpyAsync(dout.p, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) st = MRGFE_ERR_HIP;
    if (st == MRGFE_OK) st = exp_float_args_device(ctx, first_bits, count, dout.as<unsigned long long>());
    if (st == MRGFE_OK && hipMemcpyAsync(h, dout.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = MRGFE_ERR_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == MRGFE_OK) st = MRGFE_ERR_HIP;
    if (st == MRGFE_ERR_HIP) set_error("mrgfe_dbg_exp_float_args: a HIP call failed");
    if (st != MRGFE_OK) return st;
    *mismatches = h[0];
    *first_bad = h[0] ? first_bits + static_cast<uint32_t>(h[1]) : 0u;
    if (classes) for (int c = 0; c < 4; ++c) classes[c] = h[2 + c];
    return MRGFE_OK;
}

int mrgfe_dbg_ctl_math(mrgfe_ctx* ctx, const double* cases48, int n, int on_device, float* M16, double* tables69, double* x6)
{
    if (!cases48 || !M16 || !tables69 || !x6 || n < 0) { set_error("mrgfe_dbg_ctl_math: bad argument"); return MRGFE_ERR_INVALID; }
    if (!on_device) {
        for (int i = 0; i < n; ++i) {
            const double* c = cases48 + size_t(i) * 48;
            ctl::pose_to_matrix(c, M16 + size_t(i) * 16);
            double j[8][3], h[15][3];
            ctl::angle_tables(c, j, h);
            std::memcpy(tables69 + size_t(i) * 69, j, sizeof(j));
            std::memcpy(tables69 + size_t(i) * 69 + 24, h, sizeof(h));
            ctl::svd_solve6(c + 6, c + 42, x6 + size_t(i) * 6);
        }
        return MRGFE_OK;
    }
    if (!ctx) { set_error("mrgfe_dbg_ctl_math: NULL context"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf &din = ctx->scratch[0], &dM = ctx->scratch[1], &dt = ctx->scratch[2], &dx = ctx->scratch[3];
    const size_t nn = std::max(n, 1);
    MRGFE_TRY(din.ensure(nn * 48 * 8)); MRGFE_TRY(dM.ensure(nn * 64)); MRGFE_TRY(dt.ensure(nn * 69 * 8)); MRGFE_TRY(dx.ensure(nn * 48));
    MRGFE_HIP_CHECK(hipMemcpyAsync(din.p, cases48, size_t(n) * 48 * 8, hipMemcpyHostToDevice, ctx->stream));
    MRGFE_TRY(ndt_ctl_math_device(ctx, din.as<double>(), n, dM.as<float>(), dt.as<double>(), dx.as<double>()));
    if (on_device == 2) MRGFE_TRY(ndt_ctl_svd_wave_device(ctx, din.as<double>(), n, dx.as<double>()));  // x from the wavefront form of the solve
    MRGFE_HIP_CHECK(hipMemcpyAsync(M16, dM.p, size_t(n) * 64, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipMemcpyAsync(tables69, dt.p, size_t(n) * 69 * 8, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipMemcpyAsync(x6, dx.p, size_t(n) * 48, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MRGFE_OK;
}
#ifdef MRGFE_TESTING
long mrgfe_dbg_fail_alloc_after(long k) { return fail_alloc_after(k); }
long mrgfe_dbg_live_allocations(void) { return live_allocations(); }
#endif


int mrgfe_dbg_ctl_create(const mrgfe_reg_params* params, const float guess[16], uint32_t n_src, mrgfe_dbg_ctl** out)
{
    if (!params || !guess || !out) { set_error("mrgfe_dbg_ctl_create: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!is_ndt(params->method)) { set_error("mrgfe_dbg_ctl_create: NDT_HIP / PCL_NDT_HIP only"); return MRGFE_ERR_INVALID; }
    MRGFE_TRY(check_params(params));
    mrgfe_dbg_ctl* h = new mrgfe_dbg_ctl();
    float g[16];
    col2row(guess, g);
    h->c.start(ndt_params_from(*params), g, n_src, std::getenv("MRGFE_DBG_CTL_SPLIT") != nullptr);
    if (ndt_set_reference_order(-1) && params->method == MRGFE_NDT_HIP) h->c.force_reference_solve();  // (as NdtEngine::align_all does in that mode)
    *out = h;
    return MRGFE_OK;
}
void mrgfe_dbg_ctl_destroy(mrgfe_dbg_ctl* h) { delete h; }
int mrgfe_dbg_ctl_request(const mrgfe_dbg_ctl* h, int* mode, float T[16], double p[6])
{
    if (!h || h->c.done()) return 0;
    const NdtCtlState& s = h->c.state();
    if (mode) *mode = s.req_mode;
    if (T) row2col(s.final_, T);
    if (p) std::memcpy(p, s.req_p, sizeof(double) * 6);
    return 1;
}
int mrgfe_dbg_ctl_result(mrgfe_dbg_ctl* h, double score, const double grad[6], const double hess[36], double neighbours)
{
    if (!h || !grad || !hess) { set_error("mrgfe_dbg_ctl_result: NULL argument"); return MRGFE_ERR_INVALID; }
    if (h->c.done()) { set_error("mrgfe_dbg_ctl_result: no request pending"); return MRGFE_ERR_STATE; }
    double r[kNdtPartialStride] = {0};
    r[0] = score;
    std::memcpy(r + 1, grad, sizeof(double) * 6);
    std::memcpy(r + 7, hess, sizeof(double) * 36);
    r[kNdtNbIndex] = neighbours;
    h->c.on_result(r);
    return MRGFE_OK;
}
int mrgfe_dbg_ctl_final(const mrgfe_dbg_ctl* h, float T[16], int* converged, int* iterations, int* evaluations)
{
    if (!h || !T) { set_error("mrgfe_dbg_ctl_final: NULL argument"); return MRGFE_ERR_INVALID; }
    row2col(h->c.final_transformation(), T);
    if (converged) *converged = h->c.converged() ? 1 : 0;
    if (iterations) *iterations = h->c.iterations();
    if (evaluations) *evaluations = h->c.evaluations();
    return MRGFE_OK;
}
int mrgfe_dbg_ctl_record(const mrgfe_dbg_ctl* h, double hessian[36], double* trans_probability)
{
    if (!h || !hessian || !trans_probability) { set_error("mrgfe_dbg_ctl_record: NULL argument"); return MRGFE_ERR_INVALID; }
    std::memcpy(hessian, h->c.hessian(), sizeof(double) * 36);
    *trans_probability = h->c.trans_probability();
    return MRGFE_OK;
}

// ---- the ICP loop stepped by hand (no GPU involved): tests/test_icp_controller_cpu.py feeds it moment sums computed in numpy -------------
struct mrgfe_dbg_icp_ctl { IcpController c; };

int mrgfe_dbg_icp_ctl_create(const mrgfe_reg_params* params, const float guess[16], uint32_t n_src, uint32_t n_tgt, mrgfe_dbg_icp_ctl** out)
{
    if (!params || !guess || !out) { set_error("mrgfe_dbg_icp_ctl_create: NULL argument"); return MRGFE_ERR_INVALID; }
    if (params->method != MRGFE_ICP_HIP) { set_error("mrgfe_dbg_icp_ctl_create: ICP_HIP only"); return MRGFE_ERR_INVALID; }
    MRGFE_TRY(check_params(params));
    mrgfe_dbg_icp_ctl* h = new (std::nothrow) mrgfe_dbg_icp_ctl();
    if (!h) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
    float g[16];
    col2row(guess, g);
    h->c.start(gicp_params_from(*params), g, n_src, n_tgt);
    *out = h;
    return MRGFE_OK;
}
void mrgfe_dbg_icp_ctl_destroy(mrgfe_dbg_icp_ctl* h) { delete h; }
int mrgfe_dbg_icp_ctl_result(mrgfe_dbg_icp_ctl* h, const double sums[17], int* done, float Tm[16])
{
    if (!h || !sums) { set_error("mrgfe_dbg_icp_ctl_result: NULL argument"); return MRGFE_ERR_INVALID; }
    if (h->c.done()) { set_error("mrgfe_dbg_icp_ctl_result: the loop has ended"); return MRGFE_ERR_STATE; }
    double r[32] = {0};
    std::memcpy(r, sums, sizeof(double) * 17);
    h->c.on_result(r);
    if (done) *done = h->c.done() ? 1 : 0;
    if (Tm) row2col(h->c.step(), Tm);
    return MRGFE_OK;
}
int mrgfe_dbg_icp_ctl_final(const mrgfe_dbg_icp_ctl* h, float T[16], int* converged, int* iterations, int* evaluations)
{
    if (!h || !T) { set_error("mrgfe_dbg_icp_ctl_final: NULL argument"); return MRGFE_ERR_INVALID; }
    row2col(h->c.final_transformation(), T);
    if (converged) *converged = h->c.converged() ? 1 : 0;
    if (iterations) *iterations = h->c.iterations();
    if (evaluations) *evaluations = h->c.evaluations();
    return MRGFE_OK;
}

// ---- floor detection (floor.hip) ---------------------------------------------------------------------------------------------------------------
void mrgfe_floor_default_params(mrgfe_floor_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->tilt_deg = 0.0;                  // apps/floor_detection_component.cpp:55, config/mrg_slam.yaml:116
    p->sensor_height = 2.0;             // :56, yaml :117
    p->height_clip_range = 1.0;         // :57, yaml :118
    p->floor_pts_thresh = 512;          // :59, yaml :119
    p->floor_normal_thresh_deg = 10.0;  // :60, yaml :120
    p->use_normal_filtering = 1;        // enable_normal_filtering :61, yaml :121
    p->normal_filter_thresh_deg = 20.0; // :62, yaml :122
}
static int floor_check(const mrgfe_floor_params* p, const char* fn)
{
    if (!std::isfinite(p->tilt_deg) || !std::isfinite(p->sensor_height) || !std::isfinite(p->height_clip_range) || !std::isfinite(p->floor_normal_thresh_deg) ||
        !std::isfinite(p->normal_filter_thresh_deg)) {
        set_error("%s: non-finite parameter", fn);
        return MRGFE_ERR_INVALID;
    }
    return MRGFE_OK;
}
int mrgfe_floor_detect(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const float* xyzi, size_t n, size_t stride, mrgfe_floor_result* res, float* out_filtered,
                       float* out_inliers)
{
    return abi_guard("mrgfe_floor_detect", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_floor_detect"));
        if (!ctx || !p || !res || (n && !xyzi)) { set_error("mrgfe_floor_detect: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_TRY(floor_check(p, "mrgfe_floor_detect"));
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        DevBuf& din = ctx->fl_buf[10];
        MRGFE_TRY(din.ensure(std::max<size_t>(n, 1) * 16));
        if (n) MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
        return floor_detect(ctx, p, din.as<float4>(), n, res, out_filtered, out_inliers);
    });
}
int mrgfe_floor_detect_device(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const void* d_xyzi, size_t n, mrgfe_floor_result* res, float* out_filtered,
                              float* out_inliers)
{
    return abi_guard("mrgfe_floor_detect_device", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_floor_detect_device"));
        if (!ctx || !p || !res || (n && !d_xyzi)) { set_error("mrgfe_floor_detect_device: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_TRY(floor_check(p, "mrgfe_floor_detect_device"));
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        return floor_detect(ctx, p, static_cast<const float4*>(d_xyzi), n, res, out_filtered, out_inliers);
    });
}
int mrgfe_floor_callback(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const mrgfe_keyframe_params* lay, const void* data, size_t data_bytes, mrgfe_floor_result* res,
                         float* out_filtered, float* out_inliers)
{
    static const char* fn = "mrgfe_floor_callback";
    return abi_guard(fn, [&]() -> int {
        if (!p || !lay || !res) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        MRGFE_TRY(floor_check(p, fn));
        // (the message is judged before the context is asked for: without one, by the strict rules)
        KeyframeLayout l{lay->width, lay->height, lay->point_step, lay->row_step, lay->off_x, lay->off_y, lay->off_z, lay->off_intensity};
        MRGFE_TRY(check_pointcloud2_layout(ctx, fn, l.width, l.height, l.point_step, &l.row_step, l.off_x, l.off_y, l.off_z, l.off_intensity));
        const size_t n = size_t(l.width) * l.height;
        const size_t raw_bytes = n ? size_t(l.height - 1) * l.row_step + size_t(l.width) * l.point_step : 0;
        if (n && !data) { set_error("%s: NULL data", fn); return MRGFE_ERR_INVALID; }
        if (data_bytes < raw_bytes) { set_error("%s: the payload has %zu bytes, the layout needs %zu", fn, data_bytes, raw_bytes); return MRGFE_ERR_INVALID; }
        if (!ctx) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        return floor_callback(ctx, p, l, data, raw_bytes, res, out_filtered, out_inliers);  // (an empty message: EMPTY_INPUT before any upload or launch, :74-77)
    });
}

// ---- the ground fill of the first keyframe (ground_fill.hip; GraphDatabase::flush_keyframe_queue :114-129) ---------------------------------------
static_assert(sizeof(mrgfe_ground_fill_params) == 24, "mrgfe_ground_fill_params: the layout the bindings mirror");
static_assert(sizeof(mrgfe_ground_fill_result) == 40, "mrgfe_ground_fill_result: the layout the bindings mirror");
size_t mrgfe_ground_fill_params_size(void) { return sizeof(mrgfe_ground_fill_params); }
size_t mrgfe_ground_fill_result_size(void) { return sizeof(mrgfe_ground_fill_result); }
void mrgfe_ground_fill_default_params(mrgfe_ground_fill_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->radius = 5.0;            // apps/mrg_slam_component.cpp:271
    p->map_resolution = 0.05;   // :245
    p->simple = 0;              // :272
}
int mrgfe_ground_fill_counts(const mrgfe_ground_fill_params* p, uint32_t* n_rings, uint32_t* n_angles)
{
    static const char* fn = "mrgfe_ground_fill_counts";
    if (!p || !n_rings || !n_angles) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
    MRGFE_TRY(ground_fill_check(p, fn));
    return ground_fill_counts(p, 0, n_rings, n_angles, fn);
}
// What both entry points check before they touch a context: the parameters, the estimate of the simple variant, the counts behind `n` points.
static int ground_fill_begin(const char* fn, const mrgfe_ground_fill_params* p, const double* estimate, mrgfe_ground_fill_result* res)
{
    if (!p || !res) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
    std::memset(res, 0, sizeof(*res));
    MRGFE_TRY(ground_fill_check(p, fn));
    if (p->simple && !estimate) { set_error("%s: the simple variant needs the keyframe's estimate", fn); return MRGFE_ERR_INVALID; }
    return MRGFE_OK;
}
// The plane (fill_ground_plane.cpp:21-47) of the n points at d_cloud and, when there is one, the disc queued behind them (room for n + rings * angles
// points).  res->n_before / n_rings / n_angles are set by the caller; has_model, coeffs, ransac_iterations and n_added here.
static int ground_fill_plane_and_disc(mrgfe_ctx* ctx, const mrgfe_ground_fill_params* p, const double* estimate, float4* d_cloud, uint32_t n, mrgfe_ground_fill_result* res)
{
    double normal[3], offset = 0.0;
    if (p->simple) {  // base_link_pose.rotation() * (0, 0, 1): the third column; Hyperplane(normal, 0)
        for (int j = 0; j < 3; ++j) normal[j] = estimate[8 + j];
        res->has_model = 1;
        for (int j = 0; j < 3; ++j) res->coeffs[j] = static_cast<float>(normal[j]);
    } else {
        FloorRansacOut r;
        MRGFE_TRY(floor_ransac_device(ctx, d_cloud, n, 0.01, nullptr, &r));  // setDistanceThreshold(.01), computeModel() (:26-27)
        res->ransac_iterations = r.iterations;
        res->has_model = r.has_model;
        if (!r.has_model) return MRGFE_OK;
        for (int j = 0; j < 4; ++j) res->coeffs[j] = r.coeffs[j];
        for (int j = 0; j < 3; ++j) normal[j] = static_cast<double>(r.coeffs[j]);  // :31
        offset = static_cast<double>(r.coeffs[3]);                                 // :32
    }
    MRGFE_TRY(ground_fill_device(ctx, p, normal, offset, res->n_rings, res->n_angles, d_cloud + n));
    res->n_added = res->n_rings * res->n_angles;
    return MRGFE_OK;
}
int mrgfe_fill_ground_plane(mrgfe_ctx* ctx, const mrgfe_ground_fill_params* p, const double estimate[16], const float* xyzi, size_t n, size_t stride, float* out,
                            size_t capacity, mrgfe_ground_fill_result* res)
{
    static const char* fn = "mrgfe_fill_ground_plane";
    return abi_guard(fn, [&]() -> int {
        MRGFE_TRY(ground_fill_begin(fn, p, estimate, res));
        MRGFE_TRY(check_count(n, fn));
        if (!ctx || !out || (n && !xyzi)) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        MRGFE_TRY(ground_fill_counts(p, n, &res->n_rings, &res->n_angles, fn));
        res->n_before = static_cast<uint32_t>(n);
        const size_t total = n + size_t(res->n_rings) * res->n_angles;
        if (capacity < total) { set_error("%s: the filled cloud has %zu points, out_xyzi has room for %zu", fn, total, capacity); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(ctx);
        MRGFE_TRY(ctx->bind());
        DevBuf& dc = ctx->gf_cloud;
        MRGFE_TRY(dc.ensure(std::max<size_t>(total, 1) * 16));
        if (n) MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, dc.p));
        MRGFE_TRY(ground_fill_plane_and_disc(ctx, p, estimate, dc.as<float4>(), res->n_before, res));
        if (!res->has_model) return MRGFE_OK;  // (RANSAC's last wave was waited for: the stream is idle)
        const size_t filled = n + res->n_added;
        if (filled) MRGFE_HIP_CHECK(hipMemcpyAsync(out, dc.p, filled * 16, hipMemcpyDeviceToHost, ctx->stream));
        MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the one wait of the fill
        return MRGFE_OK;
    });
}
int mrgfe_map_store_fill_ground(mrgfe_map_store* s, uint64_t src_key, uint64_t dst_key, const mrgfe_ground_fill_params* p, const double estimate[16], float* out,
                                size_t capacity, mrgfe_ground_fill_result* res)
{
    static const char* fn = "mrgfe_map_store_fill_ground";
    return abi_guard(fn, [&]() -> int {
        MRGFE_TRY(ground_fill_begin(fn, p, estimate, res));
        if (!s) { set_error("%s: NULL store", fn); return MRGFE_ERR_INVALID; }
        if (src_key == 0 || dst_key == 0) { set_error("%s: key 0", fn); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(s->ctx);
        MRGFE_TRY(s->ctx->bind());
        mrgfe_ctx* ctx = s->ctx;
        auto it = s->clouds.find(src_key);
        if (it == s->clouds.end()) { set_error("%s: keyframe %llu is not in the store", fn, static_cast<unsigned long long>(src_key)); return MRGFE_ERR_INVALID; }
        const mrgfe_map_store::Entry src = it->second;
        MRGFE_TRY(ground_fill_counts(p, src.n, &res->n_rings, &res->n_angles, fn));
        res->n_before = src.n;
        const size_t total = size_t(src.n) + size_t(res->n_rings) * res->n_angles;
        if (out && capacity < total) { set_error("%s: the filled cloud has %zu points, out_xyzi has room for %zu", fn, total, capacity); return MRGFE_ERR_INVALID; }
        if (dst_key == src_key || s->clouds.count(dst_key)) {
            set_error("%s: keyframe %llu is already stored (the store is append-only: the filled cloud needs a key of its own)", fn, static_cast<unsigned long long>(dst_key));
            return MRGFE_ERR_STATE;
        }
        s->clouds.reserve(s->clouds.size() + 1);
        void* blk = nullptr;
        if (total) MRGFE_TRY(s->arena.alloc(total * 16, &blk));
        auto run = [&]() -> int {
            // the source points: device to device on the store's stream, behind whatever upload of src_key is still on its way
            if (src.n) MRGFE_HIP_CHECK(hipMemcpyAsync(blk, src.p, size_t(src.n) * 16, hipMemcpyDeviceToDevice, ctx->stream));
            MRGFE_TRY(ground_fill_plane_and_disc(ctx, p, estimate, static_cast<float4*>(blk), src.n, res));  // (RANSAC reads the copy: the same bytes)
            if (!res->has_model) return MRGFE_OK;
            if (out && total) MRGFE_HIP_CHECK(hipMemcpyAsync(out, blk, total * 16, hipMemcpyDeviceToHost, ctx->stream));
            MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the one wait of the fill: the new cloud is complete
            return MRGFE_OK;
        };
        const int rc = run();
        if (rc != MRGFE_OK || !res->has_model) {
            (void)hipStreamSynchronize(ctx->stream);  // nothing is in flight when the block goes back
            if (total) s->arena.shrink_last(blk, total * 16, 0);
            return rc;
        }
        s->clouds[dst_key] = {static_cast<const float4*>(blk), static_cast<uint32_t>(total)};
        s->bytes += total * 16;
        return MRGFE_OK;
    });
}
int mrgfe_dbg_floor_ransac(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double threshold, int* has_model, float coeffs[4], int32_t* inliers,
                           size_t* n_inliers, int32_t* iterations, int32_t* skipped)
{
    MRGFE_TRY(check_count(n, "mrgfe_dbg_floor_ransac"));
    if (!ctx || !has_model || !coeffs || !n_inliers || !iterations || !skipped || (n && (!xyzi || !inliers))) {
        set_error("mrgfe_dbg_floor_ransac: NULL argument");
        return MRGFE_ERR_INVALID;
    }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    DevBuf &din = ctx->fl_buf[10], &dfl = ctx->fl_buf[1];
    MRGFE_TRY(din.ensure(std::max<size_t>(n, 1) * 16));
    MRGFE_TRY(dfl.ensure(std::max<size_t>(n, 1) * 4));
    if (n) MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
    FloorRansacOut r;
    MRGFE_TRY(floor_ransac_device(ctx, din.as<float4>(), static_cast<uint32_t>(n), threshold, dfl.as<uint32_t>(), &r));
    *has_model = r.has_model;
    for (int j = 0; j < 4; ++j) coeffs[j] = r.coeffs[j];
    *iterations = r.iterations;
    *skipped = r.skipped;
    *n_inliers = 0;
    if (r.has_model && n) {
        std::vector<uint32_t> fl(n);
        MRGFE_HIP_CHECK(hipMemcpyAsync(fl.data(), dfl.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        size_t m = 0;
        for (size_t i = 0; i < n; ++i)
            if (fl[i]) inliers[m++] = static_cast<int32_t>(i);
        *n_inliers = m;
    }
    return MRGFE_OK;
}
int mrgfe_dbg_floor_normals(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double normal_filter_thresh_deg, float* normals_xyz, uint8_t* keep)
{
    MRGFE_TRY(check_count(n, "mrgfe_dbg_floor_normals"));
    if (!ctx || (n && (!xyzi || !normals_xyz || !keep))) { set_error("mrgfe_dbg_floor_normals: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    if (n == 0) return MRGFE_OK;
    DevBuf &din = ctx->fl_buf[10], &dfl = ctx->fl_buf[1], &dnr = ctx->fl_buf[0];
    MRGFE_TRY(din.ensure(n * 16));
    MRGFE_TRY(dfl.ensure(n * 4));
    MRGFE_TRY(dnr.ensure(n * 16));
    MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
    MRGFE_TRY(floor_normals_device(ctx, din.as<float4>(), static_cast<uint32_t>(n), normal_filter_thresh_deg, dnr.as<float4>(), dfl.as<uint32_t>()));
    std::vector<float>    nr(n * 4);
    std::vector<uint32_t> fl(n);
    MRGFE_HIP_CHECK(hipMemcpyAsync(nr.data(), dnr.p, n * 16, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipMemcpyAsync(fl.data(), dfl.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) {
        for (int j = 0; j < 3; ++j) normals_xyz[i * 3 + j] = nr[i * 4 + j];
        keep[i] = fl[i] ? 1 : 0;
    }
    return MRGFE_OK;
}
int mrgfe_dbg_floor_stats(mrgfe_ctx* ctx, double out[8])
{
    if (!ctx || !out) { set_error("mrgfe_dbg_floor_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(ctx);
    for (int j = 0; j < 8; ++j) out[j] = ctx->fl_stats[j];
    return MRGFE_OK;
}

}  // extern "C"
