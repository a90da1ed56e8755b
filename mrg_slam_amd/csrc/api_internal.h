// csrc/api_internal.h — what the two files of the extern "C" surface (api.cpp, batch.cpp) share: the matrix layout conversion, the argument and parameter
// checks, the engines' parameters made from mrgfe_reg_params, and the map store a batch may read its clouds from.
#pragma once
#include <algorithm>
#include <memory>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "gicp_engine.h"
#include "mapcloud.h"
#include "ndt_engine.h"
#include "nn_grid.h"

namespace mrgfe {

inline void col2row(const float in[16], float out[16]) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[r * 4 + c] = in[c * 4 + r]; }
inline void row2col(const float in[16], float out[16]) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out[c * 4 + r] = in[r * 4 + c]; }

// point counts the library accepts: the kernels index points with 32-bit words (and a count beyond 2^31 is a caller's bug, not a cloud)
constexpr size_t kMaxPoints = 0x7fffffffu;
inline int check_count(size_t n, const char* fn)
{
    if (n > kMaxPoints) { set_error("%s: %zu points: more than 2^31 - 1", fn, n); return MRGFE_ERR_INVALID; }
    return MRGFE_OK;
}

inline bool is_ndt(int method) { return method == MRGFE_NDT_HIP || method == MRGFE_PCL_NDT_HIP; }
inline bool is_pcl_gicp(int method) { return method == MRGFE_PCL_GICP_HIP || method == MRGFE_PCL_GICP_OMP_HIP; }

inline NdtParams ndt_params_from(const mrgfe_reg_params& p)
{
    NdtParams n;
    n.resolution = static_cast<float>(p.resolution);
    n.step_size = p.step_size;
    n.outlier_ratio = p.outlier_ratio;
    n.trans_eps = p.transformation_epsilon;
    n.max_iterations = p.maximum_iterations;
    n.search = p.nn_search_method;
    if (p.method == MRGFE_PCL_NDT_HIP) {  // pcl::NormalDistributionsTransform has one neighbourhood: target_cells_.radiusSearch(point, resolution_)
        n.formulation = 1;
        n.search = MRGFE_KDTREE;
    }
    return n;
}
inline GicpParams gicp_params_from(const mrgfe_reg_params& p)
{
    GicpParams g;
    g.k_correspondences = p.correspondence_randomness;
    g.max_corr_dist = p.max_correspondence_distance;
    g.trans_eps = p.transformation_epsilon;
    g.rot_eps = p.rotation_epsilon;
    g.max_iterations = p.maximum_iterations;
    g.variant = p.method == MRGFE_SMALL_GICP_HIP ? 1 : p.method == MRGFE_VGICP_HIP ? 2 : p.method == MRGFE_ICP_HIP ? 3 : (p.method == MRGFE_PCL_GICP_HIP || p.method == MRGFE_PCL_GICP_OMP_HIP) ? 4 : 0;
    g.max_inner_iterations = p.max_optimizer_iterations;
    g.pcl_whole_gradient_norm = p.method == MRGFE_PCL_GICP_OMP_HIP;
    // pclomp::GICP never sees reg_num_threads (registrations.cpp:104-114 does not call setNumThreads): its sums are those of omp_get_max_threads() threads
    // of the reference's host.  Here: num_threads of the params when given, 8 (the YAML's reg_num_threads) otherwise; 2..16 chains (check_params refuses more).
    // ONE thread is the serial chain over the correspondences (one partial, 0 + p_0 = p_0): pcl::GICP's order (it used to fall through to the tree)
    const int omp_threads = p.method == MRGFE_PCL_GICP_OMP_HIP ? (p.num_threads > 0 ? p.num_threads : 8) : 0;
    g.pcl_reference_order_sums = p.method == MRGFE_PCL_GICP_HIP || omp_threads == 1;
    g.pcl_omp_sum_threads = omp_threads > 1 ? std::min(16, omp_threads) : 0;
    g.use_reciprocal = p.method == MRGFE_ICP_HIP && p.use_reciprocal_correspondences != 0;
    g.voxel_resolution = p.resolution;
    return g;
}

inline int check_params(const mrgfe_reg_params* p)
{
    if (!p) { set_error("NULL params"); return MRGFE_ERR_INVALID; }
    if (p->method == MRGFE_PCL_GICP_OMP_HIP && p->num_threads > 16) {
        set_error("PCL_GICP_OMP_HIP adds its cost terms as num_threads OpenMP threads would (static chunks, partials in thread order): 1..16 threads are supported, got %d", p->num_threads);
        return MRGFE_ERR_INVALID;
    }
    if (p->method < MRGFE_NDT_HIP || p->method > MRGFE_PCL_NDT_HIP) { set_error("unknown registration method %d", p->method); return MRGFE_ERR_INVALID; }
    if ((p->method == MRGFE_PCL_GICP_HIP || p->method == MRGFE_PCL_GICP_OMP_HIP) && p->max_optimizer_iterations < 1) { set_error("max_optimizer_iterations must be >= 1"); return MRGFE_ERR_INVALID; }
    if (is_ndt(p->method)) {
        if (!(p->resolution > 0)) { set_error("resolution must be > 0"); return MRGFE_ERR_INVALID; }
        if (p->method == MRGFE_NDT_HIP && (p->nn_search_method < 0 || p->nn_search_method > 3)) { set_error("unknown nn_search_method %d", p->nn_search_method); return MRGFE_ERR_INVALID; }
    } else {
        if (p->method != MRGFE_ICP_HIP && (p->correspondence_randomness < 4 || p->correspondence_randomness > 256)) { set_error("correspondence_randomness must be in [4, 256]"); return MRGFE_ERR_INVALID; }
        if (p->method == MRGFE_VGICP_HIP && !(p->resolution > 0)) { set_error("resolution must be > 0"); return MRGFE_ERR_INVALID; }
    }
    return MRGFE_OK;
}

// GICP_HIP, SMALL_GICP_HIP, VGICP_HIP and the two PCL GICPs (PCL's form of them) keep the k-NN covariances of a stored keyframe (48 bytes per point) with
// it; NDT and ICP_HIP need the cloud alone
inline bool keeps_covariances(const mrgfe_reg_params& p) { return !is_ndt(p.method) && p.method != MRGFE_ICP_HIP; }

}  // namespace mrgfe

// one registration (api.cpp; the one-call odometry frame of odometry.cpp hands it its clouds): the engine, the clouds it owns or borrows, the last result
struct mrgfe_reg {
    explicit mrgfe_reg(mrgfe_ctx* c) : ctx(c), book(c) {}
    mrgfe_ctx*       ctx;
    mrgfe_reg_params params;
    mrgfe::PairBook  book;                // NDT: the target and the one pair (declared before the engine that reads it, so destroyed after it)
    std::unique_ptr<mrgfe::NdtEngine>  ndt;
    std::unique_ptr<mrgfe::GicpEngine> gicp;
    mrgfe::DevBuf    tgt, src;            // owned copies of host-supplied clouds
    const void*      d_tgt = nullptr;     // current clouds (owned buffer or caller's device memory)
    const void*      d_src = nullptr;
    size_t           n_tgt = 0, n_src = 0;
    bool             has_target = false, has_source = false, aligned_once = false;
    int              target_status = MRGFE_ERR_STATE;
    mrgfe::NnGrid    nn;                  // exact 1-NN structure over the target (getFitnessScore / nearestKSearch)
    bool             nn_valid = false;
    float            final_rm[16];        // row-major
    bool             converged = false;
    int              iterations = 0, evaluations = 0;
    double           trans_probability = 0;
    double           hessian[36];
    double           mean_neighbours = 0;
};

// mrgfe_batch_align_best in two stages (batch.cpp), for a caller that takes the selection between them over more pairs than this batch holds (a node:
// node.cpp).  Arguments are not checked here (max_range >= 0; group: n_pairs entries of -1 or a group id).
//   batch_align_bounds: the align, the records, the fitness grids and jobs, and the bound stage of the selection.  results[i]: the record with
//     fitness DBL_MAX; lo[i] / hi[i]: the pair's certified interval (0 / +inf: none; DBL_MAX / DBL_MAX: no job — an empty cloud, or grouped and not
//     converged).  On success the selection stays PENDING in the batch: until batch_align_finish or batch_align_abandon nothing else may run on the
//     batch's context (FitSelectRun, nn_grid.h).  On failure nothing is pending and the caller's clouds have been given back.
//   batch_align_finish: state[i] per pair (enum mrgfe_fit_state, as fit_select_prune decides) -> the contender passes; fills results[i].fitness
//     (exact, the lower bound, or DBL_MAX), mrgfe_batch_select_stats and mrgfe_batch_timing.  MRGFE_ERR_STATE when nothing is pending.
//   batch_align_abandon: waits for the batch's stream and side stream and drops the pending selection: no kernel of the call is in flight and no
//     caller buffer is read any more when it returns.
int batch_align_bounds(mrgfe_batch* b, double max_range, const int32_t* group, mrgfe_pair_result* results, double* lo, double* hi);
int batch_align_finish(mrgfe_batch* b, const int32_t* state, mrgfe_pair_result* results);
int batch_align_abandon(mrgfe_batch* b);
// A pair whose source is keyframe `key` held as a packed device cloud on the batch's device that is NOT the map store's memory (a node member's replica,
// node.cpp): entered exactly as mrgfe_batch_add_pair_from_store enters a store keyframe — for the GICP family the covariances are cached under `key`,
// ICP_HIP and the NDTs cache nothing.  The cloud must stay valid as caller device memory does.  Returns the pair index or an error (< 0).
int batch_add_pair_device_keyed(mrgfe_batch* b, int target, uint64_t key, const void* d_xyzi, size_t n, const float guess[16]);
// Keyframe `key` of a map store, on whatever device it is: its packed cloud, complete (the store's stream has been waited for).  Takes the store's lock alone.
int map_store_lookup(const char* fn, struct mrgfe_map_store* s, uint64_t key, const float4** p, size_t* n);

// map store: keyframe clouds resident in HBM (include/mrgfe.h); its entry points are in api.cpp, a batch takes targets and pairs out of it
struct mrgfe_map_store {
    mrgfe_ctx* ctx = nullptr;
    mrgfe::Arena arena;  // append-only
    struct Entry { const float4* p; uint32_t n; };
    std::unordered_map<uint64_t, Entry> clouds;
    size_t bytes = 0;
    // exact-NN grids of the keyframes that were `cloud1` of a fitness score lately (graph edges of one keyframe come in bursts:
    // its odometry edge, then the loop edges of the same optimisation cycle), least recently used first out
    struct CachedGrid { uint64_t key = 0; uint64_t tick = 0; mrgfe::NnGrid grid; };
    std::vector<std::unique_ptr<CachedGrid>> grids;
    uint64_t tick = 0;
    size_t   max_grids = 8;
    // mrgfe_map_store_edges: the grids its last grouped build made (views into the set's buffers, valid until the set is built again) and their keys
    mrgfe::NnGridSet           edge_set;
    std::vector<mrgfe::NnGrid> edge_views;
    std::vector<uint64_t>      edge_keys;
    // mrgfe_map_store_publish / _read: the working buffers and the records of the last call (grow-only; freed with the store, under its context bound)
    mrgfe::MapEgressWorkspace egress;
    mrgfe::EgressStats        egress_stats;  // of the last publish / read
};
