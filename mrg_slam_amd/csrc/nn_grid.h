// csrc/nn_grid.h — exact nearest-neighbour queries on a radix-sorted uniform grid: the MI355X stand-in for the
// pcl::search::KdTree / FLANN exact searches on the hot path
//   pcl::Registration::getFitnessScore        (/root/reference/src/mrg_slam/loop_detector.cpp:137)
//   InformationMatrixCalculator::calc_fitness_score (src/mrg_slam/information_matrix_calculator.cpp:46-81)
//   getSearchMethodTarget()->nearestKSearch   (apps/scan_matching_odometry_component.cpp:405-417)
//   RadiusOutlierRemoval / StatisticalOutlierRemoval (apps/prefiltering_component.cpp:182-204)
//   fast_gicp kNN covariances and 1-NN correspondences (src/mrg_slam/registrations.cpp:55-63)
// Points are sorted by cell (stable radix sort, so ascending index inside a cell); cell rows along x are contiguous,
// so a query walks a few contiguous ranges per ring.  Ties at equal distance resolve to the lowest index.
#pragma once
#include <new>
#include <utility>
#include <vector>

#include "cellsort.h"
#include "common.h"

namespace mrgfe {

struct NnGridDev {  // one resolution level
    float           origin[3];
    float           cell;
    float           slack;       // absolute bound on the binning error of floorf((p - origin) / cell) * cell, metres
    int32_t         dim[3];
    uint32_t        n;           // points in `sorted`
    int32_t         bdim[3];     // bricks of 4 x 4 x 4 cells per axis
    const uint32_t* cell_start;  // dim product + 1
    const float4*   sorted;      // xyz + original index (bit pattern) in w
    // occupancy: one 64-bit word per brick, bit x + 4 y + 16 z (cell offsets inside the brick) set iff the cell holds a
    // point.  A query whose 3x3x3 block is empty finds the occupied cells around it from a few of these words instead
    // of probing cell_start row by row.
    const unsigned long long* occ;
    const unsigned long long* occ1;  // per super-brick (4^3 bricks): which bricks are occupied
    const unsigned long long* occ2;  // per block (4^3 super-bricks)
};

// Up to three levels over the same points (cell edge x kLevelRatio per level).  k-NN queries whose neighbourhood is
// sparse at the finest scale climb to the coarser ones (nn_knn_kernel); 1-NN queries stay on the finest level and reach
// far neighbours through its occupancy pyramid (nn_device.h), so grids that only serve 1-NN are built with one level.
constexpr int kNnMaxLevels = 3;
struct NnGrid2Dev {
    NnGridDev level[kNnMaxLevels];
    int32_t   n_levels;  // >= 1
    int32_t   pad;
};

// one getFitnessScore evaluation: source cloud `src` (device) moved by the row-major 3x4 float transform, matched
// against `grid`
struct NnFitnessJob {
    NnGrid2Dev    grid;
    const float4* src;
    uint32_t      n;
    uint32_t      gicp_order;  // how T12 is applied: 0 pcl::transformPointCloud's order (getFitnessScore), 1 fast_gicp's trans_f * Vector4f (correspondence search)
    float         T12[12];
    int32_t*      idx_out;     // nn_nearest_batch: the index of the nearest target point per query (-1: none within the range); null in fitness jobs
};

class NnGrid {
   public:
    NnGrid() = default;
    NnGrid(NnGrid&&) noexcept = default;  // (containers of grids grow; an event moved away leaves nothing to wait for)
    NnGrid& operator=(NnGrid&& o) noexcept { if (this != &o) { this->~NnGrid(); new (this) NnGrid(std::move(o)); } return *this; }  // waits like the destructor
    ~NnGrid() { settle_crowding(); }      // the buffers and the event free themselves
    // (re)build over a packed float4 device cloud. `cell_size` is the largest cell edge; with `crowding_target` > 0 the
    // edge is halved (at most four times) while the population of the cell an average point sits in exceeds the target,
    // so a walk over the 27 cells around a query touches tens, not thousands, of candidates on dense clouds.
    static constexpr double kCrowding1nn = 12.0;  // lane-group 1-NN / radius walks: short cell runs
    static constexpr double kCrowdingKnn = 32.0;  // wave-per-query k-NN: cell rows of about one wavefront
    static constexpr float  kLevelRatio = 4.0f;
    // known_box (min xyz, max xyz): a box the caller KNOWS to enclose the cloud, all of whose points are finite — the bounding-box pass and its stream wait are
    // skipped (search results do not depend on the box, only on its enclosing the points)
    int build(mrgfe_ctx* ctx, const float4* d_pts, size_t n, float cell_size, double crowding_target = kCrowding1nn, int max_levels = kNnMaxLevels, const float* known_box = nullptr);
    void release();  // free the device arrays now (adopt); the cell-edge hints stay
    bool valid() const { return built_; }
    const NnGridDev&  dev() const { return h_.level[0]; }  // radius queries walk the finest level only
    const NnGrid2Dev& dev2() const { return h_; }
    size_t size() const { return n_; }

    // mean squared 1-NN distance of T*src over points whose squared distance <= max_range (PCL getFitnessScore)
    int fitness(mrgfe_ctx* ctx, const float4* d_src, size_t n_src, const float T_rowmajor[16], double max_range, double* out);
    NnFitnessJob make_fitness_job(const float4* d_src, size_t n_src, const float T_rowmajor[16]) const;
    // 1-NN of host queries
    int nearest_host(mrgfe_ctx* ctx, const float* q, size_t n, size_t stride, int32_t* idx, float* sqd);
    // 1-NN of device queries, optionally transformed by a row-major 3x4 float matrix in device memory (may be null)
    int nearest_device(mrgfe_ctx* ctx, const float4* d_q, size_t n, const float* d_T12, int32_t* d_idx, float* d_sqd);
    // flags[i] = 1 iff #{j : sqdist(q_i, p_j) <= r2} >= need   (queries are the device cloud d_q)
    int radius_count_flags(mrgfe_ctx* ctx, const float4* d_q, size_t n, double r2, int need, uint32_t* d_flags);
    // k nearest neighbours (ascending by (sqdist, index)) of every query: d_idx / d_sqd are [n][k]; missing -> -1.  1 <= k <= 256: up to 64 on one
    // list entry per lane, 65..256 on two to four (the wide kernel)
    int knn_device(mrgfe_ctx* ctx, const float4* d_q, size_t n, int k, int32_t* d_idx, float* d_sqd);
    // become a view of a grid whose device arrays another object owns (NnGridSet); release() then only forgets it
    void adopt(const NnGrid2Dev& h, size_t n) { release(); h_ = h; n_ = n; built_ = true; }

   private:
    bool      built_ = false;
    size_t    n_ = 0;
    float     hint_cell_ = 0, hint_cell_size_ = 0;  // the finest edge the adaptive passes chose last time, for which (cell_size, crowding target)
    double    hint_target_ = 0;
    NnGrid2Dev h_;
    DevBuf     d_cell_start_[kNnMaxLevels], d_sorted_[kNnMaxLevels];
    // the crowding of a build on the hinted edge is read back WITHOUT a wait and looked at by the next build of this object (below its own first wait):
    // search results do not depend on the edge, only the time does, so a cloud that has outgrown the hint costs one slower search, not a stream wait per build
    PinBuf      crowd_box_;
    bool        crowd_pending_ = false;
    Event       crowd_event_;
    uint32_t    crowd_n_finite_ = 0;
    void settle_crowding();  // the copy into crowd_box_ must have landed before the box goes
    int build_levels_together(mrgfe_ctx* ctx, const float4* d_pts, uint32_t nn, const BBox& bb, const float* cell, int n_levels, double* crowding, unsigned long long* h_slots_async = nullptr);
    int count_level(mrgfe_ctx* ctx, const float4* d_pts, uint32_t nn, const BBox& bb, float cell, DevBuf& d_cells, double* crowding);
};

// Grids over several clouds built TOGETHER: every step of the build (bounding boxes, binning, the radix sort, the scan of the cell
// counts, the occupancy pyramid, the gather) is one launch over all members instead of one per cloud, and the host waits three times
// per set instead of three times per cloud.  One grid over a 130k-point scan is ~20 launches of 5-10 us each and was bound by their
// issue, not by their work: 64 of them (the targets of a loop-closure batch) took 17 ms of wall time on four streams.
// The members' device arrays live packed in the set's buffers; `out[m]` become views (NnGrid::adopt) that stay valid until the set is
// built again or released.  Search results do not depend on how a grid was built.
class NnGridSet {
   public:
    int  build(mrgfe_ctx* ctx, const float4* const* d_clouds, const uint32_t* n, int count, float cell_size, double crowding_target, int max_levels, NnGrid* const* out);

   private:
    DevBuf d_cells_[kNnMaxLevels], d_sorted_[kNnMaxLevels];
    std::vector<float> hint_cell_;  // per member: the edge the adaptive passes settled on last time
    float  hint_cell_size_ = 0;
    double hint_target_ = 0;
};

// A single-level grid over a cloud whose SIZE THE HOST DOES NOT KNOW (round 4: the prefilter chain keeps its point counts on the device and
// waits once, at its end).  The point count comes from a Slice in device memory, the bounding box from bounding_boxes' device output; one
// single-thread kernel derives the geometry exactly as NnGrid::build_level does on the host and writes the build descriptor the *_many
// kernels read; launches are sized for `n_cap` points.  The cell table is written entry by entry from the sorted keys (nn_fill_body), so
// its capacity `cells_cap` only has to be allocated, never cleared; a cloud that needs more cells sets bit kNnAnomalyCells in *d_anomaly
// (the caller then falls back to the host-driven build).  No pyramid: the grid serves ring walks only — radius counts, and the one-level k-NN walk of
// nn_knn_mean_device_driven, which reads no occupancy words.
constexpr uint32_t kNnAnomalyCells = 1u << 8;
struct NnDeviceDrivenGrid {
    DevBuf cells, sorted, desc;  // cell table (cells_cap + 8 words), cell-major points (n_cap), the NnBuildDev record (behind it the state of nn_build_device_sized)
};
// d_n_boxes == NULL: d_bbox is the cloud's bounding box; else d_bbox is a list of *d_n_boxes partial boxes that the geometry kernel merges itself
int nn_build_device_driven(mrgfe_ctx* ctx, const float4* const* d_cloud_ptr, const Slice* d_slice, uint32_t n_cap, const BBox* d_bbox, const uint32_t* d_n_boxes, float cell,
                           uint32_t cells_cap, NnDeviceDrivenGrid& g, uint32_t* d_anomaly, BBox* h_box_out = nullptr);  // h_box_out: pinned; receives the (merged) box
// The same build with the cell EDGE chosen on the device from the cloud's own density — for a cloud no voxel grid has thinned, where the host knows no
// edge.  NnGrid::build's adaptive rule as a fixed sequence of launches, no host wait: the geometry at `start_edge` (doubled on the device, at most 8 times,
// until the box fits cells_cap cells), then `passes` (1..3) counting passes — a clear of the live part of the cell table, which doubles as the count table,
// the one-atomic-per-distinct-cell counting with its crowding sum, and a one-workgroup decision: crowding = 1 + 2 Σ before / n_finite; settled when it is
// <= crowding_target, else ceil(log4(crowding / target)) halvings, `max_halvings` in all and never beyond cells_cap cells; a pass whose grid is settled
// returns at once — and the key / sort / fill launches of nn_build_device_driven at the chosen edge.  The sums are integers: the edge is a function of
// the cloud.  Every size the kernels read from device memory is clamped there against n_cap and cells_cap; a box that fits at no allowed edge sets
// kNnAnomalyCells and builds the one-cell empty grid.  *h_status_out (pinned, may be NULL) receives what was chosen, to be read behind the caller's wait.
struct NnSizedStatus {
    float              start, edge;        // the start edge used (after the doublings), the chosen edge = start * 2^-halvings
    uint32_t           halvings, n_cells;  // n_cells: of the built grid
    unsigned long long crowd_sum;          // Σ before of the last counting pass that measured: its crowding is 1 + 2 crowd_sum / n_finite
    uint32_t           n_finite, measured; // measured: counting passes that ran (0: the start grid admitted no halving)
};
int nn_build_device_sized(mrgfe_ctx* ctx, const float4* const* d_cloud_ptr, const Slice* d_slice, uint32_t n_cap, const BBox* d_bbox, const uint32_t* d_n_boxes, float start_edge,
                          double crowding_target, int max_halvings, int passes, uint32_t cells_cap, NnDeviceDrivenGrid& g, uint32_t* d_anomaly, BBox* h_box_out = nullptr,
                          NnSizedStatus* h_status_out = nullptr);
// flags[i] = 1 iff #{j : sqdist(q_i, p_j) <= r2} >= need for the first d_slice->n points of d_q (the grid's own cloud): nn_radius_flags_kernel with
// the grid and the count read from device memory
int nn_radius_flags_device_driven(mrgfe_ctx* ctx, const NnDeviceDrivenGrid& g, const float4* d_q, const Slice* d_slice, uint32_t n_cap, double r2, int need, float cell, uint32_t* d_flags);
// StatisticalOutlierRemoval's search on such a grid (its own cloud, the first d_slice->n points of d_q): for every query the exact k1 = mean_k + 1 nearest
// (the query itself first), consumed in registers — d_dist[i] = the mean distance to the mean_k others as sor_mean_dist_kernel computes it from a
// row of NnGrid::knn_device, d_valid[i] = 1 iff all k1 were found.  One wavefront per query, launched for n_cap; 2 <= k1 <= 64; no host wait.
int nn_knn_mean_device_driven(mrgfe_ctx* ctx, const NnDeviceDrivenGrid& g, const float4* d_q, const Slice* d_slice, uint32_t n_cap, int k1, float* d_dist, uint32_t* d_valid);

// the context's reusable grid (created on first use; buffers grow only; freed with the context)
NnGrid& ctx_tmp_grid(mrgfe_ctx* ctx);

// all jobs in one launch (blockIdx.y = job); out[j] = mean squared distance or DBL_MAX when nothing is in range
int nn_fitness_batch(mrgfe_ctx* ctx, const NnFitnessJob* jobs, size_t count, double max_range, double* out);

// The scan-matching status of every job (ScanMatchingOdometryComponent::publish_scan_matching_status, apps/scan_matching_odometry_component.cpp:403-417):
// nn_fitness_batch's passes with max_range = DBL_MAX, then out[3 j .. 3 j + 2] = (getFitnessScore: the same bits as nn_fitness_batch, or DBL_MAX when
// nothing was counted; the number of counted queries; the number of them whose squared distance, promoted to double, is < inlier_sq).  One host wait.
int nn_status_batch(mrgfe_ctx* ctx, const NnFitnessJob* jobs, size_t count, double inlier_sq, double* out);

// The same passes as a correspondence search (fast_gicp / small_gicp update_correspondences): jobs[j].idx_out[i] = index of the target point
// nearest to T * src[i] (ties: the lowest index) if its squared distance is < max_sq, else -1.  Enqueued on ctx->stream, no host wait.
int nn_nearest_batch(mrgfe_ctx* ctx, const NnFitnessJob* jobs, size_t count, double max_sq);

// What the last nn_fitness_select / FitSelectRun did: jobs per state, queries left to the sweep / the pyramid walk after the selection, host milliseconds of
// the bound stage (block, seed, bound sums, the selection) and of the contender stage (sweep, walk, sums).
struct FitSelectStats {
    uint64_t exact = 0, pruned = 0, above_cap = 0, skipped = 0, to_sweep = 0, to_far = 0;
    double   ms_bound = 0, ms_contend = 0;
};
// getFitnessScore of every job, exact only where the best-candidate rule still needs it (mrgfe_batch_align_best), in two stages with the selection
// between them left to the caller — who may hold the jobs of ONE batch (nn_fitness_select, batch_align_bounds / batch_align_finish) or be a node
// that decides over the pair lists of all its members at once.
//   bounds(): block pass and seed write a per-query interval lo <= d <= hi (hi: the attained distance in the query's slot); the bound sums give
//     every job [Σlo, Σhi] / count over the same slices and reduction tree as the exact sum (bit-valid, no epsilon) when the counted point sets
//     agree, else no bound (0 / +inf); one host wait.  Jobs that need nothing (group[j] >= 0 and not converged[j]) run with no queries: DBL_MAX / DBL_MAX.
//     A job's interval does not depend on the other jobs of the launch (per-query values; sums over fixed slices).
//   finish(): state[j] per job as fit_select_prune gives it (fit_select.h); the queues of the jobs that are not EXACT are emptied and the sweep, the
//     walk and the 2-column sum run for the rest; one more host wait (none when no job is left).  out_fit[j]: the exact score (EXACT), the lower
//     bound (PRUNED / ABOVE_CAP), DBL_MAX (SKIPPED).  stats: the jobs per state, the queries left to the sweep / the walk, and the host
//     milliseconds from the start of bounds() to the start of finish() (ms_bound) and of finish() (ms_contend).
// BETWEEN the two calls the run lives in the context's scratch buffers 9, 12, 13 and 14 (queues, per-query distances, lo) and on its streams:
// NOTHING else may run on that context in between.  The two callers hold to that: a batch runs both stages inside one ABI call under the
// context's lock, and a node member's context is reachable only through the node, whose api_mu is held from the first stage to the last.
// A run that is not finished is simply dropped (drop(), the destructor, the next bounds()): it owns no device memory.
class FitSelectRun {
   public:
    FitSelectRun();
    ~FitSelectRun();
    FitSelectRun(const FitSelectRun&) = delete;
    FitSelectRun& operator=(const FitSelectRun&) = delete;
    int  bounds(mrgfe_ctx* ctx, const NnFitnessJob* jobs, size_t count, double max_range, const int32_t* group, const int32_t* converged, double* out_lo, double* out_hi);
    int  finish(const int32_t* state, double* out_fit, FitSelectStats* stats = nullptr);
    bool pending() const;
    void drop();

   private:
    struct Impl;
    Impl* impl_ = nullptr;
};
// bounds -> fit_select_prune over the jobs -> finish: out_state[j] the decision, out_lo / out_hi the interval.  Two host waits per call.
int nn_fitness_select(mrgfe_ctx* ctx, const NnFitnessJob* jobs, size_t count, double max_range, const int32_t* group, int n_groups, const int32_t* converged, double score_cap,
                      double* out_fit, int32_t* out_state, double* out_lo, double* out_hi, FitSelectStats* stats = nullptr);

// far pass of the fitness score: 1 = seed + sweep (nn_fit_sweep_kernel), 0 = the pyramid walk for every queued query
int nn_set_fit_sweep(int mode);
// diagnostic counters of the seed + sweep pass: 0 off, 1 counters (FitStats::words ...), 2 also phase clocks and a line on stderr
int nn_set_fit_stats(int mode);

}  // namespace mrgfe
