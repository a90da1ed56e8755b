/* include/mrgfe_debug.h — diagnostic and test entry points of libmrgfe.so, kept out of the integrator's header (include/mrgfe.h).
 *
 * None of these stands for a call of the reference.  `mrgfe_dbg_set_*` select the alternative path of the SAME arithmetic (host- or device-stepped optimiser,
 * fused or per-variant launches, …) so that tests hold the two against each other; the primitives (`sort_pairs`, `wave_sums`, `exclusive_scan`, `minmax`,
 * `grid_set_query`) expose building blocks to tests/test_gpu_primitives.py; `mrgfe_dbg_ctl_*` step the NDT optimiser by hand with no GPU involved
 * (oracle/replay.py, tests/test_controller_cpu.py).  They are exported by the shipped library.
 *
 * The two FAULT INJECTORS at the end are different: they make a correct call fail.  They are compiled only with -DMRGFE_TESTING — into
 * mrg_slam_amd/libmrgfe_testing.so, which tests/faultinject/ loads in a child process (MRGFE_LIB) — and the shipped libmrgfe.so does not contain them
 * (tests/test_abi.py checks both). */
#ifndef MRGFE_DEBUG_H
#define MRGFE_DEBUG_H
#include "mrgfe.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostic entry points for the primitive tests (tests/test_gpu_primitives.py) --------------------------- */
/* correspondence search of GICP_HIP / SMALL_GICP_HIP (fast_gicp / small_gicp update_correspondences): the batched passes of getFitnessScore
 * carrying the index of the nearest point (csrc nn_nearest_batch) or one lane group per query until its answer is final.  1 = the passes for
 * batches of >= 400k queries (default: that is where they are faster), 0 = never, 2 = always.  Same correspondences either way; tests compare. */
int mrgfe_dbg_set_gicp_corr_passes(int mode);
/* Grids over `count` host clouds (packed xyzw floats) built TOGETHER (csrc NnGridSet, the batched form of the search grid under
 * getFitnessScore and the GICP covariances), then the `nq` queries answered against each: k == 1 the exact nearest neighbour, k > 1 the k
 * nearest, as mrgfe_knn.  idx / sqd: [count][nq][k].  `rounds` > 1 rebuilds the set that often (later builds reuse the cell edges). */
int mrgfe_dbg_grid_set_query(mrgfe_ctx* ctx, const float* const* clouds, const size_t* n, int count, const float* query, size_t nq, int k, int rounds, int32_t* idx, float* sqd);
int mrgfe_dbg_sort_pairs(mrgfe_ctx* ctx, const uint32_t* keys, const uint32_t* vals, size_t n, int key_bits, uint32_t* out_keys, uint32_t* out_vals);
/* The wave reduction of the derivative kernels' epilogue (csrc/dev_utils.h): in = cases x 64 lanes x n_vals doubles (n_vals 44, 37 or 1);
 * out_fold[cases][n_vals] from wave_sum_fold (n_vals values per lane folded in six steps), out_plain from n_vals separate wave_sum
 * calls.  Same summation tree, so the two must agree bit for bit (tests/test_gpu_primitives.py). */
int mrgfe_dbg_wave_sums(mrgfe_ctx* ctx, int n_vals, const double* in, int cases, double* out_fold, double* out_plain);
int mrgfe_dbg_exclusive_scan(mrgfe_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out, uint32_t* total);
int mrgfe_dbg_minmax(mrgfe_ctx* ctx, const float* xyzi, size_t n, float min3[3], float max3[3], uint32_t* n_finite);

/* The NDT optimiser (Newton + More-Thuente state machine: pclomp computeTransformation / computeStepLengthMT, the same source
 * the device steps in ndt_reduce_kernel) driven by hand, no GPU involved: create() runs align()'s prologue for `guess`;
 * request() returns 1 and the pending derivative evaluation (mode 0 score+gradient+Hessian, 1 score+gradient, 2 f64 Hessian
 * only; T = the transform to evaluate at, column-major; p = its pose vector) or 0 when the alignment is finished; result() hands
 * that evaluation's sums over and advances to the next request.  tests/test_controller_cpu.py feeds it the CPU oracle's
 * evaluations. */
/* Who steps that optimiser during the following alignments of this process: 0 = the device (the batch advances round after round
 * without the host), 1 = the host (one synchronisation per round), -1 = automatic (default: single registrations on the host,
 * batches on the device; the environment variable MRGFE_HOST_CONTROL sets the initial value).  Results are the same either way;
 * tests/test_gpu_control.py holds the two against each other. */
int mrgfe_dbg_set_host_control(int mode);
/* How the derivative evaluations of a round are launched during the following alignments of this process: 1 = ONE launch for all
 * three kernel variants, their work items walked kind after kind (default; the environment variable MRGFE_FUSED sets the initial value),
 * 0 = one launch per variant.  Any other value only asks.  Returns the setting in effect.  Same sums either way: an item's partial
 * record does not depend on the launch it is computed in (tests/test_gpu_control.py). */
int mrgfe_dbg_set_fused_launch(int mode);
/* NDT_HIP's f64 sums during the following alignments of this process: 1 = in the REFERENCE's order — ndt_omp adds a point's voxel terms from zero, then the
 * per-point sums point after point ("invariant against the summing up order"), and computeHessian pair after pair on one thread — reproduced by a record
 * kernel + one dependent-add chain per accumulator (csrc/ndt_derivatives.hip ndt_ref_*): bit-identical to the reference-order oracle, results inside the
 * 1e-4 bar unconditionally, several times slower (a 130k-step chain per evaluation whatever the batch size; host-stepped rounds); 0 = the tree (default; the
 * environment variable MRGFE_NDT_REFERENCE_ORDER sets the initial value).  Any other value only asks.  Returns the setting in effect. */
int mrgfe_dbg_set_ndt_reference_order(int mode);
/* ---- the NDT work items and the round plan (tests/test_gpu_ndt_items.py) ------------------------------------------------------------------
 * A derivative launch cuts a pair's source into ITEMS of ppt consecutive 256-point tiles, one partial record each, and a pair's records are added in a fixed
 * order; a round picks ppt per kernel variant as clamp(tiles of the variant's busy pairs / wg_target, 1, max_ppt) with wg_target = CUs * MRGFE_WG_PER_CU and
 * max_ppt = MRGFE_MAX_PPT (8).  So a pair's f64 sums are a function of its own points and of the round's ppt, and of nothing else.
 * mrgfe_ndt_evaluate with items of `ppt` tiles (1..64, the range MRGFE_PPT accepts), for NDT_HIP and PCL_NDT_HIP: */
int mrgfe_dbg_ndt_evaluate_ppt(mrgfe_reg* reg, const float T[16], const double p[6], int mode, int ppt, double* score, double grad[6], double hess[36]);
/* *neighbours = the (point, voxel) pairs the last mrgfe_ndt_evaluate / mrgfe_dbg_ndt_evaluate_ppt of this registration met: what the neighbourhood search
 * handed over, pairs the range check of updateDerivatives then dropped included (the reference's nb_total of that evaluation); 0 before the first one. */
int mrgfe_dbg_ndt_eval_neighbours(const mrgfe_reg* reg, double* neighbours);
/* wg_target and max_ppt of that rule during the following rounds of this process, for the device's plan kernel and the host's plan alike; 0 restores a
 * default.  With wg_target = 2 a batch of a few thousand points runs through ppt 8, 7, ..., 1 as its pairs finish, as a full-size batch does. */
int mrgfe_dbg_set_ndt_round_shape(int wg_target, int max_ppt);
/* the rounds of the last align of a registration, a batch or a node member: busy pairs and work items per kernel variant, n_pairs / n_items [round][3] (either
 * may be NULL), the first `cap` rounds.  Returns the number of rounds (>= 0) or an error code. */
int mrgfe_dbg_reg_ndt_rounds(const mrgfe_reg* reg, int cap, uint32_t* n_pairs, uint32_t* n_items);
int mrgfe_dbg_batch_ndt_rounds(const mrgfe_batch* b, int cap, uint32_t* n_pairs, uint32_t* n_items);
int mrgfe_dbg_node_ndt_rounds(const mrgfe_node* node, int member, int cap, uint32_t* n_pairs, uint32_t* n_items);
/* How getFitnessScore's far pass runs during the following calls of this process: 1 = seed + sweep (nn_fit_sweep_kernel: a near occupied
 * cell found through the occupancy words gives a radius, the occupied cells inside it are enumerated top-down with bit masks; default,
 * MRGFE_FIT_SWEEP sets the initial value), 0 = round 2's pyramid walk for every queued query.  Any other value only asks.  Returns the
 * setting in effect.  Both give the exact nearest distances (tests/test_gpu_fitness_passes.py). */
int mrgfe_dbg_set_fit_sweep(int mode);
/* The prefilter chains the device-driven form serves (mrgfe_ctx_prefilter_stats lists them) and the downsample of mrgfe_odom_frame[_device]: 1 (default)
 * the stages' point counts stay on the device and the call waits once at its end, 0 every stage reports its count to the host (round 3; also what an
 * unusual scan falls back to); other values query.  Same outputs either way (mrgfe_ctx_prefilter_stats and mrgfe_odom_stats report the route a call took). */
int mrgfe_dbg_set_prefilter_device_driven(int mode);
/* The rule by which the device sizes the statistical filter's k-NN grid behind NONE / APPROX_VOXELGRID (mrgfe_ctx_set_statistical_chains), during the
 * following chain calls of this process: the start edge in metres, the crowding target (population of the cell an average point sits in) and the most
 * halvings of the start edge.  All three zero restores the defaults; otherwise a start edge or a target of zero stands for its default and
 * max_halvings is taken as given (0: the start grid stands).  The filter's output does not depend on the rule, only its time does
 * (tests/test_gpu_prefilter_statistical_chains.py); mrgfe_ctx_sor_grid_stats reports what a call chose.  Returns MRGFE_OK. */
int mrgfe_dbg_set_sor_grid_rule(float start_edge, double crowding_target, int max_halvings);
/* What the last prefilter chain call on this context left for mrgfe_reg_set_source_from_prefilter: *remembered = 1 with the point count and the box
 * (min xyz, max xyz) when a device-driven chain's output stayed in the caller's device buffer and its box is known to enclose finite points only, else 0
 * (n, box may be NULL; box is written only when remembered). */
int mrgfe_dbg_prefilter_output(mrgfe_ctx* ctx, int* remembered, size_t* n, float box[6]);
/* A context with no device behind it: the record alone, made without a HIP call, so that a machine without a GPU can hold the checks an entry point makes
 * before it touches the device, and the statistics calls, against a real handle.  Every call that reaches the device fails on it with MRGFE_ERR_HIP;
 * mrgfe_ctx_destroy frees it. */
int mrgfe_dbg_ctx_create_detached(mrgfe_ctx** out);
/* mrgfe_ctx_set_wide_statistical_chains as the context holds it: *on = 1 or 0 (no device is touched).  inherited non-NULL: a context is made like this one
 * on its device, as the library makes its helper contexts (mrgfe_ctx_create_like), *inherited = the switch it received, and it is destroyed again. */
int mrgfe_dbg_wide_statistical_chains(mrgfe_ctx* ctx, int* on, int* inherited);
/* StatisticalOutlierRemoval's threshold from the mean distances dist[n] and the flags valid[n] (1: all mean_k neighbours were found): out[0] = sum of
 * dist, out[1] = sum of float(dist * dist), out[2] = sum of valid, out[3] = mean + stddev_mul * sqrt(variance) as the reference computes it, out[4] = 1
 * iff both sums are certified to have the same bits in every order of addition (csrc/sor_threshold.h: the sum is below 2^(q + 52) for 2^q the lowest
 * set bit of its non-zero terms), out[5] = that q for the terms of out[0] (2147483647: no non-zero term; -2147483647: a negative or non-finite term).
 * on_device = 0: the reference's sequential f64 loop on the host (ctx may be NULL); 1: the tree reduction and finish kernels of the device-driven
 * prefilter chain on the uploaded arrays.  One source compiled twice; where out[4] is 1 the two agree bit for bit. */
int mrgfe_dbg_sor_threshold(mrgfe_ctx* ctx, const float* dist, const uint32_t* valid, size_t n, double stddev_mul, int on_device, double out[6]);
/* PCL_GICP_HIP (serial pcl::GeneralizedIterativeClosestPoint, registrations.cpp:93-103): 1 (default) the thirteen sums of every cost / gradient
 * evaluation are added in the reference's order, point after point (bit-identical BFGS trajectories; ~4 ns per point and evaluation), 0 in a tree
 * (round 3: faster, and outside the 1e-4 bar on one random scene in fourteen); other values query.  PCL_GICP_OMP_HIP: 1 = pclomp's per-thread chunk
 * sums for its stated thread count (n / T dependent additions per evaluation), 0 = the tree. */
int mrgfe_dbg_set_pclgicp_reference_order(int mode);
/* Counters of the seed + sweep pass (mrgfe_ctx_fitness_stats out[6..9], mrgfe_batch_fitness_stats) during the following calls of this process:
 * 0 = off (default; MRGFE_FIT_STATS sets the initial value), 1 = counted, 2 = also the kernel's phase clocks and a line on stderr (slows
 * the kernel: a clock read waits for the memory operations in flight).  Any other value only asks.  Returns the setting in effect. */
int mrgfe_dbg_set_fit_stats(int mode);
/* The optimiser's scalar routines (pose vector -> float matrix, angle derivative tables, 6x6 SVD solve) on n cases of 48 doubles
 * (p[6], A[36] row-major, b[6]), on the host (on_device = 0, ctx may be NULL) or on the device: M16 [n][16] row-major, tables69
 * [n][8*3 + 15*3], x6 [n][6]; on_device = 2: x6 from the wavefront form of the solve (three lanes rotate, 36 apply) that the
 * device controller uses.  One source (csrc/ndt_ctl.h) compiled twice; the test compares the builds bit for bit. */
/* the float sine / cosine the optimiser builds its pose matrices with (host build of csrc/ndt_ctl.h: glibc's sinf / cosf algorithm
 * restated, because the reference's Eigen::AngleAxisf calls exactly those and they are not correctly rounded) */
void mrgfe_dbg_sincosf(const float* x, size_t n, float* sin_out, float* cos_out);
/* glibc's double exp() as the kernels compute it (csrc/glibc_exp.h: the reference evaluates its per-pair weights with the host's libm, and exp is not
 * correctly rounded — the device library's differs in the last bit on one argument in ten): on the host (on_device = 0, ctx may be NULL) or on the device.
 * tests/test_glibc_exp.py holds the host build against the C library and regenerates the table; tests/test_gpu_primitives.py holds the device against the host. */
int mrgfe_dbg_exp(mrgfe_ctx* ctx, const double* x, size_t n, int on_device, double* out);
/* The exp of the float path of the default NDT kernels (csrc/dev_exp.h exp_float_arg: the device library's exp(double) restated with scalar
 * coefficients) against that library call, on the device, for the `count` <= 2^32 float bit patterns first_bits, first_bits + 1, ... (wrapping):
 * *mismatches = patterns x for which the bits of exp_float_arg((double)x) differ from exp((double)x) (two NaNs are equal), *first_bad = the first such
 * pattern in sweep order (0 if none); classes (may be NULL): how many exp_float_arg results were zero, subnormal, infinite, NaN. */
int mrgfe_dbg_exp_float_args(mrgfe_ctx* ctx, uint32_t first_bits, uint64_t count, uint64_t* mismatches, uint32_t* first_bad, uint64_t classes[4]);
int mrgfe_dbg_ctl_math(mrgfe_ctx* ctx, const double* cases48, int n, int on_device, float* M16, double* tables69, double* x6);
/* ---- floor detection stages (tests/test_gpu_floor.py; csrc/floor.hip) ------------------------------------------------------------------- */
/* RandomSampleConsensus<SampleConsensusModelPlane> alone on a cloud (floor_detection_component.cpp:139-145): *has_model, the coefficients of the
 * winning sample, the inlier indices (capacity n, ascending), their count, iterations_ and the skipped samples.  `threshold` = setDistanceThreshold. */
int mrgfe_dbg_floor_ransac(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, double threshold, int* has_model, float coeffs[4], int32_t* inliers,
                           size_t* n_inliers, int32_t* iterations, int32_t* skipped);
/* normal_filtering (:216-243) alone: per point the eigen33 vector of NormalEstimation with setKSearch(10) (normals_xyz, 3 floats; NaN with fewer
 * than three neighbours) and the keep flag |n.z| / |n| > cos(normal_filter_thresh_deg) */
int mrgfe_dbg_floor_normals(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, double normal_filter_thresh_deg, float* normals_xyz, uint8_t* keep);
/* the last floor detection on this context: out[0..3] HIP-event milliseconds of the band stage (tilt, clip, compaction), the normal stage (grid,
 * k-NN, eigen33, compaction, back-transform), RANSAC (all waves) and the inlier pass; out[4] host waits; out[5] RANSAC waves; out[6] hypotheses drawn */
int mrgfe_dbg_floor_stats(mrgfe_ctx* ctx, double out[8]);

typedef struct mrgfe_dbg_ctl mrgfe_dbg_ctl;
int  mrgfe_dbg_ctl_create(const mrgfe_reg_params* params, const float guess[16], uint32_t n_src, mrgfe_dbg_ctl** out);
void mrgfe_dbg_ctl_destroy(mrgfe_dbg_ctl* h);
int  mrgfe_dbg_ctl_request(const mrgfe_dbg_ctl* h, int* mode, float T[16], double p[6]);
int  mrgfe_dbg_ctl_result(mrgfe_dbg_ctl* h, double score, const double grad[6], const double hess[36], double neighbours);
int  mrgfe_dbg_ctl_final(const mrgfe_dbg_ctl* h, float T[16], int* converged, int* iterations, int* evaluations);
/* the f64 fields a mrgfe_pair_result takes from the optimiser: H (6 x 6 row-major) and trans_probability as they stand */
int  mrgfe_dbg_ctl_record(const mrgfe_dbg_ctl* h, double hessian[36], double* trans_probability);
/* The ICP_HIP loop (csrc/gicp_engine.h IcpController: pcl::IterativeClosestPoint::computeTransformation with TransformationEstimationSVD and
 * DefaultConvergenceCriteria) stepped by hand, no GPU involved — the one controller behind single registrations and batches.  Every step wants the
 * same thing: the correspondences of the source AS TRANSFORMED SO FAR (by `guess`, then by every Tm returned) and their 17 sums: [0] their number,
 * [1..3] sum of the source points, [4..6] sum of the target points, [7..15] sum of target * source^T (row-major), [16] sum of squared distances.
 * _result takes them, sets *done, and gives the column-major float Tm to apply to the working copy next (the identity when the loop ended on fewer
 * than 3 correspondences); MRGFE_ERR_STATE once the loop has ended.  n_src == 0 or n_tgt == 0: feed one all-zero record.  Matrices column-major. */
typedef struct mrgfe_dbg_icp_ctl mrgfe_dbg_icp_ctl;
int  mrgfe_dbg_icp_ctl_create(const mrgfe_reg_params* params, const float guess[16], uint32_t n_src, uint32_t n_tgt, mrgfe_dbg_icp_ctl** out);
void mrgfe_dbg_icp_ctl_destroy(mrgfe_dbg_icp_ctl* h);
int  mrgfe_dbg_icp_ctl_result(mrgfe_dbg_icp_ctl* h, const double sums[17], int* done, float Tm[16]);
int  mrgfe_dbg_icp_ctl_final(const mrgfe_dbg_icp_ctl* h, float T[16], int* converged, int* iterations, int* evaluations);

/* ---- bounded best-candidate selection (mrgfe_batch_align_best, loop_detector.cpp:126-145 and :156-160) ---------------------------- */
/* per pair, the certified fitness interval lower <= getFitnessScore <= upper of the last mrgfe_batch_align_best on this pair list (0 / +inf: the
 * pair's counted point set was not certain at the selection, so no interval; DBL_MAX / DBL_MAX: no job — not converged or an empty cloud).
 * MRGFE_ERR_STATE when the last align was not an align_best. */
int mrgfe_dbg_batch_fit_bounds(const mrgfe_batch* b, double* lower, double* upper);
/* the same for the node's pair list after mrgfe_node_align_best (n_pairs entries each, in list order): the intervals of ONE batch holding the whole
 * list, bit for bit.  MRGFE_ERR_STATE when the last align of the node was not an align_best (or failed). */
int mrgfe_dbg_node_fit_bounds(const mrgfe_node* node, double* lower, double* upper);
/* the product's host selection on given intervals, no GPU needed: state[i] = enum mrgfe_fit_state of every pair (group[i] -1 or in [0, n_groups),
 * else MRGFE_ERR_INVALID).  A candidate without an upper bound passes upper = +inf. */
int mrgfe_dbg_select_prune(int n_pairs, const double* lower, const double* upper, const int32_t* converged, const int32_t* group, int n_groups, double score_cap,
                           int32_t* state);

/* ---- the odometry frame's state machine and head kernel (mrgfe_odom_frame; tests/test_odom_controller_cpu.py, tests/test_gpu_odometry_frame.py) ---- */
/* The controller behind mrgfe_odom_frame (csrc/odom_ctl.h: the state and decisions of ScanMatchingOdometryComponent::matching) stepped by hand, no GPU
 * involved; only the keyframe / thresholding fields of the params are read.  _begin: the frame's stamp and prediction (column-major or NULL) -> *aligns
 * (0 on a first frame) and the guess of :266; it changes nothing _state shows.  _end: hasConverged() and getFinalTransformation() of that frame (final
 * may be NULL on a first frame only) -> outcome, new_keyframe, consecutive_rejections, converged, odom, keyframe_pose and trans of `out`, the other fields
 * zero; MRGFE_ERR_STATE without a _begin before it.  A frame that fails between the two is simply not ended. */
typedef struct mrgfe_dbg_odom_ctl mrgfe_dbg_odom_ctl;
typedef struct mrgfe_dbg_odom_state {
    int32_t has_keyframe, consecutive_rejections, has_prev_time, reserved;
    double  keyframe_stamp, prev_time;           /* keyframe_stamp_, prev_time_ (seconds) */
    float   keyframe_pose[16], prev_trans[16];   /* column-major */
} mrgfe_dbg_odom_state;                          /* 160 bytes */
int  mrgfe_dbg_odom_ctl_create(const mrgfe_odom_params* params, mrgfe_dbg_odom_ctl** out);
void mrgfe_dbg_odom_ctl_destroy(mrgfe_dbg_odom_ctl* h);
int  mrgfe_dbg_odom_ctl_begin(mrgfe_dbg_odom_ctl* h, double stamp_seconds, const float* msf_delta, int* aligns, float guess[16]);
int  mrgfe_dbg_odom_ctl_end(mrgfe_dbg_odom_ctl* h, int converged, const float* final_transformation, mrgfe_odom_result* out);
int  mrgfe_dbg_odom_ctl_state(const mrgfe_dbg_odom_ctl* h, mrgfe_dbg_odom_state* out);
/* the state of a mrgfe_odom's own controller, same record */
int  mrgfe_dbg_odom_state_of(const mrgfe_odom* odom, mrgfe_dbg_odom_state* out);
/* What the last successful frame of `odom` handed to the registration: the cloud (out_xyzi: room for *n points, may be NULL to ask for *n alone) and, for a
 * message frame, the box the head kernel found over the message's finite points (box: min xyz, max xyz; +inf / -inf without a finite point) with their
 * count; *n_finite is 0xffffffff when that frame ran no head kernel (the device form). */
int  mrgfe_dbg_odom_source(mrgfe_odom* odom, float* out_xyzi, size_t* n, float box[6], uint32_t* n_finite);

/* ---- the one-call loop detector without a GPU, and its stage reuse (mrgfe_loop_detect; tests/test_loop_ctl_cpu.py, profiles/loop_detect_profile.py) ---- */
/* Replaces BOTH stages' GPU batches of `det` by a callback (fn NULL: the batches again).  A stage hands it its targets (target_keys: the new
 * keyframes' store keys), its pairs (pair_target indexes target_keys; source_keys; guesses: 16 column-major floats per pair) and want_fitness (stage 1:
 * 1, stage 2: 0); the callback fills results[i].T, .converged and, when want_fitness, .fitness of every pair (the records arrive zeroed, fitness
 * DBL_MAX) and returns MRGFE_OK or an error code, which mrgfe_loop_detect returns.  With an aligner set the batch and the store are never touched, and a
 * detector may have been created with both NULL.  Runs without a GPU, like mrgfe_dbg_select_prune. */
typedef int (*mrgfe_dbg_loop_aligner)(void* user, int stage, int n_targets, const uint64_t* target_keys, int n_pairs, const int32_t* pair_target,
                                      const uint64_t* source_keys, const float* guesses, int want_fitness, mrgfe_pair_result* results);
int  mrgfe_dbg_loop_set_aligner(mrgfe_loop* det, mrgfe_dbg_loop_aligner fn, void* user);
/* on = 0: stage 2 clears the batch and queues its targets again (the composed route's mrgfe_batch_clear between the two batches), so they are built a
 * second time; 1 (the default): mrgfe_batch_clear_pairs.  Same loops either way.  Returns the previous setting. */
int  mrgfe_dbg_loop_set_stage_reuse(mrgfe_loop* det, int on);
/* the LoopManager of `det`: 4 words per entry — the new keyframe's slam_id, the candidate's slam_id, key1, key2 — ordered by the two ids; out: room for
 * `capacity` entries (may be NULL with capacity 0), *n the entries there are */
int  mrgfe_dbg_loop_manager(const mrgfe_loop* det, int capacity, uint64_t* out, int* n);
/* how a node's members reach a map-store keyframe (mrgfe_node_add_*_from_store): 0 (the default) in place on the store's device, a replica elsewhere;
 * 1: always a replica, also on the store's device — there the copy is a plain device-to-device copy and everything after it is the replica route, which
 * a one-card machine exercises this way.  Same records either way. */
int  mrgfe_dbg_node_set_store_copy(mrgfe_node* node, int mode);

#ifdef MRGFE_TESTING
/* hardening hook: the k-th device / pinned allocation of this process from now on (0 = the next one) fails as if the device were out of memory, every
 * later one works again; k < 0 switches the injector off (MRGFE_FAIL_ALLOC_AFTER sets the initial value).  Returns the number of allocations made
 * since the previous call: a test sweeps k over a whole entry point and wants an error code from every k, then a correct answer. */
long   mrgfe_dbg_fail_alloc_after(long k);
/* the number of device buffers, pinned buffers and arena chunks of this process that are allocated and not yet freed: a test reads it before a sweep,
 * destroys what the sweep made and wants the same number back ("no leak") */
long   mrgfe_dbg_live_allocations(void);
/* test hook: the next mrgfe_node_align fails on that member (the error path without an out-of-memory condition) */
int    mrgfe_dbg_node_fail_member(mrgfe_node* node, int member);
#endif /* MRGFE_TESTING */

#ifdef __cplusplus
}
#endif
#endif /* MRGFE_DEBUG_H */
