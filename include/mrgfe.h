/* include/mrgfe.h — C ABI of libmrgfe.so, the MI355X (gfx950) scan-matching front end for mrg_slam.
 *
 * Drop-in boundary: everything the reference reaches through
 *     pcl::Registration<PointXYZI,PointXYZI>::Ptr select_registration_method(rclcpp::Node*)
 *         /root/reference/include/mrg_slam/registrations.hpp:20, src/mrg_slam/registrations.cpp:28-152
 * and through the pcl::Filter objects held by the prefiltering component
 *         /root/reference/apps/prefiltering_component.cpp:158-229
 * is exported here as plain C: opaque handles, host (or device) pointers and sizes, int status codes.
 * No exceptions cross this boundary; no torch / PCL / Eigen types appear in it.  The existing precedent for a
 * GPU registration back end in the reference is the FAST_VGICP_CUDA branch (registrations.cpp:65-75,
 * CMakeLists.txt:45-49); include/mrgfe_pcl_adapter.hpp wraps this ABI into that same slot.
 *
 * Conventions
 *   - clouds: float x,y,z,intensity per point ("xyzi").  Every `stride_bytes` argument is a point-layout descriptor:
 *     16 (or 0) = packed x,y,z,intensity records (KITTI .bin, the replay scripts' PointCloud2, every output of this
 *     library); any other record layout is named with MRGFE_LAYOUT(stride, xyz_offset, intensity_offset) —
 *     MRGFE_LAYOUT_PCL_XYZI for the reference's in-memory pcl::PointXYZI (32 bytes: x,y,z at 0, a 1.0f padding word at 12,
 *     intensity at byte 16).  A bare stride other than 16 is refused (MRGFE_ERR_INVALID): it cannot say where the
 *     intensity lives.  Strided records go to the device as they are and are gathered there.  Inputs are copied to the
 *     device inside the call: the caller may free or reuse its buffer when the call returns.
 *   - 4x4 matrices: float[16] / double[16], COLUMN-major (Eigen's default, i.e. Eigen::Matrix4f::data()).
 *   - 6x6 matrices: double[36], row-major (symmetric in practice).
 *   - status: 0 = ok, <0 = error; mrgfe_last_error() returns a thread-local message for the last failure.
 *     Non-convergence is NOT an error (pcl::Registration::align returns void; callers test hasConverged():
 *     apps/scan_matching_odometry_component.cpp:270, src/mrg_slam/loop_detector.cpp:138).
 *   - a handle is used from one thread at a time; distinct handles may be used from different threads (the odometry
 *     and loop-closure registrations of the reference live in different threads): calls that share a context are
 *     serialised by a per-context lock, calls on different contexts (e.g. one per GPU) run concurrently.
 */
#ifndef MRGFE_H
#define MRGFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* point-layout descriptor for the `stride_bytes` arguments: stride (<= 65532) | (intensity byte offset + 1) << 16 | (byte offset of
 * x; y and z follow it) << 24; offsets < 252, multiples of 4 */
#define MRGFE_LAYOUT(stride, xyz_offset, intensity_offset) \
    ((size_t)(stride) | ((size_t)((intensity_offset) + 1) << 16) | ((size_t)(xyz_offset) << 24))
#define MRGFE_LAYOUT_PACKED ((size_t)16)
#define MRGFE_LAYOUT_PCL_XYZI MRGFE_LAYOUT(32, 0, 16) /* sizeof(pcl::PointXYZI) == 32, intensity behind the padded xyz quad */

#define MRGFE_OK 0
#define MRGFE_ERR_INVALID (-1)   /* bad argument / handle */
#define MRGFE_ERR_HIP (-2)       /* HIP runtime error (no GPU, out of memory, launch failure) */
#define MRGFE_ERR_OVERFLOW (-3)  /* voxel index would overflow int32 ("Leaf size is too small for the input dataset") */
#define MRGFE_ERR_EMPTY (-4)     /* operation needs a non-empty cloud */
#define MRGFE_ERR_STATE (-5)     /* target / source not set */

typedef struct mrgfe_ctx mrgfe_ctx; /* one per (process, GPU): stream + grow-only device workspace */
typedef struct mrgfe_reg mrgfe_reg; /* one registration object == one pcl::Registration instance */

/* registration_method strings of the reference that this library serves (registrations.cpp:45-151) */
enum mrgfe_method {
    MRGFE_NDT_HIP = 0,  /* replaces "NDT_OMP"  : pclomp::NormalDistributionsTransform (registrations.cpp:130-148) */
    MRGFE_GICP_HIP = 1, /* replaces "FAST_GICP": fast_gicp::FastGICP                  (registrations.cpp:55-63)   */
    MRGFE_SMALL_GICP_HIP = 2, /* replaces "SMALL_GICP" (the YAML default, config/mrg_slam.yaml:100): small_gicp::RegistrationPCL
                                 (registrations.cpp:46-54): the same GICP factor perturbed on the right, small_gicp's LM schedule */
    MRGFE_VGICP_HIP = 3, /* replaces "FAST_VGICP" (fast_gicp::FastVGICP, registrations.cpp:76-84) and the reference's own GPU slot
                            "FAST_VGICP_CUDA" (:65-75): voxelised GICP, target as a Gaussian voxel map of edge `resolution` */
    MRGFE_ICP_HIP = 4, /* replaces "ICP": pcl::IterativeClosestPoint (registrations.cpp:85-92), use_reciprocal_correspondences as in :91;
                          also in mrgfe_batch_* / mrgfe_node_* (LoopDetector::matching with registration_method "ICP") */
    MRGFE_PCL_GICP_HIP = 5, /* replaces "GICP": pcl::GeneralizedIterativeClosestPoint (registrations.cpp:93-103): PCL's covariances, nearest-point
                               correspondences, inner BFGS with max_optimizer_iterations steps; single registrations only */
    MRGFE_PCL_GICP_OMP_HIP = 6, /* replaces "GICP_OMP": pclomp::GeneralizedIterativeClosestPoint (registrations.cpp:104-114): the same algorithm with
                                   the older stopping rule of the inner BFGS (norm of the whole gradient < 1e-2) and pclomp's accumulation: per-thread
                                   partial sums over static chunks of the correspondences, added in thread order — for num_threads threads (0: 8; at
                                   most 16).  Upstream the count is omp_get_max_threads() of the host: the reference's result depends on it */
    MRGFE_PCL_NDT_HIP = 7 /* replaces "NDT" and every name the factory does not know: pcl::NormalDistributionsTransform (registrations.cpp:115-129;
                             PCL 1.12): f64 pair terms, the radius search over the voxel centroids (nn_search_method is ignored), PCL's own
                             iteration test (squared translation of the last step <= transformation_epsilon); also in mrgfe_batch_* */
};
/* reg_nn_search_method (registrations.cpp:140-146) */
enum mrgfe_ndt_search { MRGFE_KDTREE = 0, MRGFE_DIRECT26 = 1, MRGFE_DIRECT7 = 2, MRGFE_DIRECT1 = 3 };

/* Mirrors the ten reg_* ROS parameters read by select_registration_method (registrations.cpp:34-43) plus the
 * library defaults those classes carry (ndt_omp: step_size 0.1, outlier_ratio 0.55; fast_gicp: rotation_epsilon 2e-3). */
typedef struct mrgfe_reg_params {
    int    method;                          /* enum mrgfe_method                        "registration_method"               */
    int    num_threads;                     /* unused on the GPU, except PCL_GICP_OMP_HIP: "reg_num_threads"
                                               the OpenMP thread count whose order of additions is reproduced: 1..16
                                               (0 = 8, the YAML's value; 1 = one chain; more than 16 is refused)            */
    double transformation_epsilon;          /*                                          "reg_transformation_epsilon"        */
    int    maximum_iterations;              /*                                          "reg_maximum_iterations"            */
    double max_correspondence_distance;     /* GICP                                     "reg_max_correspondence_distance"   */
    int    max_optimizer_iterations;        /* PCL_GICP_HIP: steps of the inner BFGS    "reg_max_optimizer_iterations"      */
    int    use_reciprocal_correspondences;  /* ICP_HIP (pcl::GICP ignores it upstream)  "reg_use_reciprocal_correspondences"*/
    int    correspondence_randomness;       /* GICP k neighbours, 4 .. 256              "reg_correspondence_randomness"     */
    double resolution;                      /* NDT / VGICP voxel size                   "reg_resolution"                    */
    int    nn_search_method;                /* enum mrgfe_ndt_search                    "reg_nn_search_method"              */
    double step_size;                       /* NDT More-Thuente step_max (0.1)    */
    double outlier_ratio;                   /* NDT (0.55)                         */
    double rotation_epsilon;                /* GICP (2e-3)                        */
} mrgfe_reg_params;

/* ---- library / context ------------------------------------------------------------------------------------- */
const char* mrgfe_last_error(void);
const char* mrgfe_version(void);
int  mrgfe_ctx_create(int device_id, mrgfe_ctx** out);
/* the same with the context's stream at the device's highest stream priority (high_priority != 0): workgroups of its kernels are
 * dispatched ahead of those of normal contexts as slots free up — for the latency-critical odometry registration of a process that
 * also runs loop-closure batches (scan_matching_odometry_component next to mrg_slam_component's LoopDetector) */
int  mrgfe_ctx_create_priority(int device_id, int high_priority, mrgfe_ctx** out);
/* a context whose kernels never occupy `reserve_cus` of the device's compute units (HIP stream with a CU mask; its helper streams too): for the
 * throughput work of a process — loop-closure batches (mrg_slam_component's LoopDetector) — so that the small per-scan launches of the odometry
 * contexts beside it always find free compute units instead of waiting for a batch's workgroups to drain.  reserve_cus = 0: mrgfe_ctx_create;
 * MRGFE_RESERVE_AUTO: sized from the device; reserve_cus >= the device's compute units: MRGFE_ERR_INVALID. */
#define MRGFE_RESERVE_AUTO (-1) /* reserve_cus: a quarter of the device's compute units, at most 64 (MI355X: 64 of 256; a 32-CU partition: 8) */
int  mrgfe_ctx_create_reserving(int device_id, int reserve_cus, mrgfe_ctx** out);
/* (HIP creates compute-unit-masked streams with default flags: unlike every other stream of this library they synchronise with the legacy NULL stream.  A
 * process that also enqueues work on the NULL stream — torch's default stream, a synchronous hipMemcpy — serialises a reserving context's kernels
 * against it; keep NULL-stream work out of such a process or use per-thread default streams.  Results never depend on it.) */
void mrgfe_ctx_destroy(mrgfe_ctx* ctx);
int  mrgfe_ctx_synchronize(mrgfe_ctx* ctx);
/* page-lock a host buffer the caller keeps between calls (hipHostRegister): downloads into it and uploads out of it are direct DMA at PCIe rate
 * instead of staged through the runtime's bounce buffers — worth it for the 60 MB map cloud of mrgfe_map_store_generate / mrgfe_map_cloud_generate
 * (map_cloud_generator.cpp:14-86 returns a fresh pcl cloud per call; a caller of this library reuses one buffer).  Unpin before freeing it. */
int  mrgfe_pin_host_buffer(mrgfe_ctx* ctx, void* p, size_t bytes);
int  mrgfe_unpin_host_buffer(mrgfe_ctx* ctx, void* p);
/* Zero-copy uploads (round 5; off by default).  on = 1: a packed cloud (stride 16) of 64 KB or more that is handed to mrgfe_*_set_* / mrgfe_batch_add_* /
 * mrgfe_node_add_* on this context out of page-locked host memory is read by DMA straight from the caller's buffer instead of through the context's
 * staging ring (a single-thread copy at about half the link's rate: 256 config[1] pairs from host clouds 44 -> 34.5 ms per step, 28.4 ms with two
 * batches in flight = 37 GB/s over the link).  The DMA is stream-ordered, so the CONTRACT CHANGES for such buffers: keep them unchanged until the call
 * that consumes the cloud (…_align / …_wait, mrgfe_ctx_synchronize) has returned — the reference's keyframe clouds are immutable ConstPtr clouds.
 * Pageable buffers, and everything while the switch is off, keep the default contract: free or reuse the memory as soon as the add / set call returns.
 * (mrgfe_node_* declares its clouds by pointer and uploads them inside mrgfe_node_align: its members always run with the switch on.) */
int  mrgfe_ctx_set_zero_copy_uploads(mrgfe_ctx* ctx, int on);
/* Byte-aligned PointCloud2 layouts (off by default).  Every call that reads the bytes of a sensor_msgs/PointCloud2 — mrgfe_ingest_pointcloud2,
 * mrgfe_scan_callback[_device], mrgfe_keyframe_callback, mrgfe_map_store_add_keyframes, mrgfe_odom_frame — by default demands FLOAT32 fields at offsets
 * that are multiples of 4 and a point_step and row_step that are multiples of 4 (MRGFE_ERR_INVALID otherwise).  pcl::fromROSMsg demands none of this:
 * the Velodyne driver's XYZIRT records are 22 bytes (x@0 y@4 z@8 intensity@12 FLOAT32, ring@16 UINT16, time@18 FLOAT32), others publish 26-byte
 * records with a FLOAT64 stamp at byte 18.  on = 1: calls that run on this context (a store's or a registration's context is the one it was made on)
 * take any point_step >= 1, any row_step >= width * point_step and any field offset with off + 4 <= point_step; fields may overlap.  The size and
 * count limits, the data_bytes checks and off_intensity < 0 stay as they are.  Such records are read by second instantiations of the same kernels
 * (each field put together from at most two aligned 4-byte words, its bits as they are, NaN payloads and denormals included); a layout that satisfies
 * the default rules launches exactly the kernels it launches with the switch off.  Contexts made like this one (mrgfe_ctx_create_like) inherit it. */
int  mrgfe_ctx_set_byte_layouts(mrgfe_ctx* ctx, int on);
/* Batches of the BFGS methods (off by default).  on = 1: mrgfe_batch_create on this context accepts MRGFE_PCL_GICP_HIP and MRGFE_PCL_GICP_OMP_HIP
 * (registration_method "GICP" / "GICP_OMP"): the candidates' BFGS loops advance in lock step, one round per functor evaluation of the pairs still running,
 * and every record is that of a single registration of the same pair, bit for bit (see mrgfe_batch_create).  Off: mrgfe_batch_create refuses the two
 * methods as it always did ("offered for single registrations only").  Contexts made like this one (mrgfe_ctx_create_like) inherit the switch.
 * mrgfe_node_create makes its own contexts and keeps refusing the two methods: nodes of BFGS batches are not offered. */
int  mrgfe_ctx_set_bfgs_batches(mrgfe_ctx* ctx, int on);
/* NDT sums in the reference's own order (off by default).  on = 1: every registration, evaluation (mrgfe_ndt_evaluate) and batch of MRGFE_NDT_HIP or
 * MRGFE_PCL_NDT_HIP that STARTS on this context from now on — and what borrows them: the odometry frame, loop detection over a batch — adds its sums as the
 * reference's host does instead of in a tree: NDT_HIP per point, then point after point (pclomp), PCL_NDT_HIP pair after pair on one chain
 * (pcl::NormalDistributionsTransform::computeDerivatives / computeHessian, all 36 Hessian entries: the reference's Hessian is not symmetric in its last bits),
 * every Newton solve through Eigen's two-sided JacobiSVD.  Every evaluation and every alignment then equals the CPU reference bit for bit; the default tree
 * moves a sum by ~1e-16 relative, which an optimisation that does not settle can amplify past 1e-4 (2 of 1200 random PCL NDT scenes).  The rounds are
 * stepped by the host, a record per point (NDT_HIP) or per (point, voxel) pair (PCL_NDT_HIP: up to 1.2 GB per 130k-point evaluation) goes through a
 * workspace bounded by MRGFE_REF_WORKSPACE_MB (default 16384; a round's evaluations are cut into launches that fit), and every sum is one dependent chain of
 * additions: a 130k-point PCL_NDT_HIP alignment of 8 iterations takes 1.1 s instead of 1.4 ms, NDT_HIP 75 ms instead of 1.3 ms (one MI355X).  A mode for
 * verification, not for the robot.  Off: everything is as it always was; the process-wide MRGFE_NDT_REFERENCE_ORDER=1 keeps governing
 * NDT_HIP only and never touches PCL_NDT_HIP.  Contexts made like this one (mrgfe_ctx_create_like) inherit the switch.  mrgfe_node_create makes its own
 * contexts: nodes are not offered the mode.  NULL ctx: MRGFE_ERR_INVALID. */
int  mrgfe_ctx_set_ndt_reference_order(mrgfe_ctx* ctx, int on);
/* STATISTICAL outlier removal behind downsample NONE or APPROX_VOXELGRID on the device-driven prefilter chain (off by default).  on = 1: from the next
 * chain call on this context (mrgfe_prefilter[_device | _records], mrgfe_scan_callback[_device | _records]) those chains wait for the device once, as
 * VOXELGRID -> STATISTICAL does (statistical_mean_k in 1..63, or 1..255 with mrgfe_ctx_set_wide_statistical_chains on as well): without a voxel leaf to take it from, the cell edge of the filter's k-NN grid is chosen ON THE
 * DEVICE from the cloud's own density, in a fixed sequence of launches (mrgfe_ctx_sor_grid_stats reports the choice).  The search does not depend on the
 * edge: the output is that of the host-driven passes bit for bit, and an unusual scan is handed back to them (mrgfe_ctx_prefilter_stats route 2).  Off:
 * those chains run the host-driven passes (route 0) as they always did.  VOXELGRID -> STATISTICAL is the same either way.  Contexts made like this one
 * (mrgfe_ctx_create_like) inherit the switch.  NULL ctx: MRGFE_ERR_INVALID. */
int  mrgfe_ctx_set_statistical_chains(mrgfe_ctx* ctx, int on);
/* statistical_mean_k 64..255 on the device-driven prefilter chain (off by default).  on = 1: from the next chain call on this context (mrgfe_prefilter[_device
 * | _records], mrgfe_scan_callback[_device | _records]) a STATISTICAL chain with statistical_mean_k in 64..255 is served where the same chain with 1..63 is:
 * behind VOXELGRID always, behind NONE / APPROX_VOXELGRID when mrgfe_ctx_set_statistical_chains is on too.  It then waits for the device once and writes no
 * [points][mean_k + 1] neighbour rows: the mean distances come out of a search that keeps up to four list entries per lane in registers.  The output is that
 * of the host-driven passes bit for bit, and an unusual scan is handed back to them (mrgfe_ctx_prefilter_stats route 2), as for 1..63.  Off: such chains run
 * the host-driven passes (route 0) as they always did.  statistical_mean_k 1..63 is served the same either way; 256 and more stays MRGFE_ERR_INVALID.
 * Contexts made like this one (mrgfe_ctx_create_like) inherit the switch.  NULL ctx: MRGFE_ERR_INVALID. */
int  mrgfe_ctx_set_wide_statistical_chains(mrgfe_ctx* ctx, int on);
/* HIP stream of the context as an opaque pointer (hipStream_t), for callers that order their own work after it */
void* mrgfe_ctx_stream(mrgfe_ctx* ctx);
/* Measurement hook ("1-NN fitness on hash grid: N (16 + 27*8 + m*16)"): what the last getFitnessScore pass on this context
 * did — mrgfe_reg_fitness, mrgfe_batch_align(fitness_max_range >= 0), mrgfe_calc_fitness_score, mrgfe_map_store_fitness.
 * out[0..2] = HIP-event milliseconds of the block pass / the seed + sweep pass / the pyramid walk of what could not be seeded (events on
 * the context's stream), out[3] = queries, out[4] = queries their 3x3x3 block did not settle, out[5] = queries without a seed within three
 * blocks, out[6..9] = occupancy words fetched / boxes tested against the sphere / cells opened / candidate points measured by the seed +
 * sweep pass (0 unless MRGFE_FIT_STATS=1), out[10] = number of passes run on this context so far. */
int mrgfe_ctx_fitness_stats(mrgfe_ctx* ctx, double out[11]);
/* The same for the last exact k-NN launch on this context (nn_knn_kernel: the k = 20 neighbourhoods behind the GICP covariances of
 * setInputSource / setInputTarget, registrations.cpp:46-63; StatisticalOutlierRemoval; mrgfe_knn): out[0] = HIP-event milliseconds of the
 * launch, out[1] = queries, out[2] = k, out[3] = candidate points measured (0 unless the diagnostic counters are on,
 * mrgfe_dbg_set_fit_stats), out[4] = k-NN launches on this context so far.  Waits for that launch to finish. */
int mrgfe_ctx_knn_stats(mrgfe_ctx* ctx, double out[5]);
/* Which route served the last prefilter chain call on this context (mrgfe_prefilter[_device], mrgfe_scan_callback[_device]):
 * out[0] = route — 0 the host-driven passes (every stage hands its point count to the host), 1 the device-driven chain (one wait; [distance filter] ->
 * NONE, VOXELGRID or APPROX_VOXELGRID -> NONE or RADIUS, and VOXELGRID -> STATISTICAL with statistical_mean_k in 1..63, 64..255 too when mrgfe_ctx_set_wide_statistical_chains is on; STATISTICAL behind NONE or
 * APPROX_VOXELGRID stays on route 0 unless mrgfe_ctx_set_statistical_chains is on), 2 the device-driven chain attempted and handed back to the host-driven passes (same output); out[1] = the
 * device-driven chain's anomaly word (routes 1 and 2): 1 a stage in front of another one left no (finite) point, 2 PCL's "leaf size too small"
 * pass-through, 4 no voxel, 8 a sum of the statistical filter's threshold could have depended on the order of addition, 16 the host's re-check of
 * that threshold differs from the device's, 32 a non-finite point reached the outlier filter (distance filter off and no VOXELGRID in front of it),
 * 256 the outlier filter's search grid needs more cells than its table — an EMPTY RESULT is no anomaly (route 1, 0 points); out[2..6] = its stage counts
 * (points after the distance filter, finite among them, voxels, points after the downsample — both the emitted centroids with APPROX_VOXELGRID, both
 * out[2] without a downsample —, points after the outlier filter, out[5] again without one; routes 1 and 2); out[7] = points out; out[8] = chain calls
 * on this context so far; out[9] = calls served device-driven so far. */
int mrgfe_ctx_prefilter_stats(mrgfe_ctx* ctx, double out[10]);
/* The statistical filter's k-NN grid of the last prefilter chain call on this context (no device is touched): out[0] = 1 when that call's statistical
 * stage sized its grid on the device (mrgfe_ctx_set_statistical_chains on, downsample NONE or APPROX_VOXELGRID, routes 1 and 2), else 0 and the rest 0;
 * out[1] = the start edge used, in metres (the rule's start edge, doubled until the cloud's box fits the cell table); out[2] = the chosen edge = out[1]
 * * 2^-out[3]; out[3] = halvings; out[4] = the crowding last measured (population of the cell an average point sits in, at the edge in front of the last
 * decision; 0: no counting pass measured); out[5] = cells of the built grid. */
int mrgfe_ctx_sor_grid_stats(mrgfe_ctx* ctx, double out[6]);
/* The record stage of the last mrgfe_scan_callback_records / mrgfe_prefilter_records / mrgfe_cloud_records_device on this context (no device is touched):
 * out[0] = 1 the record kernel wrote into the caller's page-locked buffer, 0 into the context's pinned buffer; out[1] = launches of the record stage (route 2:
 * the one that found the anomaly word set and wrote nothing, and the one behind the host-driven passes); out[2] = stream waits the call made in addition to
 * the chain's own (0 on route 1; mrgfe_cloud_records_device: its one); out[3] = record bytes that reached the host; out[4] = bytes of them copied by the
 * host (0 when direct); out[5] = such calls on this context so far.  mrgfe_ctx_prefilter_stats keeps reporting the chain itself. */
int mrgfe_ctx_egress_stats(mrgfe_ctx* ctx, int64_t out[6]);
/* The same six values for the SECOND record sink of the last call on this context that had one: the coloured cloud of mrgfe_scan_callback_outputs, the removed
 * cloud of mrgfe_keyframe_callback_records[_device].  out[2] counts the waits that sink added to its call (0 where the call's own wait covered it); out[5] the
 * calls that had a second sink.  A call without one leaves out[0..4] at 0; mrgfe_ctx_egress_stats never counts a second sink. */
int mrgfe_ctx_second_egress_stats(mrgfe_ctx* ctx, int64_t out[6]);

/* ---- cloud ingest --------------------------------------------------------------------------------- */
/* replaces pcl::fromROSMsg(*cloud_msg, *cloud) (apps/prefiltering_component.cpp:119-120, scan_matching_odometry_component.cpp:144-145):
 * the byte payload of a sensor_msgs/PointCloud2 (little-endian FLOAT32 fields at the given byte offsets — multiples of 4 inside a point_step and
 * row_step that are multiples of 4, or any with mrgfe_ctx_set_byte_layouts; mrgfe_pointcloud2_layout below finds them in the message's field list,
 * matching as pcl::fromROSMsg does, NOT by name alone; row_step 0 means
 * width * point_step; off_intensity < 0: no such field, intensity 0 like PointXYZI's default) becomes a packed x,y,z,intensity
 * cloud in host memory (out_xyzi, width*height*16 bytes, may be NULL) and / or device memory (d_out_xyzi, may be NULL) — the
 * latter feeds mrgfe_reg_set_*_device / mrgfe_batch_add_*_device / mrgfe_prefilter_device without the cloud leaving HBM.
 * The replay scripts' layout (point_step 16, offsets 0/4/8/12: python_scripts/kitti_singlerobot_processor.py:164-185) is a plain
 * copy; anything else is gathered on the device.  `data` must hold (height - 1) * row_step + width * point_step bytes: there is no
 * length argument (a sensor_msgs/PointCloud2 guarantees it; the Python wrapper checks it). */
int mrgfe_ingest_pointcloud2(mrgfe_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step, uint32_t off_x, uint32_t off_y,
                             uint32_t off_z, int32_t off_intensity, float* out_xyzi, void* d_out_xyzi);
/* The layout arguments of the calls that read a PointCloud2 from the message's own description.  mrgfe_pointcloud2_field is sensor_msgs/PointField;
 * the result is a mrgfe_keyframe_params (declared here; the FIRST EIGHT members of mrgfe_scan_params are this struct, in this order, so a caller may
 * copy it over the head of one; mrgfe_ingest_pointcloud2 takes the same eight values as arguments).  Runs on the host and needs no context.
 * The matching rule is pcl::fromROSMsg's (pcl::createMapping / FieldMatches): the first field with the name, datatype FLOAT32 (7) and count 1.
 * x, y or z without a match: MRGFE_ERR_INVALID, naming the field (PCL would leave it unset).  intensity without a match — no such field, or one that
 * is UINT8 / UINT16 / has count 2 —: off_intensity = -1, the intensity PCL leaves at 0; matching by name alone would read such a field as float bits.
 * is_bigendian != 0: MRGFE_ERR_INVALID.  width, height, point_step and row_step are copied as they are: whether the fields fit point_step and the rows
 * fit row_step is checked, as before, by the entry point the layout is handed to, which refuses under its own name.
 * *needs_byte_layouts (may be NULL) = 1 when the layout is outside the default rules, i.e. needs mrgfe_ctx_set_byte_layouts(ctx, 1). */
typedef struct mrgfe_pointcloud2_field {
    const char* name;
    uint32_t    offset;
    uint8_t     datatype;  /* sensor_msgs/PointField: INT8 1, UINT8 2, INT16 3, UINT16 4, INT32 5, UINT32 6, FLOAT32 7, FLOAT64 8 */
    uint32_t    count;
} mrgfe_pointcloud2_field;
struct mrgfe_keyframe_params;
size_t mrgfe_pointcloud2_field_size(void); /* sizeof(mrgfe_pointcloud2_field) as the library was compiled */
int    mrgfe_pointcloud2_layout(const mrgfe_pointcloud2_field* fields, int n_fields, uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step,
                                int is_bigendian, struct mrgfe_keyframe_params* out, int* needs_byte_layouts);

/* ---- registration: the pcl::Registration call surface the reference uses (SURVEY.md §8b "Seam") ---------------- */
/* defaults of select_registration_method's parameters (registrations.cpp:34-43 comments) for `method` */
void mrgfe_reg_default_params(int method, mrgfe_reg_params* out);
/* replaces: new pclomp::NormalDistributionsTransform + setters (registrations.cpp:133-146) / new fast_gicp::FastGICP (:57-62) */
int  mrgfe_reg_create(mrgfe_ctx* ctx, const mrgfe_reg_params* params, mrgfe_reg** out);
void mrgfe_reg_destroy(mrgfe_reg* reg);
/* replaces registration_->setInputTarget(cloud): scan_matching_odometry_component.cpp:203,295,333; loop_detector.cpp:104.
 * NDT: builds the voxel covariance grid (pclomp::VoxelGridCovariance::filter). Returns MRGFE_ERR_OVERFLOW like PCL's
 * index-overflow abort (the registration then has no target). */
int  mrgfe_reg_set_target(mrgfe_reg* reg, const float* xyzi, size_t n, size_t stride_bytes);
/* replaces registration_->setInputSource(cloud): scan_matching_odometry_component.cpp:208; loop_detector.cpp:127,229,272 */
int  mrgfe_reg_set_source(mrgfe_reg* reg, const float* xyzi, size_t n, size_t stride_bytes);
/* same, from packed float4 clouds already resident in device memory (zero-copy ingest; bench.py's timed region) */
int  mrgfe_reg_set_target_device(mrgfe_reg* reg, const void* d_xyzi, size_t n);
int  mrgfe_reg_set_source_device(mrgfe_reg* reg, const void* d_xyzi, size_t n);
/* mrgfe_reg_set_source_device for the cloud the last mrgfe_prefilter_device call on this registration's context left in `d_xyzi` (n = the count it
 * returned), UNTOUCHED since: the prefilter chain knows a box that encloses its output, so the GICP family builds the source's search grid without its own
 * bounding-box pass and stream wait.  Anything else (another pointer or count, a cloud that went to the host, NDT) is mrgfe_reg_set_source_device. */
int  mrgfe_reg_set_source_from_prefilter(mrgfe_reg* reg, const void* d_xyzi, size_t n);
/* replaces registration_->setInputTarget(keyframe) where the keyframe IS the cloud last given to set_source (the odometry's keyframe update,
 * scan_matching_odometry_component.cpp:326-339 -> :333): same result as set_target of that cloud, without uploading it again and, for the GICP
 * family, without recomputing its k-NN covariances and search grid (they were made when it was the source).  The source stays set;
 * a later set_target leaves it untouched. */
int  mrgfe_reg_source_becomes_target(mrgfe_reg* reg);
/* replaces registration_->align(*aligned, guess): scan_matching_odometry_component.cpp:265-266; loop_detector.cpp:134,236,279.
 * `aligned_xyzi` (n_source packed float4, may be NULL) receives final_transformation * source. */
int  mrgfe_reg_align(mrgfe_reg* reg, const float guess[16], float* aligned_xyzi);
/* replaces hasConverged() / getFinalTransformation(): scan_matching_odometry_component.cpp:270,275; loop_detector.cpp:138,144 */
int  mrgfe_reg_has_converged(const mrgfe_reg* reg);
int  mrgfe_reg_final_transformation(const mrgfe_reg* reg, float out[16]);
/* replaces getFitnessScore(max_range): loop_detector.cpp:137; scan_matching_odometry_component.cpp:403.
 * PCL semantics: mean squared 1-NN distance over source points whose SQUARED distance is <= max_range. */
int  mrgfe_reg_fitness(mrgfe_reg* reg, double max_range, double* out);
/* replaces getSearchMethodTarget()->nearestKSearch(pt, 1, ..): scan_matching_odometry_component.cpp:405-417 (batched) */
int  mrgfe_reg_nn1_target(mrgfe_reg* reg, const float* query_xyzi, size_t n, size_t stride_bytes, int32_t* idx, float* sqdist);
/* replaces ScanMatchingOdometryComponent::publish_scan_matching_status (scan_matching_odometry_component.cpp:391-431), the call the odometry makes after
 * every align while its status topic has a subscriber: the fields of mrg_slam_msgs/ScanMatchingStatus from ONE fitness pass over the source and one host
 * wait.  The grid of mrgfe_reg_fitness / mrgfe_reg_nn1_target is searched; no cloud is uploaded or downloaded.  matching_error has the bits of
 * mrgfe_reg_fitness with max_range = DBL_MAX; num_inliers counts the source points whose squared 1-NN distance (float, promoted to double) is strictly
 * below max_correspondence_dist squared (:413; the reference uses 0.5).  msf_delta (column-major 4x4, may be NULL): the prediction of :393; with NULL,
 * prediction_error is zero and has_prediction 0.  Errors as mrgfe_reg_fitness; an empty target or source gives matching_error = DBL_MAX and no inliers. */
typedef struct mrgfe_matching_status {
    int32_t  has_converged;       /* hasConverged()                                                                               :402 */
    uint32_t n_points;            /* aligned->size(): the source's point count                                                         */
    uint32_t num_inliers;         /*                                                                                          :407-416 */
    float    inlier_fraction;     /* static_cast<float>(num_inliers) / n_points (n_points == 0: NaN, as 0.0f / 0)                 :417 */
    double   matching_error;      /* getFitnessScore(), max_range = DBL_MAX                                                       :403 */
    double   relative_pose[7];    /* isometry2pose(Isometry3f(final).cast<double>()): position x y z, orientation x y z w         :419 */
    double   prediction_error[7]; /* isometry2pose((Isometry3f(final).inverse() * msf_delta).cast<double>())                  :426-427 */
    int32_t  has_prediction;      /* msf_delta was given                                                                               */
    int32_t  reserved;
} mrgfe_matching_status;          /* 144 bytes */
size_t mrgfe_matching_status_size(void); /* sizeof(mrgfe_matching_status) as the library was compiled */
int    mrgfe_reg_matching_status(mrgfe_reg* reg, double max_correspondence_dist, const float* msf_delta, mrgfe_matching_status* out);
/* The two poses of the status alone, pure host arithmetic (no context, no GPU): relative_pose from the column-major final transformation, and, when
 * msf_delta is not NULL, prediction_error (else left untouched; may then be NULL).  The inverse and the product are float, the quaternions double. */
int    mrgfe_status_poses(const float final_transformation[16], const float* msf_delta, double relative_pose[7], double prediction_error[7]);
/* extra read-outs (pcl: getFinalNumIteration / ndt: getTransformationProbability; 6x6 Hessian for the pose gather of §8e) */
int    mrgfe_reg_iterations(const mrgfe_reg* reg);
int    mrgfe_reg_evaluations(const mrgfe_reg* reg); /* derivative (NDT) / linearize+error (GICP) passes of the last align */
double mrgfe_reg_trans_probability(const mrgfe_reg* reg);
int    mrgfe_reg_hessian(const mrgfe_reg* reg, double out[36]);

/* ---- NDT internals exposed for kernel-level parity tests and the roofline accounting --------------------------- */
/* one derivative evaluation at pose vector p (tx,ty,tz,rx,ry,rz) with the source transformed by T:
 * mode 0 = score+gradient+Hessian, 1 = score+gradient, 2 = Hessian only in double (pclomp computeHessian).  PCL_NDT_HIP: all three in f64. */
int mrgfe_ndt_evaluate(mrgfe_reg* reg, const float T[16], const double p[6], int mode, double* score, double grad[6], double hess[36]);
/* target grid: number of voxels with >= 1 point; per-voxel key (ascending), point count (-1: rejected by the
 * eigenvalue / inf checks), mean[3], inverse covariance[9] (row-major). Arrays sized by mrgfe_ndt_num_leaves. */
int mrgfe_ndt_num_leaves(const mrgfe_reg* reg);
int mrgfe_ndt_grid(const mrgfe_reg* reg, int32_t min_b[3], int32_t max_b[3], int32_t div_b[3]);
int mrgfe_ndt_leaves(mrgfe_reg* reg, int32_t* keys, int32_t* nr_points, double* mean3, double* icov9);
/* mean number of valid neighbour voxels per source point over the evaluations of the last align (k-bar of SURVEY §8d) */
double mrgfe_ndt_mean_neighbours(const mrgfe_reg* reg);

/* k nearest neighbours of every query among the points of `cloud` (pcl::search::KdTree::nearestKSearch(pt, k, ...), the
 * search behind fast_gicp's covariances and StatisticalOutlierRemoval): idx / sqd are [nq][k], ascending by (squared
 * distance, index); entries beyond the cloud's size are -1 / -1.  1 <= k <= 256, the library's limit (anything else is MRGFE_ERR_INVALID): up to
 * 64 the neighbour list of a query holds one entry per lane of its wavefront, 65 .. 256 run a wide kernel with two to four.  Non-finite queries
 * get no neighbours. */
int mrgfe_knn(mrgfe_ctx* ctx, const float* cloud_xyzi, size_t n, const float* query_xyzi, size_t nq, size_t stride_bytes, int k, int32_t* idx, float* sqd);

/* ---- GICP internals exposed for kernel-level parity tests ------------------------------------------------------------ */
/* update_correspondences + linearize at the pose T (column-major double 4x4, T_target_source): H (row-major 6x6,
 * rotation block first), b, the sum of r^T M r over the correspondences (the variants scale it themselves) and their
 * number.  The Jacobian is the one of the registration's method (fast_gicp: left, small_gicp: right perturbation). */
int mrgfe_gicp_linearize(mrgfe_reg* reg, const double T[16], double H[36], double b[6], double* sum_errors, int* n_correspondences);
/* compute_error at the pose T: the sum of r^T M r over the correspondences and Mahalanobis matrices FROZEN by the last mrgfe_gicp_linearize or
 * alignment on this registration, and the number of its terms — the cost a Levenberg-Marquardt trial is judged by, through the launch the
 * loop makes.  The raw sum (small_gicp's 1/2 is the controller's).  MRGFE_ERR_STATE when nothing was linearised since the clouds were set,
 * MRGFE_ERR_INVALID for ICP_HIP and the PCL_GICP methods. */
int mrgfe_gicp_error(mrgfe_reg* reg, const double T[16], double* sum_errors, int* n_terms);
/* regularised k-NN covariances (row-major 3x3 per point) of the source (which = 0) or target (1) cloud */
/* PCL_GICP_HIP (tests): the correspondences and Mahalanobis matrices pcl::GICP's search loop finds at transformation_ = T (column-major, guess
 * = identity), and the cost estimateRigidTransformationBFGS minimises at x = (t, euler ZYX) over them: *f, grad[6], number of correspondences */
int mrgfe_pclgicp_evaluate(mrgfe_reg* reg, const float T[16], const double x[6], double* f, double grad[6], int* n_correspondences);
int mrgfe_gicp_covariances(mrgfe_reg* reg, int which, double* cov9_per_point);

/* ---- prefilter chain (apps/prefiltering_component.cpp:149-151). Outputs: caller-allocated capacity-n packed float4
 *      buffers + count.  Order-preserving where the reference is. ------------------------------------------------- */
/* The whole chain of PrefilteringComponent::cloud_callback (:149-151: distance_filter -> downsample -> outlier_removal) in
 * one call: the cloud goes up once, stays in HBM between the three passes, and comes down once.  Same output as the three
 * calls below one after the other.  Parameter names / YAML defaults: config/mrg_slam.yaml:41-64
 * (prefiltering_component.cpp:92-112 declares them). */
typedef struct mrgfe_prefilter_params {
    int    enable_distance_filter;            /* 1                                     */
    double distance_near_thresh;              /* 0.1                                   */
    double distance_far_thresh;               /* 35.0                                  */
    int    downsample_method;                 /* 0 NONE, 1 VOXELGRID, 2 APPROX_VOXELGRID */
    double downsample_resolution;             /* 0.1                                   */
    int    downsample_min_points_per_voxel;   /* 1                                     */
    int    outlier_removal_method;            /* 0 NONE, 1 RADIUS, 2 STATISTICAL       */
    double radius_radius;                     /* 0.5                                   */
    int    radius_min_neighbors;              /* 2                                     */
    int    statistical_mean_k;                /* 30                                    */
    double statistical_stddev;                /* 1.2                                   */
} mrgfe_prefilter_params;
void mrgfe_prefilter_default_params(mrgfe_prefilter_params* out);
int  mrgfe_prefilter(mrgfe_ctx* ctx, const mrgfe_prefilter_params* params, const float* xyzi, size_t n, size_t stride_bytes, float* out_xyzi, size_t* out_n);
/* the same with the result left in device memory (packed float4, capacity >= n points) for mrgfe_reg_set_source_device /
 * mrgfe_batch_add_*_device: the filtered scan goes from the prefiltering callback to the scan matcher without leaving HBM */
int  mrgfe_prefilter_device(mrgfe_ctx* ctx, const mrgfe_prefilter_params* params, const float* xyzi, size_t n, size_t stride_bytes, void* d_out_xyzi, size_t* out_n);
/* the same with the result as the records of the message the component publishes (point_step 32 or 16, capacity_bytes >= n * point_step) and, with
 * d_out_xyzi non-NULL, left in device memory as mrgfe_prefilter_device leaves it: see mrgfe_scan_callback_records below for the records, the destination
 * and the refusals — the points, their order, their bits and *out_n are mrgfe_prefilter's */
int  mrgfe_prefilter_records(mrgfe_ctx* ctx, const mrgfe_prefilter_params* params, const float* xyzi, size_t n, size_t stride_bytes, int point_step, void* records,
                             size_t capacity_bytes, void* d_out_xyzi, size_t* out_n);

/* ---- the scan callback in one call (PrefilteringComponent::cloud_callback, apps/prefiltering_component.cpp:116-156) --- */
/* pcl::fromROSMsg (:119-120) -> deskewing (:125, :231-295) -> pcl_ros::transformPointCloud into base_link_frame (:141-146) -> distance_filter ->
 * downsample -> outlier_removal (:149-151) on the byte payload of a sensor_msgs/PointCloud2.  The payload goes up ONCE as it is; one kernel reads
 * the records, deskews, transforms, stores the packed cloud and (on the usual chains) is the distance filter's first pass; nothing comes down but
 * the chain's status words and, for the host form, the filtered cloud; every chain but STATISTICAL behind NONE or APPROX_VOXELGRID (unless
 * mrgfe_ctx_set_statistical_chains is on), or with statistical_mean_k outside 1..63, waits for the device once (mrgfe_ctx_prefilter_stats says which route served a call).
 * statistical_mean_k 64 .. 255 is served by the host-driven passes (route 0, the wide k-NN kernel) unless mrgfe_ctx_set_wide_statistical_chains is on — then it
 * waits once like 1..63; 256 and more is MRGFE_ERR_INVALID.
 * The output equals, bit for bit and in order, mrgfe_ingest_pointcloud2 -> mrgfe_deskew (if `deskew`) -> mrgfe_transform_cloud (if `transform`)
 * -> mrgfe_prefilter[_device] for the same inputs.  The reference's quirks are kept: deskewing counts i and n = width * height over the UNFILTERED
 * cloud (:286), non-finite points included; the transform leaves non-finite points as they are; the distance filter is what drops them. */
typedef struct mrgfe_scan_params {
    /* the message's layout, as for mrgfe_ingest_pointcloud2 (little-endian FLOAT32 fields; offsets and steps multiples of 4 unless the context has
     * mrgfe_ctx_set_byte_layouts on).  These first eight members are a mrgfe_keyframe_params: what mrgfe_pointcloud2_layout fills in. */
    uint32_t width, height, point_step, row_step;   /* row_step 0: width * point_step                                      */
    uint32_t off_x, off_y, off_z;
    int32_t  off_intensity;                         /* < 0: no such field, intensity 0                                     */
    int      deskew;                                /* 0: imu_queue_ was empty (:234-236), the cloud is not deskewed        */
    float    ang_v[3];                              /* imu_msg->angular_velocity, NOT negated (the call negates it, :275)  */
    double   scan_period;                           /* 0.1                                                                 */
    int      transform;                             /* 0: base_link_frame is empty (:129)                                  */
    float    T[16];                                 /* column-major Matrix4f of the tf transform                           */
    mrgfe_prefilter_params filters;
} mrgfe_scan_params;
/* height 1, the packed 16-byte layout (offsets 0/4/8/12), no deskewing (scan_period 0.1), no transform (T = identity), mrgfe_prefilter_default_params;
 * `width` is left 0 for the caller */
void   mrgfe_scan_default_params(mrgfe_scan_params* out);
size_t mrgfe_scan_params_size(void); /* sizeof(mrgfe_scan_params) as the library was compiled: a binding checks its mirror of the struct against it */
/* `data`: (height - 1) * row_step + width * point_step bytes (no length argument, as for mrgfe_ingest_pointcloud2); out_xyzi: room for
 * width * height packed points.  An empty message (width * height == 0) is MRGFE_OK with *out_n = 0: the reference returns early (:121-123). */
int    mrgfe_scan_callback(mrgfe_ctx* ctx, const mrgfe_scan_params* params, const uint8_t* data, float* out_xyzi, size_t* out_n);
/* the same with the filtered scan left in device memory (packed float4, room for width * height points): what mrgfe_prefilter_device leaves,
 * mrgfe_reg_set_source_from_prefilter(reg, d_out_xyzi, *out_n) included */
int    mrgfe_scan_callback_device(mrgfe_ctx* ctx, const mrgfe_scan_params* params, const uint8_t* data, void* d_out_xyzi, size_t* out_n);
/* The callback to its end: pcl::toROSMsg(*filtered, filtered_ros) (apps/prefiltering_component.cpp:152-155).  The filtered scan comes down as the `data` of
 * the message the component publishes, written on the device:
 *   point_step 32: x, y, z, 1.0f, intensity, 0, 0, 0 — the pcl::PointXYZI in memory, which toROSMsg copies as it is (fields x@0 y@4 z@8 intensity@16);
 *   point_step 16: x, y, z, intensity (intensity@12)
 * the two layouts of mrgfe_map_store_publish, and as there the message's other members are the caller's (width = *out_n, height 1, row_step = *out_n *
 * point_step, is_dense false, little endian, FLOAT32 fields).  The points, their order, their bits (a NaN's payload included) and *out_n are those of
 * mrgfe_scan_callback for the same inputs; every refusal of that call is kept, and an empty message is MRGFE_OK with *out_n = 0 and no byte written.
 * records: room for capacity_bytes >= width * height * point_step (the "room for width * height points" of out_xyzi); only its first *out_n * point_step bytes
 * are ever written.  MRGFE_ERR_INVALID before anything is launched, `records` untouched: a NULL ctx / params / records / out_n (data: of a message that is
 * not empty), a point_step other than 16 or 32, a capacity_bytes below that.
 * d_out_xyzi non-NULL (device memory, room for width * height packed points): the packed scan is left there as well, exactly as mrgfe_scan_callback_device
 * leaves it, mrgfe_reg_set_source_from_prefilter(reg, d_out_xyzi, *out_n) included — the prefiltering and odometry components of one container get the message
 * and the device cloud from one call.  NULL: an internal buffer, nothing is remembered.
 * On the chains that wait once (mrgfe_ctx_prefilter_stats route 1) the record kernel runs behind the last stage from the count the device holds, in front of
 * that one wait: the call has no other.  If `records` starts at a multiple of 16 bytes and both ends of [records, records + capacity_bytes) lie in
 * page-locked host memory (mrgfe_pin_host_buffer, hipHostMalloc, hipHostRegister), the kernel writes the caller's buffer itself; otherwise it writes a pinned
 * buffer of the context and the host copies *out_n * point_step bytes out behind the wait.  A route-1 STATISTICAL chain always takes the
 * second way (the host re-checks that chain's threshold behind the wait and may still hand the call back: the caller's buffer must not have been written
 * beyond the final *out_n by then).  On routes 0 and 2 the host-driven passes make the cloud and mrgfe_cloud_records_device's kernel follows with the host's
 * count, behind one more wait.  mrgfe_ctx_egress_stats says what a call did. */
int    mrgfe_scan_callback_records(mrgfe_ctx* ctx, const mrgfe_scan_params* params, const uint8_t* data, int point_step, void* records, size_t capacity_bytes,
                                   void* d_out_xyzi, size_t* out_n);
/* The callback with its second publish: prefiltering/colored_points, the loop of deskewing() (apps/prefiltering_component.cpp:239-257) — the raw scan as
 * pcl::PointXYZRGB, the colour saying where a point stands in the point sequence — written on the device from the SAME uploaded payload.
 *   colored_records NULL: the call is mrgfe_scan_callback_records(ctx, params, data, point_step, records, capacity_bytes, d_out_xyzi, out_n), bit for bit:
 *     results, refusals, mrgfe_ctx_prefilter_stats, mrgfe_ctx_egress_stats.
 *   colored_records non-NULL (colored_capacity_bytes >= 32 * width * height): it receives n = width * height records of 32 bytes in message order, non-finite
 *     points included, of the cloud as pcl::fromROSMsg left it (:119-120) — before deskewing, before the transform, before any filter (:125 hands deskewing()
 *     the unpacked cloud) — and *out_n_colored = n.  One more kernel reads the wire records of the raw device buffer the scan's head kernel reads (the same
 *     reader, the byte-aligned one for a layout of mrgfe_ctx_set_byte_layouts).  [UPSTREAM-RECALL] the record is the pcl::PointXYZRGB in memory, which
 *     pcl::toROSMsg copies as it is (fields x@0 y@4 z@8 rgb@16, point_step 32):
 *       bytes 0..11 the bits of x, y, z as read (a NaN's payload included); 12..15 1.0f; 16 b, 17 g = 128, 18 r, 19 a = 255; 20..31 zero
 *     with t = (double)i / (double)n, r = (uint8_t)(255 * t), b = (uint8_t)(255 * (1 - t)): IEEE f64, a real division, truncated toward zero (:248-252).
 *     The kernel is queued in front of the chain: on route 1 the chain's one wait covers it and the call gains none; on routes 0 and 2 it is waited for behind
 *     the host-driven passes.  The destination rule is that of `records`; what is staged goes through a second pinned buffer of the context, so the filtered
 *     records keep their own path (a route-1 STATISTICAL chain's stay staged).  mrgfe_ctx_second_egress_stats says what the colour stage did.
 *   records NULL: no filtered records are wanted; with d_out_xyzi non-NULL the call is mrgfe_scan_callback_device plus the coloured records, with d_out_xyzi
 *     NULL as well only the coloured records are made (no chain runs, *out_n = 0, mrgfe_ctx_prefilter_stats untouched).
 *   Whether to publish is the caller's decision — a subscriber and a non-empty IMU queue (:234,239); the call colours whenever it is asked.
 *   MRGFE_ERR_INVALID before anything is launched, no byte written: a NULL ctx / params / outputs / out_n / out_n_colored, records and colored_records both NULL,
 *     colored_capacity_bytes < 32 * width * height, and every refusal of mrgfe_scan_callback_records.  An empty message is MRGFE_OK with both counts 0. */
typedef struct mrgfe_scan_outputs {
    int    point_step;                 /* 16 or 32: the filtered scan's records, as mrgfe_scan_callback_records (ignored when records is NULL) */
    void*  records;                    /* may be NULL: no filtered records wanted                                                           */
    size_t capacity_bytes;
    void*  colored_records;            /* may be NULL; 32-byte records only                                                                 */
    size_t colored_capacity_bytes;
    void*  d_out_xyzi;                 /* may be NULL, as mrgfe_scan_callback_records                                                       */
} mrgfe_scan_outputs;
size_t mrgfe_scan_outputs_size(void); /* sizeof(mrgfe_scan_outputs) as the library was compiled */
int    mrgfe_scan_callback_outputs(mrgfe_ctx* ctx, const mrgfe_scan_params* params, const uint8_t* data, const mrgfe_scan_outputs* outputs, size_t* out_n,
                                   size_t* out_n_colored);
/* The n packed 16-byte points at d_xyzi (device memory of the context's GPU: what mrgfe_scan_callback_device, mrgfe_prefilter_device, mrgfe_floor_detect_device's
 * caller or a keyframe callback's caller hold) as the same records: one launch, one wait, the same destination rule; capacity_bytes >= n * point_step.
 * MRGFE_ERR_INVALID, nothing read or written: a NULL argument, another point_step, too little capacity, a d_xyzi that is not device memory of the context's
 * GPU (as mrgfe_keyframe_callback_device refuses it).  n = 0 is MRGFE_OK. */
int    mrgfe_cloud_records_device(mrgfe_ctx* ctx, const void* d_xyzi, size_t n, int point_step, void* records, size_t capacity_bytes);

/* replaces PrefilteringComponent::distance_filter (:206-229): keep iff near < |p| < far */
int mrgfe_distance_filter(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, double near_thresh, double far_thresh,
                          float* out_xyzi, size_t* out_n);
/* replaces pcl::VoxelGrid<PointXYZI>::filter with setLeafSize(l,l,l), setMinimumPointsNumberPerVoxel (:168-171;
 * scan_matching_odometry_component.cpp:176-179). Returns MRGFE_OK with *overflow=1 and output == input when PCL would
 * warn "Leaf size is too small" and pass the cloud through. */
int mrgfe_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, float leaf, int min_points_per_voxel,
                    float* out_xyzi, size_t* out_n, int* overflow);
/* replaces pcl::ApproximateVoxelGrid<PointXYZI>::filter (downsample_method APPROX_VOXELGRID: prefiltering_component.cpp:172-175,
 * scan_matching_odometry_component.cpp:180-183): the 512-entry direct-mapped history of cells (hash (ix*7171 + iy*3079 + iz*4231) & 511), an entry
 * flushed — its float centroid of x, y, z, intensity emitted — whenever a point of another cell arrives at it, the rest flushed in entry order at
 * the end.  The output depends on the order of the input, a cell can be emitted several times, and there is no minimum point count: all of
 * that is reproduced point for point (csrc/filters.hip decomposes the sequential loop into the 512 independent per-entry sequences).
 * out_xyzi: capacity n points. */
int mrgfe_approx_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, float leaf, float* out_xyzi, size_t* out_n);
/* replaces pcl::RadiusOutlierRemoval::filter with setRadiusSearch / setMinNeighborsInRadius (:195-198) */
int mrgfe_radius_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, double radius, int min_neighbors,
                         float* out_xyzi, size_t* out_n);
/* replaces pcl::StatisticalOutlierRemoval::filter with setMeanK / setStddevMulThresh (:189-192).  1 <= mean_k <= 255: the mean_k + 1 nearest of a
 * point, itself first, must fit the k-NN search's list of 256 (mrgfe_knn); anything else is MRGFE_ERR_INVALID */
int mrgfe_statistical_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, int mean_k, double stddev_mul,
                              float* out_xyzi, size_t* out_n);
/* replaces InformationMatrixCalculator::calc_fitness_score (src/mrg_slam/information_matrix_calculator.cpp:46-81) */
int mrgfe_calc_fitness_score(mrgfe_ctx* ctx, const float* cloud1, size_t n1, const float* cloud2, size_t n2, size_t stride_bytes,
                             const double relpose[16], double max_range, double* out);

/* InformationMatrixCalculator's parameters (apps/mrg_slam_component.cpp:313-322 declares them; defaults: config/mrg_slam.yaml:216-223,173) */
typedef struct mrgfe_inf_params {
    int    use_const_inf_matrix;          /* 0    */
    double const_stddev_x, const_stddev_q; /* 0.5, 0.1 */
    double var_gain_a;                    /* 2.0  */
    double min_stddev_x, max_stddev_x;    /* 0.1, 0.75 */
    double min_stddev_q, max_stddev_q;    /* 0.05, 0.2 */
    double fitness_score_thresh;          /* 1.25 */
} mrgfe_inf_params;
void   mrgfe_inf_default_params(mrgfe_inf_params* out);
/* replaces InformationMatrixCalculator::weight (information_matrix_calculator.cpp:83-88) */
double mrgfe_inf_weight(double a, double max_x, double min_y, double max_y, double x);
/* the 6x6 information matrix (row-major) of a graph edge from its fitness score: :19-24 (constant) / :30-43 (weights) */
int    mrgfe_inf_matrix_from_fitness(const mrgfe_inf_params* params, double fitness_score, double inf[36]);
/* replaces InformationMatrixCalculator::calc_information_matrix(cloud1, cloud2, relpose) (:14-44; call sites
 * src/mrg_slam/graph_database.cpp:139-142 for every odometry edge, :579-581 for every loop edge): fitness score with the header's
 * default max_range (DBL_MAX), then the weights.  fitness_out (may be NULL) receives the score. */
int    mrgfe_calc_information_matrix(mrgfe_ctx* ctx, const mrgfe_inf_params* params, const float* cloud1, size_t n1, const float* cloud2, size_t n2, size_t stride_bytes,
                                     const double relpose[16], double inf[36], double* fitness_out);

/* ---- per-point passes around the path ------------------------------------------------ */
/* replaces MapCloudGenerator::generate (src/mrg_slam/map_cloud_generator.cpp:14-86) including its
 * pcl::ApproximateMeanVoxelGrid pass (include/pcl/filters/ApproximateMeanVoxelGrid.hpp:63-126): every keyframe cloud is
 * moved by its pose (poses: n_keyframes column-major 4x4 doubles, Eigen::Isometry3d::matrix()), points farther than
 * distance_far_thresh (if > 0) from their sensor are dropped, the union is voxel-filtered (true mean of x, y, z,
 * intensity per voxel of edge `resolution`, voxels with fewer than min_points_per_voxel points dropped; resolution <= 0
 * returns the unfiltered union).  first_keyframe (may be NULL) marks the clouds skip_first_cloud leaves out.
 * Output order: ascending voxel index (z, y, x) — the reference emits boost::unordered_map order, which is unspecified.
 * Returns MRGFE_ERR_EMPTY where the reference returns nullptr (no keyframes; or nothing left although n_keyframes > 1),
 * MRGFE_ERR_INVALID with *out_n = needed points when capacity is too small. */
int mrgfe_map_cloud_generate(mrgfe_ctx* ctx, int n_keyframes, const float* const* clouds_xyzi, const size_t* n_points, size_t stride_bytes, const double* poses,
                             const uint8_t* first_keyframe, float resolution, int min_points_per_voxel, float distance_far_thresh, int skip_first_cloud,
                             float* out_xyzi, size_t capacity, size_t* out_n);
/* The same over keyframe clouds that stay in HBM.  The map is regenerated from ALL keyframes whenever it is published or
 * saved (apps/mrg_slam_component.cpp:727,781,1097) and only their poses change between calls (graph optimisation), while
 * the reference walks the host clouds every time.  A map store keeps each keyframe's packed cloud resident (append-only,
 * 16 B/point, no cap: the keyframes of a session fit 288 GB many times over); generate() then moves K poses instead of
 * the clouds.  Same output as mrgfe_map_cloud_generate for the same keyframes in the same order. */
typedef struct mrgfe_map_store mrgfe_map_store;
int    mrgfe_map_store_create(mrgfe_ctx* ctx, mrgfe_map_store** out);
void   mrgfe_map_store_destroy(mrgfe_map_store* store);
/* adds keyframe `key` (non-zero); adding a key again with the same point count is a no-op, with another count an error */
int    mrgfe_map_store_add(mrgfe_map_store* store, uint64_t key, const float* xyzi, size_t n, size_t stride_bytes);
int    mrgfe_map_store_has(const mrgfe_map_store* store, uint64_t key, size_t* n);
size_t mrgfe_map_store_bytes(const mrgfe_map_store* store);
int    mrgfe_map_store_generate(mrgfe_map_store* store, int n_keyframes, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe, float resolution,
                                int min_points_per_voxel, float distance_far_thresh, int skip_first_cloud, float* out_xyzi, size_t capacity, size_t* out_n);

/* ---- the map as the message or file its three callers make of it, and stored keyframes read back ---- */
/* update_map_cloud_msg (apps/mrg_slam_component.cpp:712-740), publish_map_service (:764-796) and save_map_service (:1078-1144) run
 * MapCloudGenerator::generate and then pcl::toROSMsg, or the two `+=` offset passes (:1104-1116) and pcl::io::savePCDFileBinary, over every map point.
 * mrgfe_map_store_publish is mrgfe_map_store_generate for the same keys, poses, flags and parameters — the same points in the same order (ascending
 * (z, y, x) cell) with the same bits, the same MRGFE_ERR_EMPTY rules — followed, ON THE DEVICE and in the kernel that writes the final points (the
 * scatter of the last compaction, or the copy of the unfiltered union), by
 *   the offsets: n_offsets separate f32 additions per coordinate, in the order given, after the voxel filter as :1106-1115 apply them;
 *   the record:  point_step 32: x, y, z, 1.0f, intensity, 0, 0, 0 — the pcl::PointXYZI of the reference in memory, which toROSMsg copies as it is;
 *                point_step 16: x, y, z, intensity — the body of the binary PCD.
 * Only the records come down.  The message's other members are the caller's: width = n_points, height 1, row_step = data_bytes, is_dense false,
 * little endian, fields x@0 y@4 z@8 intensity@off_intensity, all FLOAT32. */
typedef struct mrgfe_map_publish_params {   /* config/mrg_slam.yaml:235-237; SaveMap / PublishMap requests            */
    float   resolution;                     /* 0.1; <= 0: the unfiltered union (map_cloud_generator.cpp:66-70)       */
    int32_t min_points_per_voxel;           /* 1                                                                     */
    float   distance_far_thresh;            /* 10000.0; <= 0: no cut (:27)                                           */
    int32_t skip_first_cloud;               /* 0                                                                     */
    int32_t point_step;                     /* 32: pcl::toROSMsg records; 16: packed x, y, z, intensity (PCD body)   */
    int32_t n_offsets;                      /* 0..2: zero_utm, then zero_enu (mrg_slam_component.cpp:1104-1116)      */
    float   offsets[6];                     /* each already cast to float, x y z                                     */
} mrgfe_map_publish_params;                 /* 48 bytes */
typedef struct mrgfe_map_publish_result {
    uint64_t n_points, n_unfiltered, data_bytes;   /* width; points before the voxel filter; n_points * point_step   */
    int32_t  point_step, off_intensity;            /* 32 / 16; 16 / 12                                               */
} mrgfe_map_publish_result;                 /* 32 bytes */
void   mrgfe_map_publish_default_params(mrgfe_map_publish_params* out); /* 0.1, 1, 10000, 0, point_step 32, no offsets */
size_t mrgfe_map_publish_params_size(void); /* sizeof(mrgfe_map_publish_params) as the library was compiled */
size_t mrgfe_map_publish_result_size(void); /* sizeof(mrgfe_map_publish_result) as the library was compiled */
/* data: room for capacity_bytes.  MRGFE_ERR_INVALID: a NULL argument; point_step other than 16 or 32; n_offsets outside 0..2; a key the store lacks
 * (before any launch; a first keyframe that skip_first_cloud leaves out is not looked up, as in mrgfe_map_store_generate); capacity_bytes too small —
 * then out->n_points and out->data_bytes say what is needed and `data` is untouched.  MRGFE_ERR_EMPTY: as mrgfe_map_store_generate.
 * The working buffers and the records live in a grow-only workspace of the store (freed with it) and in the context's scratch buffers: a call whose
 * sizes do not exceed an earlier call's allocates and frees no device memory.  The store's keyframes are only read. */
int    mrgfe_map_store_publish(mrgfe_map_store* store, int n_keyframes, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe,
                               const mrgfe_map_publish_params* params, void* data, size_t capacity_bytes, mrgfe_map_publish_result* out);
/* The same, with the records left in the store's workspace: *d_data (NULL for 0 points) is device memory of the store's GPU, complete when the call
 * returns (the hand-over rule of the other `_device` producers) and valid until the next publish, read or destroy on this store. */
int    mrgfe_map_store_publish_device(mrgfe_map_store* store, int n_keyframes, const uint64_t* keys, const double* poses, const uint8_t* first_keyframe,
                                      const mrgfe_map_publish_params* params, const void** d_data, mrgfe_map_publish_result* out);
/* The stored clouds of `keys` as records, back to back in list order — what KeyFrame::save (src/mrg_slam/keyframe.cpp:109, the PCD body: point_step 16)
 * and the cloud_msg of publish_graph_service (keyframe.cpp:200, apps/mrg_slam_component.cpp:434: point_step 32) are made of, so the host need not keep
 * a second copy of every keyframe.  offsets_bytes (n_keys + 1 entries): where keyframe i begins, and the total.  A key may repeat; a keyframe of 0
 * points is an empty range.  point_step 16: copies out of the store, no kernel; point_step 32: ONE launch over a tile table for the whole list.  Either
 * way ONE host wait.  MRGFE_ERR_INVALID: a NULL argument, another point_step, a key the store lacks (nothing is written, offsets_bytes included), more
 * than 2^31 - 1 points, capacity_bytes too small (offsets_bytes is filled, `data` untouched). */
int    mrgfe_map_store_read(mrgfe_map_store* store, int n_keys, const uint64_t* keys, int point_step, void* data, size_t capacity_bytes, uint64_t* offsets_bytes);
/* What the last publish / read on the store did: out[0] kernel launches of its record stage (publish: the record kernel and, where points are dropped,
 * the three of the scan in front of it — the generator's passes before them are not counted; read: all of the call's), out[1] host waits of the whole
 * call, out[2] bytes brought down, out[3] device bytes the workspace and the context's scratch buffers grew by. */
int    mrgfe_map_store_egress_stats(const mrgfe_map_store* store, int64_t out[4]);

/* The same two calls for keyframes that already sit in a map store: a graph edge names its two keyframes, so
 * neither cloud is uploaded again, and the exact-NN grid of key1's cloud is kept for the next edges of that keyframe (the
 * reference builds a fresh kd-tree over cloud1 for every edge: information_matrix_calculator.cpp:51-52). */
int mrgfe_map_store_fitness(mrgfe_map_store* store, uint64_t key1, uint64_t key2, const double relpose[16], double max_range, double* out);
int mrgfe_map_store_information_matrix(mrgfe_map_store* store, const mrgfe_inf_params* params, uint64_t key1, uint64_t key2, const double relpose[16], double inf[36],
                                       double* fitness_out);

/* replaces the other-robot point removal of apps/mrg_slam_component.cpp:396-429: drops every point whose squared float
 * distance to one of the centres (sensor frame, <= 64) is < radius_sqr; kept / removed (may be NULL) keep the input order */
int mrgfe_remove_points_near(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, const float* centres_xyz, int n_centres, float radius_sqr,
                             float* kept_xyzi, size_t* n_kept, float* removed_xyzi, size_t* n_removed);
/* ---- the keyframe callback in one call (MrgSlamComponent::cloud_callback, apps/mrg_slam_component.cpp:358-456, once KeyframeUpdater::update said yes) ---- */
/* pcl::fromROSMsg (:372) -> the other-robot point removal (:396-430) -> the keyframe's cloud (:446) on the byte payload of a sensor_msgs/PointCloud2,
 * with the kept cloud left in the map store as keyframe `key`: the payload goes up ONCE as it is, one kernel reads the records, stores the packed cloud
 * and flags every point inside a sphere (the test of mrgfe_remove_points_near), a second one splits the cloud into kept and removed points in input
 * order, and the kept cloud is where mrgfe_map_store_generate / _fitness / _information_matrix and the mrgfe_batch_*_from_store calls below read it.
 * Kept and removed clouds and both counts equal, bit for bit and in order, mrgfe_ingest_pointcloud2 -> mrgfe_remove_points_near for the same inputs.
 * The layout of the message, as for mrgfe_ingest_pointcloud2 / mrgfe_scan_params: */
typedef struct mrgfe_keyframe_params {
    uint32_t width, height, point_step, row_step;   /* row_step 0: width * point_step                                      */
    uint32_t off_x, off_y, off_z;                   /* little-endian FLOAT32 fields inside point_step; offsets and steps multiples of 4 unless
                                                     * the store's context has mrgfe_ctx_set_byte_layouts on                 */
    int32_t  off_intensity;                         /* < 0: no such field, intensity 0                                     */
} mrgfe_keyframe_params;
/* height 1, the packed 16-byte layout (offsets 0/4/8/12); `width` is left 0 for the caller */
void   mrgfe_keyframe_default_params(mrgfe_keyframe_params* out);
size_t mrgfe_keyframe_params_size(void); /* sizeof(mrgfe_keyframe_params) as the library was compiled */
/* `data`: data_bytes >= (height - 1) * row_step + width * point_step bytes of the message (less is MRGFE_ERR_INVALID); centres_xyz: n_centres <= 64
 * positions in the sensor frame (NULL with n_centres 0: nothing is removed, the kernel is a plain gather into the store and nothing has to come down —
 * the reference keeps the original message there, :396,436); kept_xyzi / removed_xyzi: room for width * height packed 16-byte points each, either may
 * be NULL (not downloaded; the counts are still returned); n_removed may be NULL.  mrgfe_map_store_bytes grows by exactly 16 * *n_kept.
 * The call returns only after the store's stream has been waited for (at most twice: the counts, then the downloads; once without centres), so the
 * stored cloud is complete and immutable for every other stream.  MRGFE_ERR_INVALID: key 0, more than 64 centres, a bad layout, a short payload;
 * MRGFE_ERR_STATE: `key` is already stored.  After any failure the store has no new entry and its byte count is unchanged. */
int    mrgfe_keyframe_callback(mrgfe_map_store* store, uint64_t key, const mrgfe_keyframe_params* layout, const void* data, size_t data_bytes,
                               const float* centres_xyz, int n_centres, float radius_sqr, float* kept_xyzi, size_t* n_kept, float* removed_xyzi,
                               size_t* n_removed);
/* The same callback for a filtered scan that is already in HBM — all four components in one component_container_mt (launch/mrg_slam.launch.py:214-319):
 * the cloud that becomes a keyframe (apps/mrg_slam_component.cpp:372 would unpack it from the message) is the packed float4 cloud
 * mrgfe_scan_callback_device / mrgfe_prefilter_device left in the caller's buffer.  d_xyzi: n packed 16-byte points in the memory of the store's
 * device, COMPLETE when the call is made — the `_device` producers of this header return only after their wait, so a buffer one of them filled is;
 * work the caller queued on a stream of its own must have been waited for.  A packed device cloud is a PointCloud2 payload with point_step 16 that
 * already sits where the head kernel reads it: this is mrgfe_keyframe_callback without its upload — the same two kernels, the same arena block, the
 * same waits (with 0 centres one gather into the store and one wait) — and stored cloud, kept, removed, both counts, mrgfe_map_store_bytes and the
 * refusals equal mrgfe_keyframe_callback on the bytes of the same cloud in the packed layout.  The caller's buffer is only read and is free on return.
 * MRGFE_ERR_INVALID: key 0, more than 64 centres, n > 2^31 - 1, a NULL d_xyzi with n > 0, and a d_xyzi that hipPointerGetAttributes does not show to
 * be memory of the store's device (host memory, another GPU's: it is not read); MRGFE_ERR_STATE: `key` is already stored.  After any failure the store
 * has no new entry and its byte count is unchanged. */
int    mrgfe_keyframe_callback_device(mrgfe_map_store* store, uint64_t key, const void* d_xyzi, size_t n, const float* centres_xyz, int n_centres,
                                      float radius_sqr, float* kept_xyzi, size_t* n_kept, float* removed_xyzi, size_t* n_removed);
/* The callback to its two publishes: the keyframe's cloud_msg_filtered (pcl::toROSMsg of the kept cloud, apps/mrg_slam_component.cpp:432-435) and
 * other_robots_removed_points (:437-443) come down as the `data` of those messages, written on the device — point_step 32 or 16, the two layouts of
 * mrgfe_scan_callback_records, the same destination rule per sink (the removed cloud's staging and statistics are the second sink's:
 * mrgfe_ctx_second_egress_stats).  The stored cloud, both counts, mrgfe_map_store_bytes, the refusals and "no new entry after a failure" are
 * mrgfe_keyframe_callback[_device]'s; the records hold the points of that call's kept_xyzi / removed_xyzi, same order, same bits.
 * kept_records / removed_records: room for width * height (device form: n) records each; either may be NULL (not written; the counts are still returned);
 * only the first *n_kept / *n_removed records are ever written.  One record kernel runs directly behind the partition over the two compacted clouds — the
 * stored cloud and the removed points — in ONE launch: at most the two waits of mrgfe_keyframe_callback (the counts, then the records).
 * n_centres == 0: nothing is removed and the reference keeps the original message (:396,436): *n_removed = 0, and a kept_records sink still receives the
 * whole cloud as records (one gather, one record launch, one wait).
 * MRGFE_ERR_INVALID, nothing launched, no new entry: what mrgfe_keyframe_callback[_device] refuses, a point_step other than 16 or 32 (when a sink is given),
 * a capacity below width * height * point_step of a sink that is given, a NULL n_kept. */
int    mrgfe_keyframe_callback_records(mrgfe_map_store* store, uint64_t key, const mrgfe_keyframe_params* layout, const void* data, size_t data_bytes,
                                       const float* centres_xyz, int n_centres, float radius_sqr, int point_step, void* kept_records, size_t kept_capacity_bytes,
                                       size_t* n_kept, void* removed_records, size_t removed_capacity_bytes, size_t* n_removed);
int    mrgfe_keyframe_callback_records_device(mrgfe_map_store* store, uint64_t key, const void* d_xyzi, size_t n, const float* centres_xyz, int n_centres,
                                              float radius_sqr, int point_step, void* kept_records, size_t kept_capacity_bytes, size_t* n_kept,
                                              void* removed_records, size_t removed_capacity_bytes, size_t* n_removed);

/* ---- the graph database's keyframe and edge loops in one call each (src/mrg_slam/graph_database.cpp) ---- */
/* Many keyframe messages at once: the point work of GraphDatabase::add_static_keyframes (:181-182), flush_graph_queue (:294-295, another robot's whole
 * graph at a rendezvous) and load_graph (:449-461), which unpack one sensor_msgs/PointCloud2 per keyframe in a loop (pcl::fromROSMsg); none of the
 * three removes other robots' points.  Message i becomes keyframe msgs[i].key; layouts (checked as mrgfe_keyframe_callback checks them) may differ
 * from message to message.  Known keys follow mrgfe_map_store_add, which is the reference's rule (:173-178, :272-274): a key that is already stored,
 * or comes a second time inside the call, with the same point count is skipped (added[i] = 0); with another count the call fails with
 * MRGFE_ERR_STATE; key 0, a bad layout, NULL data or a short payload: MRGFE_ERR_INVALID, naming the message.  The new clouds take ONE block of the
 * store's arena, the payloads go up behind one another through the staging ring, ONE launch gathers all of them (a tile table in device memory names
 * every 2048-point tile's message) and the stream is waited for ONCE.  After any failure the store has no new entry, mrgfe_map_store_bytes is
 * unchanged and `added` (n bytes, may be NULL) is all 0; after success the store has grown by exactly 16 * the points added, and every stored cloud
 * equals, bit for bit, what mrgfe_keyframe_callback with 0 centres stores for the same message. */
typedef struct mrgfe_keyframe_msg {
    uint64_t              key;
    mrgfe_keyframe_params layout;
    const void*           data;        /* data_bytes >= (height - 1) * row_step + width * point_step */
    size_t                data_bytes;
} mrgfe_keyframe_msg;
size_t mrgfe_keyframe_msg_size(void); /* sizeof(mrgfe_keyframe_msg) as the library was compiled */
int    mrgfe_map_store_add_keyframes(mrgfe_map_store* store, int n, const mrgfe_keyframe_msg* msgs, uint8_t* added);
/* Many graph edges at once: InformationMatrixCalculator::calc_information_matrix (information_matrix_calculator.cpp:14-44, max_range = DBL_MAX as
 * :24 has it) for every edge of GraphDatabase::flush_keyframe_queue (:139-142, up to max_keyframes_per_update odometry edges per tick) or
 * insert_loops (:579-581).  Edge e: cloud1 = keyframe key1, cloud2 = keyframe key2, relpose column-major (Isometry3d::matrix()); inf receives 36
 * doubles per edge (row-major 6x6), fitness (may be NULL) the scores.  use_const_inf_matrix touches no GPU and needs no key to exist (nor a store).
 * Otherwise a key the store does not hold gives MRGFE_ERR_INVALID, names the key and writes nothing; an empty cloud on either side gives the score
 * DBL_MAX and whatever mrgfe_inf_matrix_from_fitness makes of it.  The distinct key1 clouds without a usable search grid get theirs from ONE grouped
 * build (three stream waits for the set, not per cloud), all edges are scored by ONE batch of the fitness passes (one wait), and the matrices come
 * from mrgfe_inf_matrix_from_fitness on the host.  Scores and matrices are those of mrgfe_map_store_information_matrix edge by edge.
 * Which grids outlive the call: a grid in the 8-entry cache of mrgfe_map_store_fitness is used where it fits (and counts as used) but the call adds
 * none to it; the grids it builds are kept as ONE set until the next call that has to build — so insert_loops after flush_keyframe_queue in the same
 * tick finds the new keyframes' grids, and a call all of whose key1 are in the cache or in that set builds nothing.  Results do not depend on it. */
typedef struct mrgfe_graph_edge {
    uint64_t key1, key2;
    double   relpose[16];
} mrgfe_graph_edge;
size_t mrgfe_graph_edge_size(void); /* sizeof(mrgfe_graph_edge) as the library was compiled */
int    mrgfe_map_store_edges(mrgfe_map_store* store, const mrgfe_inf_params* params, int n_edges, const mrgfe_graph_edge* edges, double* inf, double* fitness);

/* ---- the ground fill of the first keyframe (GraphDatabase::flush_keyframe_queue, src/mrg_slam/graph_database.cpp:114-129; src/pcl/fill_ground_plane.cpp) ---- */
/* With enable_fill_first_cloud the reference replaces the first keyframe's cloud by cloud_filled: the cloud plus a disc of synthetic ground points
 * (intensity 0) under the robot, appended behind the cloud's own points, rings outermost and angles inner (fill_cloud, fill_ground_plane.cpp:49-65).
 * The plane of the disc:
 *   simple == 0  fill_ground_plane_ransac (:21-35): RandomSampleConsensus<SampleConsensusModelPlane> over the WHOLE cloud, distance threshold 0.01,
 *                computeModel() only — the coefficients of the winning sample, nothing refined; the RANSAC of mrgfe_floor_detect with that threshold.
 *                normal = (double)c[0..2], offset = (double)c[3].  `estimate` is ignored.
 *   simple != 0  fill_ground_plane_simple (:37-47): normal = the third column of the rotation of keyframe->node->estimate(), offset 0.  `estimate`:
 *                that pose, column-major 4x4 double; NULL is MRGFE_ERR_INVALID.
 * The disc, all in double: angle_inc = map_resolution / radius; rings `for (r = map_resolution; r <= radius; r += map_resolution)` and angles
 * `for (angle = 0; angle < 2 * M_PI; angle += angle_inc)`, both ACCUMULATED as written (resolution 0.1 with radius 0.3 gives 2 rings: 0.1 + 0.1 + 0.1 >
 * 0.3); per ring sample = p - (normal . p + offset) * normal with p = (r, 0, 0) (Eigen::Hyperplane::projection: the normal is not normalised); per point
 * AngleAxis<double>(angle, normal).toRotationMatrix() * sample — the axis as it is given, the rotation about the axis THROUGH THE ORIGIN, as the reference
 * has it — cast to float.  The host walks the two loops and takes sin and cos of every angle from the C library, as the reference's host does; the device
 * does the rest in IEEE double operations in a fixed order (three-term sums left to right), so no device sin / cos enters the result.
 * config/mrg_slam_ouster.yaml:158-160 ships the fill ON (radius 7.5, RANSAC): at the declared map_cloud_resolution 0.05 that is 150 rings x 943 angles =
 * 141450 points. */
typedef struct mrgfe_ground_fill_params {
    double  radius;          /* 5.0   "fill_first_cloud_radius"  apps/mrg_slam_component.cpp:271, config/mrg_slam.yaml:159  */
    double  map_resolution;  /* 0.05  "map_cloud_resolution"     apps/mrg_slam_component.cpp:245 (the YAMLs set 0.1, :235) */
    int32_t simple;          /* 0     "fill_first_cloud_simple"  apps/mrg_slam_component.cpp:272, config/mrg_slam.yaml:160  */
    int32_t pad;
} mrgfe_ground_fill_params;  /* 24 bytes */
typedef struct mrgfe_ground_fill_result {
    int32_t  has_model;          /* a plane was found: always 1 with simple != 0; 0 when RANSAC found none — then nothing was filled                  */
    int32_t  ransac_iterations;  /* RandomSampleConsensus::iterations_ at the end of computeModel (0 with simple != 0)                              */
    float    coeffs[4];          /* RANSAC: the model coefficients; simple: the normal rounded to float and 0 (the fill itself uses the doubles)     */
    uint32_t n_before;           /* points of the source cloud                                                                                      */
    uint32_t n_rings, n_angles;  /* the two loop counts                                                                                             */
    uint32_t n_added;            /* n_rings * n_angles, or 0 without a model                                                                        */
} mrgfe_ground_fill_result;      /* 40 bytes */
void   mrgfe_ground_fill_default_params(mrgfe_ground_fill_params* out); /* 5.0, 0.05, 0: apps/mrg_slam_component.cpp:245,271-272 */
size_t mrgfe_ground_fill_params_size(void); /* sizeof(mrgfe_ground_fill_params) as the library was compiled */
size_t mrgfe_ground_fill_result_size(void); /* sizeof(mrgfe_ground_fill_result) as the library was compiled */
/* The two loop counts alone, on the host, no context.  MRGFE_ERR_INVALID: a NULL argument; a radius or map_resolution that is not finite and > 0 (the
 * reference's loops would not terminate); more than 2^31 - 1 points.  radius < map_resolution is a valid fill of 0 rings. */
int    mrgfe_ground_fill_counts(const mrgfe_ground_fill_params* params, uint32_t* n_rings, uint32_t* n_angles);
/* The fill of a host cloud (`stride_bytes` as for mrgfe_map_store_add): out_xyzi (required, room for `capacity` packed 16-byte points) receives the n
 * points of the cloud, packed, and the disc behind them.
 * Outcomes, for this call and the next:
 *   MRGFE_OK with has_model = 0, n_added = 0: RANSAC found no model (fewer than 3 points, no non-collinear sample).  Nothing is written to out_xyzi and
 *     the store gets NO dst_key entry.  (The reference would index an empty coefficient vector here: ransac.getModelCoefficients(c) leaves c empty and
 *     :31 reads c[0..3].)
 *   MRGFE_OK with n_rings = 0 (radius < map_resolution): a valid fill of 0 points; the output is a copy of the cloud.
 *   MRGFE_ERR_INVALID: a NULL argument (`estimate` may be NULL with simple == 0; the store call's out_xyzi may be NULL); radius or map_resolution not
 *     finite and > 0; n + n_rings * n_angles > 2^31 - 1; key 0; a src_key the store lacks; capacity < n + n_rings * n_angles (the message names the count;
 *     checked before any work, so also where RANSAC would have found no model).
 *   MRGFE_ERR_STATE: dst_key is already stored, or equals src_key.
 * One host wait with simple != 0; with RANSAC those of its waves (one per wave of hypotheses) plus one. */
int    mrgfe_fill_ground_plane(mrgfe_ctx* ctx, const mrgfe_ground_fill_params* params, const double estimate[16], const float* xyzi, size_t n, size_t stride_bytes,
                               float* out_xyzi, size_t capacity, mrgfe_ground_fill_result* result);
/* The same for keyframe src_key of a map store, which is where mrgfe_keyframe_callback left the first keyframe's cloud.  The filled cloud is stored as a
 * NEW keyframe dst_key — the integrator names the first keyframe by dst_key from then on (`keyframe->cloud = cloud_filled`, :125) — and src_key stays as
 * it was: the store stays append-only, no device pointer handed out earlier (batch targets, node replicas, cached edge grids) changes or dangles, and
 * nothing needs invalidating.  The source points reach the new cloud by a device-to-device copy on the store's stream, the disc by one launch behind
 * them.  out_xyzi (may be NULL; else room for `capacity` points) receives the filled cloud.  mrgfe_map_store_bytes grows by exactly
 * 16 * (n_before + n_added).  The call returns after the store's stream has been waited for: the new cloud is complete and immutable.  After any failure,
 * and without a model, the store has no new entry and its byte count is unchanged (the arena block is handed back). */
int    mrgfe_map_store_fill_ground(mrgfe_map_store* store, uint64_t src_key, uint64_t dst_key, const mrgfe_ground_fill_params* params, const double estimate[16],
                                   float* out_xyzi, size_t capacity, mrgfe_ground_fill_result* result);

/* replaces PrefilteringComponent::deskewing (apps/prefiltering_component.cpp:231-292): point i is rotated by the inverse of
 * Quaternionf(1, dt/2 * -w) with dt = scan_period * i / n and w the IMU angular velocity */
int mrgfe_deskew(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, const float ang_v_xyz[3], double scan_period, float* out_xyzi);
/* replaces pcl_ros::transformPointCloud(*src_cloud, *transformed, transform) of PrefilteringComponent::cloud_callback
 * (apps/prefiltering_component.cpp:141: the scan into base_link_frame) = pcl::transformPointCloud with the Matrix4f of the transform:
 * T column-major 4x4 float; non-finite points pass through unchanged, intensity is copied */
int mrgfe_transform_cloud(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, const float T[16], float* out_xyzi);

/* ---- the odometry frame in one call (ScanMatchingOdometryComponent::cloud_callback -> matching(), apps/scan_matching_odometry_component.cpp:138-150, 195-350) ----
 * A mrgfe_odom is the state of matching() — keyframe pose and stamp, prev_trans_, the rejection counter — over ONE mrgfe_reg it borrows (the registration
 * and its context outlive it; nothing else sets that registration's clouds while the handle is in use).  One mrgfe_odom_frame stands for pcl::fromROSMsg
 * (:144-145), downsample (:166-187), setInputTarget on a first frame (:197-205), else setInputSource, align(prev_trans * msf_delta) (:266), the status of
 * :268 when asked, the decisions of :270-339 (non-convergence, transform thresholding, the keyframe switch) and transformPointCloud(*cloud, odom) (:341-343).
 * The imu / robot-odometry prediction (:213-263) is TF and message handling and stays with the caller: its result is msf_delta.
 * Arithmetic of the state machine (csrc/odom_ctl.h): float 4x4 products row times column with every product and sum rounded to float; the thresholding
 * delta uses the rigid inverse (R^T, -R^T t) as mrgfe_status_poses forms it; norms in float, promoted; angles acosf of the clamped Quaternionf w. */
typedef struct mrgfe_odom mrgfe_odom;
typedef struct mrgfe_odom_params {                 /* :98-132, config/mrg_slam.yaml:77-95                                                       */
    int32_t downsample_method;                     /* 0 NONE (yaml default), 1 VOXELGRID, 2 APPROX_VOXELGRID                            :166-187 */
    float   downsample_resolution;                 /* 0.1                                                                                        */
    int32_t downsample_min_points_per_voxel;       /* 1 (VOXELGRID only)                                                                         */
    int32_t reserved0;
    double  keyframe_delta_translation, keyframe_delta_angle, keyframe_delta_time;   /* 1.0 m, 0.5236 rad, 10000 s                      :326-331 */
    int32_t enable_transform_thresholding, max_consecutive_rejections;               /* 0, 5                                            :278-315 */
    double  max_acceptable_translation, max_acceptable_angle;                        /* 1.0 m, 1.0 rad                                           */
    double  status_max_correspondence_dist;        /* 0.5                                                                                   :413 */
} mrgfe_odom_params;                               /* 72 bytes */
void   mrgfe_odom_default_params(mrgfe_odom_params* out);
size_t mrgfe_odom_params_size(void);               /* sizeof(mrgfe_odom_params) as the library was compiled */
/* MRGFE_ERR_INVALID: a NULL argument, an unknown downsample method, a resolution that is not > 0 with a downsample, max_consecutive_rejections < 1 with
 * thresholding on.  The handle is destroyed BEFORE its registration. */
int    mrgfe_odom_create(mrgfe_reg* reg, const mrgfe_odom_params* params, mrgfe_odom** out);
void   mrgfe_odom_destroy(mrgfe_odom* odom);
int    mrgfe_odom_reset(mrgfe_odom* odom);         /* forgets the keyframe: the next frame is a first frame (:197-205).  The registration is not touched. */
/* What the last completed frame's downsample did (needs no GPU; NULL arguments: MRGFE_ERR_INVALID): out[0] = its route — 0 none or the host-driven filter,
 * 1 device-driven (one wait), 2 device-driven attempted and handed back; out[1] = the anomaly word (mrgfe_ctx_prefilter_stats: 1 no finite point, 2 PCL's
 * "leaf size too small" pass-through, 4 no voxel); out[2] = points in; out[3] = points handed to the registration; out[4] = 1 if the source grid was built
 * in a box the frame handed over; out[5] = frames served device-driven so far. */
int    mrgfe_odom_stats(const mrgfe_odom* odom, int64_t out[6]);

enum mrgfe_odom_outcome {
    MRGFE_ODOM_FIRST_FRAME = 0,    /* :197-205: the cloud became the keyframe, odom = identity, nothing was aligned          */
    MRGFE_ODOM_ACCEPTED = 1,       /* :317-349                                                                               */
    MRGFE_ODOM_NOT_CONVERGED = 2,  /* :270-273: odom = keyframe_pose * prev_trans, nothing else changes                      */
    MRGFE_ODOM_REJECTED = 3,       /* :306-307: a large transform below the rejection limit                                  */
    MRGFE_ODOM_REJECTED_RESET = 4  /* :291-304: the rejection that reaches the limit: the frame becomes the keyframe         */
};
typedef struct mrgfe_odom_result {
    int32_t  outcome;              /* enum mrgfe_odom_outcome                                                                */
    int32_t  new_keyframe;         /* this frame's cloud became the keyframe (:203, :294-295, :332-333)                      */
    int32_t  consecutive_rejections, converged, iterations;
    uint32_t n_source;             /* points after the downsample                                                            */
    float    odom[16];             /* what matching() returns, column-major                                                  */
    float    keyframe_pose[16];    /* keyframe_pose_ as :323 reads it (before a switch made by this frame)                   */
    float    trans[16];            /* getFinalTransformation(); the identity on FIRST_FRAME                                  */
    int32_t  has_status, reserved; /* `status` is filled: want_status and the frame was aligned (:268)                       */
    mrgfe_matching_status status;
} mrgfe_odom_result;               /* 368 bytes */
size_t mrgfe_odom_result_size(void); /* sizeof(mrgfe_odom_result) as the library was compiled */

/* One frame from the message as it arrives (layout and payload as for mrgfe_keyframe_callback; an empty message is MRGFE_ERR_INVALID).
 *   First frame: the (downsampled) cloud becomes the registration's target; afterwards the registration is exactly where mrgfe_reg_set_target of that
 *     cloud leaves it (a target, the source untouched).
 *   Later frames: the cloud becomes the source, align(prev_trans * msf_delta) runs, the status is taken when want_status (before every decision, and
 *     against the keyframe the frame was aligned to), the decisions follow; when the frame becomes the keyframe the hand-over is that of
 *     mrgfe_reg_source_becomes_target (GICP family: nothing is recomputed; NDT builds its grid).  Non-convergence is an outcome, not an error.
 *   msf_delta: column-major 4x4 or NULL (the identity, :211).  aligned_xyzi (may be NULL): room for width * height packed points; on ACCEPTED it receives
 *     the WHOLE input cloud, before the downsample, moved by `odom` with the bits of mrgfe_transform_cloud(cloud, odom); other outcomes leave it untouched.
 *   The wire records go up once; one kernel gathers them straight into the buffer the registration takes over (the one mrgfe_reg_set_source uploads into)
 *     and finds the exact box of the finite points on the way, which the GICP family's source grid is built in (no bounding-box pass of its own).
 *     With a downsample the prefilter chain's downsample stage runs directly behind that kernel: the voxel parameters come from its per-tile boxes (device
 *     form: from a pass over the cloud), ONE wait brings down the kept count, the kept points' exact box, the finite count and an anomaly word, and that
 *     box serves the source grid when every kept point is finite; an anomaly (PCL's "leaf size too small" pass-through, no finite point, no voxel) goes
 *     through the host-driven filter, same result (mrgfe_odom_stats).  The stage leaves mrgfe_ctx_prefilter_stats and the remembered chain output alone.  The
 *     registration owns every cloud it keeps: `data` is free when the call returns, and a keyframe never aliases caller memory.
 *   A failing call (a bad layout, a short payload, a NULL argument: MRGFE_ERR_INVALID; a cloud with nothing left after the downsample: MRGFE_ERR_EMPTY; an
 *     alignment or target build that returns an error code: that code) leaves the handle's state and the registration's source and target as they were:
 *     the next good frame gives what it would have given without the failed call.  The context lock is held once for the whole call. */
int mrgfe_odom_frame(mrgfe_odom* odom, const mrgfe_keyframe_params* layout, const void* data, size_t data_bytes, double stamp_seconds, const float* msf_delta,
                     int want_status, float* aligned_xyzi, mrgfe_odom_result* out);
/* the same for a packed cloud already in HBM on the registration's device (n > 0 points of 16 bytes; the output of mrgfe_scan_callback_device): it is copied
 * device to device into the registration's buffer, so the caller may overwrite d_xyzi as soon as the call returns.  When d_xyzi / n are what the last
 * device-driven prefilter chain on the SAME context left (the rule of mrgfe_reg_set_source_from_prefilter) the source grid is built in the chain's box;
 * otherwise the registration's own bounding-box pass runs. */
int mrgfe_odom_frame_device(mrgfe_odom* odom, const void* d_xyzi, size_t n, double stamp_seconds, const float* msf_delta, int want_status, float* aligned_xyzi,
                            mrgfe_odom_result* out);
/* The frame to its publish: scan_matching_odometry/aligned_points, pcl::transformPointCloud(*cloud, *aligned, odom) and pcl::toROSMsg
 * (apps/scan_matching_odometry_component.cpp:341-347).  Everything about the frame is mrgfe_odom_frame[_device], field for field: state, decisions,
 * hand-over, failure atomicity, mrgfe_odom_stats.  On MRGFE_ODOM_ACCEPTED aligned_records receives the WHOLE input cloud, before the downsample, moved by
 * `odom`, as records of point_step 32 or 16 (the layouts and the destination rule of mrgfe_scan_callback_records) and *n_aligned = width * height (device
 * form: n); ONE kernel transforms and writes the records in one pass over the input cloud — no intermediate cloud, no copy command — and the call has the one
 * wait the aligned_xyzi path of mrgfe_odom_frame has.  The point bits are those of mrgfe_transform_cloud(cloud, odom): a non-finite point stays as it is,
 * the intensity is copied.  On every other outcome *n_aligned = 0 and the buffer is untouched.
 * MRGFE_ERR_INVALID with the state left as it was: a point_step other than 16 or 32, capacity_bytes < width * height * point_step, a NULL aligned_records or
 * n_aligned, and what mrgfe_odom_frame[_device] refuses. */
int mrgfe_odom_frame_records(mrgfe_odom* odom, const mrgfe_keyframe_params* layout, const void* data, size_t data_bytes, double stamp_seconds,
                             const float* msf_delta, int want_status, int point_step, void* aligned_records, size_t capacity_bytes, size_t* n_aligned,
                             mrgfe_odom_result* out);
int mrgfe_odom_frame_records_device(mrgfe_odom* odom, const void* d_xyzi, size_t n, double stamp_seconds, const float* msf_delta, int want_status, int point_step,
                                    void* aligned_records, size_t capacity_bytes, size_t* n_aligned, mrgfe_odom_result* out);

/* ---- batched candidate matching (LoopDetector::matching candidate loop, src/mrg_slam/loop_detector.cpp:126-145) ---- */
typedef struct mrgfe_pair_result {
    float   T[16];      /* final transformation, column-major                */
    double  H[36];      /* 6x6 Hessian of the last iteration, row-major      */
    double  fitness;    /* getFitnessScore(max_range); DBL_MAX if not computed */
    double  trans_probability;
    int32_t converged;
    int32_t iterations;
    int32_t evaluations;
    int32_t pair_id;
} mrgfe_pair_result; /* 384 bytes: the record the ranks all-gather over RCCL */

typedef struct mrgfe_batch mrgfe_batch;
/* A batch holds `n_targets` target clouds and `n_pairs` (target index, source cloud, guess) alignments.  NDT_HIP: they are
 * advanced together, one launch per derivative evaluation for all pairs still running.  GICP_HIP / SMALL_GICP_HIP / VGICP_HIP:
 * the candidates of a target share its covariances and correspondence grid or voxel map (computed once, like the single
 * setInputTarget of loop_detector.cpp:104), the source covariances are computed on a few parallel streams (or taken from the
 * keyframe store below), and the Levenberg-Marquardt loops of all pairs advance together.  ICP_HIP: the candidates of a target share
 * its exact-NN grid, and the ICP loops of all pairs advance in lock step — per round one correspondence + moment launch and one
 * reduction over the pairs still running, one host wait for their 17-sum records, one transform launch; no covariances are computed
 * and H of the records is all zero.  The records are those of a single ICP_HIP registration of the same pair, bit for bit.
 * PCL_GICP_HIP and PCL_GICP_OMP_HIP are offered for single registrations only, unless the context has mrgfe_ctx_set_bfgs_batches on.  Then: the
 * candidates of a target share its covariances (PCL's form) and correspondence grid, the source covariances are computed as for GICP_HIP (or taken
 * from the keyframe store), and the pairs' BFGS loops advance in lock step — per round the correspondence searches of the pairs that begin an outer
 * iteration, one cost / gradient launch and one sum launch (ONE workgroup per pair: the sums are chains in the reference's order) over the pairs still
 * running, one host wait for their 14-sum records.  H of the records is all zero, trans_probability 0, evaluations = functor evaluations + outer
 * iterations; the records are those of a single registration of the same pair, bit for bit.  mrgfe_batch_rounds counts the rounds. */
int  mrgfe_batch_create(mrgfe_ctx* ctx, const mrgfe_reg_params* params, mrgfe_batch** out);
void mrgfe_batch_destroy(mrgfe_batch* b);
int  mrgfe_batch_clear(mrgfe_batch* b);
/* Forgets the PAIRS and keeps the targets with everything built for them — NDT voxel grids, GICP target covariances and grids or voxel maps, ICP target
 * grids, getFitnessScore grids — and the device copies of the host clouds the batch uploaded.  The keyframe store, the epoch and mrgfe_batch_timing
 * behave as after mrgfe_batch_clear (stored keyframes stay, none is referenced by a pair; the next align's time starts here), except that the targets
 * stay referenced.  Pairs added afterwards may name the old target indices (an index out of range is refused as always), and the next
 * mrgfe_batch_align / _align_best / _async returns the records a fresh batch holding the same targets and those pairs returns, bit for bit, for every
 * batch method: a pair's sums depend on its own clouds and guess and on the pair list (the round plan's tiles per item), never on a target.  A target no pair names enters no launch and no NDT round plan.  This is what a
 * second matching stage against the same target is in the reference: registration_->setInputTarget(new_keyframe->cloud) happens ONCE per new keyframe
 * (loop_detector.cpp:104) before the candidate loop (:126-145) and the consistency alignments (:222-231, :265-274) alike. */
int  mrgfe_batch_clear_pairs(mrgfe_batch* b);
/* returns the target index (>= 0) or an error (< 0) */
int  mrgfe_batch_add_target(mrgfe_batch* b, const float* xyzi, size_t n, size_t stride_bytes);
int  mrgfe_batch_add_target_device(mrgfe_batch* b, const void* d_xyzi, size_t n);
/* returns the pair index (>= 0) or an error (< 0) */
int  mrgfe_batch_add_pair(mrgfe_batch* b, int target_index, const float* src_xyzi, size_t n, size_t stride_bytes, const float guess[16]);
int  mrgfe_batch_add_pair_device(mrgfe_batch* b, int target_index, const void* d_src_xyzi, size_t n, const float guess[16]);
/* n_targets device clouds and n_pairs alignments against them in one call — what a loop over mrgfe_batch_add_target_device /
 * mrgfe_batch_add_pair_device does (pair_target[i] indexes the targets of THIS call; guesses: n_pairs column-major 4x4).
 * Returns the index of the first pair added (the others follow in order) or an error (< 0). */
int  mrgfe_batch_add_device(mrgfe_batch* b, int n_targets, const void* const* d_targets, const size_t* target_points, int n_pairs, const int32_t* pair_target,
                            const void* const* d_sources, const size_t* source_points, const float* guesses);
/* Keyframe store.  The candidates of LoopDetector::matching are old keyframes that come back call after call
 * (loop_detector.cpp:66-100 selects them from the same pool for every new keyframe), while the reference hands their
 * clouds to setInputSource from host memory each time (:128).  A pair added with a non-zero `cloud_key` (the keyframe id)
 * keeps its packed cloud — and, for the GICP methods (not ICP_HIP, which has none), its k-NN covariances — resident in HBM inside the batch object,
 * across mrgfe_batch_clear: the next pair with the same key and point count uses them and `src_xyzi` may be NULL.
 * The store is bounded (MRGFE_KEYFRAME_STORE_MB, default 16384; least recently used keyframes not referenced by the
 * current batch are dropped first); mrgfe_batch_forget drops one key (0: all).  Results are identical to the unkeyed call. */
int  mrgfe_batch_add_pair_keyed(mrgfe_batch* b, int target_index, uint64_t cloud_key, const float* src_xyzi, size_t n, size_t stride_bytes,
                                const float guess[16]);
/* 1 if the store holds that key (a keyed add with the same point count may then pass NULL), else 0; *n = its point count */
int  mrgfe_batch_has_cloud(const mrgfe_batch* b, uint64_t cloud_key, size_t* n);
size_t mrgfe_batch_store_bytes(const mrgfe_batch* b);
int  mrgfe_batch_forget(mrgfe_batch* b, uint64_t cloud_key);
/* A target / a pair whose cloud is keyframe `key` of a map store (mrgfe_keyframe_callback, mrgfe_map_store_add) on the SAME device: the batch reads
 * the store's memory — nothing is uploaded or copied, the keyframe lives in HBM once.  The store is append-only, so the pointer stays valid; like
 * caller device memory handed to mrgfe_batch_add_*_device, the STORE MUST OUTLIVE the batch's use of it (destroy the batch, or clear it, first).
 * The key is looked up and the store's stream waited for under the store's lock alone (mrgfe_map_store_add uploads asynchronously), which is released
 * before the batch's lock is taken.  For the GICP methods (not ICP_HIP: nothing is cached, the batch's store is untouched) the pair is entered in the batch's keyframe store under `key` with an empty cloud: its k-NN
 * covariances are cached there as for mrgfe_batch_add_pair_keyed (mrgfe_batch_store_bytes counts the covariances only; mrgfe_batch_has_cloud does not
 * report such an entry), and mrgfe_batch_forget / mrgfe_batch_clear treat it like a keyed pair.  Records are those of the same batch fed from host
 * memory, bit for bit.  Return the target / pair index (>= 0) or an error (< 0): MRGFE_ERR_INVALID for a key the store does not hold or a store on
 * another device.  The node's form is mrgfe_node_add_target_from_store / _add_pair_from_store (below): a member on the store's device goes through these two
 * calls, a member on another device reads a replica it keeps of the keyframe. */
int  mrgfe_batch_add_target_from_store(mrgfe_batch* b, mrgfe_map_store* store, uint64_t key);
int  mrgfe_batch_add_pair_from_store(mrgfe_batch* b, int target_index, mrgfe_map_store* store, uint64_t key, const float guess[16]);
int  mrgfe_batch_set_guess(mrgfe_batch* b, int pair_index, const float guess[16]);
/* build every target grid (setInputTarget), then align every pair; fitness_max_range < 0 skips getFitnessScore */
int  mrgfe_batch_build_targets(mrgfe_batch* b);
int  mrgfe_batch_align(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results /* n_pairs */);
/* The same align on a worker thread of the batch's own: returns as soon as the worker holds the batch's context, mrgfe_batch_wait returns the align's
 * status (and sets mrgfe_last_error() in the waiting thread).  `results` must stay valid until then; every other call on this batch waits for the
 * align to finish.  A caller that keeps TWO batches on two contexts in flight — queue batch k + 1 while batch k aligns — fills one batch's target
 * build and straggler rounds with the other's derivative launches: config[1], 256 pairs per batch, 10.2 -> 9.3 ms per batch on one MI355X, same
 * records (a pair's record does not depend on what else runs on the chip).  One align in flight per batch: a second _async before _wait is
 * MRGFE_ERR_STATE. */
int  mrgfe_batch_align_async(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results /* n_pairs */);
int  mrgfe_batch_wait(mrgfe_batch* b);
int  mrgfe_batch_num_pairs(const mrgfe_batch* b);
/* Accounting of the NDT derivative kernel in the last mrgfe_batch_align / mrgfe_reg_align, per kind of evaluation
 * `mode` (0: score+gradient+Hessian, 1: score+gradient, 2: f64 Hessian; -1: all): device time in ms from HIP events recorded
 * around each launch on the context stream, launch count, and the algorithmic bytes of SURVEY.md §8(d): sum over launches and
 * active pairs of N_src*(16 + probes*8) + valid_neighbours*48.  With the default ONE launch per round for all kinds
 * (ndt_derivatives_all_kernel, see mrgfe_dbg_set_fused_launch) time and launch count are reported under mode 0 (and -1), the bytes
 * still per kind; with one launch per kind (ndt_derivatives_kernel<0|1|2,*>) everything is per kind.
 * For GICP_HIP registrations `mode` is ignored and the linearize kernel is reported. */
int  mrgfe_batch_kernel_stats(const mrgfe_batch* b, int mode, double* deriv_ms, int64_t* deriv_launches, double* deriv_alg_bytes);
int  mrgfe_reg_kernel_stats(const mrgfe_reg* reg, int mode, double* deriv_ms, int64_t* deriv_launches, double* deriv_alg_bytes);
/* source points and valid (point, voxel) pairs of the derivative evaluations the last mrgfe_batch_align launched: their ratio
 * is the k-bar of SURVEY.md §8(d) (evaluations answered from a controller's cache are not launched and not counted) */
int  mrgfe_batch_pair_counts(const mrgfe_batch* b, int mode, double* points, double* neighbours);
/* the longest timed derivative launch of the last mrgfe_batch_align: out[0] = device ms (HIP events), out[1..3] = pairs of each evaluation kind
 * (score+gradient+Hessian, score+gradient, f64 Hessian) busy in its round — the launch a rocprofv3 trace shows as the kernel's maximum
 * (diagnostic, like the two calls above: no reference counterpart) */
int  mrgfe_batch_largest_launch(const mrgfe_batch* b, double out[4]);
/* getFitnessScore passes of the last mrgfe_batch_align(fitness_max_range >= 0) of this batch, all launches added up (finished pairs are
 * scored in waves beside the remaining alignment rounds, the rest afterwards): the layout of mrgfe_ctx_fitness_stats, out[10] = launches. */
int  mrgfe_batch_fitness_stats(const mrgfe_batch* b, double out[11]);

/* ---- bounded best-candidate selection (loop_detector.cpp:126-145, the fitness_score_thresh gate :156-160) ---------------------------------
 * LoopDetector::matching consumes only the ARG-MIN of getFitnessScore over the converged candidates of one new keyframe:
 *     if( !registration_->hasConverged() || score > best_score ) continue;  best_score = score; best_matched = candidate; ...
 * mrgfe_batch_align_best aligns the batch exactly as mrgfe_batch_align does (T, H, trans_probability, converged, iterations, evaluations and
 * pair_id bit for bit) and then scores exactly only the candidates that can still win.  Every pair has a group, group[i] = -1 (scored exactly,
 * as mrgfe_batch_align would) or in [0, n_groups); within a group candidate order is pair order; groups need not be contiguous and may span
 * targets.  The block and seed passes of getFitnessScore give every pair a certified interval lower <= fitness <= upper (bit-valid: the same
 * slices and reduction tree as the exact sum over per-point bounds); a converged candidate whose lower bound is strictly above the least upper
 * bound in its group is PRUNED, one whose lower bound exceeds score_cap is ABOVE_CAP, and only the rest run the exact passes.
 * Per pair, fit_state[i] (nullable):
 *   MRGFE_FIT_EXACT      fitness is bit-identical to mrgfe_batch_align's;
 *   MRGFE_FIT_PRUNED     fitness holds a certified lower bound, strictly above the upper bound of a converged candidate of the same group;
 *   MRGFE_FIT_ABOVE_CAP  fitness holds a certified lower bound > score_cap;
 *   MRGFE_FIT_SKIPPED    not converged (grouped pairs), or an empty cloud: fitness = DBL_MAX.
 * INVARIANT: the candidate attaining the least upper bound of a group is never pruned and is scored exactly, and every pruned value is strictly
 * above its exact score, so the sequential rule (mrgfe_node_select_best, loop_closure.select_best, LoopDetector's best_of) returns the same winner
 * and score on these records as on mrgfe_batch_align's — for every group and for any union of groups.  A group that holds a NaN bound is scored
 * exactly throughout (the rule lets a NaN through and then accepts every later candidate).
 * best[g] / best_score[g]: the rule's result on the full path's records — a pair index, or -1 when the group has no converged candidate; ties go
 * to the LAST of equal scores, +inf never matches.  score_cap = DBL_MAX is off; otherwise best[g] = -2 exactly when the full rule's best score of a
 * group with a converged candidate exceeds the cap (fitness_score_thresh: no loop from that group in the reference either), best_score[g] then
 * being the least fitness in the group (> score_cap), and the result is identical to the full path's everywhere else.
 * fitness_max_range: as mrgfe_batch_align, >= 0 (else MRGFE_ERR_INVALID; so is a group id outside [-1, n_groups)).  With a finite range a pair
 * is pruned only when its counted point set is already certain.  One extra host wait per call.  No early fitness pass in this mode.
 * The asynchronous form is mrgfe_batch_align_best_async, the node's mrgfe_node_align_best (below). */
enum mrgfe_fit_state { MRGFE_FIT_EXACT = 0, MRGFE_FIT_PRUNED = 1, MRGFE_FIT_ABOVE_CAP = 2, MRGFE_FIT_SKIPPED = 3 };
int  mrgfe_batch_align_best(mrgfe_batch* b, double fitness_max_range, double score_cap, const int32_t* group /* n_pairs */, int n_groups,
                            mrgfe_pair_result* results /* n_pairs */, int32_t* fit_state /* n_pairs, nullable */, int32_t* best /* n_groups */,
                            double* best_score /* n_groups */);
/* the last mrgfe_batch_align_best: out[0..3] = pairs EXACT / PRUNED / ABOVE_CAP / SKIPPED, out[4] / out[5] = queries left to the sweep / the
 * pyramid walk after the selection, out[6] = host ms of the bound stage (block, seed, bound sums, selection), out[7] = of the contender stage */
int  mrgfe_batch_select_stats(const mrgfe_batch* b, double out[8]);
/* mrgfe_batch_align_best on the batch's worker thread, as mrgfe_batch_align_async runs mrgfe_batch_align: returns once the worker holds the batch's
 * context, mrgfe_batch_wait returns the align's status.  The arguments are checked in the calling thread, before anything is posted: the codes and texts
 * of mrgfe_batch_align_best, returned by this call.  `group` is copied here; results, fit_state (nullable), best and best_score must stay valid until
 * mrgfe_batch_wait has returned, which leaves in them what the synchronous call would, bit for bit.  One align in flight per batch: a second _async of
 * either kind before _wait is MRGFE_ERR_STATE and leaves the running align and its outputs alone. */
int  mrgfe_batch_align_best_async(mrgfe_batch* b, double fitness_max_range, double score_cap, const int32_t* group /* n_pairs */, int n_groups,
                                  mrgfe_pair_result* results /* n_pairs */, int32_t* fit_state /* n_pairs, nullable */, int32_t* best /* n_groups */,
                                  double* best_score /* n_groups */);

/* ---- LoopDetector::detect in one call over the map store (src/mrg_slam/loop_detector.cpp:15-303) -----------------------------------------
 * A mrgfe_loop is the state of a LoopDetector — the LoopManager (include/mrg_slam/loop_detector.hpp:39-115) and the counters of :22-34 — over ONE batch
 * and ONE map store it borrows (both outlive it and sit on one device; nothing else queues on that batch while a detect call runs).  One
 * mrgfe_loop_detect stands for the loop of :17-36 over the new keyframes: find_candidates (:41-95), matching (:97-180) with its candidate loop
 * (:126-145), the fitness gate (:156-160), the consistency check (:162-166, :190-303) and LoopManager::add_loop (:176), in the batched form of
 * mrg_slam_amd/loop_detector.py::detect_batched:
 *   1. the candidate supersets: :41-76 WITHOUT the LoopManager gates of :77-90 (the gates only remove candidates, and all of a SLAM instance or none);
 *   2. stage 1: ONE batch over all (new keyframe, candidate) pairs, one target per new keyframe that has pairs — mrgfe_batch_align, or with
 *      fitness_selection 1 mrgfe_batch_align_best grouped by (new keyframe, slam_id) and capped at fitness_score_thresh;
 *   3. the best match (:137-144: the last of equal scores wins, non-converged candidates never) of every subset of gated instances;
 *   4. mrgfe_batch_clear_pairs: the targets stay built;
 *   5. stage 2: the previous and next keyframe of those best matches against the same targets (:222-231, :265-274), no fitness;
 *   6. the replay, keyframe after keyframe, of :21-31 with the gates of :77-90, :137-144, :156-166 and :190-303 on the records — `prev` is tried before
 *      `next`, first and static keyframes are consistent without an alignment, a loop found for new keyframe k prunes the candidates of k + 1;
 *   7. add_loop for every loop.
 * Same loops as the sequential loop.  Clouds are named by map-store key alone (mrgfe_batch_add_target_from_store / _add_pair_from_store).  OUT OF SCOPE:
 * host clouds; the PCL_GICP_* methods (batches and nodes refuse them, and that stays).  mrgfe_loop_create_node (below, after mrgfe_node_*) runs the same
 * detector over the GPUs of a node: the two stages on a mrgfe_node fed by key from the store, everything else — handle, controller, validation — as here.
 * Arithmetic (csrc/loop_ctl.h): normalize_estimate and the guess in double, cast to float (:124,129-133,183-188; Isometry3d::inverse() is the rigid
 * inverse); the consistency deltas (:242-245, :285-291) with Matrix4f products, the general float inverse and Quaternionf::angularDistance. */
typedef struct mrgfe_loop mrgfe_loop;
typedef struct mrgfe_loop_params {                  /* config/mrg_slam.yaml:169-179                                                           */
    double  candidate_max_xy_distance;              /* 15.0                                                                          :60-65 */
    double  accum_distance_thresh_same_robot;       /* 15.0                                                                    :68-73,81-84 */
    double  accum_distance_thresh_other_robot;      /* 5.0                                                                           :85-89 */
    double  fitness_score_max_range;                /* +inf                                                                            :136 */
    double  fitness_score_thresh;                   /* 1.25                                                                        :156-160 */
    double  loop_closure_consistency_max_delta_trans;  /* 0.3 m                                                               :246,292 */
    double  loop_closure_consistency_max_delta_angle;  /* 0.0523599 rad                                                       :246,292 */
    int32_t fitness_selection;                      /* 0 full (mrgfe_batch_align), 1 bounded (mrgfe_batch_align_best): same loops             */
    int32_t use_planar_registration_guess;          /* 0                                                                           :131-133 */
    int32_t enable_loop_closure_consistency_check;  /* 1                                                                           :162,196 */
    int32_t reserved;
} mrgfe_loop_params;                                /* 72 bytes */
void   mrgfe_loop_default_params(mrgfe_loop_params* out);
size_t mrgfe_loop_params_size(void);                /* sizeof(mrgfe_loop_params) as the library was compiled */
typedef struct mrgfe_loop_keyframe {                /* the slice of KeyFrame the detector reads (include/mrg_slam/keyframe.hpp)                 */
    uint64_t key;                                   /* the map-store key of the cloud, non-zero                                                */
    uint64_t slam_id;                               /* any stable id of slam_uuid                                                              */
    double   estimate[16];                          /* node->estimate().matrix(), column-major                                                 */
    double   accum_distance;
    int32_t  first_keyframe, static_keyframe;
    uint64_t prev_key, next_key;                    /* prev_edge->to_keyframe / next_edge->from_keyframe (:213,256); 0: no such edge           */
    double   prev_relpose[16], next_relpose[16];    /* prev_edge->relative_pose() / next_edge->relative_pose() (:226,269), column-major        */
} mrgfe_loop_keyframe;                              /* 432 bytes */
size_t mrgfe_loop_keyframe_size(void);              /* sizeof(mrgfe_loop_keyframe) as the library was compiled */
typedef struct mrgfe_loop_result {                  /* a Loop (loop_detector.hpp:23-37)                                                        */
    uint64_t key1, key2;                            /* the new keyframe, the best matched candidate                                            */
    float    relative_pose[16];                     /* key1 -> key2: getFinalTransformation() of that pair, column-major, copied from its record */
    double   score;                                 /* its fitness score                                                                       */
} mrgfe_loop_result;                                /* 88 bytes */
size_t mrgfe_loop_result_size(void);                /* sizeof(mrgfe_loop_result) as the library was compiled */
/* MRGFE_ERR_INVALID: a NULL argument (batch and store may be NULL only once mrgfe_dbg_loop_set_aligner has replaced them, include/mrgfe_debug.h: a
 * detector created with both NULL refuses to detect until then), fitness_selection not 0 or 1.  The handle is destroyed BEFORE its batch and store. */
int    mrgfe_loop_create(mrgfe_batch* batch, mrgfe_map_store* store, const mrgfe_loop_params* params, mrgfe_loop** out);
void   mrgfe_loop_destroy(mrgfe_loop* det);
int    mrgfe_loop_reset(mrgfe_loop* det);           /* forgets the loops (the LoopManager) and the counters; the batch and the store are not touched */
/* keyframes: the keyframes of the graph in the reference's order (candidate order decides ties); new_keyframes: those that test for a loop (:17);
 * edge_keys: 2 keys per edge, the unordered pairs of KeyFrame::edge_exists (:55).  loops_out: room for `capacity` records, *n_loops the loops found.
 * MRGFE_ERR_INVALID, before anything is queued: a key 0; a prev_key / next_key of `keyframes` that appears in neither list; a key the store lacks
 * (named in mrgfe_last_error(); checked are the new keyframes that have candidates, their candidates, and the neighbours the consistency check can
 * reach); capacity too small (*n_loops = the loops found; then, after the alignments).  Any failing call — also a failing align — leaves the
 * LoopManager, the counters, mrgfe_loop_stats and mrgfe_loop_timing as they were.  With n_new == 0, no keyframes or no candidates the call returns
 * MRGFE_OK with 0 loops and touches no GPU. */
int    mrgfe_loop_detect(mrgfe_loop* det, int n_keyframes, const mrgfe_loop_keyframe* keyframes, int n_new, const mrgfe_loop_keyframe* new_keyframes, int n_edges,
                         const uint64_t* edge_keys /* 2 per edge */, mrgfe_loop_result* loops_out, int capacity, int* n_loops);
/* the last successful call (all 0 but out[3] when it had no candidates): out[0] superset pairs (stage 1), out[1] sequential pairs (the candidates the reference's loop would
 * have aligned), out[2] consistency pairs (stage 2), out[3] new keyframes, out[4] target_builds: the targets the two stages queued for building — the new
 * keyframes that had candidates, since stage 2 runs on the targets stage 1 built */
int    mrgfe_loop_stats(const mrgfe_loop* det, int64_t out[5]);
/* The reference's only performance counters (:22-34, written out as average_time_per_candidate_us by apps/mrg_slam_component.cpp:1032-1037), since
 * create / reset: loop_candidates_sizes and loop_detection_times (microseconds) per new keyframe that had candidates after the gates; a call's time is
 * shared out by candidate count.  candidates / micros: room for `capacity` entries each (may be NULL with capacity 0); *n the entries there are. */
int    mrgfe_loop_timing(const mrgfe_loop* det, int capacity, int32_t* candidates, int64_t* micros, int* n);
/* The arithmetic of :183-188 and of :124,129-133 alone, on the host, no context (as mrgfe_status_poses): normalize_estimate — linear() =
 * Quaterniond(linear()).normalized().toRotationMatrix() — and the guess (new_estimate.inverse() * normalize_estimate(candidate)).cast<float>(), its z
 * translation zeroed when planar (:131-133).  Matrices column-major; `in` and `out` may be the same array. */
int    mrgfe_loop_normalize_estimate(const double in[16], double out[16]);
int    mrgfe_loop_guess(const double new_estimate_normalized[16], const double candidate_estimate[16], int planar, float guess[16]);

/* ---- the same batch over the GPUs of one node ---------------------------------------------------------------------------
 * LoopDetector::matching runs in ONE host process per robot (src/mrg_slam/loop_detector.cpp:104,126-145 under mrg_slam_component's main
 * thread mutex): a node object lets that process reach every GPU of the machine through this header.  It owns one MEMBER per entry of
 * device_ids — a context, a batch and a host thread each; the same ordinal may appear several times (members sharing a card).
 * mrgfe_node_align cuts the declared pair list into n_members contiguous blocks whose sizes differ by at most one (the list is in the
 * reference's order — new keyframe after new keyframe, candidates in candidate order — so a block touches few distinct targets), every
 * member builds the targets and aligns the pairs of its block on its GPU (no data-path collective), and the 384-byte records are gathered
 * into `results` in pair order: with one ncclAllGather over the members' streams (RCCL over xGMI; librccl is loaded with dlopen) when there
 * are two or more members on distinct devices, through host memory otherwise (MRGFE_NODE_GATHER=host / rccl forces either).  The records —
 * and so the best candidates — are those of ONE batch holding the whole list, bit for bit, whatever n_members is.
 * Unlike mrgfe_batch_add_*, the clouds are only REFERENCED by the add calls (which member a pair goes to is known once the list is complete):
 * the host buffers must stay valid until mrgfe_node_align returns.  Keys (non-zero keyframe ids) keep a cloud resident on the member that
 * used it — candidates in the member's batch store (mrgfe_batch_add_pair_keyed), targets in the node's own per-member store —, and a later
 * call that names a resident key with the same point count may pass NULL.  A member that fails (out of memory, a bad cloud) makes
 * mrgfe_node_align return its error code with the member named in mrgfe_last_error(); the node stays usable. */
typedef struct mrgfe_node mrgfe_node;
int    mrgfe_node_create(int n_members, const int* device_ids, const mrgfe_reg_params* params, mrgfe_node** out);
void   mrgfe_node_destroy(mrgfe_node* node);
int    mrgfe_node_num_members(const mrgfe_node* node);
int    mrgfe_node_clear(mrgfe_node* node);
/* registration_->setInputTarget(new_keyframe->cloud), loop_detector.cpp:104: returns the target index (>= 0) or an error (< 0) */
int    mrgfe_node_add_target(mrgfe_node* node, const float* xyzi, size_t n, size_t stride_bytes);
int    mrgfe_node_add_target_keyed(mrgfe_node* node, uint64_t cloud_key, const float* xyzi, size_t n, size_t stride_bytes);
/* one candidate: setInputSource(candidate->cloud) + align(guess), loop_detector.cpp:127-134: returns the pair index (>= 0) or an error (< 0) */
int    mrgfe_node_add_pair(mrgfe_node* node, int target_index, const float* src_xyzi, size_t n, size_t stride_bytes, const float guess[16]);
int    mrgfe_node_add_pair_keyed(mrgfe_node* node, int target_index, uint64_t cloud_key, const float* src_xyzi, size_t n, size_t stride_bytes, const float guess[16]);
/* A target / a pair whose cloud is keyframe `key` of a map store (mrgfe_keyframe_callback, mrgfe_map_store_add) on ANY device: nothing comes from host
 * memory.  The key is looked up when the call is made, under the store's lock alone, and the store's stream is waited for there (mrgfe_map_store_add
 * uploads asynchronously); MRGFE_ERR_INVALID for a NULL argument, a target index out of range, or a key the store lacks (named in mrgfe_last_error();
 * nothing is queued).  Like mrgfe_batch_add_*_from_store, the STORE MUST OUTLIVE the node's use of it: destroy the node, or mrgfe_node_clear and
 * mrgfe_node_forget(0) it, first.
 *   A member on the store's device reads the store's memory in place, through mrgfe_batch_add_target_from_store / _add_pair_from_store (for the GICP
 * methods, not ICP_HIP, the k-NN covariances of a source are cached in the member's batch under `key`).
 *   A member on another device keeps a REPLICA of the keyframe on its own device, copied store device -> member device on the member's stream
 * (hipMemcpyPeerAsync; peer access need not be enabled, the runtime stages the copy when it is not).  Replicas are kept by key across calls next to the
 * member's keyed targets, under the same byte cap (MRGFE_KEYFRAME_STORE_MB) and least-recently-named rule; one the current call names, or one under a target
 * the member still holds built (mrgfe_node_clear_pairs), is never dropped.  A replicated source enters the member's batch so that its covariances are
 * cached under `key` exactly as above.  mrgfe_node_store_bytes counts replicas (16 bytes per point), mrgfe_node_forget drops them, mrgfe_node_clear
 * drops nothing resident.
 * Store-fed and host-fed targets and pairs may be mixed in one list; the records of mrgfe_node_align / mrgfe_node_align_best are those of ONE mrgfe_batch
 * holding the same list from the same store, bit for bit, for every member count and batch method. */
int    mrgfe_node_add_target_from_store(mrgfe_node* node, mrgfe_map_store* store, uint64_t key);
int    mrgfe_node_add_pair_from_store(mrgfe_node* node, int target_index, mrgfe_map_store* store, uint64_t key, const float guess[16]);
/* The pairs go, the declared targets keep their indices (mrgfe_batch_clear_pairs over the node).  A member keeps the targets its previous align built —
 * it clears the pairs of its batch alone — as long as the node's target list has not been cleared, and builds only the targets its new block needs and
 * lacks.  Blocks move with the length of the list, so reuse is an optimisation, never a condition: the records are those of a fresh node given the same
 * targets and the new pairs, bit for bit.  Host-fed targets without a key stay declared too: THEIR BUFFERS MUST STAY VALID until the last align that names
 * them (a member that lacks one uploads it then), not only until the first. */
int    mrgfe_node_clear_pairs(mrgfe_node* node);
/* the last mrgfe_node_align / _align_best, the members' counts added up: out[0] clouds read in place in the store, out[1] clouds copied to a replica in this
 * call, out[2] bytes copied, out[3] targets a member found already built (mrgfe_node_clear_pairs) */
int    mrgfe_node_store_stats(const mrgfe_node* node, int64_t out[4]);
int    mrgfe_node_num_pairs(const mrgfe_node* node);
int    mrgfe_node_align(mrgfe_node* node, double fitness_max_range, mrgfe_pair_result* results /* n_pairs, pair_id = index in the list */);
/* mrgfe_batch_align_best over the node: the records (pose fields; fitness exact, a certified bound or DBL_MAX), fit_state, best[g] — an index into the
 * node's pair list —, best_score[g] and the intervals are those of mrgfe_batch_align_best on ONE batch holding the whole list, bit for bit, for any
 * member count; score_cap behaves as there; pair_id is the index in the list; the blocks are those of mrgfe_node_align.  A group is the candidates of one
 * new keyframe and regularly straddles a block boundary, where a member holding only its wrong candidates could prune none of them; so the selection
 * — a pure function of per-pair values — is taken ONCE for the whole list, between two stages that every member runs on its own block:
 *   1. every member aligns its block and computes the interval of each of its pairs (block pass, seed, bound sums: one host wait per member);
 *   2. the calling thread prunes over the whole list;
 *   3. every member runs the exact passes for the contenders of its block (a second host wait); the records are gathered as in mrgfe_node_align.
 * Arguments are checked before any member runs: NULL node / results / group (with pairs) / best or best_score (with n_groups > 0), fitness_max_range
 * not >= 0, a NaN score_cap, a group id outside [-1, n_groups): MRGFE_ERR_INVALID.  A member that fails in either stage makes the call return its code
 * with the member named in mrgfe_last_error(), as mrgfe_node_align does; the members whose first stage had succeeded give their stage up first (their
 * streams are waited for), so no kernel of the call is in flight and no caller buffer is being read when the call returns.  The node stays usable.
 * With no pairs: MRGFE_OK, best[g] = -1 and best_score[g] = DBL_MAX for every g, nothing else written. */
int    mrgfe_node_align_best(mrgfe_node* node, double fitness_max_range, double score_cap, const int32_t* group /* n_pairs */, int n_groups,
                             mrgfe_pair_result* results /* n_pairs */, int32_t* fit_state /* n_pairs, nullable */, int32_t* best /* n_groups */,
                             double* best_score /* n_groups */);
/* the last mrgfe_node_align_best, in the layout of mrgfe_batch_select_stats: out[0..5] the members' counts added up, out[6] / out[7] the largest
 * member's host ms of the bound stage (which ends when the second stage reaches that member: the wait for the slowest member and the selection are
 * in it) and of the contender stage */
int    mrgfe_node_select_stats(const mrgfe_node* node, double out[8]);
/* block of member `member` in the last mrgfe_node_align / mrgfe_node_align_best; how its records were gathered (0 host memory, 1 RCCL all-gather) */
int    mrgfe_node_shard(const mrgfe_node* node, int member, int* first_pair, int* n_pairs);
int    mrgfe_node_last_gather(const mrgfe_node* node);
int    mrgfe_node_forget(mrgfe_node* node, uint64_t cloud_key); /* drops a key from every member's stores (0: all) */
size_t mrgfe_node_store_bytes(const mrgfe_node* node);
/* LoopDetector::detect in one call (mrgfe_loop_*, above) over a NODE: the same handle, mrgfe_loop_detect / _reset / _stats / _timing, controller and
 * validation before anything is queued as a detector of mrgfe_loop_create; only the two stages run elsewhere.  Stage 1: mrgfe_node_clear, the targets
 * and pairs by key from `store` (mrgfe_node_add_*_from_store), mrgfe_node_align — with fitness_selection 1 mrgfe_node_align_best, same groups and cap as
 * on a batch.  Stage 2: mrgfe_node_clear_pairs, the consistency pairs on the same target indices, mrgfe_node_align without fitness.  Same loops,
 * relative poses and scores as the detector over one batch, bit for bit, for any member count.  mrgfe_loop_stats out[4] counts the targets the stages
 * declared.  A failing call — also a failing member, named in mrgfe_last_error() — leaves the LoopManager, the counters, the stats and the timing as they
 * were, and the node usable.  MRGFE_ERR_INVALID: a NULL argument, fitness_selection not 0 or 1.  The store may sit on any device; nothing else queues on
 * the node while a detect call runs.  The handle is destroyed BEFORE its node and its store. */
int    mrgfe_loop_create_node(mrgfe_node* node, mrgfe_map_store* store, const mrgfe_loop_params* params, mrgfe_loop** out);
/* the reference's sequential rule on gathered records (loop_detector.cpp:126-145: "if( !hasConverged() || score > best_score ) continue;"): group g
 * = records group_first[g] .. group_first[g + 1] - 1 (the candidates of one new keyframe, in candidate order); best[g] = position within the
 * group or -1, best_score[g] = its fitness or DBL_MAX.  Among equal scores the LAST candidate wins, as there. */
int    mrgfe_node_select_best(const mrgfe_pair_result* results, int n_groups, const int32_t* group_first, int32_t* best, double* best_score);
/* rounds (plan -> derivative launches -> reduce / controller step) of the last mrgfe_batch_align of an NDT_HIP batch; of an ICP_HIP batch its
 * lock-step rounds (correspondences + sums -> reduce -> controller steps -> transform), which is the largest evaluation count of its pairs; of a
 * PCL_GICP_HIP / PCL_GICP_OMP_HIP batch its rounds (searches -> cost / gradient terms -> sums -> controller steps), which is the largest number of
 * functor evaluations of its pairs (at most the largest `evaluations` of the records) */
int mrgfe_batch_rounds(const mrgfe_batch* b);
/* The reference's own performance counters (loop_detector.cpp:22-34: per new keyframe with candidates the wall microseconds of find_candidates + matching
 * and the candidate count; apps/mrg_slam_component.cpp:1032-1037 writes their ratio as average_time_per_candidate_us) for this batch object:
 * out[0] = average_time_per_candidate_us = wall time of all mrgfe_batch_align calls so far (queueing to records, microseconds) / pairs aligned so far,
 * out[1] = wall microseconds of the LAST align, out[2] = its pairs, out[3] = pairs aligned so far.  mrgfe_batch_timing_reset zeroes the totals. */
int mrgfe_batch_timing(const mrgfe_batch* b, double out[4]);
int mrgfe_batch_timing_reset(mrgfe_batch* b);

/* ---- floor detection (apps/floor_detection_component.cpp:100-183, FloorDetectionComponent::detect) ------------------------------------------ *
 * Tilt compensation, the height band (PlaneClipper3D + ExtractIndices), the k = 10 normal filter (NormalEstimation on a KdTree), and
 * RandomSampleConsensus<SampleConsensusModelPlane> with threshold 0.1 — all on the GPU.  Parameter names / defaults: the component's
 * declare_parameter calls (:55-62) and config/mrg_slam.yaml:113-122.  The reference DECLARES enable_normal_filtering (:61) but READS
 * use_normal_filtering (:120); this port has one field with the evident intent. */
typedef struct mrgfe_floor_params {
    double tilt_deg;                  /* 0.0   "tilt_deg"                                                        */
    double sensor_height;             /* 2.0   "sensor_height"                                                   */
    double height_clip_range;         /* 1.0   "height_clip_range"                                               */
    int    floor_pts_thresh;          /* 512   "floor_pts_thresh"                                                */
    double floor_normal_thresh_deg;   /* 10.0  "floor_normal_thresh_deg"                                         */
    int    use_normal_filtering;      /* 1     "enable_normal_filtering" (:61; read as "use_normal_filtering" :120) */
    double normal_filter_thresh_deg;  /* 20.0  "normal_filter_thresh_deg"                                        */
} mrgfe_floor_params;
void mrgfe_floor_default_params(mrgfe_floor_params* out);
/* why detect() returned what it returned */
enum mrgfe_floor_reason {
    MRGFE_FLOOR_FOUND = 0,
    MRGFE_FLOOR_EMPTY_INPUT = 1,        /* cloud_callback returns before detect() (:79-82)                       */
    MRGFE_FLOOR_NONE_AFTER_CLIP = 2,    /* no point in the height band (:115-118)                                */
    MRGFE_FLOOR_TOO_FEW_FILTERED = 3,   /* filtered->size() < floor_pts_thresh (:134-136)                        */
    MRGFE_FLOOR_NO_MODEL = 4,           /* RandomSampleConsensus found no model (fewer than 3 points, no non-collinear sample) */
    MRGFE_FLOOR_TOO_FEW_INLIERS = 5,    /* inliers < floor_pts_thresh (:148)                                     */
    MRGFE_FLOOR_NOT_VERTICAL = 6        /* |n . (tilt^-1 z)| < cos(floor_normal_thresh_deg) (:153-162)           */
};
typedef struct mrgfe_floor_result {
    int32_t  found;        /* 1: coeffs is the boost::optional<Vector4f> detect() returns; 0: boost::none          */
    int32_t  reason;       /* enum mrgfe_floor_reason                                                             */
    float    coeffs[4];    /* a, b, c, d with the normal pointing up (:164-167); set when a model was found        */
    uint32_t n_clipped;    /* points in the height band                                                          */
    uint32_t n_filtered;   /* points after the normal filter (= n_clipped without it): floor_filtered_points       */
    uint32_t n_inliers;    /* RANSAC inliers of the winning plane: floor_points                                  */
    int32_t  iterations;   /* RandomSampleConsensus::iterations_ at the end of computeModel                       */
    int32_t  skipped;      /* samples whose coefficients could not be computed                                    */
    int32_t  reserved;
} mrgfe_floor_result;
/* replaces detect(cloud) (:100-183) — and what the component publishes next to it: out_filtered (nullable, capacity n packed points) receives
 * floor_filtered_points (:126-131: the RANSAC input, back in the sensor frame), out_inliers (nullable, capacity n) floor_points (:169-180: the
 * inliers of the accepted plane, written only when found).  Returns MRGFE_OK whether or not a floor was found. */
int  mrgfe_floor_detect(mrgfe_ctx* ctx, const mrgfe_floor_params* params, const float* xyzi, size_t n, size_t stride_bytes, mrgfe_floor_result* result,
                        float* out_filtered, float* out_inliers);
/* the same for a cloud already in device memory (packed float4): the output of mrgfe_prefilter_device — prefiltering/filtered_points, the topic
 * the component subscribes to — without a round trip through the host */
int  mrgfe_floor_detect_device(mrgfe_ctx* ctx, const mrgfe_floor_params* params, const void* d_xyzi, size_t n, mrgfe_floor_result* result,
                               float* out_filtered, float* out_inliers);
/* FloorDetectionComponent::cloud_callback (apps/floor_detection_component.cpp:69-93) in one call on the bytes of the sensor_msgs/PointCloud2 it
 * receives (prefiltering/filtered_points, in a floor-detection process of its own): pcl::fromROSMsg (:72), the empty-cloud return (:74-77) and
 * detect() (:80).  `layout`: what mrgfe_pointcloud2_layout fills, checked under this entry point's name by the rules of mrgfe_keyframe_callback (a
 * row_step that does not hold a row, offsets or steps that are not multiples of 4 unless the context has mrgfe_ctx_set_byte_layouts on:
 * MRGFE_ERR_INVALID); `data`: data_bytes >= (height - 1) * row_step + width * point_step bytes (less, or NULL with points: MRGFE_ERR_INVALID).
 * width * height == 0: MRGFE_OK with reason MRGFE_FLOOR_EMPTY_INPUT, nothing is sent or launched.  The payload goes up ONCE as it is and the first
 * kernel reads the records, applies the tilt and flags the height band: no packed copy of the cloud is written and read back in front of it.
 * out_filtered / out_inliers: as for mrgfe_floor_detect, room for width * height packed points each, either may be NULL.  result and both clouds equal,
 * bit for bit, mrgfe_ingest_pointcloud2 followed by mrgfe_floor_detect_device for the same message and parameters, with the same number of host
 * waits; a failing call leaves nothing behind. */
int  mrgfe_floor_callback(mrgfe_ctx* ctx, const mrgfe_floor_params* params, const mrgfe_keyframe_params* layout, const void* data, size_t data_bytes,
                          mrgfe_floor_result* result, float* out_filtered, float* out_inliers);

/* Diagnostic entry points (alternative paths of the same arithmetic, primitives, the optimiser stepped by hand) are declared in mrgfe_debug.h; the two
 * fault injectors there exist only in a library built with -DMRGFE_TESTING (mrg_slam_amd/libmrgfe_testing.so): the shipped libmrgfe.so has neither. */

#ifdef __cplusplus
}
#endif
#endif /* MRGFE_H */
