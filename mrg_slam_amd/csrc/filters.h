// csrc/filters.h — prefilter chain launchers (filters.hip). Device-pointer forms chain without leaving HBM; the
// host-pointer forms back the C ABI (include/mrgfe.h).
#pragma once
#include "cellsort.h"
#include "common.h"

namespace mrgfe {

int filter_distance_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, double near_t, double far_t, float4* d_out, size_t* out_n);
int filter_voxelgrid_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, float leaf, int min_pts, float4* d_out, size_t* out_n, int* overflow);
int filter_radius_outlier_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, double radius, int min_neighbors, float4* d_out, size_t* out_n);
// pcl::ApproximateVoxelGrid: the sequential 512-entry history loop decomposed into independent per-entry sequences (filters.hip)
int filter_approx_voxelgrid_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, float leaf, float4* d_out, size_t* out_n);
int filter_statistical_outlier_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, int mean_k, double stddev_mul, float4* d_out, size_t* out_n);

// order-preserving compaction of the points whose flag is 1 (exclusive scan of the flags + scatter); synchronises and
// returns the kept count.  Uses ctx scratch slots 0, 4 and 8.
// per-run float centroids (sums in ascending sorted position) and the count-threshold flags: the tail of the voxel-grid passes
int launch_voxel_centroids(mrgfe_ctx* ctx, const float4* d_pts, const uint32_t* d_sorted_vals, const uint32_t* d_seg_start, uint32_t n_seg, int min_pts, float4* d_centroids,
                           uint32_t* d_keep);
int compact_by_flags(mrgfe_ctx* ctx, const float4* d_in, uint32_t n, uint32_t* d_flags, float4* d_out, uint32_t* h_total);

struct PrefilterChain {
    bool   distance = true;
    double near_t = 0.1, far_t = 35.0;
    bool   voxelgrid = true;
    bool   approx_voxelgrid = false;  // downsample_method APPROX_VOXELGRID (instead of voxelgrid; same leaf)
    float  leaf = 0.1f;
    int    min_pts = 1;
    int    outlier = 1;  // 0 none, 1 radius, 2 statistical
    double radius = 0.5;
    int    radius_min_neighbors = 2;
    int    mean_k = 30;
    double stddev_mul = 1.2;
};
// 1: the chains keep their point counts on the device and wait once (default; every chain but the statistical filter behind anything other than a voxel
// grid — unless the context has mrgfe_ctx_set_statistical_chains on —, or with mean_k outside 1..63, 1..255 with mrgfe_ctx_set_wide_statistical_chains on), and so does the odometry frame's downsample;
// 0: host-driven stages; < 0: query
int prefilter_set_device_driven(int mode);
// mrgfe_dbg_set_sor_grid_rule (include/mrgfe_debug.h): the rule of the statistical filter's device-sized k-NN grid, process-wide; a zero restores that default
void prefilter_set_sor_grid_rule(float start_edge, double crowding_target, int max_halvings);
// The chain's downsample stage alone, behind a caller's own head kernel (the odometry frame; filters.hip): method 1 VoxelGrid, 2 ApproximateVoxelGrid.
struct DownsampleReport {
    int      route;        // 0 the switch is off (nothing was launched), 1 served, 2 an anomaly: the caller runs the host-driven filter
    uint32_t anomaly;      // the chain's anomaly word
    uint32_t n_finite_in;  // finite points of the input
    uint32_t kept;         // points in d_out (route 1)
    uint32_t kept_finite;  // ... finite among them
    float    box[6];       // ... and their box: min xyz, max xyz
};
int downsample_device_driven(mrgfe_ctx* ctx, int method, const float4* d_in, size_t n, const BBox* d_tile_boxes, float leaf, int min_pts, float4* d_out, DownsampleReport* rep);
// mrgfe_dbg_sor_threshold (include/mrgfe_debug.h): the statistical filter's sums, threshold and certificate, host loop or the chain's kernels
int sor_threshold_debug(mrgfe_ctx* ctx, const float* dist, const uint32_t* valid, size_t n, double stddev_mul, int on_device, double out[6]);
// Where a call's records go (mrgfe_scan_callback_records, mrgfe_prefilter_records, mrgfe_cloud_records_device).  The entry point has checked point_step
// (16 or 32: record_store.h) and that `capacity` holds one record per INPUT point; the chain decides the rest: a range whose two ends lie in page-locked
// host memory (upload_cloud's test) and that starts at a multiple of 16 bytes is written by the record kernel itself, anything else through the context's
// pinned buffer and one memcpy of the kept records behind the wait.
struct RecordSink {
    int    point_step = 32;
    void*  records = nullptr;
    size_t capacity = 0;
};
// the three passes back to back on the device (one upload, one download).  `rec`: the result goes to the host as records instead of packed points —
// `out` is then device memory for n points (out_on_device) or NULL (an internal buffer; nothing is remembered for mrgfe_reg_set_source_from_prefilter)
int filter_chain(mrgfe_ctx* ctx, const PrefilterChain& chain, const float* xyzi, size_t n, size_t stride, void* out, size_t* out_n, bool out_on_device = false,
                 const RecordSink* rec = nullptr);
// the n packed points at d_xyzi (device memory of the context's GPU) as records: one launch, one wait
int cloud_records_device(mrgfe_ctx* ctx, const float4* d_xyzi, size_t n, const RecordSink& rec);
// A call with TWO record sinks (the scan callback's coloured cloud beside its filtered scan, the keyframe callback's removed cloud beside its kept one)
// resolves the second by the same rule; what is staged of it goes through a pinned buffer of its own (mrgfe_ctx::rec_pin2) and its record stage is counted
// apart (mrgfe_ctx_second_egress_stats), so the first sink's path and mrgfe_ctx_egress_stats are those of the call without the second.
// Two packed device clouds as records in ONE launch behind ONE wait (mrgfe_keyframe_callback_records: the kept and the removed cloud); either sink may be
// NULL (that cloud is not read), both sinks have one point_step.
int cloud_pair_records_device(mrgfe_ctx* ctx, const float4* d_first, size_t n_first, const RecordSink* first, const float4* d_second, size_t n_second, const RecordSink* second);
// pcl::transformPointCloud(cloud, odom) and pcl::toROSMsg in one pass (mrgfe_odom_frame_records): point i of d_xyzi moved by T (row-major, the body of
// transform_cloud_kernel: scan_point.h) and stored as record i; one launch, one wait, no intermediate cloud
int transformed_records_device(mrgfe_ctx* ctx, const float4* d_xyzi, size_t n, const float T_rowmajor[16], const RecordSink& rec);

// What PrefilteringComponent::cloud_callback does to a scan BEFORE its filters (apps/prefiltering_component.cpp:119-146), as the scan head kernel's work
// order: read the x / y / z / intensity fields out of the wire records of a sensor_msgs/PointCloud2 (validated: ingest.h check_pointcloud2_layout),
// deskew, transform into base_link_frame.
struct ScanHead {
    const uint8_t* data = nullptr;  // host payload, (height - 1) * row_step + width * point_step bytes
    uint32_t width = 0, height = 0, point_step = 16, row_step = 0, off_x = 0, off_y = 4, off_z = 8;
    int32_t  off_intensity = 12;    // < 0: no such field, intensity 0
    bool     deskew = false;
    float    ang_v[3] = {0, 0, 0};  // as the IMU message gives it (negated on the way to the kernel, :275)
    double   scan_period = 0.1;
    bool     transform = false;
    float    T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // row-major 3x4
};
// the same chain fed by the wire records of a scan: they go up once, and the scan head kernel writes the chain's packed input (and, in front of the
// device-driven chain, the distance filter's flags and tile counts with it) — same output as mrgfe_ingest_pointcloud2 -> mrgfe_deskew ->
// mrgfe_transform_cloud -> filter_chain, bit for bit
// `colored` (mrgfe_scan_callback_outputs; 32-byte records, room for width * height of them): the raw scan as pcl::PointXYZRGB records, colour = position in
// the point sequence (apps/prefiltering_component.cpp:239-257) — one kernel over the uploaded wire records, queued in front of the chain, so the chain's one
// wait covers it (routes 0 and 2: a wait of its own behind the host-driven passes)
int scan_chain(mrgfe_ctx* ctx, const PrefilterChain& chain, const ScanHead& head, void* out, size_t* out_n, bool out_on_device, const RecordSink* rec = nullptr,
               const RecordSink* colored = nullptr);
// the coloured records alone: the payload goes up, the one kernel, one wait; no chain runs and mrgfe_ctx_prefilter_stats / mrgfe_ctx_egress_stats stay as they were
int scan_colored_records(mrgfe_ctx* ctx, const ScanHead& head, const RecordSink& colored);

int filter_distance(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double near_t, double far_t, float* out, size_t* out_n);
int filter_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float leaf, int min_pts, float* out, size_t* out_n, int* overflow);
int filter_approx_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float leaf, float* out, size_t* out_n);
int filter_radius_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double radius, int min_neighbors, float* out, size_t* out_n);
int filter_statistical_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, int mean_k, double stddev_mul, float* out, size_t* out_n);

}  // namespace mrgfe
