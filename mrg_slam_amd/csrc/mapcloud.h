// csrc/mapcloud.h — per-point passes next to the hot path, launchers of mapcloud.hip.
#pragma once
#include "common.h"

namespace mrgfe {

// MapCloudGenerator::generate (/root/reference/src/mrg_slam/map_cloud_generator.cpp:14-86): transform every keyframe
// cloud by its pose, optional far-distance cut, concatenate, pcl::ApproximateMeanVoxelGrid
// (include/pcl/filters/ApproximateMeanVoxelGrid.hpp:63-126).  d_cat: the keyframe clouds back to back (packed float4),
// kf_off[K + 1]: first point of every keyframe (host), poses_f[K][16]: column-major float 4x4 (host).
// d_out needs room for kf_off[K] points.  resolution <= 0: no voxel filter.
int map_cloud_device(mrgfe_ctx* ctx, const float4* d_cat, const uint32_t* kf_off, const float* poses_f, int K, float resolution, int min_points_per_voxel,
                     float distance_far_thresh, float4* d_out, size_t* out_n, size_t* n_unfiltered /* points after the distance cut */,
                     const float4* const* kf_ptrs = nullptr /* host array of K device pointers: read keyframe k there instead of in d_cat */);

// The map as wire records (mrgfe_map_store_publish): the points of map_cloud_device for keyframes read through kf_ptrs — same points, same order, same
// bits —, then up to two f32 offsets added one after the other, written as 32-byte pcl::PointXYZI records or packed 16-byte points by the kernel that
// writes the final points (the scatter of the last compaction, or the copy of the unfiltered map).  Every buffer of the call is one of `ws` (grow-only,
// owned by the store) or a scratch slot of the context: a call no larger than an earlier one allocates and frees nothing.  The *out_n records are left in
// ws.rec; *records_complete: the stream was waited for behind the kernel that wrote them (false: the unfiltered map without a far cut, whose record kernel
// is only queued — a caller that hands the records out waits first).  stats: the launches of the record stage (the record kernel and the scan in front of
// it) and the stream waits of the whole call are added.
struct EgressFormat { int point_step; int n_offsets; float offsets[6]; };  // 32 or 16; 0..2 offsets, x y z each
struct EgressStats { int64_t launches = 0, waits = 0, bytes_down = 0, grown = 0; };
struct MapEgressWorkspace {
    DevBuf tab, trans, flags, comp, rec;  // offset / pose / pointer tables; transformed points; far-cut flags; points behind the far cut; the records
    size_t footprint(const mrgfe_ctx* ctx) const;  // device bytes held by the workspace and by the context's scratch slots the passes use
};
int map_publish_device(mrgfe_ctx* ctx, MapEgressWorkspace& ws, const uint32_t* kf_off, const float* poses_f, int K, const float4* const* kf_ptrs, float resolution,
                       int min_points_per_voxel, float distance_far_thresh, const EgressFormat& format, size_t* out_n, size_t* n_unfiltered, bool* records_complete,
                       EgressStats* stats);
// Stored keyframes as 32-byte records (mrgfe_map_store_read): ONE launch over a tile table (scratch[0], staged through the descriptor ring); keyframe m's
// point i becomes record first_record + i of d_records; no wait
struct KeyframeRecordItem { const float4* d_cloud; uint32_t n; uint64_t first_record; };
int keyframe_records_many_device(mrgfe_ctx* ctx, const KeyframeRecordItem* items, size_t count, void* d_records);

// other-robot point removal (apps/mrg_slam_component.cpp:396-429): order-preserving split into kept / removed
int remove_points_near_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, const float* centres_xyz, int n_centres, float radius_sqr, float4* d_kept, size_t* n_kept,
                              float4* d_removed, size_t* n_removed);

// The point work of MrgSlamComponent::cloud_callback (apps/mrg_slam_component.cpp:372, 396-430) on the wire records of a PointCloud2 already on
// the device (ingest.h upload_raw_records; the layout was checked by check_pointcloud2_layout).
struct KeyframeLayout { uint32_t width, height, point_step, row_step, off_x, off_y, off_z; int32_t off_intensity; };
// no other robot: the records are gathered straight into d_cloud (width * height packed points); one launch, no wait
int keyframe_gather_device(mrgfe_ctx* ctx, const void* d_raw, const KeyframeLayout& lay, float4* d_cloud);
// the same gather for MANY messages in ONE launch (mrgfe_map_store_add_keyframes): a tile table in device memory (scratch[0], staged through the descriptor
// ring) names every 2048-point tile's message — raw base, layout, first point, destination — so keyframes of any size and layout share the launch; no wait
struct KeyframeGatherItem { const void* d_raw; KeyframeLayout lay; float4* d_cloud; };
int keyframe_gather_many_device(mrgfe_ctx* ctx, const KeyframeGatherItem* items, size_t count);
// with centres (1 <= n_centres <= 64): two launches — records -> packed cloud + keep flags + tile counts, then the stable two-way partition into
// d_kept / d_removed (room for width * height points each; d_removed may be nullptr) — and ONE wait for the two totals
int keyframe_split_device(mrgfe_ctx* ctx, const void* d_raw, const KeyframeLayout& lay, const float* centres_xyz, int n_centres, float radius_sqr, float4* d_kept,
                          size_t* n_kept, float4* d_removed, size_t* n_removed);

// PrefilteringComponent::deskewing (apps/prefiltering_component.cpp:231-292)
int deskew_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, const float ang_v[3], double scan_period, float4* d_out);
// pcl::transformPointCloud(in, out, Matrix4f): the float arithmetic of dev_float.h's transform_point, intensity copied
int transform_cloud_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, const float T_rowmajor[16], float4* d_out);

}  // namespace mrgfe
