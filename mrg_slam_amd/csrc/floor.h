// csrc/floor.h — floor detection (floor.hip): FloorDetectionComponent::detect (the reference's apps/floor_detection_component.cpp:100-183) on the
// GPU — tilt + height band, k = 10 normal filter, RANSAC plane fit — and its two stage entry points for the tests.
#pragma once
#include "common.h"
#include "mapcloud.h"

namespace mrgfe {

// the whole of detect() on a packed float4 device cloud (the input may be the caller's: it is only read)
int floor_detect(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const float4* d_in, size_t n, mrgfe_floor_result* res, float* out_filtered, float* out_inliers);
// the same on the bytes of a sensor_msgs/PointCloud2 (FloorDetectionComponent::cloud_callback :69-93): `raw_bytes` of `data` go up once through the raw
// staging path and the first kernel reads the records (`lay` was checked by check_pointcloud2_layout, row_step filled in); behind it the same stages,
// waits and results as floor_detect on the cloud mrgfe_ingest_pointcloud2 makes of the message
int floor_callback(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const KeyframeLayout& lay, const void* data, size_t raw_bytes, mrgfe_floor_result* res, float* out_filtered,
                   float* out_inliers);

// RandomSampleConsensus<SampleConsensusModelPlane> on a device cloud: coefficients of the winning sample, inlier flags (device, n words; may be null),
// iterations, skipped samples; *has_model = 0 when RANSAC found none (coeffs untouched then)
struct FloorRansacOut {
    int      has_model = 0;
    float    coeffs[4] = {0, 0, 0, 0};
    uint32_t n_inliers = 0;
    int32_t  iterations = 0;
    int32_t  skipped = 0;
};
int floor_ransac_device(mrgfe_ctx* ctx, const float4* d_pts, uint32_t n, double threshold, uint32_t* d_inlier_flags, FloorRansacOut* out);

// NormalEstimation(k = 10) + the |n_z| test of normal_filtering (:216-243) on a device cloud: d_normals (float4: the eigen33 vector, NaN when fewer than
// three neighbours) may be null; d_keep = 1 / 0 per point
int floor_normals_device(mrgfe_ctx* ctx, const float4* d_pts, uint32_t n, double normal_filter_thresh_deg, float4* d_normals, uint32_t* d_keep);

}  // namespace mrgfe
