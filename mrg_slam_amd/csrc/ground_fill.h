// csrc/ground_fill.h — first-keyframe ground fill (ground_fill.hip): mrg_slam_pcl::fill_cloud (the reference's src/pcl/fill_ground_plane.cpp:49-65) — a disc
// of synthetic points on a plane, written behind a cloud that is already in device memory.  The plane comes from the caller: the RANSAC variant (:21-35)
// takes it from floor_ransac_device (floor.h), the simple variant (:37-47) from the pose.
#pragma once
#include "common.h"

namespace mrgfe {

// radius and map_resolution finite and > 0 (the reference's loops would not terminate otherwise): MRGFE_ERR_INVALID under the name `fn`
int ground_fill_check(const mrgfe_ground_fill_params* p, const char* fn);

// The two loop counts of fill_cloud, walked as the reference walks them: r and angle are ACCUMULATED doubles (`r += map_resolution`, `angle += angle_inc`).
// MRGFE_ERR_INVALID when n_before + rings * angles would pass 2^31 - 1 points.  `p` has passed ground_fill_check.
int ground_fill_counts(const mrgfe_ground_fill_params* p, uint64_t n_before, uint32_t* n_rings, uint32_t* n_angles, const char* fn);

// Queues on the context's stream: the two tables (r per ring; sin, cos per angle — the host's, from the C library) and ONE launch that writes
// n_rings * n_angles points to d_dst, rings outermost.  No wait.  normal / offset: the Hyperplane<double, 3> of :32 / :44, the normal as it is given.
int ground_fill_device(mrgfe_ctx* ctx, const mrgfe_ground_fill_params* p, const double normal[3], double offset, uint32_t n_rings, uint32_t n_angles, float4* d_dst);

}  // namespace mrgfe
