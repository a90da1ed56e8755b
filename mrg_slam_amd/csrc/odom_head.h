// csrc/odom_head.h — the head kernel of the one-call odometry frame (odom_head.hip), launched by odometry.cpp.
#pragma once
#include "cellsort.h"
#include "common.h"

namespace mrgfe {

inline uint32_t odom_head_tiles(uint32_t n) { return (n + kTile - 1) / kTile; }
// The wire records at d_raw (layout checked: ingest.h check_pointcloud2_layout, row_step filled in) -> the packed cloud d_out (width * height points) and
// the box of its finite points in *d_box; d_partial: odom_head_tiles(n) entries of scratch.  Two launches on ctx->stream, no wait.
int launch_odom_head(mrgfe_ctx* ctx, const void* d_raw, const mrgfe_keyframe_params& lay, float4* d_out, BBox* d_partial, BBox* d_box);

}  // namespace mrgfe
