// csrc/odom_head.hip — the head of the one-call odometry frame (odometry.cpp; ScanMatchingOdometryComponent::cloud_callback,
// apps/scan_matching_odometry_component.cpp:138-150): pcl::fromROSMsg of the message (:144-145) and the bounding box of its finite points
// in ONE pass over the wire records.  Per point: the strided record is read (scan_point.h load_point_record, the body of gather_points_kernel, so the
// gather cannot round or read differently from mrgfe_ingest_pointcloud2), stored as the packed float4 with one 16-byte store, and added to the thread's
// box (bbox_device.h BoxAcc: min, max and an integer count over the finite points, as pcl::getMinMax3D).  Same tile shape as keyframe_head_kernel /
// scan_head_kernel: one workgroup of 256 per 2048 points, one partial box per workgroup.  A second launch of ONE workgroup on the same stream merges the
// partial boxes; no workgroup waits for or signals another inside a launch.  min / max / integer count: the box is the exact box of the
// finite points, whatever the tiling — the one the separate pass (cellsort.hip bounding_boxes) gives.
#include "bbox_device.h"
#include "common.h"
#include "ingest.h"
#include "odom_head.h"
#include "scan_point.h"

namespace mrgfe {

struct OdomHeadArgs {
    const uint8_t* raw;
    float4*        out;
    BBox*          partial;  // one per tile
    uint32_t       n, width, row_step, point_step, ox, oy, oz;
    int32_t        oi;
};

// kBytes: the layout is not a strict one (ingest.h layout_is_strict) and the record's fields are put together from aligned words
template <bool kBytes>
__global__ __launch_bounds__(256) void odom_head_kernel(const OdomHeadArgs a)
{
    const uint32_t base = blockIdx.x * kTile;
    BoxAcc acc;
    acc.init();
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        if (i < a.n) {
            const float4 p = load_point_record_as<kBytes>(a.raw, i, a.width, a.row_step, a.point_step, a.ox, a.oy, a.oz, a.oi);
            a.out[i] = p;
            acc.add(p);
        }
    }
    const BBox b = block_merge_box(acc);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void odom_box_merge_kernel(const BBox* __restrict__ partial, uint32_t n_partial, BBox* __restrict__ out)
{
    const BBox b = block_merge_partials(partial, n_partial);
    if (threadIdx.x == 0) *out = b;
}

int launch_odom_head(mrgfe_ctx* ctx, const void* d_raw, const mrgfe_keyframe_params& lay, float4* d_out, BBox* d_partial, BBox* d_box)
{
    OdomHeadArgs a;
    a.raw = static_cast<const uint8_t*>(d_raw);
    a.out = d_out;
    a.partial = d_partial;
    a.n = lay.width * lay.height;
    a.width = lay.width; a.row_step = lay.row_step; a.point_step = lay.point_step;
    a.ox = lay.off_x; a.oy = lay.off_y; a.oz = lay.off_z; a.oi = lay.off_intensity;
    const uint32_t nblk = odom_head_tiles(a.n);
    const auto     kern = layout_is_strict(lay.point_step, lay.row_step, lay.off_x, lay.off_y, lay.off_z, lay.off_intensity) ? odom_head_kernel<false> : odom_head_kernel<true>;
    if (nblk > 0) hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(odom_box_merge_kernel, dim3(1), dim3(256), 0, ctx->stream, d_partial, nblk, d_box);  // (no tile: the empty box, n_finite 0)
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

}  // namespace mrgfe
