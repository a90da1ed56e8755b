// csrc/ingest.hip — point-layout ingest: gathers x, y, z, intensity out of strided point records into the packed float4
// layout every kernel of libmrgfe works on.  What it replaces in the reference:
//   * pcl::fromROSMsg(*cloud_msg, *cloud) — sensor_msgs/PointCloud2 (any point_step / field offsets) -> pcl::PointXYZI:
//     /root/reference/apps/prefiltering_component.cpp:119-120, apps/scan_matching_odometry_component.cpp:144-145;
//     the replay scripts publish point_step 16, offsets 0/4/8/12 (python_scripts/kitti_singlerobot_processor.py:164-185);
//   * the 32-byte in-memory pcl::PointXYZI (x, y, z, 1.0f padding; intensity at byte 16; 12 bytes of padding) that the
//     reference's clouds live in (include/mrg_slam/keyframe.hpp, PointT = pcl::PointXYZI) and that keyframe .pcd files are
//     read into (src/mrg_slam/keyframe.cpp:196).
// The raw records are copied to the device as they are (one contiguous H2D copy through the pinned staging ring, no host
// repacking loop) and gathered there: one lane per point, four 4-byte loads, one 16-byte store.
// Which layouts: by default FLOAT32 fields at offsets that are multiples of 4 inside a point_step and row_step that are multiples of 4 (the "strict"
// layouts, check_pointcloud2_layout); with mrgfe_ctx_set_byte_layouts on the context, any point_step / row_step / field offsets, as pcl::fromROSMsg
// takes them (Velodyne's 22-byte XYZIRT records) — such records are read by the kernels' byte-aligned instantiations (scan_point.h: up to two aligned
// words per field), the strict ones by the loads they always had.
#include "common.h"
#include "ingest.h"
#include "scan_point.h"

namespace mrgfe {

// kBytes: the layout is not a strict one (ingest.h layout_is_strict) and the fields are put together from aligned words
template <bool kBytes>
__global__ __launch_bounds__(256) void gather_points_kernel(const uint8_t* __restrict__ raw, float4* __restrict__ dst, uint32_t n, uint32_t width, uint32_t row_step, uint32_t point_step,
                                                            uint32_t ox, uint32_t oy, uint32_t oz, int32_t oi)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    dst[i] = load_point_record_as<kBytes>(raw, i, width, row_step, point_step, ox, oy, oz, oi);  // (scan_point.h: the scan head kernel reads records the same way)
}

int launch_gather_points(mrgfe_ctx* ctx, const void* d_raw, float4* d_dst, size_t n, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz,
                         int32_t oi)
{
    if (n == 0) return MRGFE_OK;
    const auto kern = layout_is_strict(point_step, row_step, ox, oy, oz, oi) ? gather_points_kernel<false> : gather_points_kernel<true>;
    hipLaunchKernelGGL(kern, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, ctx->stream, static_cast<const uint8_t*>(d_raw), d_dst,
                       static_cast<uint32_t>(n), width, row_step, point_step, ox, oy, oz, oi);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// raw host bytes -> d_dst: one contiguous copy through the staging ring, stream-ordered (`raw` is free on return)
int upload_raw_records_to(mrgfe_ctx* ctx, const void* raw, size_t raw_bytes, void* d_dst)
{
    const int slot = ctx->up_next;
    ctx->up_next ^= 1;
    if (!ctx->up_ev[slot]) MRGFE_HIP_CHECK(hipEventCreateWithFlags(&ctx->up_ev[slot], hipEventDisableTiming));
    if (ctx->up_busy[slot]) { MRGFE_HIP_CHECK(hipEventSynchronize(ctx->up_ev[slot])); ctx->up_busy[slot] = false; }
    PinBuf& pb = ctx->up_pin[slot];
    MRGFE_TRY(pb.ensure(raw_bytes));
    std::memcpy(pb.p, raw, raw_bytes);
    MRGFE_HIP_CHECK(hipMemcpyAsync(d_dst, pb.p, raw_bytes, hipMemcpyHostToDevice, ctx->stream));
    MRGFE_HIP_CHECK(hipEventRecord(ctx->up_ev[slot], ctx->stream));
    ctx->up_busy[slot] = true;
    return MRGFE_OK;
}

// raw host bytes -> the context's raw record buffer
int upload_raw_records(mrgfe_ctx* ctx, const void* raw, size_t raw_bytes, const void** d_raw)
{
    // the raw device buffer is reused by the next upload of records: stream order (copy k+1 after the kernel that reads copy k) keeps that safe
    MRGFE_TRY(ctx->up_raw.ensure(raw_bytes));
    MRGFE_TRY(upload_raw_records_to(ctx, raw, raw_bytes, ctx->up_raw.p));
    *d_raw = ctx->up_raw.p;
    return MRGFE_OK;
}

// raw host bytes -> device scratch -> gather into d_dst
int upload_gathered(mrgfe_ctx* ctx, const void* raw, size_t raw_bytes, size_t n, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz,
                    int32_t oi, void* d_dst)
{
    if (n == 0) return MRGFE_OK;
    const void* d_raw = nullptr;
    MRGFE_TRY(upload_raw_records(ctx, raw, raw_bytes, &d_raw));
    return launch_gather_points(ctx, d_raw, static_cast<float4*>(d_dst), n, width, row_step, point_step, ox, oy, oz, oi);
}

// the layout rules of a PointCloud2 payload with FLOAT32 x / y / z / intensity fields: shared by every entry point that reads one (`fn` names it in the message)
// With the context's byte-layout switch on (mrgfe_ctx_set_byte_layouts) the multiple-of-4 demands fall away: any point_step >= 1, any row_step that
// holds a row, any offset with off + 4 <= point_step.
int check_pointcloud2_layout(const mrgfe_ctx* ctx, const char* fn, uint32_t width, uint32_t height, uint32_t point_step, uint32_t* row_step, uint32_t off_x, uint32_t off_y,
                             uint32_t off_z, int32_t off_intensity)
{
    const uint32_t unit = ctx && ctx->byte_layouts.load(std::memory_order_relaxed) ? 1u : 4u;
    if (uint64_t(width) * point_step > 0xffffffffull) { set_error("%s: width %u x point_step %u does not fit a row", fn, width, point_step); return MRGFE_ERR_INVALID; }
    if (*row_step == 0) *row_step = width * point_step;
    const uint32_t offs[4] = {off_x, off_y, off_z, off_intensity >= 0 ? static_cast<uint32_t>(off_intensity) : 0u};
    for (uint32_t o : offs)
        if ((o % unit) != 0 || uint64_t(o) + 4 > point_step) {
            set_error(unit == 4 ? "%s: FLOAT32 field offset %u does not fit point_step %u (offsets must be multiples of 4)" : "%s: FLOAT32 field offset %u does not fit point_step %u", fn, o, point_step);
            return MRGFE_ERR_INVALID;
        }
    if ((point_step % unit) != 0 || (*row_step % unit) != 0 || uint64_t(width) * point_step > *row_step) { set_error("%s: bad point_step %u / row_step %u", fn, point_step, *row_step); return MRGFE_ERR_INVALID; }
    if (size_t(width) * height > 0x7fffffffu) { set_error("%s: cloud too large", fn); return MRGFE_ERR_INVALID; }
    return MRGFE_OK;
}

}  // namespace mrgfe

using namespace mrgfe;

extern "C" int mrgfe_ingest_pointcloud2(mrgfe_ctx* ctx, const uint8_t* data, uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step, uint32_t off_x,
                                        uint32_t off_y, uint32_t off_z, int32_t off_intensity, float* out_xyzi, void* d_out_xyzi)
{
    if (!ctx) { set_error("mrgfe_ingest_pointcloud2: NULL context"); return MRGFE_ERR_INVALID; }
    const size_t n = size_t(width) * height;
    if (n == 0) return MRGFE_OK;
    if (!data || (!out_xyzi && !d_out_xyzi)) { set_error("mrgfe_ingest_pointcloud2: NULL data / no output"); return MRGFE_ERR_INVALID; }
    MRGFE_TRY(check_pointcloud2_layout(ctx, "mrgfe_ingest_pointcloud2", width, height, point_step, &row_step, off_x, off_y, off_z, off_intensity));
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    void* d_dst = d_out_xyzi;
    if (!d_dst) { MRGFE_TRY(ctx->up_out.ensure(n * 16)); d_dst = ctx->up_out.p; }
    const size_t raw_bytes = size_t(height - 1) * row_step + size_t(width) * point_step;
    if (point_step == 16 && off_x == 0 && off_y == 4 && off_z == 8 && off_intensity == 12 && uint64_t(row_step) == uint64_t(width) * 16u) {
        MRGFE_TRY(upload_cloud(ctx, reinterpret_cast<const float*>(data), n, 16, d_dst));  // the replay layout is the device layout: plain copy
    } else {
        MRGFE_TRY(upload_gathered(ctx, data, raw_bytes, n, width, row_step, point_step, off_x, off_y, off_z, off_intensity, d_dst));
    }
    if (out_xyzi) MRGFE_HIP_CHECK(hipMemcpyAsync(out_xyzi, d_dst, n * 16, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MRGFE_OK;
}

// ---- sensor_msgs/PointField list -> the layout the entry points take (host only, no context) ---------------------------------------------------------
static_assert(sizeof(mrgfe_pointcloud2_field) == 24, "mrgfe_pointcloud2_field: the layout the bindings mirror");
extern "C" size_t mrgfe_pointcloud2_field_size(void) { return sizeof(mrgfe_pointcloud2_field); }

extern "C" int mrgfe_pointcloud2_layout(const mrgfe_pointcloud2_field* fields, int n_fields, uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step, int is_bigendian,
                                        mrgfe_keyframe_params* out, int* needs_byte_layouts)
{
    static const char* fn = "mrgfe_pointcloud2_layout";
    if (needs_byte_layouts) *needs_byte_layouts = 0;
    if (!out || n_fields < 0 || (n_fields > 0 && !fields)) { set_error("%s: NULL argument or a negative count", fn); return MRGFE_ERR_INVALID; }
    if (is_bigendian) { set_error("%s: a big-endian payload", fn); return MRGFE_ERR_INVALID; }
    // pcl::fromROSMsg -> createMapping -> FieldMatches: the FIRST field with the name, datatype FLOAT32 (7) and count 1; the others are not looked at
    auto find = [&](const char* name, uint32_t* off) {
        for (int i = 0; i < n_fields; ++i)
            if (fields[i].name && std::strcmp(fields[i].name, name) == 0 && fields[i].datatype == 7 && fields[i].count == 1) { *off = fields[i].offset; return true; }
        return false;
    };
    uint32_t off[4] = {0, 0, 0, 0};
    static const char* const names[3] = {"x", "y", "z"};
    for (int k = 0; k < 3; ++k)
        if (!find(names[k], &off[k])) { set_error("%s: no FLOAT32 field '%s' with count 1 (pcl::fromROSMsg would leave it unset)", fn, names[k]); return MRGFE_ERR_INVALID; }
    const bool has_i = find("intensity", &off[3]);
    if (has_i && off[3] > 0x7fffffffu) { set_error("%s: field 'intensity' at offset %u", fn, off[3]); return MRGFE_ERR_INVALID; }
    // (whether the fields fit point_step and the rows fit row_step is for the entry point the layout goes to: it refuses under its own name)
    out->width = width; out->height = height; out->point_step = point_step; out->row_step = row_step;
    out->off_x = off[0]; out->off_y = off[1]; out->off_z = off[2];
    out->off_intensity = has_i ? static_cast<int32_t>(off[3]) : -1;
    const uint32_t row = row_step ? row_step : width * point_step;  // (what the entry point fills in; only its low two bits matter here)
    if (needs_byte_layouts) *needs_byte_layouts = layout_is_strict(point_step, row, off[0], off[1], off[2], out->off_intensity) ? 0 : 1;
    return MRGFE_OK;
}
