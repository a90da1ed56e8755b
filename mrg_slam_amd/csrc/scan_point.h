// csrc/scan_point.h — the per-point work of PrefilteringComponent::cloud_callback before its filters (apps/prefiltering_component.cpp:119-146),
// shared by the standalone kernels (ingest.hip: gather_points_kernel; mapcloud.hip: deskew_kernel, transform_cloud_kernel) and the scan head kernel
// (filters.hip): ONE body each, so the fused call cannot round differently from the separate calls.  Likewise the other-robot test of
// MrgSlamComponent::cloud_callback (apps/mrg_slam_component.cpp:412-423), shared by near_flags_kernel and the keyframe head kernel (mapcloud.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "dev_float.h"
#include "dev_utils.h"

namespace mrgfe {

// pcl::fromROSMsg for point i of a PointCloud2 payload (:119-120): four 4-byte loads at the FLOAT32 field offsets of the strided record; a missing
// intensity field (oi < 0) stays at PointXYZI's default, 0.  Offsets and steps are multiples of 4 (check_pointcloud2_layout).
__device__ __forceinline__ float4 load_point_record(const uint8_t* __restrict__ raw, uint32_t i, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox, uint32_t oy,
                                                    uint32_t oz, int32_t oi)
{
    const uint32_t row = i / width, col = i - row * width;
    const uint8_t* p = raw + size_t(row) * row_step + size_t(col) * point_step;
    float4 o;
    o.x = *reinterpret_cast<const float*>(p + ox);
    o.y = *reinterpret_cast<const float*>(p + oy);
    o.z = *reinterpret_cast<const float*>(p + oz);
    o.w = oi >= 0 ? *reinterpret_cast<const float*>(p + oi) : 0.0f;
    return o;
}

// The same for a layout whose field offsets or steps are NOT multiples of 4 (mrgfe_ctx_set_byte_layouts: Velodyne's 22-byte XYZIRT records, 26-byte
// records with a FLOAT64 stamp; pcl::fromROSMsg copies a field wherever it sits).  `raw` is 4-byte aligned — every raw device buffer of the library
// starts on a 256-byte line — so the FLOAT32 at byte address a is in the aligned word a >> 2 and, when a & 3 is not 0, the word behind it: the two are
// shifted together.  At most two aligned words per field and never a word that holds none of the field's bytes, so nothing is read past
// round_up(payload bytes, 4), which every raw buffer has room for.  The result is the field's bits as they are: NaN payloads and denormals survive.
__device__ __forceinline__ float load_f32_at_byte(const uint32_t* __restrict__ words, size_t a)
{
    const size_t   w = a >> 2;
    const uint32_t s = 8u * (static_cast<uint32_t>(a) & 3u);
    uint32_t       v = words[w];
    if (s) v = (v >> s) | (words[w + 1] << (32u - s));
    return __uint_as_float(v);
}
__device__ __forceinline__ float4 load_point_record_bytes(const uint8_t* __restrict__ raw, uint32_t i, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox,
                                                          uint32_t oy, uint32_t oz, int32_t oi)
{
    const uint32_t  row = i / width, col = i - row * width;
    const size_t    at = size_t(row) * row_step + size_t(col) * point_step;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(raw);
    float4 o;
    o.x = load_f32_at_byte(words, at + ox);
    o.y = load_f32_at_byte(words, at + oy);
    o.z = load_f32_at_byte(words, at + oz);
    o.w = oi >= 0 ? load_f32_at_byte(words, at + static_cast<uint32_t>(oi)) : 0.0f;
    return o;
}
// the reader of a kernel's instantiation: kBytes is chosen on the host (ingest.h layout_is_strict), a strict layout always reads as it did
template <bool kBytes>
__device__ __forceinline__ float4 load_point_record_as(const uint8_t* __restrict__ raw, uint32_t i, uint32_t width, uint32_t row_step, uint32_t point_step, uint32_t ox, uint32_t oy,
                                                       uint32_t oz, int32_t oi)
{
    if (kBytes) return load_point_record_bytes(raw, i, width, row_step, point_step, ox, oy, oz, oi);
    return load_point_record(raw, i, width, row_step, point_step, ox, oy, oz, oi);
}

// PrefilteringComponent::deskewing (:272-290) for point i of a cloud of n points (n counts the non-finite points too): the point is rotated by the
// inverse of Quaternionf(1, dt/2 * w) with dt = scan_period * i / n; `av*` is the angular velocity ALREADY negated (:275).
__device__ __forceinline__ float4 deskew_point(float4 p, uint32_t i, uint32_t n, float avx, float avy, float avz, double scan_period)
{
#pragma clang fp contract(off)
    const double delta_t = scan_period * static_cast<double>(i) / static_cast<double>(n);  // prefiltering_component.cpp:289
    const float  qw = 1.0f;
    const float  qx = static_cast<float>(delta_t / 2.0 * static_cast<double>(avx)), qy = static_cast<float>(delta_t / 2.0 * static_cast<double>(avy)),
                 qz = static_cast<float>(delta_t / 2.0 * static_cast<double>(avz));
    float n2 = qx * qx + qy * qy;  // delta_q.inverse() = conjugate / squaredNorm
    n2 = n2 + qz * qz;
    n2 = n2 + qw * qw;
    const float ix = -qx / n2, iy = -qy / n2, iz = -qz / n2, iw = qw / n2;
    float uvx = iy * p.z - iz * p.y, uvy = iz * p.x - ix * p.z, uvz = ix * p.y - iy * p.x;  // uv = 2 * vec x v
    uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz;
    const float cx = iy * uvz - iz * uvy, cy = iz * uvx - ix * uvz, cz = ix * uvy - iy * uvx;
    return make_float4((p.x + iw * uvx) + cx, (p.y + iw * uvy) + cy, (p.z + iw * uvz) + cz, p.w);
}

// pcl::transformPointCloud on one point of a non-dense cloud: a non-finite point is left as it is, the intensity is copied.  T: row-major 3x4.
__device__ __forceinline__ float4 transform_finite_point(const float* __restrict__ T, float4 p)
{
    if (finite3(p.x, p.y, p.z)) {
        float x, y, z;
        transform_point(T, p.x, p.y, p.z, x, y, z);
        p.x = x; p.y = y; p.z = z;
    }
    return p;
}

// The other-robot test of MrgSlamComponent::cloud_callback for one point (apps/mrg_slam_component.cpp:412-423): 1 when the point lies inside the sphere of
// one of the K centres (sensor frame) — (point - centre).squaredNorm() < radius_sqr in float, unfused, the first hit ends the loop.  A non-finite point
// compares false against every centre and is kept.  The centres travel by value in the kernel's arguments.
constexpr int kMaxCentres = 64;
struct Centres { float xyz[kMaxCentres][3]; };
__device__ __forceinline__ uint32_t near_a_centre(float4 p, const Centres& c, int K, float radius_sqr)
{
#pragma clang fp contract(off)
    for (int k = 0; k < K; ++k) {
        const float dx = p.x - c.xyz[k][0], dy = p.y - c.xyz[k][1], dz = p.z - c.xyz[k][2];
        float s = dx * dx + dy * dy;  // (point - other).squaredNorm()
        s = s + dz * dz;
        if (s < radius_sqr) return 1u;  // :417-421
    }
    return 0u;
}

}  // namespace mrgfe
