// csrc/ground_fill.hip — first-keyframe ground fill: mrg_slam_pcl::fill_cloud (the reference's src/pcl/fill_ground_plane.cpp:49-65) on the GPU.
//
//   reference                                                   here
//   angle_inc = map_resolution / radius (:53)                   host, ground_fill_walk
//   for (r = map_resolution; r <= radius; r += ..) (:54)        host: the ACCUMULATED r of every ring -> table `ring_r`
//   for (angle = 0; angle < 2 * M_PI; angle += ..) (:56)        host: sin / cos (the C library's, as the reference's host) of every ACCUMULATED angle -> `angle_sc`
//   plane.projection(Vector3d(r, 0, 0)) (:55)                   ground_fill_kernel, per point (a dozen f64 operations: cheaper than a third table)
//   AngleAxis<double>(angle, normal).toRotationMatrix() * sample (:57)   ground_fill_kernel
//   p.x / p.y / p.z = rot[..] (double -> float), intensity 0 (:58-62)    ground_fill_kernel: one float4 store per point
//
// Everything on the device is IEEE f64 multiplication, addition and subtraction in a fixed order with contraction off, and one rounding to float: the
// output equals a host model (tests/ground_fill_reference.py) to the last bit.  No device sin / cos enters the result.
//
// Upstream arithmetic restated from recall, Eigen 3.3 [UPSTREAM-RECALL] (it is not in the reference tree) — all of it in ground_fill_point below:
//   * Hyperplane::projection(p) = p - signedDistance(p) * normal(), signedDistance(p) = normal().dot(p) + offset(): nothing normalises the normal;
//   * AngleAxis::toRotationMatrix(): sin_axis = sin(angle) * axis, c = cos(angle), cos1_axis = (1 - c) * axis, the off-diagonal pairs from
//     tmp = cos1_axis.x * axis.y / cos1_axis.x * axis.z / cos1_axis.y * axis.z (tmp -/+ sin_axis.z, tmp +/- sin_axis.y, tmp -/+ sin_axis.x), the
//     diagonal cos1_axis.cwiseProduct(axis) + c: the axis is used as it is given, so a normal that is not of unit length gives no rotation matrix;
//   * the 3x3 . 3 product and the dot product add their three terms left to right (Eigen's order for 3-vectors of doubles depends on its
//     vectorisation; this port states one).
#include <cmath>

#include "ground_fill.h"

namespace mrgfe {
namespace {

constexpr uint32_t kFillTile = 2048;  // points per workgroup of 256, as the keyframe kernels have it
constexpr uint64_t kMaxPointsFill = 0x7fffffffu;  // the kernels index points with 32-bit words
constexpr double   kMaxRingRatio = 1.0e5;  // radius / map_resolution beyond this: more than 2^31 points for certain (rings * angles ~ 2 pi ratio^2), not walked

// The two loops of fill_cloud (:53-56), walked as the reference walks them.  on_ring(r) / on_angle(angle) see the accumulated values.  Callers walk only
// ratios radius / map_resolution <= kMaxRingRatio: at most 1e5 rings and 6.3e5 angles, and every step moves the accumulated value.
template <class Ring, class Angle>
void ground_fill_walk(double radius, double map_resolution, uint64_t* n_rings, uint64_t* n_angles, Ring on_ring, Angle on_angle)
{
#pragma clang fp contract(off)
    const double angle_inc = map_resolution / radius;
    uint64_t     rings = 0, angles = 0;
    for (double r = map_resolution; r <= radius; r += map_resolution) {
        on_ring(r);
        ++rings;
    }
    for (double angle = 0; angle < 2 * M_PI; angle += angle_inc) {
        on_angle(angle);
        ++angles;
    }
    *n_rings = rings;
    *n_angles = angles;
}

// One point of the disc: ring radius r, sin / cos of the angle, the plane (normal n, offset d).  [UPSTREAM-RECALL] Eigen 3.3 Geometry/Hyperplane.h
// (projection) and Geometry/AngleAxis.h (toRotationMatrix), see the head of this file; the one place they are restated.
__device__ __forceinline__ float4 ground_fill_point(double r, double s, double c, double nx, double ny, double nz, double d)
{
#pragma clang fp contract(off)
    // sample = plane.projection(Vector3d(r, 0, 0))
    const double px = r, py = 0.0, pz = 0.0;
    const double sd = ((nx * px + ny * py) + nz * pz) + d;
    const double sx = px - sd * nx, sy = py - sd * ny, sz = pz - sd * nz;
    // AngleAxis<double>(angle, normal).toRotationMatrix()
    const double sin_x = s * nx, sin_y = s * ny, sin_z = s * nz;
    const double c1 = 1.0 - c;
    const double cos1_x = c1 * nx, cos1_y = c1 * ny, cos1_z = c1 * nz;
    double       tmp = cos1_x * ny;
    const double r01 = tmp - sin_z, r10 = tmp + sin_z;
    tmp = cos1_x * nz;
    const double r02 = tmp + sin_y, r20 = tmp - sin_y;
    tmp = cos1_y * nz;
    const double r12 = tmp - sin_x, r21 = tmp + sin_x;
    const double r00 = cos1_x * nx + c, r11 = cos1_y * ny + c, r22 = cos1_z * nz + c;
    // rot = R * sample
    const double ox = (r00 * sx + r01 * sy) + r02 * sz;
    const double oy = (r10 * sx + r11 * sy) + r12 * sz;
    const double oz = (r20 * sx + r21 * sy) + r22 * sz;
    return make_float4(static_cast<float>(ox), static_cast<float>(oy), static_cast<float>(oz), 0.0f);
}

// One thread per generated point, 2048 points per workgroup: point i is (ring i / n_angles, angle i % n_angles), rings outermost.  Neighbouring lanes
// store neighbouring float4s; the tables are a few KB read through L1 (the ring entry is the same for nearly every lane of a wave).
__global__ __launch_bounds__(256) void ground_fill_kernel(const double* __restrict__ ring_r, const double2* __restrict__ angle_sc, uint32_t n_rings, uint32_t n_angles,
                                                          double nx, double ny, double nz, double d, float4* __restrict__ out)
{
    const uint32_t total = n_rings * n_angles;  // <= 2^31 - 1 (ground_fill_counts)
    const uint32_t base = blockIdx.x * kFillTile + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < kFillTile / 256; ++k) {
        const uint32_t i = base + k * 256;
        if (i >= total) continue;
        const uint32_t ring = i / n_angles, angle = i - ring * n_angles;
        const double2  sc = angle_sc[angle];
        out[i] = ground_fill_point(ring_r[ring], sc.x, sc.y, nx, ny, nz, d);
    }
}

}  // namespace

int ground_fill_check(const mrgfe_ground_fill_params* p, const char* fn)
{
    if (!std::isfinite(p->radius) || !std::isfinite(p->map_resolution) || !(p->radius > 0) || !(p->map_resolution > 0)) {
        set_error("%s: radius %g and map_resolution %g must be finite and > 0 (the reference's loops would not end)", fn, p->radius, p->map_resolution);
        return MRGFE_ERR_INVALID;
    }
    return MRGFE_OK;
}

int ground_fill_counts(const mrgfe_ground_fill_params* p, uint64_t n_before, uint32_t* n_rings, uint32_t* n_angles, const char* fn)
{
    *n_rings = 0;
    *n_angles = 0;
    uint64_t rings = 0, angles = 0;
    const bool walked = p->radius / p->map_resolution <= kMaxRingRatio;
    if (walked) ground_fill_walk(p->radius, p->map_resolution, &rings, &angles, [](double) {}, [](double) {});
    if (!walked || n_before + rings * angles > kMaxPointsFill) {
        set_error("%s: radius %g at map_resolution %g behind %llu points: more than 2^31 - 1 points", fn, p->radius, p->map_resolution, static_cast<unsigned long long>(n_before));
        return MRGFE_ERR_INVALID;
    }
    *n_rings = static_cast<uint32_t>(rings);
    *n_angles = static_cast<uint32_t>(angles);
    return MRGFE_OK;
}

int ground_fill_device(mrgfe_ctx* ctx, const mrgfe_ground_fill_params* p, const double normal[3], double offset, uint32_t n_rings, uint32_t n_angles, float4* d_dst)
{
    const uint64_t total = uint64_t(n_rings) * n_angles;
    if (total == 0) return MRGFE_OK;
    if (total > kMaxPointsFill || !d_dst) { set_error("ground fill: %llu points", static_cast<unsigned long long>(total)); return MRGFE_ERR_INVALID; }
    std::vector<double> tab, ring;  // (sin, cos) [n_angles] first — the kernel reads them as 16-byte pairs —, then r [n_rings]
    tab.reserve(2 * size_t(n_angles) + size_t(n_rings));
    ring.reserve(n_rings);
    uint64_t rings = 0, angles = 0;
    ground_fill_walk(p->radius, p->map_resolution, &rings, &angles, [&](double r) { ring.push_back(r); },
                     [&](double a) { tab.push_back(std::sin(a)); tab.push_back(std::cos(a)); });
    if (rings != n_rings || angles != n_angles) { set_error("ground fill: the counts do not belong to these parameters"); return MRGFE_ERR_INVALID; }
    tab.insert(tab.end(), ring.begin(), ring.end());
    DevBuf& dtab = ctx->gf_tab;
    MRGFE_TRY(dtab.ensure(tab.size() * sizeof(double)));
    MRGFE_TRY(ctx->stage_h2d(dtab.p, tab.data(), tab.size() * sizeof(double), ctx->stream));
    const double2* d_sc = dtab.as<double2>();
    const double*  d_ring = dtab.as<double>() + 2 * size_t(n_angles);
    hipLaunchKernelGGL(ground_fill_kernel, dim3(static_cast<uint32_t>((total + kFillTile - 1) / kFillTile)), dim3(256), 0, ctx->stream, d_ring, d_sc, n_rings, n_angles,
                       normal[0], normal[1], normal[2], offset, d_dst);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

}  // namespace mrgfe
