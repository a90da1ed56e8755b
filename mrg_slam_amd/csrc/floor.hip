// csrc/floor.hip — FloorDetectionComponent::detect (the reference's apps/floor_detection_component.cpp:100-183) on the GPU.
//
//   tilt + height band (:103-113, plane_clip :192-208)  floor_band_kernel -> compact_by_flags (order kept, as ExtractIndices)
//   ... on the message's bytes (cloud_callback :72)      floor_head_kernel<kBytes>: pcl::fromROSMsg, the tilt and the band flag in one pass over the records
//   normal_filtering (:216-243)                          NnGrid k = 10 -> floor_normals_kernel (PCL's float covariance, eigen33) -> compact_by_flags
//   transform back (:124)                                floor_transform_kernel
//   RandomSampleConsensus (:139-145)                     floor_sample_kernel (one wave: MT19937 + the index swaps) -> floor_count_kernel
//                                                        (hypotheses x points) -> the adaptive stop rule replayed on the host after each wave
//   getInliers / floor_points (:146-180)                 floor_inlier_kernel -> compact_by_flags
//
// Upstream arithmetic restated from recall, PCL 1.12.1 / Eigen 3.3 [UPSTREAM-RECALL] (it is not in the reference tree):
//   - RandomSampleConsensus::computeModel: max_iterations_ 10000, probability_ 0.99, max_skip = 10 * max_iterations_;
//     `while (iterations_ < k && skipped_count < max_skip)`; a sample whose coefficients cannot be computed counts as skipped and does not
//     advance iterations_; after the better-model test `++iterations_; if (iterations_ > max_iterations_) break;`;
//     k = log(1 - p) / log(clamp(1 - w^3, eps, 1 - eps)) in double, w = best inlier count / N.
//   - SampleConsensusModel: boost::mt19937 seeded 12345 in every new model; rnd() = uniform_int<>(0, INT_MAX) over it, which is mt() >> 1
//     (boost's bucket size for 2^32 -> 2^31 values is 2); drawIndexSample swaps shuffled_indices_[i] <-> shuffled_indices_[i + rnd() % (N - i)],
//     i = 0, 1, 2, on an identity permutation that keeps its swaps from one draw to the next; getSamples draws up to 1000 times until
//     isSampleGood passes, and gives up (no samples: computeModel stops) after that; with N < 3 it sets iterations_ = INT_MAX - 1 and gives up.
//   - SampleConsensusModelPlane::isSampleGood: the ratio test dy1dy2 = (p1 - p0) / (p2 - p0) (Array4f), good iff
//     dy1dy2[0] != dy1dy2[1] || dy1dy2[2] != dy1dy2[1].  computeModelCoefficients: cross = (p1 - p0) x (p2 - p0), crossNorm = cross.stableNorm(),
//     fails iff crossNorm < 1e-5 (dummy_precision) — that failure is the "skipped" sample; n = cross / crossNorm, d = -1 * n . p0.
//   - countWithinDistance / selectWithinDistance: |c . (x, y, z, 1)| < threshold with Eigen's SSE Vector4f dot, (c0 x + c2 z) + (c1 y + c3).
//     (Builds whose countWithinDistance takes the SSE / AVX four-point path sum (c0 x + c1 y) + (c2 z + c3) there; this port uses one form for both.)
//   - computeMeanAndCovarianceMatrix (float, 1.11+ form): sums of the neighbours' coordinates shifted by the FIRST neighbour, in neighbour order,
//     divided by the count; pcl::eigen33 (scaled matrix, computeRoots / computeRoots2, the longest of the three row cross products) gives the
//     normal.  Device atan2f / sinf / cosf are not glibc's: normals agree with the reference to a few ulp, not bit for bit.
//   - transformPointCloud (SSE): x' = m00 x + (m01 y + (m02 z + m03)) (dev_float.h transform_point).
//   - tilt_matrix.inverse() is taken as the transpose of the rotation (exact for tilt 0; Eigen's cofactor inverse may differ in the last ulp).
#include "floor.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <limits>
#include <vector>

#include "dev_float.h"
#include "filters.h"
#include "ingest.h"
#include "nn_grid.h"
#include "scan_point.h"

namespace mrgfe {

namespace {

constexpr int      kFloorK = 10;         // ne.setKSearch(10) (:230)
constexpr int      kPPT = 4;             // points per thread in the count kernel
constexpr uint32_t kHypPerBlock = 256;   // hypotheses per workgroup row of the count kernel
constexpr int      kMaxIterations = 10000;
constexpr double   kProbability = 0.99;
constexpr int      kMaxSkip = 10 * kMaxIterations;
constexpr int      kMaxSampleChecks = 1000;
// RANSAC waves: the first decides the usual case (w ~ 0.5 - 0.9 stops within 4 - 35 iterations); later ones grow so that a low inlier ratio
// (up to 10001 iterations, or 100000 skipped samples) costs a few host round trips, not hundreds
constexpr uint32_t kWaves[] = {64, 512, 4096, 16384};
constexpr uint32_t kMaxWave = 16384;

enum : int32_t { kHypNoSample = 0, kHypModel = 1, kHypSkipped = 2 };
struct FloorHyp {  // one RANSAC iteration as the sampler left it
    int32_t idx[3];
    int32_t status;
    float   c[4];
};
static_assert(sizeof(FloorHyp) == 32, "FloorHyp layout");

struct Rot12 { float m[12]; };  // row-major 3 x 4

// tilt + height band for one point (:109-112): ONE body for the band kernel and the head kernel, so the route over the message's bytes cannot round or
// flag differently from the route over a packed cloud
__device__ __forceinline__ void floor_band_point(const Rot12& T, float4 p, float lo, float hi, float4* __restrict__ out, uint32_t* __restrict__ flag)
{
#pragma clang fp contract(off)
    float x, y, z;
    transform_point(T.m, p.x, p.y, p.z, x, y, z);  // pcl::transformPointCloud(*cloud, *filtered, tilt_matrix) (:109)
    *out = make_float4(x, y, z, p.w);
    // PlaneClipper3D::clipPoint3D with plane (0, 0, 1, d): (0 x + 0 y + 1 z) >= -d.  Kept by the first clip (d = h + r, :111) and not removed by the
    // second (d = h - r, setNegative(true), :112)
    const float h = dot3f(0.0f, x, 0.0f, y, 1.0f, z);
    *flag = (h >= lo && !(h >= hi)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void floor_band_kernel(const float4* __restrict__ in, uint32_t n, Rot12 T, float lo, float hi, float4* __restrict__ out,
                                                         uint32_t* __restrict__ flags)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    floor_band_point(T, in[i], lo, hi, out + i, flags + i);
}

// The head of FloorDetectionComponent::cloud_callback on the message's bytes (:72 pcl::fromROSMsg, then :109-112): point i is read out of its strided
// record (scan_point.h load_point_record_as, the body every reader of PointCloud2 bytes uses), tilted and flagged as floor_band_kernel does.  One point
// per thread; reads 16 B of fields (within point_step bytes of record), writes 16 + 4 B.  No LDS, no atomics.
// kBytes: the layout is not a strict one (ingest.h layout_is_strict) and the record's fields are put together from aligned words.
struct FloorHeadArgs {
    const uint8_t* raw;
    uint32_t       n, width, row_step, point_step, ox, oy, oz;
    int32_t        oi;
};
template <bool kBytes>
__global__ __launch_bounds__(256) void floor_head_kernel(const FloorHeadArgs a, Rot12 T, float lo, float hi, float4* __restrict__ out, uint32_t* __restrict__ flags)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const float4 p = load_point_record_as<kBytes>(a.raw, i, a.width, a.row_step, a.point_step, a.ox, a.oy, a.oz, a.oi);
    floor_band_point(T, p, lo, hi, out + i, flags + i);
}

__global__ __launch_bounds__(256) void floor_transform_kernel(const float4* __restrict__ in, uint32_t n, Rot12 T, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    float x, y, z;
    transform_point(T.m, p.x, p.y, p.z, x, y, z);
    out[i] = make_float4(x, y, z, p.w);
}

// pcl::computeRoots2
__device__ __forceinline__ void roots2(float b, float c, float r[3])
{
#pragma clang fp contract(off)
    r[0] = 0.0f;
    float d = static_cast<float>(static_cast<double>(b * b) - 4.0 * static_cast<double>(c));
    if (d < 0.0f) d = 0.0f;
    const float sd = sqrtf(d);
    r[2] = 0.5f * (b + sd);
    r[1] = 0.5f * (b - sd);
}

// pcl::eigen33(mat, eigenvalue, eigenvector): the eigenvector of the smallest eigenvalue of a symmetric 3 x 3 (row-major m)
__device__ void eigen33_smallest(const float m[9], float v[3])
{
#pragma clang fp contract(off)
    float scale = 0.0f;
    for (int i = 0; i < 9; ++i) scale = fmaxf(scale, fabsf(m[i]));
    if (scale <= FLT_MIN) scale = 1.0f;
    float s[9];
    for (int i = 0; i < 9; ++i) s[i] = m[i] / scale;
    // computeRoots
    const float m00 = s[0], m01 = s[1], m02 = s[2], m11 = s[4], m12 = s[5], m22 = s[8];
    const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
    const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
    const float c2 = m00 + m11 + m22;
    float r[3];
    if (fabsf(c0) < FLT_EPSILON) {
        roots2(c2, c1, r);
    } else {
        const float s_inv3 = static_cast<float>(1.0 / 3.0);
        const float s_sqrt3 = sqrtf(3.0f);
        const float c2_over_3 = c2 * s_inv3;
        float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
        if (a_over_3 > 0.0f) a_over_3 = 0.0f;
        const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
        float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
        if (q > 0.0f) q = 0.0f;
        const float rho = sqrtf(-a_over_3);
        const float theta = atan2f(sqrtf(-q), half_b) * s_inv3;
        const float cos_t = cosf(theta), sin_t = sinf(theta);
        r[0] = c2_over_3 + 2.0f * rho * cos_t;
        r[1] = c2_over_3 - rho * (cos_t + s_sqrt3 * sin_t);
        r[2] = c2_over_3 - rho * (cos_t - s_sqrt3 * sin_t);
        float t;
        if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
        if (r[1] >= r[2]) {
            t = r[1]; r[1] = r[2]; r[2] = t;
            if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
        }
        if (r[0] <= 0.0f) roots2(c2, c1, r);
    }
    s[0] -= r[0];
    s[4] -= r[0];
    s[8] -= r[0];
    float vec[3][3];
    const float* a[3] = {s, s, s + 3};
    const float* b[3] = {s + 3, s + 6, s + 6};
    float len[3];
    for (int j = 0; j < 3; ++j) {
        vec[j][0] = a[j][1] * b[j][2] - a[j][2] * b[j][1];
        vec[j][1] = a[j][2] * b[j][0] - a[j][0] * b[j][2];
        vec[j][2] = a[j][0] * b[j][1] - a[j][1] * b[j][0];
        len[j] = vec[j][0] * vec[j][0] + vec[j][1] * vec[j][1] + vec[j][2] * vec[j][2];
    }
    const int pick = (len[0] >= len[1] && len[0] >= len[2]) ? 0 : (len[1] >= len[0] && len[1] >= len[2]) ? 1 : 2;
    const float l = sqrtf(len[pick]);
    v[0] = vec[pick][0] / l;
    v[1] = vec[pick][1] / l;
    v[2] = vec[pick][2] / l;
}

// NormalEstimation::computePointNormal over the k = 10 neighbours of point i (ascending by (distance, index): the point itself first unless it has a
// duplicate of lower index), then normal_filtering's test |normalized(n) . z| > cos(thresh) in double (a NaN normal fails it)
__global__ __launch_bounds__(256) void floor_normals_kernel(const float4* __restrict__ pts, uint32_t n, const int32_t* __restrict__ nbr, double cos_thr,
                                                            float4* __restrict__ normals, uint32_t* __restrict__ keep)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int32_t* nb = nbr + size_t(i) * kFloorK;
    float          nx = __builtin_nanf(""), ny = nx, nz = nx;
    int            cnt = 0;
    float          kx = 0, ky = 0, kz = 0;
    float          acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < kFloorK; ++j) {
        const int32_t q = nb[j];
        if (q < 0 || static_cast<uint32_t>(q) >= n) continue;
        const float4 p = pts[q];
        if (cnt == 0) { kx = p.x; ky = p.y; kz = p.z; }  // K = the first neighbour
        const float x = p.x - kx, y = p.y - ky, z = p.z - kz;
        acc[0] += x * x; acc[1] += x * y; acc[2] += x * z;
        acc[3] += y * y; acc[4] += y * z; acc[5] += z * z;
        acc[6] += x; acc[7] += y; acc[8] += z;
        ++cnt;
    }
    if (cnt >= 3) {
        const float c = static_cast<float>(cnt);
        for (int j = 0; j < 9; ++j) acc[j] /= c;
        float m[9];
        m[0] = acc[0] - acc[6] * acc[6];
        m[1] = acc[1] - acc[6] * acc[7];
        m[2] = acc[2] - acc[6] * acc[8];
        m[4] = acc[3] - acc[7] * acc[7];
        m[5] = acc[4] - acc[7] * acc[8];
        m[8] = acc[5] - acc[8] * acc[8];
        m[3] = m[1]; m[6] = m[2]; m[7] = m[5];
        float v[3];
        eigen33_smallest(m, v);
        nx = v[0]; ny = v[1]; nz = v[2];
    }
    if (normals) normals[i] = make_float4(nx, ny, nz, 0.0f);
    // getNormalVector3fMap().normalized().dot(UnitZ())
    const float sq = nx * nx + ny * ny + nz * nz;
    float ux = nx, uy = ny, uz = nz;
    if (sq > 0.0f) {
        const float r = sqrtf(sq);
        ux /= r; uy /= r; uz /= r;
    }
    const float d = dot3f(ux, 0.0f, uy, 0.0f, uz, 1.0f);
    keep[i] = (fabs(static_cast<double>(d)) > cos_thr) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void floor_iota_kernel(uint32_t* __restrict__ a, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) a[i] = i;
}

// MT19937 over a 624-word state in LDS, shared by the 64 lanes of the sampler wave: every lane runs the same sequential program on the same values
// (uniform control flow), and only the twist is split among them — in three phases whose inputs the sequential twist has already produced
// (words 0..226 read the old words + 397; 227..453 the new words - 227; 454..623 the new words - 227 and, for 623, the new word 0)
struct Mt {
    uint32_t* s;    // LDS, 624 words
    uint32_t  mti;  // uniform
    __device__ void twist_phase(int begin, int end)
    {
        uint32_t v[4];
        const int lane = threadIdx.x;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = begin + lane + 64 * u;
            if (kk < end) {
                const uint32_t y = (s[kk] & 0x80000000u) | (s[(kk + 1) % 624] & 0x7fffffffu);
                v[u] = s[(kk + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = begin + lane + 64 * u;
            if (kk < end) s[kk] = v[u];
        }
        __syncthreads();
    }
    __device__ uint32_t next()
    {
        if (mti >= 624) {
            twist_phase(0, 227);
            twist_phase(227, 454);
            twist_phase(454, 624);
            mti = 0;
        }
        uint32_t y = s[mti++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
};

// the plane of three points: SampleConsensusModelPlane::computeModelCoefficients (false: the cross product's stableNorm < 1e-5)
__device__ bool plane_from_sample(float4 p0, float4 p1, float4 p2, float c[4])
{
#pragma clang fp contract(off)
    const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
    const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    // Eigen stableNorm (one block): scale = max |v_i|, invScale = 1 / scale, scale * sqrt(sum (v_i * invScale)^2)
    const float mx = fmaxf(fmaxf(fabsf(cx), fabsf(cy)), fabsf(cz));
    float       scale = 0.0f, inv = 1.0f;
    if (mx > 0.0f) {
        const float tmp = 1.0f / mx;
        if (tmp > FLT_MAX) { inv = FLT_MAX; scale = 1.0f / inv; }
        else if (mx > FLT_MAX) { inv = 1.0f; scale = mx; }
        else { scale = mx; inv = tmp; }
    } else if (mx != mx) {
        scale = mx;
    }
    float ssq = 0.0f;
    if (scale > 0.0f) {
        const float sx = cx * inv, sy = cy * inv, sz = cz * inv;
        ssq = ssq + (sx * sx + sy * sy + sz * sz);
    }
    const float norm = scale * sqrtf(ssq);
    if (norm < 1e-5f) return false;
    c[0] = cx / norm;
    c[1] = cy / norm;
    c[2] = cz / norm;
    c[3] = -1.0f * dot3f(c[0], p0.x, c[1], p0.y, c[2], p0.z);
    return true;
}

// SampleConsensusModelPlane::isSampleGood: (p1 - p0) / (p2 - p0) over x, y, z
__device__ __forceinline__ bool sample_good(float4 p0, float4 p1, float4 p2)
{
#pragma clang fp contract(off)
    const float d0 = (p1.x - p0.x) / (p2.x - p0.x);
    const float d1 = (p1.y - p0.y) / (p2.y - p0.y);
    const float d2 = (p1.z - p0.z) / (p2.z - p0.z);
    return (d0 != d1) || (d2 != d1);
}

// H iterations of getSamples + computeModelCoefficients, in order, continuing from the generator state and the permutation a previous wave left
__global__ __launch_bounds__(64) void floor_sample_kernel(const float4* __restrict__ pts, uint32_t n, uint32_t* __restrict__ shuffled, uint32_t* __restrict__ mt_state,
                                                          int first, uint32_t H, FloorHyp* __restrict__ hyps)
{
#pragma clang fp contract(off)
    __shared__ uint32_t s[624];
    const int lane = threadIdx.x;
    Mt        mt{s, 0};
    if (first) {
        if (lane == 0) {  // boost::mt19937::seed(12345u)
            s[0] = 12345u;
            for (uint32_t i = 1; i < 624; ++i) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + i;
        }
        mt.mti = 624;
    } else {
        for (int i = lane; i < 624; i += 64) s[i] = mt_state[i];
        mt.mti = mt_state[624];
    }
    __syncthreads();
    uint32_t h = 0;
    for (; h < H; ++h) {
        FloorHyp out;
        out.status = kHypNoSample;
        out.idx[0] = out.idx[1] = out.idx[2] = -1;
        out.c[0] = out.c[1] = out.c[2] = out.c[3] = 0.0f;
        if (n >= 3) {
            for (int attempt = 0; attempt < kMaxSampleChecks; ++attempt) {
                for (uint32_t i = 0; i < 3; ++i) {  // drawIndexSample: every lane makes the same swap (same addresses, same values)
                    const uint32_t j = i + (mt.next() >> 1) % (n - i);
                    const uint32_t a = shuffled[i], b = shuffled[j];
                    shuffled[i] = b;
                    shuffled[j] = a;
                }
                const uint32_t i0 = shuffled[0], i1 = shuffled[1], i2 = shuffled[2];
                const float4   p0 = pts[i0], p1 = pts[i1], p2 = pts[i2];
                if (!sample_good(p0, p1, p2)) continue;
                out.idx[0] = static_cast<int32_t>(i0);
                out.idx[1] = static_cast<int32_t>(i1);
                out.idx[2] = static_cast<int32_t>(i2);
                out.status = plane_from_sample(p0, p1, p2, out.c) ? kHypModel : kHypSkipped;
                break;
            }
        }
        if (lane == 0) hyps[h] = out;
        if (out.status == kHypNoSample) break;  // computeModel stops here: the rest of the wave is not drawn
    }
    for (uint32_t r = h + 1 + lane; r < H; r += 64) hyps[r].status = kHypNoSample;
    __syncthreads();
    for (int i = lane; i < 624; i += 64) mt_state[i] = s[i];
    if (lane == 0) mt_state[624] = mt.mti;
}

// |c . (x, y, z, 1)| with Eigen's SSE Vector4f dot: (c0 x + c2 z) + (c1 y + c3)
__device__ __forceinline__ float plane_dist(const float c[4], float x, float y, float z)
{
#pragma clang fp contract(off)
    const float a = c[0] * x, b = c[1] * y, cz = c[2] * z, d = c[3] * 1.0f;
    return fabsf((a + cz) + (b + d));
}

// inlier counts of hypotheses [blockIdx.y * kHypPerBlock, +kHypPerBlock) over a tile of 256 * kPPT points: one ballot + popcount per point slot and
// one atomic per wave and hypothesis
__global__ __launch_bounds__(256) void floor_count_kernel(const float4* __restrict__ pts, uint32_t n, const FloorHyp* __restrict__ hyps, uint32_t H, double thr,
                                                          uint32_t* __restrict__ counts)
{
    const uint32_t base = blockIdx.x * (256u * kPPT) + threadIdx.x;
    float          px[kPPT], py[kPPT], pz[kPPT];
    bool           ok[kPPT];
#pragma unroll
    for (int u = 0; u < kPPT; ++u) {
        const uint32_t i = base + 256u * u;
        ok[u] = i < n;
        const float4 p = ok[u] ? pts[i] : make_float4(0, 0, 0, 0);
        px[u] = p.x; py[u] = p.y; pz[u] = p.z;
    }
    const uint32_t h0 = blockIdx.y * kHypPerBlock, h1 = min(H, h0 + kHypPerBlock);
    for (uint32_t h = h0; h < h1; ++h) {
        const FloorHyp hy = hyps[h];
        if (hy.status != kHypModel) continue;
        uint32_t c = 0;
#pragma unroll
        for (int u = 0; u < kPPT; ++u) c += __popcll(__ballot(ok[u] && static_cast<double>(plane_dist(hy.c, px[u], py[u], pz[u])) < thr));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[h], c);
    }
}

// selectWithinDistance of the winning plane
__global__ __launch_bounds__(256) void floor_inlier_kernel(const float4* __restrict__ pts, uint32_t n, float c0, float c1, float c2, float c3, double thr,
                                                           uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const float  c[4] = {c0, c1, c2, c3};
    flags[i] = static_cast<double>(plane_dist(c, p.x, p.y, p.z)) < thr ? 1u : 0u;
}

inline dim3 blocks(uint32_t n) { return dim3((n + 255) / 256); }

int ensure_events(mrgfe_ctx* ctx)
{
    for (auto& e : ctx->fl_ev)
        if (!e) MRGFE_HIP_CHECK(hipEventCreate(&e));
    return MRGFE_OK;
}

}  // namespace

int floor_normals_device(mrgfe_ctx* ctx, const float4* d_pts, uint32_t n, double normal_filter_thresh_deg, float4* d_normals, uint32_t* d_keep)
{
    if (n == 0) return MRGFE_OK;
    NnGrid& grid = ctx_tmp_grid(ctx);
    MRGFE_TRY(grid.build(ctx, d_pts, n, 1.0f, NnGrid::kCrowdingKnn));
    DevBuf &di = ctx->fl_buf[3], &dd = ctx->fl_buf[4];
    MRGFE_TRY(di.ensure(size_t(n) * kFloorK * 4));
    MRGFE_TRY(dd.ensure(size_t(n) * kFloorK * 4));
    MRGFE_TRY(grid.knn_device(ctx, d_pts, n, kFloorK, di.as<int32_t>(), dd.as<float>()));
    const double cos_thr = std::cos(normal_filter_thresh_deg * M_PI / 180.0);  // :238
    hipLaunchKernelGGL(floor_normals_kernel, blocks(n), dim3(256), 0, ctx->stream, d_pts, n, di.as<int32_t>(), cos_thr, d_normals, d_keep);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

int floor_ransac_device(mrgfe_ctx* ctx, const float4* d_pts, uint32_t n, double threshold, uint32_t* d_inlier_flags, FloorRansacOut* out)
{
    *out = FloorRansacOut{};
    hipStream_t st = ctx->stream;
    DevBuf &dsh = ctx->fl_buf[5], &dmt = ctx->fl_buf[6], &dhyp = ctx->fl_buf[7], &dcnt = ctx->fl_buf[8];
    MRGFE_TRY(dsh.ensure(size_t(n > 0 ? n : 1) * 4));
    MRGFE_TRY(dmt.ensure(625 * 4));
    MRGFE_TRY(dhyp.ensure(size_t(kMaxWave) * sizeof(FloorHyp)));
    MRGFE_TRY(dcnt.ensure(size_t(kMaxWave) * 4));
    MRGFE_TRY(ctx->fl_pin.ensure(size_t(kMaxWave) * (sizeof(FloorHyp) + 4)));
    FloorHyp* h_hyp = ctx->fl_pin.as<FloorHyp>();
    uint32_t* h_cnt = reinterpret_cast<uint32_t*>(h_hyp + kMaxWave);
    if (n > 0) {
        hipLaunchKernelGGL(floor_iota_kernel, blocks(n), dim3(256), 0, st, dsh.as<uint32_t>(), n);
        MRGFE_HIP_CHECK(hipGetLastError());
    }
    const double log_probability = std::log(1.0 - kProbability);
    const double one_over_indices = 1.0 / static_cast<double>(n);
    double       k = DBL_MAX;
    int32_t      iterations = 0, skipped = 0;
    uint32_t     best = 0;
    int          wave = 0;
    uint32_t     avail = 0, pos = 0;
    while (iterations < k && skipped < kMaxSkip) {
        if (pos == avail) {  // draw and count the next wave of hypotheses
            const uint32_t H = kWaves[wave < 3 ? wave : 3];
            hipLaunchKernelGGL(floor_sample_kernel, dim3(1), dim3(64), 0, st, d_pts, n, dsh.as<uint32_t>(), dmt.as<uint32_t>(), wave == 0 ? 1 : 0, H, dhyp.as<FloorHyp>());
            MRGFE_HIP_CHECK(hipGetLastError());
            MRGFE_HIP_CHECK(hipMemsetAsync(dcnt.p, 0, size_t(H) * 4, st));
            if (n > 0) {
                const dim3 grid((n + 256 * kPPT - 1) / (256 * kPPT), (H + kHypPerBlock - 1) / kHypPerBlock);
                hipLaunchKernelGGL(floor_count_kernel, grid, dim3(256), 0, st, d_pts, n, dhyp.as<FloorHyp>(), H, threshold, dcnt.as<uint32_t>());
                MRGFE_HIP_CHECK(hipGetLastError());
            }
            MRGFE_HIP_CHECK(hipMemcpyAsync(h_hyp, dhyp.p, size_t(H) * sizeof(FloorHyp), hipMemcpyDeviceToHost, st));
            MRGFE_HIP_CHECK(hipMemcpyAsync(h_cnt, dcnt.p, size_t(H) * 4, hipMemcpyDeviceToHost, st));
            MRGFE_HIP_CHECK(hipStreamSynchronize(st));
            ctx->fl_stats[4] += 1;  // host waits
            ctx->fl_stats[5] += 1;  // waves
            ctx->fl_stats[6] += H;  // hypotheses drawn
            ++wave;
            avail = H;
            pos = 0;
        }
        const FloorHyp& hy = h_hyp[pos];
        const uint32_t  cnt = h_cnt[pos];
        ++pos;
        if (hy.status == kHypNoSample) {
            if (n < 3) iterations = INT_MAX - 1;  // getSamples: "one of these will make it stop"
            break;
        }
        if (hy.status == kHypSkipped) {
            ++skipped;
            continue;
        }
        if (cnt > best) {
            best = cnt;
            out->has_model = 1;
            for (int j = 0; j < 4; ++j) out->coeffs[j] = hy.c[j];
            const double w = static_cast<double>(best) * one_over_indices;
            double p_no_outliers = 1.0 - std::pow(w, 3.0);
            p_no_outliers = std::max(std::numeric_limits<double>::epsilon(), p_no_outliers);
            p_no_outliers = std::min(1.0 - std::numeric_limits<double>::epsilon(), p_no_outliers);
            k = log_probability / std::log(p_no_outliers);
        }
        ++iterations;
        if (iterations > kMaxIterations) break;
    }
    out->iterations = iterations;
    out->skipped = skipped;
    out->n_inliers = out->has_model ? best : 0;  // selectWithinDistance uses the arithmetic of the count
    if (out->has_model && d_inlier_flags && n > 0) {
        hipLaunchKernelGGL(floor_inlier_kernel, blocks(n), dim3(256), 0, st, d_pts, n, out->coeffs[0], out->coeffs[1], out->coeffs[2], out->coeffs[3], threshold,
                           d_inlier_flags);
        MRGFE_HIP_CHECK(hipGetLastError());
    }
    return MRGFE_OK;
}

// detect() behind its first stage.  `head(T, lo, hi, d_tilt, d_flags)` queues on the context's stream whatever leaves the n_in tilted points and their
// height-band flags in those two buffers (floor_detect: floor_band_kernel over a packed cloud; floor_callback: the upload and floor_head_kernel over the
// message's records); everything from the band's compaction on — normal filter, inverse tilt, RANSAC, verticality, inlier extraction, the event timings,
// fl_stats — is this one body for both routes.
template <class Head>
static int floor_detect_behind(mrgfe_ctx* ctx, const mrgfe_floor_params* p, size_t n_in, Head&& head, mrgfe_floor_result* res, float* out_filtered, float* out_inliers)
{
    std::memset(res, 0, sizeof(*res));
    for (double& s : ctx->fl_stats) s = 0;
    if (n_in == 0) { res->reason = MRGFE_FLOOR_EMPTY_INPUT; return MRGFE_OK; }  // cloud_callback :74-77
    const uint32_t n = static_cast<uint32_t>(n_in);
    hipStream_t    st = ctx->stream;
    MRGFE_TRY(ensure_events(ctx));
    MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[0], st));
    // tilt_matrix: AngleAxisf(tilt_deg * M_PI / 180.0f, UnitY).toRotationMatrix() (:103-106)
    const float a = static_cast<float>(p->tilt_deg * M_PI / 180.0f);
    const float sn = std::sin(a), cs = std::cos(a);
    const float r11 = (1.0f - cs) * 1.0f + cs;
    const Rot12 T = {{cs, 0.0f, sn, 0.0f, 0.0f, r11, 0.0f, 0.0f, -sn, 0.0f, cs, 0.0f}};
    const Rot12 Ti = {{cs, 0.0f, -sn, 0.0f, 0.0f, r11, 0.0f, 0.0f, sn, 0.0f, cs, 0.0f}};  // tilt_matrix.inverse(): the transpose
    const float lo = -static_cast<float>(p->sensor_height + p->height_clip_range);  // -plane[3] of Vector4f(0, 0, 1, h + r)
    const float hi = -static_cast<float>(p->sensor_height - p->height_clip_range);
    DevBuf &dtilt = ctx->fl_buf[0], &dflags = ctx->fl_buf[1], &dband = ctx->fl_buf[2], &dfilt = ctx->fl_buf[9];
    MRGFE_TRY(dtilt.ensure(size_t(n) * 16));
    MRGFE_TRY(dflags.ensure(size_t(n) * 4));
    MRGFE_TRY(dband.ensure(size_t(n) * 16));
    MRGFE_TRY(dfilt.ensure(size_t(n) * 16));
    MRGFE_TRY(head(T, lo, hi, dtilt.as<float4>(), dflags.as<uint32_t>()));
    uint32_t n_clip = 0;
    MRGFE_TRY(compact_by_flags(ctx, dtilt.as<float4>(), n, dflags.as<uint32_t>(), dband.as<float4>(), &n_clip));
    ctx->fl_stats[4] += 1;
    MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[1], st));
    res->n_clipped = n_clip;
    if (n_clip == 0) {
        res->reason = MRGFE_FLOOR_NONE_AFTER_CLIP;
        MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[2], st));
        MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[3], st));
        MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[4], st));
        MRGFE_HIP_CHECK(hipStreamSynchronize(st));
        return MRGFE_OK;
    }
    const float4* d_sel = dband.as<float4>();
    uint32_t      n_f = n_clip;
    if (p->use_normal_filtering) {  // :120-122
        MRGFE_TRY(floor_normals_device(ctx, dband.as<float4>(), n_clip, p->normal_filter_thresh_deg, nullptr, dflags.as<uint32_t>()));
        MRGFE_TRY(compact_by_flags(ctx, dband.as<float4>(), n_clip, dflags.as<uint32_t>(), dtilt.as<float4>(), &n_f));
        ctx->fl_stats[4] += 1;
        d_sel = dtilt.as<float4>();
    }
    if (n_f) {
        hipLaunchKernelGGL(floor_transform_kernel, blocks(n_f), dim3(256), 0, st, d_sel, n_f, Ti, dfilt.as<float4>());  // :124
        MRGFE_HIP_CHECK(hipGetLastError());
    }
    MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[2], st));
    res->n_filtered = n_f;
    if (out_filtered && n_f) MRGFE_HIP_CHECK(hipMemcpyAsync(out_filtered, dfilt.p, size_t(n_f) * 16, hipMemcpyDeviceToHost, st));
    FloorRansacOut rr;
    const bool     run = static_cast<int64_t>(n_f) >= p->floor_pts_thresh;  // :134-136
    if (run) MRGFE_TRY(floor_ransac_device(ctx, dfilt.as<float4>(), n_f, 0.1, dflags.as<uint32_t>(), &rr));  // :139-145
    MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[3], st));
    if (!run) {
        res->reason = MRGFE_FLOOR_TOO_FEW_FILTERED;
    } else {
        res->iterations = rr.iterations;
        res->skipped = rr.skipped;
        res->n_inliers = rr.n_inliers;
        for (int j = 0; j < 4; ++j) res->coeffs[j] = rr.coeffs[j];
        if (!rr.has_model) {
            res->reason = MRGFE_FLOOR_NO_MODEL;
        } else if (static_cast<int64_t>(rr.n_inliers) < p->floor_pts_thresh) {  // :148
            res->reason = MRGFE_FLOOR_TOO_FEW_INLIERS;
        } else {
            // reference = tilt_matrix.inverse() * UnitZ (:153): column 2 of the inverse
            const float  rx = Ti.m[2], ry = Ti.m[6], rz = Ti.m[10];
            const float  c0 = rr.coeffs[0], c1 = rr.coeffs[1], c2 = rr.coeffs[2];
            const float  pr0 = c0 * rx, pr1 = c1 * ry, pr2 = c2 * rz;
            const double dot = static_cast<double>((pr0 + pr1) + pr2);
            if (std::abs(dot) < std::cos(p->floor_normal_thresh_deg * M_PI / 180.0)) {  // :158
                res->reason = MRGFE_FLOOR_NOT_VERTICAL;
            } else {
                const float up = (c0 * 0.0f + c1 * 0.0f) + c2 * 1.0f;
                if (up < 0.0f)  // :164-167
                    for (int j = 0; j < 4; ++j) res->coeffs[j] *= -1.0f;
                res->found = 1;
                res->reason = MRGFE_FLOOR_FOUND;
                if (out_inliers && rr.n_inliers) {  // ExtractIndices of the inliers (:169-180)
                    uint32_t m = 0;
                    MRGFE_TRY(compact_by_flags(ctx, dfilt.as<float4>(), n_f, dflags.as<uint32_t>(), dband.as<float4>(), &m));
                    ctx->fl_stats[4] += 1;
                    if (m != rr.n_inliers) { set_error("floor detection: %u inliers selected, %u counted", m, rr.n_inliers); return MRGFE_ERR_HIP; }
                    MRGFE_HIP_CHECK(hipMemcpyAsync(out_inliers, dband.p, size_t(m) * 16, hipMemcpyDeviceToHost, st));
                }
            }
        }
    }
    MRGFE_HIP_CHECK(hipEventRecord(ctx->fl_ev[4], st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    ctx->fl_stats[4] += 1;
    for (int s = 0; s < 4; ++s) {
        float ms = 0;
        MRGFE_HIP_CHECK(hipEventElapsedTime(&ms, ctx->fl_ev[s], ctx->fl_ev[s + 1]));
        ctx->fl_stats[s] = ms;
    }
    return MRGFE_OK;
}

int floor_detect(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const float4* d_in, size_t n_in, mrgfe_floor_result* res, float* out_filtered, float* out_inliers)
{
    const uint32_t n = static_cast<uint32_t>(n_in);
    auto head = [&](const Rot12& T, float lo, float hi, float4* d_tilt, uint32_t* d_flags) -> int {
        hipLaunchKernelGGL(floor_band_kernel, blocks(n), dim3(256), 0, ctx->stream, d_in, n, T, lo, hi, d_tilt, d_flags);
        MRGFE_HIP_CHECK(hipGetLastError());
        return MRGFE_OK;
    };
    return floor_detect_behind(ctx, p, n_in, head, res, out_filtered, out_inliers);
}

int floor_callback(mrgfe_ctx* ctx, const mrgfe_floor_params* p, const KeyframeLayout& lay, const void* data, size_t raw_bytes, mrgfe_floor_result* res, float* out_filtered,
                   float* out_inliers)
{
    FloorHeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = lay.width * lay.height;
    a.width = lay.width; a.row_step = lay.row_step; a.point_step = lay.point_step;
    a.ox = lay.off_x; a.oy = lay.off_y; a.oz = lay.off_z; a.oi = lay.off_intensity;
    auto head = [&](const Rot12& T, float lo, float hi, float4* d_tilt, uint32_t* d_flags) -> int {
        const void* d_raw = nullptr;
        MRGFE_TRY(upload_raw_records(ctx, data, raw_bytes, &d_raw));  // stream-ordered, no wait: `data` is free on return
        a.raw = static_cast<const uint8_t*>(d_raw);
        const auto kern = layout_is_strict(a.point_step, a.row_step, a.ox, a.oy, a.oz, a.oi) ? floor_head_kernel<false> : floor_head_kernel<true>;
        hipLaunchKernelGGL(kern, blocks(a.n), dim3(256), 0, ctx->stream, a, T, lo, hi, d_tilt, d_flags);
        MRGFE_HIP_CHECK(hipGetLastError());
        return MRGFE_OK;
    };
    return floor_detect_behind(ctx, p, a.n, head, res, out_filtered, out_inliers);
}

}  // namespace mrgfe
