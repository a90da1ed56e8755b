// csrc/mapcloud.hip — SURVEY.md §8(f) rows 2 and 4 on MI355X: streaming per-point kernels (16 B in, 16 B out per point,
// HBM bound) in front of the compaction and voxel-grid machinery of filters.hip.
//   MapCloudGenerator::generate         /root/reference/src/mrg_slam/map_cloud_generator.cpp:14-86
//   pcl::ApproximateMeanVoxelGrid       /root/reference/include/pcl/filters/ApproximateMeanVoxelGrid.hpp:63-126
//   other-robot point removal           /root/reference/apps/mrg_slam_component.cpp:396-429
//   the keyframe callback's point work  apps/mrg_slam_component.cpp:372,396-430 (wire records -> kept / removed clouds)
//   PrefilteringComponent::deskewing    /root/reference/apps/prefiltering_component.cpp:231-292
// Float expressions run in the order documented in oracle/mapcloud.cpp (left to right, no FMA).
#include "mapcloud.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cellsort.h"
#include "dev_float.h"
#include "dev_utils.h"
#include "filters.h"
#include "ingest.h"
#include "record_store.h"
#include "scan_point.h"

namespace mrgfe {

// one lane per point of the concatenated keyframe clouds; the keyframe of a point is found by bisection of kf_off
// cat: the keyframe clouds back to back, or nullptr when every keyframe is read through its own pointer srcs[k]
__global__ __launch_bounds__(256) void map_transform_kernel(const float4* __restrict__ cat, const float4* const* __restrict__ srcs, uint32_t n, const uint32_t* __restrict__ kf_off,
                                                             const float* __restrict__ poses, int K, int use_far, float far_sq, float4* __restrict__ out,
                                                             uint32_t* __restrict__ flags)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = K;  // kf_off[lo] <= i < kf_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kf_off[mid] <= i) lo = mid; else hi = mid;
    }
    const float4 p = cat ? cat[i] : srcs[lo][i - kf_off[lo]];
    uint32_t keep = 1u;
    if (use_far) {
        float s = p.x * p.x + p.y * p.y;  // getVector3fMap().squaredNorm()
        s = s + p.z * p.z;
        if (s > far_sq) keep = 0u;        // map_cloud_generator.cpp:39-41
    }
    const float* P = poses + 16 * lo;  // column-major
    float q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {  // pose * (x, y, z, 1), column by column
        float s = P[0 * 4 + r] * p.x;
        s = s + P[1 * 4 + r] * p.y;
        s = s + P[2 * 4 + r] * p.z;
        q[r] = s + P[3 * 4 + r] * 1.0f;
    }
    out[i] = make_float4(q[0], q[1], q[2], p.w);
    flags[i] = keep;
}

// ---- pcl::ApproximateMeanVoxelGrid on occupied cells ------------------------------------------------------------------------
// The reference keys a hash map on the integer cell (floor(p * inverse_leaf) per axis, ApproximateMeanVoxelGrid.hpp:85-91): no limit
// on the extent of the map.  A dense linear voxel index over the bounding box (what pcl::VoxelGrid uses, and the prefilter with it)
// overflows int32 at 200 m x 200 m x 30 m / 0.1 m — smaller than a KITTI map (round 1 returned MRGFE_ERR_OVERFLOW there).  Here the key
// is the cell itself, bit-packed: (iz - min) | (iy - min) | (ix - min) with just the bits each axis needs (up to 21 per axis), one
// more bit on top marking non-finite points so that they sort behind every cell.  Up to 32 key bits are one stable radix sort of
// (key, index) pairs as before; longer keys are sorted low word first, then — stably — by the gathered high word.  Runs of equal
// keys, float sums in input order, division by float(count) and the count threshold are the voxel-grid pass of filters.hip.
// Output order: ascending (z, y, x) cell — the same order the dense index gave.
struct CellKeyParams { float inv_leaf; int32_t min_c[3]; uint32_t shift_y, shift_z, total_bits; };

__global__ __launch_bounds__(256) void mapvox_keys_kernel(const float4* __restrict__ pts, uint32_t n, CellKeyParams kp, uint32_t* __restrict__ key_lo, uint32_t* __restrict__ key_hi,
                                                           uint32_t* __restrict__ vals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    uint64_t key = uint64_t(1) << kp.total_bits;  // non-finite: behind every cell
    if (finite3(p.x, p.y, p.z)) {
        const uint64_t cx = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int>(floorf(p.x * kp.inv_leaf))) - kp.min_c[0]);
        const uint64_t cy = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int>(floorf(p.y * kp.inv_leaf))) - kp.min_c[1]);
        const uint64_t cz = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int>(floorf(p.z * kp.inv_leaf))) - kp.min_c[2]);
        key = cx | (cy << kp.shift_y) | (cz << kp.shift_z);
    }
    key_lo[i] = static_cast<uint32_t>(key);
    key_hi[i] = static_cast<uint32_t>(key >> 32);
    vals[i] = i;
}
__global__ __launch_bounds__(256) void gather_u32_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ dst)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
// run heads of the sorted 64-bit keys among the first n_valid positions (the non-finite points sit behind them)
__global__ __launch_bounds__(256) void heads64_kernel(const uint32_t* __restrict__ key_lo, const uint32_t* __restrict__ key_hi, const uint32_t* __restrict__ sorted_vals, uint32_t n,
                                                       uint32_t n_valid, uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 0;
    if (i < n_valid) {
        if (i == 0) f = 1;
        else {
            const uint32_t a = sorted_vals[i], b = sorted_vals[i - 1];
            f = (key_lo[a] != key_lo[b] || key_hi[a] != key_hi[b]) ? 1u : 0u;
        }
    }
    flags[i] = f;
}
__global__ __launch_bounds__(256) void seg_from_heads_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ ordinal, uint32_t n, uint32_t n_valid, uint32_t n_seg,
                                                              uint32_t* __restrict__ seg_start)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) seg_start[ordinal[i]] = i;
    if (i + 1 == n_valid) seg_start[n_seg] = n_valid;
}

int mean_voxelgrid_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, float leaf, int min_pts, float4* d_out, size_t* out_n)
{
    *out_n = 0;
    if (n == 0) return MRGFE_OK;
    hipStream_t st = ctx->stream;
    uint32_t    nn = static_cast<uint32_t>(n);
    SliceTable  tab;
    tab.build(&nn, 1);
    struct Desc { Slice sl; const float4* cp; };
    PinBuf& hp = ctx->pin[1];
    MRGFE_TRY(hp.ensure(sizeof(Desc) + sizeof(BBox) + 16));
    Desc* hd = hp.as<Desc>();
    hd->sl = tab.h[0];
    hd->cp = d_in;
    DevBuf& dd = ctx->scratch[0];
    MRGFE_TRY(dd.ensure(sizeof(Desc)));
    Desc* d_desc = dd.as<Desc>();
    MRGFE_HIP_CHECK(hipMemcpyAsync(d_desc, hd, sizeof(Desc), hipMemcpyHostToDevice, st));
    DevBuf& dbb = ctx->scratch[1];
    MRGFE_TRY(dbb.ensure(sizeof(BBox) * (tab.total_blks + 1)));
    BBox* d_part = dbb.as<BBox>();
    BBox* d_bbo = d_part + tab.total_blks;
    MRGFE_TRY(bounding_boxes(ctx, &d_desc->cp, &d_desc->sl, tab, d_part, d_bbo));
    BBox* h_bb = reinterpret_cast<BBox*>(hp.as<char>() + sizeof(Desc));
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_bb, d_bbo, sizeof(BBox), hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t n_valid = h_bb->n_finite;
    if (n_valid == 0) return MRGFE_OK;
    // cells of the extreme points (float multiply and floor are monotonic, so these are the extreme cells)
    CellKeyParams kp;
    kp.inv_leaf = 1.0f / leaf;  // ApproximateMeanVoxelGrid::setLeafSize: inverse_leaf_size_ = 1 / leaf_size_ (float)
    uint32_t bits[3];
    for (int a = 0; a < 3; ++a) {
        const double lo = std::floor(static_cast<double>(h_bb->mn[a] * kp.inv_leaf)), hi = std::floor(static_cast<double>(h_bb->mx[a] * kp.inv_leaf));
        if (!(lo > -2147483000.0 && hi < 2147483000.0)) { set_error("map cloud: cell index beyond int32 (the reference's int cast overflows there too)"); return MRGFE_ERR_OVERFLOW; }
        kp.min_c[a] = static_cast<int32_t>(lo);
        const uint64_t span = static_cast<uint64_t>(hi - lo);
        bits[a] = 1;
        while ((uint64_t(1) << bits[a]) <= span) ++bits[a];
    }
    kp.shift_y = bits[0];
    kp.shift_z = bits[0] + bits[1];
    kp.total_bits = bits[0] + bits[1] + bits[2];
    if (kp.total_bits > 62) { set_error("map cloud: %u key bits needed (extent / resolution)", kp.total_bits); return MRGFE_ERR_OVERFLOW; }
    DevBuf &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6], &dfl = ctx->scratch[7], &dblk = ctx->scratch[8],
           &dkh = ctx->scratch[12], &dlo = ctx->scratch[13];
    MRGFE_TRY(dk.ensure(n * 4)); MRGFE_TRY(dv.ensure(n * 4)); MRGFE_TRY(dkt.ensure(n * 4)); MRGFE_TRY(dvt.ensure(n * 4)); MRGFE_TRY(dkh.ensure(n * 4)); MRGFE_TRY(dlo.ensure(n * 4));
    MRGFE_TRY(dh.ensure(sizeof(uint32_t) * 256 * (tab.total_blks + 1)));
    MRGFE_TRY(dfl.ensure(n * 4));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    const dim3 grid((nn + 255) / 256);
    // dlo / dkh keep the keys by POINT index; dk is the sort's working copy
    hipLaunchKernelGGL(mapvox_keys_kernel, grid, dim3(256), 0, st, d_in, nn, kp, dlo.as<uint32_t>(), dkh.as<uint32_t>(), dv.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    MRGFE_HIP_CHECK(hipMemcpyAsync(dk.p, dlo.p, n * 4, hipMemcpyDeviceToDevice, st));
    const int key_bits = static_cast<int>(kp.total_bits) + 1;
    uint32_t *sk, *sv;
    MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), &d_desc->sl, tab, std::min(key_bits, 32), dh.as<uint32_t>(), &sk, &sv));
    if (key_bits > 32) {
        // second, stable pass over the high word, gathered into the order the first pass produced
        uint32_t* k2 = (sk == dk.as<uint32_t>()) ? dk.as<uint32_t>() : dkt.as<uint32_t>();       // the buffer holding the sorted low words: no longer needed
        uint32_t* k2t = (sk == dk.as<uint32_t>()) ? dkt.as<uint32_t>() : dk.as<uint32_t>();
        uint32_t* v2t = (sv == dv.as<uint32_t>()) ? dvt.as<uint32_t>() : dv.as<uint32_t>();
        hipLaunchKernelGGL(gather_u32_kernel, grid, dim3(256), 0, st, dkh.as<uint32_t>(), sv, nn, k2);
        MRGFE_HIP_CHECK(hipGetLastError());
        MRGFE_TRY(radix_sort_pairs(ctx, k2, sv, k2t, v2t, &d_desc->sl, tab, key_bits - 32, dh.as<uint32_t>(), &sk, &sv));
    }
    hipLaunchKernelGGL(heads64_kernel, grid, dim3(256), 0, st, dlo.as<uint32_t>(), dkh.as<uint32_t>(), sv, nn, n_valid, dfl.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    uint32_t* d_ord = (sk == dk.as<uint32_t>()) ? dkt.as<uint32_t>() : dk.as<uint32_t>();  // the sort buffer that does not hold the result
    uint32_t* d_tot = dblk.as<uint32_t>() + tab.total_blks;
    MRGFE_TRY(exclusive_scan(ctx, dfl.as<uint32_t>(), d_ord, &d_desc->sl, tab, dblk.as<uint32_t>(), d_tot));
    uint32_t* h_tot = reinterpret_cast<uint32_t*>(hp.as<char>() + sizeof(Desc) + sizeof(BBox));
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_tot, d_tot, 4, hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t V = *h_tot;
    if (V == 0) return MRGFE_OK;
    DevBuf &dseg = ctx->scratch[9], &dcent = ctx->scratch[10], &dkeep = ctx->scratch[11];
    MRGFE_TRY(dseg.ensure(sizeof(uint32_t) * (size_t(V) + 4)));
    MRGFE_TRY(dcent.ensure(sizeof(float4) * size_t(V)));
    MRGFE_TRY(dkeep.ensure(sizeof(uint32_t) * size_t(V)));
    hipLaunchKernelGGL(seg_from_heads_kernel, grid, dim3(256), 0, st, dfl.as<uint32_t>(), d_ord, nn, n_valid, V, dseg.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    MRGFE_TRY(launch_voxel_centroids(ctx, d_in, sv, dseg.as<uint32_t>(), V, min_pts, dcent.as<float4>(), dkeep.as<uint32_t>()));
    uint32_t kept = 0;
    MRGFE_TRY(compact_by_flags(ctx, dcent.as<float4>(), V, dkeep.as<uint32_t>(), d_out, &kept));
    *out_n = kept;
    return MRGFE_OK;
}

int map_cloud_device(mrgfe_ctx* ctx, const float4* d_cat, const uint32_t* kf_off, const float* poses_f, int K, float resolution, int min_pts, float far_thresh, float4* d_out,
                     size_t* out_n, size_t* n_unfiltered, const float4* const* kf_ptrs)
{
    *out_n = 0;
    *n_unfiltered = 0;
    const uint32_t n = kf_off[K];
    if (n == 0) return MRGFE_OK;
    hipStream_t st = ctx->stream;
    DevBuf dcomp, dfl, dtrans, dtab;  // per-call buffers (the scratch slots are in use by the voxel-grid pass below), freed at the return, `dtab` first
    const size_t ptr_at = (sizeof(uint32_t) * (K + 1) + sizeof(float) * 16 * K + 15) & ~size_t(15);
    MRGFE_TRY(dtab.ensure(ptr_at + sizeof(void*) * K));
    MRGFE_TRY(dtrans.ensure(size_t(n) * 16));
    MRGFE_TRY(dfl.ensure(size_t(n) * 4));
    uint32_t* d_off = dtab.as<uint32_t>();
    float*    d_pose = reinterpret_cast<float*>(d_off + (K + 1));
    const float4* const* d_ptrs = kf_ptrs ? reinterpret_cast<const float4* const*>(dtab.as<char>() + ptr_at) : nullptr;
    const bool use_far = far_thresh > 0;  // map_cloud_generator.cpp:27-28
    if ((kf_ptrs && hipMemcpyAsync(dtab.as<char>() + ptr_at, kf_ptrs, sizeof(void*) * K, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemcpyAsync(d_off, kf_off, sizeof(uint32_t) * (K + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_pose, poses_f, sizeof(float) * 16 * K, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        set_error("map cloud: table upload failed");
        return MRGFE_ERR_HIP;
    }
    hipLaunchKernelGGL(map_transform_kernel, dim3((n + 255) / 256), dim3(256), 0, st, kf_ptrs ? nullptr : d_cat, d_ptrs, n, d_off, d_pose, K, use_far ? 1 : 0, far_thresh * far_thresh, dtrans.as<float4>(),
                       dfl.as<uint32_t>());
    if (hipGetLastError() != hipSuccess) { set_error("map cloud: transform kernel launch failed"); return MRGFE_ERR_HIP; }
    const float4* d_cloud = dtrans.as<float4>();
    size_t        total = n;
    if (use_far) {
        MRGFE_TRY(dcomp.ensure(size_t(n) * 16));
        uint32_t kept = 0;
        MRGFE_TRY(compact_by_flags(ctx, dtrans.as<float4>(), n, dfl.as<uint32_t>(), dcomp.as<float4>(), &kept));
        d_cloud = dcomp.as<float4>();
        total = kept;
    }
    *n_unfiltered = total;
    int rc = MRGFE_OK;
    if (resolution <= 0.0f) {  // :66-70: the unfiltered cloud
        if (total && hipMemcpyAsync(d_out, d_cloud, total * 16, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = MRGFE_ERR_HIP;
        if (hipStreamSynchronize(st) != hipSuccess) rc = MRGFE_ERR_HIP;
        *out_n = total;
    } else if (total) {
        // ApproximateMeanVoxelGrid: cells floor(p * inverse_leaf), f32 sums in input order (the radix sort is stable), division by
        // float(count), count threshold; only the output order differs (ascending cell instead of the reference's hash-map order)
        rc = mean_voxelgrid_device(ctx, d_cloud, total, resolution, min_pts, d_out, out_n);
    }
    return rc;
}

// ---- egress: the map as wire records (mrgfe_map_store_publish) -----------------------------------------------------------------
// update_map_cloud_msg / publish_map_service / save_map_service (apps/mrg_slam_component.cpp:712-740, 764-796, 1078-1144) run the generator and
// then pcl::toROSMsg or the two `+=` offset passes and savePCDFileBinary over every map point.  Here the kernel that writes the FINAL points
// writes them as the records the caller sends or saves: the scatter of the last compaction (the voxel count threshold, or the far cut of the
// unfiltered map), or the copy of the unfiltered map without a far cut.  Per kept point: up to two f32 offset additions per coordinate, one after
// the other (:1106-1115 add zero_utm, then zero_enu, to the filtered cloud), then
//   point_step 32: x, y, z, 1.0f | intensity, 0, 0, 0   the pcl::PointXYZI in memory, which is what toROSMsg copies (two 16-byte stores)
//   point_step 16: x, y, z, intensity                   the body of a binary PCD (one 16-byte store)
// Without offsets no arithmetic touches the point: its bits, a NaN's payload included, are those of the generator.  (store_record: record_store.h,
// shared with the scan egress of filters.hip.)
// flags / pos: the keep flags and their exclusive scan; both nullptr: every point is kept where it stands
template <int kStep>
__global__ __launch_bounds__(256) void egress_records_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos, uint32_t n,
                                                              EgressOffsets o, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (flags && !flags[i]) return;
    store_record<kStep>(out, flags ? pos[i] : i, in[i], o);  // pos[i] <= i < n: inside the n records of `out`
}

static EgressOffsets egress_offsets(const EgressFormat& f)
{
    EgressOffsets o{};
    o.n = f.n_offsets;
    for (int k = 0; k < f.n_offsets; ++k) for (int a = 0; a < 3; ++a) o.v[k][a] = f.offsets[3 * k + a];
    return o;
}
// compact_by_flags with the record kernel as its scatter: *total records in d_rec (room for n).  d_flags nullptr: all n points, no scan and no wait —
// *waited says whether the stream was waited for BEHIND the record kernel (the records are complete) or the kernel is only queued.
static int egress_records(mrgfe_ctx* ctx, const float4* d_in, uint32_t n, const uint32_t* d_flags, const EgressFormat& f, void* d_rec, uint32_t* total, bool* waited, EgressStats* stats)
{
    *total = 0;
    *waited = false;
    if (n == 0) return MRGFE_OK;
    hipStream_t st = ctx->stream;
    const auto kern = f.point_step == 16 ? egress_records_kernel<16> : egress_records_kernel<32>;
    const dim3 grid((n + 255) / 256);
    if (!d_flags) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, d_in, nullptr, nullptr, n, egress_offsets(f), static_cast<float4*>(d_rec));
        MRGFE_HIP_CHECK(hipGetLastError());
        stats->launches += 1;
        *total = n;
        return MRGFE_OK;
    }
    SliceTable tab;
    tab.build(&n, 1);
    DevBuf &ds = ctx->scratch[0], &dpos = ctx->scratch[4], &dblk = ctx->scratch[8];  // (the slots of compact_by_flags)
    MRGFE_TRY(ds.ensure(sizeof(Slice)));
    MRGFE_TRY(dpos.ensure(size_t(n) * 4));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    MRGFE_HIP_CHECK(hipMemcpyAsync(ds.p, tab.h.data(), sizeof(Slice), hipMemcpyHostToDevice, st));
    uint32_t* d_tot = dblk.as<uint32_t>() + tab.total_blks;
    MRGFE_TRY(exclusive_scan(ctx, d_flags, dpos.as<uint32_t>(), ds.as<Slice>(), tab, dblk.as<uint32_t>(), d_tot));
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, d_in, d_flags, dpos.as<uint32_t>(), n, egress_offsets(f), static_cast<float4*>(d_rec));
    MRGFE_HIP_CHECK(hipGetLastError());
    stats->launches += 4;  // the three of the scan, the record kernel
    MRGFE_HIP_CHECK(hipMemcpyAsync(total, d_tot, 4, hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    stats->waits += 1;
    *waited = true;
    return MRGFE_OK;
}

// mean_voxelgrid_device up to its centroids and keep flags (ctx->scratch[10] / [11], *n_cells of each; 0: no finite point).  The passes, their order
// and their buffers are that function's, which stays as it is — the generator is what the egress tests hold this against — so a change there is a
// change here; only its last step, compact_by_flags into a packed cloud, is not taken: the caller's record kernel is that step.
static int mean_voxel_cells(mrgfe_ctx* ctx, const float4* d_in, size_t n, float leaf, int min_pts, uint32_t* n_cells, EgressStats* stats)
{
    *n_cells = 0;
    hipStream_t st = ctx->stream;
    uint32_t    nn = static_cast<uint32_t>(n);
    SliceTable  tab;
    tab.build(&nn, 1);
    struct Desc { Slice sl; const float4* cp; };
    PinBuf& hp = ctx->pin[1];
    MRGFE_TRY(hp.ensure(sizeof(Desc) + sizeof(BBox) + 16));
    Desc* hd = hp.as<Desc>();
    hd->sl = tab.h[0];
    hd->cp = d_in;
    DevBuf& dd = ctx->scratch[0];
    MRGFE_TRY(dd.ensure(sizeof(Desc)));
    Desc* d_desc = dd.as<Desc>();
    MRGFE_HIP_CHECK(hipMemcpyAsync(d_desc, hd, sizeof(Desc), hipMemcpyHostToDevice, st));
    DevBuf& dbb = ctx->scratch[1];
    MRGFE_TRY(dbb.ensure(sizeof(BBox) * (tab.total_blks + 1)));
    BBox* d_part = dbb.as<BBox>();
    BBox* d_bbo = d_part + tab.total_blks;
    MRGFE_TRY(bounding_boxes(ctx, &d_desc->cp, &d_desc->sl, tab, d_part, d_bbo));
    BBox* h_bb = reinterpret_cast<BBox*>(hp.as<char>() + sizeof(Desc));
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_bb, d_bbo, sizeof(BBox), hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    stats->waits += 1;
    const uint32_t n_valid = h_bb->n_finite;
    if (n_valid == 0) return MRGFE_OK;
    CellKeyParams kp;
    kp.inv_leaf = 1.0f / leaf;
    uint32_t bits[3];
    for (int a = 0; a < 3; ++a) {
        const double lo = std::floor(static_cast<double>(h_bb->mn[a] * kp.inv_leaf)), hi = std::floor(static_cast<double>(h_bb->mx[a] * kp.inv_leaf));
        if (!(lo > -2147483000.0 && hi < 2147483000.0)) { set_error("map cloud: cell index beyond int32 (the reference's int cast overflows there too)"); return MRGFE_ERR_OVERFLOW; }
        kp.min_c[a] = static_cast<int32_t>(lo);
        const uint64_t span = static_cast<uint64_t>(hi - lo);
        bits[a] = 1;
        while ((uint64_t(1) << bits[a]) <= span) ++bits[a];
    }
    kp.shift_y = bits[0];
    kp.shift_z = bits[0] + bits[1];
    kp.total_bits = bits[0] + bits[1] + bits[2];
    if (kp.total_bits > 62) { set_error("map cloud: %u key bits needed (extent / resolution)", kp.total_bits); return MRGFE_ERR_OVERFLOW; }
    DevBuf &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6], &dfl = ctx->scratch[7], &dblk = ctx->scratch[8],
           &dkh = ctx->scratch[12], &dlo = ctx->scratch[13];
    MRGFE_TRY(dk.ensure(n * 4)); MRGFE_TRY(dv.ensure(n * 4)); MRGFE_TRY(dkt.ensure(n * 4)); MRGFE_TRY(dvt.ensure(n * 4)); MRGFE_TRY(dkh.ensure(n * 4)); MRGFE_TRY(dlo.ensure(n * 4));
    MRGFE_TRY(dh.ensure(sizeof(uint32_t) * 256 * (tab.total_blks + 1)));
    MRGFE_TRY(dfl.ensure(n * 4));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    const dim3 grid((nn + 255) / 256);
    hipLaunchKernelGGL(mapvox_keys_kernel, grid, dim3(256), 0, st, d_in, nn, kp, dlo.as<uint32_t>(), dkh.as<uint32_t>(), dv.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    MRGFE_HIP_CHECK(hipMemcpyAsync(dk.p, dlo.p, n * 4, hipMemcpyDeviceToDevice, st));
    const int key_bits = static_cast<int>(kp.total_bits) + 1;
    uint32_t *sk, *sv;
    MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), &d_desc->sl, tab, std::min(key_bits, 32), dh.as<uint32_t>(), &sk, &sv));
    if (key_bits > 32) {
        uint32_t* k2 = (sk == dk.as<uint32_t>()) ? dk.as<uint32_t>() : dkt.as<uint32_t>();
        uint32_t* k2t = (sk == dk.as<uint32_t>()) ? dkt.as<uint32_t>() : dk.as<uint32_t>();
        uint32_t* v2t = (sv == dv.as<uint32_t>()) ? dvt.as<uint32_t>() : dv.as<uint32_t>();
        hipLaunchKernelGGL(gather_u32_kernel, grid, dim3(256), 0, st, dkh.as<uint32_t>(), sv, nn, k2);
        MRGFE_HIP_CHECK(hipGetLastError());
        MRGFE_TRY(radix_sort_pairs(ctx, k2, sv, k2t, v2t, &d_desc->sl, tab, key_bits - 32, dh.as<uint32_t>(), &sk, &sv));
    }
    hipLaunchKernelGGL(heads64_kernel, grid, dim3(256), 0, st, dlo.as<uint32_t>(), dkh.as<uint32_t>(), sv, nn, n_valid, dfl.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    uint32_t* d_ord = (sk == dk.as<uint32_t>()) ? dkt.as<uint32_t>() : dk.as<uint32_t>();
    uint32_t* d_tot = dblk.as<uint32_t>() + tab.total_blks;
    MRGFE_TRY(exclusive_scan(ctx, dfl.as<uint32_t>(), d_ord, &d_desc->sl, tab, dblk.as<uint32_t>(), d_tot));
    uint32_t* h_tot = reinterpret_cast<uint32_t*>(hp.as<char>() + sizeof(Desc) + sizeof(BBox));
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_tot, d_tot, 4, hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    stats->waits += 1;
    const uint32_t V = *h_tot;
    if (V == 0) return MRGFE_OK;
    DevBuf &dseg = ctx->scratch[9], &dcent = ctx->scratch[10], &dkeep = ctx->scratch[11];
    MRGFE_TRY(dseg.ensure(sizeof(uint32_t) * (size_t(V) + 4)));
    MRGFE_TRY(dcent.ensure(sizeof(float4) * size_t(V)));
    MRGFE_TRY(dkeep.ensure(sizeof(uint32_t) * size_t(V)));
    hipLaunchKernelGGL(seg_from_heads_kernel, grid, dim3(256), 0, st, dfl.as<uint32_t>(), d_ord, nn, n_valid, V, dseg.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    MRGFE_TRY(launch_voxel_centroids(ctx, d_in, sv, dseg.as<uint32_t>(), V, min_pts, dcent.as<float4>(), dkeep.as<uint32_t>()));
    *n_cells = V;
    return MRGFE_OK;
}

size_t MapEgressWorkspace::footprint(const mrgfe_ctx* ctx) const
{
    size_t b = tab.cap + trans.cap + flags.cap + comp.cap + rec.cap + ctx->sort_chunks.cap;
    for (const DevBuf& d : ctx->scratch) b += d.cap;
    return b;
}

int map_publish_device(mrgfe_ctx* ctx, MapEgressWorkspace& ws, const uint32_t* kf_off, const float* poses_f, int K, const float4* const* kf_ptrs, float resolution, int min_pts,
                       float far_thresh, const EgressFormat& f, size_t* out_n, size_t* n_unfiltered, bool* records_complete, EgressStats* stats)
{
    *out_n = 0;
    *n_unfiltered = 0;
    *records_complete = true;  // (no record kernel queued yet)
    const uint32_t n = kf_off[K];
    if (n == 0) return MRGFE_OK;
    hipStream_t st = ctx->stream;
    // the tables of map_cloud_device in one staged copy: offsets, poses, cloud pointers
    const size_t pose_at = sizeof(uint32_t) * (K + 1), ptr_at = (pose_at + sizeof(float) * 16 * K + 15) & ~size_t(15), tab_bytes = ptr_at + sizeof(void*) * K;
    std::vector<char> h_tab(tab_bytes, 0);
    std::memcpy(h_tab.data(), kf_off, pose_at);
    std::memcpy(h_tab.data() + pose_at, poses_f, sizeof(float) * 16 * K);
    std::memcpy(h_tab.data() + ptr_at, kf_ptrs, sizeof(void*) * K);
    MRGFE_TRY(ws.tab.ensure(tab_bytes));
    MRGFE_TRY(ws.trans.ensure(size_t(n) * 16));
    MRGFE_TRY(ws.flags.ensure(size_t(n) * 4));
    MRGFE_TRY(ctx->stage_h2d(ws.tab.p, h_tab.data(), tab_bytes, st));
    const bool use_far = far_thresh > 0;  // map_cloud_generator.cpp:27-28
    hipLaunchKernelGGL(map_transform_kernel, dim3((n + 255) / 256), dim3(256), 0, st, static_cast<const float4*>(nullptr), reinterpret_cast<const float4* const*>(ws.tab.as<char>() + ptr_at), n,
                       ws.tab.as<uint32_t>(), reinterpret_cast<const float*>(ws.tab.as<char>() + pose_at), K, use_far ? 1 : 0, far_thresh * far_thresh, ws.trans.as<float4>(), ws.flags.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    uint32_t m = 0;
    if (resolution <= 0.0f) {  // :66-70: the unfiltered cloud — the far cut is the last compaction, or there is none
        MRGFE_TRY(ws.rec.ensure(size_t(n) * f.point_step));
        MRGFE_TRY(egress_records(ctx, ws.trans.as<float4>(), n, use_far ? ws.flags.as<uint32_t>() : nullptr, f, ws.rec.p, &m, records_complete, stats));
        *n_unfiltered = m;
        *out_n = m;
        return MRGFE_OK;
    }
    const float4* d_cloud = ws.trans.as<float4>();
    uint32_t      total = n;
    if (use_far) {
        MRGFE_TRY(ws.comp.ensure(size_t(n) * 16));
        MRGFE_TRY(compact_by_flags(ctx, ws.trans.as<float4>(), n, ws.flags.as<uint32_t>(), ws.comp.as<float4>(), &total));
        stats->waits += 1;
        d_cloud = ws.comp.as<float4>();
    }
    *n_unfiltered = total;
    if (total == 0) return MRGFE_OK;
    uint32_t V = 0;
    MRGFE_TRY(mean_voxel_cells(ctx, d_cloud, total, resolution, min_pts, &V, stats));
    if (V == 0) return MRGFE_OK;
    MRGFE_TRY(ws.rec.ensure(size_t(V) * f.point_step));
    MRGFE_TRY(egress_records(ctx, ctx->scratch[10].as<float4>(), V, ctx->scratch[11].as<uint32_t>(), f, ws.rec.p, &m, records_complete, stats));
    *out_n = m;
    return MRGFE_OK;
}

// ---- egress: stored keyframes as 32-byte records (mrgfe_map_store_read) ----------------------------------------------------------------
// KeyFrame::save / the cloud_msg of publish_graph_service (src/mrg_slam/keyframe.cpp:109, 200) for a list of keyframes: ONE launch over a tile table,
// as keyframe_gather_many_kernel is driven — a workgroup-uniform 32-byte read names the tile's cloud, its first point and the record that point becomes.
struct RecordTile {
    const float4* src;    // the keyframe's cloud
    uint64_t      out;    // the record of the keyframe's point 0 in the output
    uint32_t      first;  // the tile's first point within the keyframe
    uint32_t      n;      // points of the keyframe
    uint32_t      pad[2];
};
static_assert(sizeof(RecordTile) == 32, "RecordTile: one 32-byte record per tile");
__global__ __launch_bounds__(256) void keyframe_records_many_kernel(const RecordTile* __restrict__ tiles, float4* __restrict__ out)
{
    const RecordTile t = tiles[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = t.first + k * 256 + threadIdx.x;
        if (i < t.n) store_record<32>(out, t.out + i, t.src[i], EgressOffsets{});
    }
}

int keyframe_records_many_device(mrgfe_ctx* ctx, const KeyframeRecordItem* items, size_t count, void* d_records)
{
    std::vector<RecordTile> tiles;
    for (size_t m = 0; m < count; ++m) {
        RecordTile t;
        std::memset(&t, 0, sizeof(t));
        t.src = items[m].d_cloud; t.out = items[m].first_record; t.n = items[m].n;
        for (uint64_t first = 0; first < t.n; first += kTile) {  // (an empty keyframe has no tile)
            t.first = static_cast<uint32_t>(first);
            tiles.push_back(t);
        }
    }
    if (tiles.empty()) return MRGFE_OK;
    if (tiles.size() > 0x7fffffffu) { set_error("keyframe records: %zu tiles in one launch", tiles.size()); return MRGFE_ERR_INVALID; }
    DevBuf& dtab = ctx->scratch[0];
    MRGFE_TRY(dtab.ensure(tiles.size() * sizeof(RecordTile)));
    MRGFE_TRY(ctx->stage_h2d(dtab.p, tiles.data(), tiles.size() * sizeof(RecordTile), ctx->stream));
    hipLaunchKernelGGL(keyframe_records_many_kernel, dim3(static_cast<uint32_t>(tiles.size())), dim3(256), 0, ctx->stream, dtab.as<RecordTile>(), static_cast<float4*>(d_records));
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// ---- other-robot point removal -----------------------------------------------------------------------------------
// (the sphere test itself: scan_point.h near_a_centre, shared with the keyframe head kernel below)
__global__ __launch_bounds__(256) void near_flags_kernel(const float4* __restrict__ in, uint32_t n, Centres c, int K, float radius_sqr, uint32_t* __restrict__ keep,
                                                          uint32_t* __restrict__ drop)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t gone = near_a_centre(in[i], c, K, radius_sqr);  // mrg_slam_component.cpp:413
    keep[i] = gone ^ 1u;
    drop[i] = gone;
}

int remove_points_near_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, const float* centres, int K, float radius_sqr, float4* d_kept, size_t* n_kept, float4* d_removed,
                              size_t* n_removed)
{
    *n_kept = 0;
    if (n_removed) *n_removed = 0;
    if (n == 0) return MRGFE_OK;
    if (K > kMaxCentres) { set_error("remove_points_near: at most %d centres", kMaxCentres); return MRGFE_ERR_INVALID; }
    const uint32_t nn = static_cast<uint32_t>(n);
    Centres c{};
    for (int k = 0; k < K; ++k) for (int a = 0; a < 3; ++a) c.xyz[k][a] = centres[3 * k + a];
    DevBuf dd, dk;  // (per-call flags, freed at the return, `dk` first)
    MRGFE_TRY(dk.ensure(n * 4));
    MRGFE_TRY(dd.ensure(n * 4));
    hipLaunchKernelGGL(near_flags_kernel, dim3((nn + 255) / 256), dim3(256), 0, ctx->stream, d_in, nn, c, K, radius_sqr, dk.as<uint32_t>(), dd.as<uint32_t>());
    if (hipGetLastError() != hipSuccess) { set_error("remove_points_near: kernel launch failed"); return MRGFE_ERR_HIP; }
    uint32_t kept = 0, gone = 0;
    MRGFE_TRY(compact_by_flags(ctx, d_in, nn, dk.as<uint32_t>(), d_kept, &kept));
    if (d_removed) MRGFE_TRY(compact_by_flags(ctx, d_in, nn, dd.as<uint32_t>(), d_removed, &gone));
    *n_kept = kept;
    if (n_removed) *n_removed = d_removed ? gone : nn - kept;
    return MRGFE_OK;
}

// ---- the keyframe callback: wire records -> kept / removed clouds (apps/mrg_slam_component.cpp:372, 396-430) ----------------------
// The head: pcl::fromROSMsg and the other-robot test in one pass over the wire records.  Per point: the strided record is read (scan_point.h
// load_point_record, the body of gather_points_kernel) and stored as the packed float4; with kCentres the point is held against the spheres
// (near_a_centre, the body of near_flags_kernel), its keep flag is written and the tile's kept count is left for the partition.  Same tile shape
// as scan_head_kernel / pf_distance_tiles_kernel: one workgroup per 2048 points.  The switch is compile-time: without centres the kernel is a plain
// gather (no flags, no counts, no centre table in registers) that writes straight into the store's buffer.
struct KeyframeHeadArgs {
    const uint8_t* raw;
    float4*        out;
    uint32_t       n, width, row_step, point_step, ox, oy, oz;
    int32_t        oi;
    uint32_t*      flags;  // kCentres: 1 = kept
    uint32_t*      blk;    // kCentres: kept points per tile
    int            K;
    float          radius_sqr;
};
// kBytes: the layout is not a strict one (ingest.h layout_is_strict) and the record's fields are put together from aligned words.
template <bool kCentres, bool kBytes>
__global__ __launch_bounds__(256) void keyframe_head_kernel(const KeyframeHeadArgs a, const Centres c)
{
    const uint32_t base = blockIdx.x * kTile;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        if (i < a.n) {
            const float4 p = load_point_record_as<kBytes>(a.raw, i, a.width, a.row_step, a.point_step, a.ox, a.oy, a.oz, a.oi);
            a.out[i] = p;
            if (kCentres) {
                const uint32_t f = near_a_centre(p, c, a.K, a.radius_sqr) ^ 1u;
                a.flags[i] = f;
                cnt += f;
            }
        }
    }
    if (!kCentres) return;
    __shared__ uint32_t sw[4];
    cnt = wave_sum(cnt);
    if (lane_id() == 0) sw[wave_id()] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.blk[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}
// Stable two-way partition in ONE launch behind the tile counts (pf_compact_kernel's scheme, filters.hip): a workgroup adds up the counts of the tiles
// before its own (and of all tiles) itself and ranks its tile's kept points by wave ballots; point i with `rank` kept points before it goes to
// kept[rank] when its flag is set and to removed[i - rank] otherwise, so both outputs are in input order.  Workgroup 0 leaves both totals for the host.
// On this route it stands for near_flags_kernel, two exclusive scans and two scatters.  Launched with ceil(n / 2048) workgroups, n > 0.
__global__ __launch_bounds__(256) void keyframe_partition_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ blk, uint32_t n,
                                                                  float4* __restrict__ kept, float4* __restrict__ removed /* nullable */, uint32_t* __restrict__ totals)
{
    const uint32_t nblk = (n + kTile - 1) / kTile;
    __shared__ uint32_t s_red[2][4];
    __shared__ uint32_t s_cnt[kTile / 256][4], s_off[kTile / 256][4];
    uint32_t before = 0, total = 0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 256) {
        const uint32_t v = blk[b];
        total += v;
        before += b < blockIdx.x ? v : 0u;
    }
    before = wave_sum(before);
    total = wave_sum(total);
    const int lane = lane_id(), w = wave_id();
    if (lane == 0) { s_red[0][w] = before; s_red[1][w] = total; }
    __syncthreads();
    before = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
    total = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    if (blockIdx.x == 0 && threadIdx.x == 0) { totals[0] = total; totals[1] = n - total; }
    // kept points before point i = kept points of earlier tiles + of earlier rounds and wavefronts of the tile + kept lanes below its own
    const uint32_t base = blockIdx.x * kTile;
    uint32_t f[kTile / 256], lr[kTile / 256];
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        f[k] = i < n ? flags[i] : 0u;
        const uint64_t m = __ballot(f[k] != 0u);
        lr[k] = static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
        if (lane == 0) s_cnt[k][w] = static_cast<uint32_t>(__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < (kTile / 256) * 4) {  // 32 lanes of wavefront 0: exclusive prefix in (round, wavefront) order
        const uint32_t v = s_cnt[threadIdx.x / 4][threadIdx.x % 4];
        uint32_t incl = v;
#pragma unroll
        for (int off = 1; off < (kTile / 256) * 4; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += t;
        }
        s_off[threadIdx.x / 4][threadIdx.x % 4] = incl - v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        if (i >= n) continue;
        const uint32_t rank = before + s_off[k][w] + lr[k];  // <= i, and < total when the point is kept
        if (f[k]) kept[rank] = in[i];
        else if (removed) removed[i - rank] = in[i];
    }
}

static KeyframeHeadArgs keyframe_head_args(const void* d_raw, const KeyframeLayout& lay, float4* d_out)
{
    KeyframeHeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.raw = static_cast<const uint8_t*>(d_raw);
    a.out = d_out;
    a.n = lay.width * lay.height;
    a.width = lay.width; a.row_step = lay.row_step; a.point_step = lay.point_step;
    a.ox = lay.off_x; a.oy = lay.off_y; a.oz = lay.off_z; a.oi = lay.off_intensity;
    return a;
}
static bool head_is_strict(const KeyframeHeadArgs& a) { return layout_is_strict(a.point_step, a.row_step, a.ox, a.oy, a.oz, a.oi); }

int keyframe_gather_device(mrgfe_ctx* ctx, const void* d_raw, const KeyframeLayout& lay, float4* d_cloud)
{
    const KeyframeHeadArgs a = keyframe_head_args(d_raw, lay, d_cloud);
    if (a.n == 0) return MRGFE_OK;
    const auto kern = head_is_strict(a) ? keyframe_head_kernel<false, false> : keyframe_head_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3((a.n + kTile - 1) / kTile), dim3(256), 0, ctx->stream, a, Centres{});
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// The gather of keyframe_head_kernel<false> for many messages at once (GraphDatabase::add_static_keyframes / flush_graph_queue / load_graph hand over
// whole lists of PointCloud2 clouds: src/mrg_slam/graph_database.cpp:181-182, 294-295, 449-461).  One workgroup per 2048-point tile as there; what the
// head kernel takes as kernel arguments comes from the tile's record instead — a workgroup-uniform 64-byte read (scalar loads), then the same per-point
// body.  A 33k-point keyframe alone is 17 workgroups on 256 compute units; ten of them in one launch are 170.
struct KeyframeTile {
    const uint8_t* raw;    // the message's records
    float4*        out;    // the message's cloud
    uint32_t       first;  // the tile's first point within the message
    uint32_t       n;      // points of the message
    uint32_t       width, row_step, point_step, ox, oy, oz;
    int32_t        oi;
    uint32_t       bytes;  // 1: not a strict layout, the tile reads its records by aligned words (messages of one call may differ)
    uint32_t       pad[2];
};
static_assert(sizeof(KeyframeTile) == 64, "KeyframeTile: one 64-byte record per tile");
// kAnyBytes: some tile of the launch has its `bytes` flag set (a workgroup-uniform branch); a call of strict messages only launches the kernel without it.
template <bool kAnyBytes>
__global__ __launch_bounds__(256) void keyframe_gather_many_kernel(const KeyframeTile* __restrict__ tiles)
{
    const KeyframeTile t = tiles[blockIdx.x];
    if (kAnyBytes && t.bytes) {
#pragma unroll
        for (int k = 0; k < kTile / 256; ++k) {
            const uint32_t i = t.first + k * 256 + threadIdx.x;
            if (i < t.n) t.out[i] = load_point_record_bytes(t.raw, i, t.width, t.row_step, t.point_step, t.ox, t.oy, t.oz, t.oi);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = t.first + k * 256 + threadIdx.x;
        if (i < t.n) t.out[i] = load_point_record(t.raw, i, t.width, t.row_step, t.point_step, t.ox, t.oy, t.oz, t.oi);
    }
}

int keyframe_gather_many_device(mrgfe_ctx* ctx, const KeyframeGatherItem* items, size_t count)
{
    std::vector<KeyframeTile> tiles;
    bool any_bytes = false;
    for (size_t m = 0; m < count; ++m) {
        const KeyframeHeadArgs a = keyframe_head_args(items[m].d_raw, items[m].lay, items[m].d_cloud);
        KeyframeTile t;
        std::memset(&t, 0, sizeof(t));
        t.raw = a.raw; t.out = a.out; t.n = a.n;
        t.width = a.width; t.row_step = a.row_step; t.point_step = a.point_step;
        t.ox = a.ox; t.oy = a.oy; t.oz = a.oz; t.oi = a.oi;
        t.bytes = head_is_strict(a) ? 0u : 1u;
        any_bytes = any_bytes || (t.bytes && a.n);
        for (uint64_t first = 0; first < a.n; first += kTile) {  // (an empty message has no tile)
            t.first = static_cast<uint32_t>(first);
            tiles.push_back(t);
        }
    }
    if (tiles.empty()) return MRGFE_OK;
    if (tiles.size() > 0x7fffffffu) { set_error("keyframe gather: %zu tiles in one launch", tiles.size()); return MRGFE_ERR_INVALID; }
    DevBuf& dtab = ctx->scratch[0];
    MRGFE_TRY(dtab.ensure(tiles.size() * sizeof(KeyframeTile)));
    MRGFE_TRY(ctx->stage_h2d(dtab.p, tiles.data(), tiles.size() * sizeof(KeyframeTile), ctx->stream));
    hipLaunchKernelGGL(any_bytes ? keyframe_gather_many_kernel<true> : keyframe_gather_many_kernel<false>, dim3(static_cast<uint32_t>(tiles.size())), dim3(256), 0, ctx->stream, dtab.as<KeyframeTile>());
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

int keyframe_split_device(mrgfe_ctx* ctx, const void* d_raw, const KeyframeLayout& lay, const float* centres, int K, float radius_sqr, float4* d_kept, size_t* n_kept,
                          float4* d_removed, size_t* n_removed)
{
    *n_kept = 0;
    *n_removed = 0;
    if (K < 1 || K > kMaxCentres) { set_error("keyframe callback: 1 to %d centres", kMaxCentres); return MRGFE_ERR_INVALID; }
    DevBuf &dcloud = ctx->scratch[0], &dfl = ctx->scratch[1];
    KeyframeHeadArgs a = keyframe_head_args(d_raw, lay, nullptr);
    if (a.n == 0) return MRGFE_OK;
    const uint32_t nblk = (a.n + kTile - 1) / kTile;
    MRGFE_TRY(dcloud.ensure(size_t(a.n) * 16));
    MRGFE_TRY(dfl.ensure(sizeof(uint32_t) * (size_t(a.n) + nblk + 2)));  // flags, tile counts, the two totals
    PinBuf& hp = ctx->pin[1];
    MRGFE_TRY(hp.ensure(2 * sizeof(uint32_t)));
    a.out = dcloud.as<float4>();
    a.flags = dfl.as<uint32_t>();
    a.blk = a.flags + a.n;
    a.K = K;
    a.radius_sqr = radius_sqr;
    uint32_t* d_tot = a.blk + nblk;
    Centres c{};
    for (int k = 0; k < K; ++k) for (int x = 0; x < 3; ++x) c.xyz[k][x] = centres[3 * k + x];
    hipStream_t st = ctx->stream;
    const auto kern = head_is_strict(a) ? keyframe_head_kernel<true, false> : keyframe_head_kernel<true, true>;
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), 0, st, a, c);
    MRGFE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(keyframe_partition_kernel, dim3(nblk), dim3(256), 0, st, a.out, a.flags, a.blk, a.n, d_kept, d_removed, d_tot);
    MRGFE_HIP_CHECK(hipGetLastError());
    uint32_t* h_tot = hp.as<uint32_t>();
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_tot, d_tot, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    if (size_t(h_tot[0]) + h_tot[1] != a.n) { set_error("keyframe callback: the partition reported %u + %u of %u points", h_tot[0], h_tot[1], a.n); return MRGFE_ERR_HIP; }
    *n_kept = h_tot[0];
    *n_removed = h_tot[1];
    return MRGFE_OK;
}

// ---- deskewing ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void deskew_kernel(const float4* __restrict__ in, uint32_t n, float avx, float avy, float avz, double scan_period, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = deskew_point(in[i], i, n, avx, avy, avz, scan_period);  // (scan_point.h: the scan head kernel runs the same body)
}

int deskew_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, const float ang_v[3], double scan_period, float4* d_out)
{
    if (n == 0) return MRGFE_OK;
    const uint32_t nn = static_cast<uint32_t>(n);
    // ang_v *= -1 (:275)
    hipLaunchKernelGGL(deskew_kernel, dim3((nn + 255) / 256), dim3(256), 0, ctx->stream, d_in, nn, ang_v[0] * -1.0f, ang_v[1] * -1.0f, ang_v[2] * -1.0f, scan_period, d_out);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// ---- rigid transform of a cloud ------------------------------------------------------------------------------------
struct Transform12 { float m[12]; };
__global__ __launch_bounds__(256) void transform_cloud_kernel(const float4* __restrict__ in, uint32_t n, Transform12 T, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = transform_finite_point(T.m, in[i]);  // pcl::transformPointCloud leaves the non-finite points of a non-dense cloud as they are (scan_point.h)
}

int transform_cloud_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, const float T_rowmajor[16], float4* d_out)
{
    if (n == 0) return MRGFE_OK;
    Transform12 T;
    std::memcpy(T.m, T_rowmajor, sizeof(T.m));
    const uint32_t nn = static_cast<uint32_t>(n);
    hipLaunchKernelGGL(transform_cloud_kernel, dim3((nn + 255) / 256), dim3(256), 0, ctx->stream, d_in, nn, T, d_out);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

}  // namespace mrgfe
