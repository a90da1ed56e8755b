// csrc/filters.hip — the prefilter chain of /root/reference/apps/prefiltering_component.cpp:149-151 on MI355X:
//   distance_filter (:206-229)            flag + exclusive scan + order-preserving compaction
//   pcl::VoxelGrid (:158-180)             bounding box -> voxel keys -> stable radix sort -> runs -> f32 centroids
//   pcl::RadiusOutlierRemoval (:195-198)  neighbour counts on the radix-sorted grid (cell = radius) + compaction
//   pcl::StatisticalOutlierRemoval (:189-192) k-NN mean distances on the grid, threshold from f64 statistics
// All passes are streaming / gather kernels bound by HBM and L2; nothing here is GEMM-shaped.
#include "filters.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bbox_device.h"
#include "cellsort.h"
#include "dev_float.h"
#include "dev_utils.h"
#include "ingest.h"
#include "ndt_build.h"
#include "nn_grid.h"
#include "record_store.h"
#include "scan_point.h"
#include "sor_threshold.h"

namespace mrgfe {

// ---- shared: order-preserving compaction -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos, uint32_t n,
                                                       float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && flags[i]) out[pos[i]] = in[i];
}

// scan flags (one problem) and compact; returns the kept count through *h_total (synchronises)
int compact_by_flags(mrgfe_ctx* ctx, const float4* d_in, uint32_t n, uint32_t* d_flags, float4* d_out, uint32_t* h_total)
{
    *h_total = 0;
    if (n == 0) return MRGFE_OK;
    hipStream_t st = ctx->stream;
    SliceTable  tab;
    tab.build(&n, 1);
    DevBuf &ds = ctx->scratch[0], &dpos = ctx->scratch[4], &dblk = ctx->scratch[8];
    MRGFE_TRY(ds.ensure(sizeof(Slice)));
    MRGFE_TRY(dpos.ensure(size_t(n) * 4));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    MRGFE_HIP_CHECK(hipMemcpyAsync(ds.p, tab.h.data(), sizeof(Slice), hipMemcpyHostToDevice, st));
    uint32_t* d_tot = dblk.as<uint32_t>() + tab.total_blks;
    MRGFE_TRY(exclusive_scan(ctx, d_flags, dpos.as<uint32_t>(), ds.as<Slice>(), tab, dblk.as<uint32_t>(), d_tot));
    hipLaunchKernelGGL(compact_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_in, d_flags, dpos.as<uint32_t>(), n, d_out);
    MRGFE_HIP_CHECK(hipGetLastError());
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_total, d_tot, 4, hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    return MRGFE_OK;
}

static int download(mrgfe_ctx* ctx, const void* d_src, size_t n, float* out)
{
    if (n == 0) return MRGFE_OK;
    MRGFE_HIP_CHECK(hipMemcpyAsync(out, d_src, n * 16, hipMemcpyDeviceToHost, ctx->stream));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MRGFE_OK;
}

// ---- distance filter -------------------------------------------------------------------------------------------
// p.getVector3fMap().norm(): float sqrt((x*x + y*y) + z*z), compared as double with strict inequalities (a non-finite point fails them)
__device__ __forceinline__ uint32_t distance_keep(const float4& p, double near_t, double far_t)
{
    const float  s = dot3f(p.x, p.x, p.y, p.y, p.z, p.z);
    const double d = static_cast<double>(sqrtf(s));
    return (d > near_t && d < far_t) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void distance_flags_kernel(const float4* __restrict__ in, uint32_t n, double near_t, double far_t, uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    flags[i] = distance_keep(in[i], near_t, far_t);
}

int filter_distance_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, double near_t, double far_t, float4* d_out, size_t* out_n)
{
    *out_n = 0;
    if (n == 0) return MRGFE_OK;
    const uint32_t nn = static_cast<uint32_t>(n);
    DevBuf& dfl = ctx->scratch[7];
    MRGFE_TRY(dfl.ensure(n * 4));
    hipLaunchKernelGGL(distance_flags_kernel, dim3((nn + 255) / 256), dim3(256), 0, ctx->stream, d_in, nn, near_t, far_t, dfl.as<uint32_t>());
    uint32_t kept = 0;
    MRGFE_TRY(compact_by_flags(ctx, d_in, nn, dfl.as<uint32_t>(), d_out, &kept));
    *out_n = kept;
    return MRGFE_OK;
}

// ---- voxel grid ------------------------------------------------------------------------------------------------
// one thread per voxel run: float running sums in ascending point index (the stable order), then divide by the count
__global__ __launch_bounds__(256) void voxel_centroid_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ sorted_vals, const uint32_t* __restrict__ seg_start,
                                                              uint32_t n_seg, int min_pts, float4* __restrict__ centroids, uint32_t* __restrict__ keep)
{
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_seg) return;
    const uint32_t b = seg_start[s], e = seg_start[s + 1];
    float sx = 0, sy = 0, sz = 0, si = 0;
    // four indices, then their four points, in flight at a time (two dependent loads per point otherwise); the additions stay in point order
    for (uint32_t k = b; k < e; k += 4) {
        uint32_t id[4];
        float4   p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) id[u] = sorted_vals[min(k + u, e - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = pts[id[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k + u < e) { sx += p[u].x; sy += p[u].y; sz += p[u].z; si += p[u].w; }
    }
    const float cnt = static_cast<float>(e - b);
    centroids[s] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
    keep[s] = (e - b) >= static_cast<uint32_t>(min_pts) ? 1u : 0u;
}

int launch_voxel_centroids(mrgfe_ctx* ctx, const float4* d_pts, const uint32_t* d_sorted_vals, const uint32_t* d_seg_start, uint32_t n_seg, int min_pts, float4* d_centroids,
                           uint32_t* d_keep)
{
    if (n_seg == 0) return MRGFE_OK;
    hipLaunchKernelGGL(voxel_centroid_kernel, dim3((n_seg + 255) / 256), dim3(256), 0, ctx->stream, d_pts, d_sorted_vals, d_seg_start, n_seg, min_pts, d_centroids, d_keep);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

int filter_voxelgrid_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, float leaf, int min_pts, float4* d_out, size_t* out_n, int* overflow)
{
    *out_n = 0;
    if (overflow) *overflow = 0;
    if (n == 0) return MRGFE_OK;
    hipStream_t st = ctx->stream;
    uint32_t    nn = static_cast<uint32_t>(n);
    SliceTable  tab;
    tab.build(&nn, 1);
    // descriptor block: slice | cloud ptr | n_valid | voxel params | leaf slice
    struct Desc { Slice sl; const float4* cp; uint32_t nv; uint32_t pad; VoxelParams vp; LeafSlice ls; };
    PinBuf& hp = ctx->pin[1];
    MRGFE_TRY(hp.ensure(sizeof(Desc) + sizeof(BBox) + 16));
    Desc* hd = hp.as<Desc>();
    std::memset(hd, 0, sizeof(Desc));
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
    if (h_bb->n_finite == 0) return MRGFE_OK;
    int32_t max_b[3], div_b[3];
    if (voxel_params_from_bbox(*h_bb, leaf, &hd->vp, max_b, div_b) != MRGFE_OK) {
        // PCL: warn and pass the input through
        if (overflow) *overflow = 1;
        MRGFE_HIP_CHECK(hipMemcpyAsync(d_out, d_in, n * 16, hipMemcpyDeviceToDevice, st));
        MRGFE_HIP_CHECK(hipStreamSynchronize(st));
        *out_n = n;
        return MRGFE_OK;
    }
    hd->nv = h_bb->n_finite;
    MRGFE_HIP_CHECK(hipMemcpyAsync(d_desc, hd, sizeof(Desc), hipMemcpyHostToDevice, st));
    int key_bits = 1;
    while (key_bits < 32 && (uint64_t(1) << key_bits) <= hd->vp.n_cells) ++key_bits;
    DevBuf &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6], &dblk = ctx->scratch[8];
    MRGFE_TRY(dk.ensure(n * 4)); MRGFE_TRY(dv.ensure(n * 4)); MRGFE_TRY(dkt.ensure(n * 4)); MRGFE_TRY(dvt.ensure(n * 4));
    MRGFE_TRY(dh.ensure(sizeof(uint32_t) * 256 * (tab.total_blks + 1)));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    MRGFE_TRY(ndt_launch_cellkeys(ctx, &d_desc->cp, &d_desc->sl, tab, &d_desc->vp, dk.as<uint32_t>(), dh.as<uint32_t>()));
    uint32_t *sk, *sv;
    MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), &d_desc->sl, tab, key_bits, dh.as<uint32_t>(), &sk, &sv, true, true));
    uint32_t* d_tot = dblk.as<uint32_t>() + tab.total_blks;
    MRGFE_TRY(exclusive_scan_run_heads(ctx, sk, nullptr, &d_desc->sl, tab, &d_desc->nv, dblk.as<uint32_t>(), d_tot));
    uint32_t* h_tot = reinterpret_cast<uint32_t*>(hp.as<char>() + sizeof(Desc) + sizeof(BBox));
    MRGFE_HIP_CHECK(hipMemcpyAsync(h_tot, d_tot, 4, hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    const uint32_t V = *h_tot;
    if (V == 0) return MRGFE_OK;
    hd->ls.n_leaves = V;
    hd->ls.leaf_off = 0;
    hd->ls.seg_off = 0;
    hd->ls.n_valid = hd->nv;
    MRGFE_HIP_CHECK(hipMemcpyAsync(&d_desc->ls, &hd->ls, sizeof(LeafSlice), hipMemcpyHostToDevice, st));
    DevBuf &dseg = ctx->scratch[9], &dcent = ctx->scratch[10], &dkeep = ctx->scratch[11];
    MRGFE_TRY(dseg.ensure(sizeof(uint32_t) * (size_t(V) + 4) + sizeof(int32_t) * size_t(V)));
    MRGFE_TRY(dcent.ensure(sizeof(float4) * size_t(V)));
    MRGFE_TRY(dkeep.ensure(sizeof(uint32_t) * size_t(V)));
    uint32_t* d_seg = dseg.as<uint32_t>();
    int32_t*  d_segkey = reinterpret_cast<int32_t*>(d_seg + V + 4);
    MRGFE_TRY(ndt_launch_segments(ctx, sk, &d_desc->sl, tab, &d_desc->nv, dblk.as<uint32_t>(), &d_desc->ls, d_seg, d_segkey));
    hipLaunchKernelGGL(voxel_centroid_kernel, dim3((V + 255) / 256), dim3(256), 0, st, d_in, sv, d_seg, V, min_pts, dcent.as<float4>(), dkeep.as<uint32_t>());
    MRGFE_HIP_CHECK(hipGetLastError());
    uint32_t kept = 0;
    MRGFE_TRY(compact_by_flags(ctx, dcent.as<float4>(), V, dkeep.as<uint32_t>(), d_out, &kept));
    *out_n = kept;
    return MRGFE_OK;
}

// ---- approximate voxel grid -----------------------------------------------------------------------------------------------------------
// pcl::ApproximateVoxelGrid (downsample_method APPROX_VOXELGRID: prefiltering_component.cpp:172-175, scan_matching_odometry_component.cpp:180-183)
// is a sequential algorithm on the CPU — every point looks up a 512-entry direct-mapped history keyed by a hash of its cell, flushes the entry
// (emits its centroid) when another cell holds it, and takes it over; the occupied entries are flushed at the end — and SURVEY.md left it there
// ("order dependent, effectively unparallelisable").  It decomposes exactly:
//   * an entry only ever sees the points that hash to it, in arrival order, so the 512 entries are independent sequences — a stable sort of
//     (hash, index) pairs lays them out; inside a sequence a maximal stretch of points of ONE cell is one emitted centroid (float sums in
//     arrival order / float count: one thread per stretch, like the voxel grid's runs);
//   * a stretch is emitted when the first point of the NEXT stretch of its entry arrives, so its place in the output is the number of such
//     "flushing" points with a smaller index — an exclusive scan over the cloud in its original order — and the last stretch of every entry
//     follows behind all of those, in entry order.
// Same output, point for point and bit for bit, as the sequential loop (oracle/filters.cpp approx_voxelgrid): no sequential pass anywhere.
__device__ __forceinline__ int avg_cell(float v)
{
    const float f = floorf(v);
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT_MIN;  // the x86 conversion's answer out of range and for NaN (the GPU's saturates)
    return static_cast<int>(f);
}
__device__ __forceinline__ void avg_cell3(const float4& p, float inv, int c[3])
{
#pragma clang fp contract(off)
    c[0] = avg_cell(p.x * inv); c[1] = avg_cell(p.y * inv); c[2] = avg_cell(p.z * inv);
}
// The five passes take the point count as an argument (the single filter: the host knows it) or read it from a Slice in device memory (the
// device-driven chain, whose launches are sized for the input and skip what lies beyond the live count): one body each.
__device__ __forceinline__ void avg_keys_body(const float4* __restrict__ in, uint32_t n, float inv, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    int c[3];
    avg_cell3(in[i], inv, c);
    keys[i] = (static_cast<uint32_t>(c[0]) * 7171u + static_cast<uint32_t>(c[1]) * 3079u + static_cast<uint32_t>(c[2]) * 4231u) & 511u;
}
// sorted position j starts a stretch iff its entry or its cell differs from position j - 1's; the first point of a stretch that is not its entry's first flushes
__device__ __forceinline__ void avg_heads_body(const float4* __restrict__ in, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint32_t n, float inv,
                                               uint32_t* __restrict__ head, uint32_t* __restrict__ flusher)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    uint32_t h = 1;
    if (j > 0) {
        const bool same_entry = sk[j] == sk[j - 1];
        int a[3], b[3];
        avg_cell3(in[sv[j]], inv, a);
        avg_cell3(in[sv[j - 1]], inv, b);
        const bool same_cell = a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
        h = (same_entry && same_cell) ? 0u : 1u;
        if (h && same_entry) flusher[sv[j]] = 1u;
    }
    head[j] = h;
}
__device__ __forceinline__ void avg_segments_body(const uint32_t* __restrict__ head, const uint32_t* __restrict__ ord, uint32_t n, const uint32_t* __restrict__ n_runs,
                                                  uint32_t* __restrict__ seg_start)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    if (head[j]) seg_start[ord[j]] = j;
    if (j + 1 == n) seg_start[*n_runs] = n;
}
// rank of every entry among the occupied ones (their last stretches close the output in entry order); the binary search runs over the first n sorted keys
__device__ __forceinline__ void avg_entry_ranks_body(const uint32_t* __restrict__ sk, uint32_t n, uint32_t* __restrict__ rank)
{
    __shared__ uint32_t lds[16];
    const uint32_t b = threadIdx.x;
    auto lower = [&](uint32_t key) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sk[mid] < key) lo = mid + 1; else hi = mid; }
        return lo;
    };
    const uint32_t occupied = lower(b + 1) > lower(b) ? 1u : 0u;
    uint32_t total;
    rank[b] = block_exclusive_scan<512>(occupied, lds, &total);
}
__device__ __forceinline__ void avg_emit_body(const float4* __restrict__ in, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint32_t n,
                                              const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ totals /* runs, flushing points */,
                                              const uint32_t* __restrict__ fpos, const uint32_t* __restrict__ entry_rank, float4* __restrict__ out)
{
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= totals[0]) return;
    const uint32_t b = seg_start[r], e = seg_start[r + 1];
    float sx = 0, sy = 0, sz = 0, si = 0;
    for (uint32_t k = b; k < e; ++k) {
        const float4 p = in[sv[k]];
        sx += p.x; sy += p.y; sz += p.z; si += p.w;
    }
    const float cnt = static_cast<float>(e - b);
    const uint32_t entry = sk[b];
    const uint32_t op = (e < n && sk[e] == entry) ? fpos[sv[e]] : totals[1] + entry_rank[entry];
    out[op] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
}
__global__ __launch_bounds__(256) void avg_keys_kernel(const float4* __restrict__ in, uint32_t n, float inv, uint32_t* __restrict__ keys) { avg_keys_body(in, n, inv, keys); }
__global__ __launch_bounds__(256) void avg_heads_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint32_t n, float inv,
                                                         uint32_t* __restrict__ head, uint32_t* __restrict__ flusher)
{
    avg_heads_body(in, sk, sv, n, inv, head, flusher);
}
__global__ __launch_bounds__(256) void avg_segments_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ ord, uint32_t n, const uint32_t* __restrict__ n_runs,
                                                            uint32_t* __restrict__ seg_start)
{
    avg_segments_body(head, ord, n, n_runs, seg_start);
}
__global__ __launch_bounds__(512) void avg_entry_ranks_kernel(const uint32_t* __restrict__ sk, uint32_t n, uint32_t* __restrict__ rank) { avg_entry_ranks_body(sk, n, rank); }
__global__ __launch_bounds__(256) void avg_emit_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint32_t n,
                                                        const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ fpos,
                                                        const uint32_t* __restrict__ entry_rank, float4* __restrict__ out)
{
    avg_emit_body(in, sk, sv, n, seg_start, totals, fpos, entry_rank, out);
}
// the device-driven forms: the live count is sl->n (the chain's PfState::sl_in); the numbers of stretches and of flushing points stay in `totals`
__global__ __launch_bounds__(256) void avg_keys_dd_kernel(const float4* __restrict__ in, const Slice* __restrict__ sl, float inv, uint32_t* __restrict__ keys)
{
    avg_keys_body(in, sl->n, inv, keys);
}
__global__ __launch_bounds__(256) void avg_heads_dd_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, const Slice* __restrict__ sl,
                                                            float inv, uint32_t* __restrict__ head, uint32_t* __restrict__ flusher)
{
    avg_heads_body(in, sk, sv, sl->n, inv, head, flusher);
}
__global__ __launch_bounds__(256) void avg_segments_dd_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ ord, const Slice* __restrict__ sl,
                                                               const uint32_t* __restrict__ n_runs, uint32_t* __restrict__ seg_start)
{
    avg_segments_body(head, ord, sl->n, n_runs, seg_start);
}
__global__ __launch_bounds__(512) void avg_entry_ranks_dd_kernel(const uint32_t* __restrict__ sk, const Slice* __restrict__ sl, uint32_t* __restrict__ rank)
{
    avg_entry_ranks_body(sk, sl->n, rank);
}
__global__ __launch_bounds__(256) void avg_emit_dd_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, const Slice* __restrict__ sl,
                                                           const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ fpos,
                                                           const uint32_t* __restrict__ entry_rank, float4* __restrict__ out)
{
    avg_emit_body(in, sk, sv, sl->n, seg_start, totals, fpos, entry_rank, out);
}

int filter_approx_voxelgrid_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, float leaf, float4* d_out, size_t* out_n)
{
    *out_n = 0;
    if (n == 0) return MRGFE_OK;
    if (n > 0x7fffffffu) { set_error("approximate voxel grid: cloud too large"); return MRGFE_ERR_INVALID; }
    hipStream_t st = ctx->stream;
    uint32_t    nn = static_cast<uint32_t>(n);
    SliceTable  tab;
    tab.build(&nn, 1);
    DevBuf &ds = ctx->scratch[0], &drank = ctx->scratch[1], &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6],
           &dhead = ctx->scratch[7], &dblk = ctx->scratch[8], &dseg = ctx->scratch[9], &dfpos = ctx->scratch[10], &dflush = ctx->scratch[11], &dord = ctx->scratch[12];
    MRGFE_TRY(ds.ensure(sizeof(Slice)));
    MRGFE_TRY(drank.ensure(sizeof(uint32_t) * 512));
    MRGFE_TRY(dk.ensure(n * 4)); MRGFE_TRY(dv.ensure(n * 4)); MRGFE_TRY(dkt.ensure(n * 4)); MRGFE_TRY(dvt.ensure(n * 4));
    MRGFE_TRY(dh.ensure(sizeof(uint32_t) * 256 * (tab.total_blks + 1)));
    MRGFE_TRY(dhead.ensure(n * 4)); MRGFE_TRY(dord.ensure(n * 4)); MRGFE_TRY(dflush.ensure(n * 4)); MRGFE_TRY(dfpos.ensure(n * 4));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    MRGFE_TRY(dseg.ensure(sizeof(uint32_t) * (n + 4)));
    MRGFE_TRY(ctx->stage_h2d(ds.p, tab.h.data(), sizeof(Slice), st));
    const float inv = 1.0f / leaf;  // inverse_leaf_size_ = Array3f::Ones() / leaf_size_
    const dim3  g256((nn + 255) / 256), b256(256);
    uint32_t*   d_tot = dblk.as<uint32_t>() + tab.total_blks;  // [0] stretches, [1] flushing points
    hipLaunchKernelGGL(avg_keys_kernel, g256, b256, 0, st, d_in, nn, inv, dk.as<uint32_t>());
    uint32_t *sk, *sv;
    MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), ds.as<Slice>(), tab, 9, dh.as<uint32_t>(), &sk, &sv, true));
    MRGFE_HIP_CHECK(hipMemsetAsync(dflush.p, 0, n * 4, st));
    hipLaunchKernelGGL(avg_heads_kernel, g256, b256, 0, st, d_in, sk, sv, nn, inv, dhead.as<uint32_t>(), dflush.as<uint32_t>());
    MRGFE_TRY(exclusive_scan(ctx, dhead.as<uint32_t>(), dord.as<uint32_t>(), ds.as<Slice>(), tab, dblk.as<uint32_t>(), d_tot));
    hipLaunchKernelGGL(avg_segments_kernel, g256, b256, 0, st, dhead.as<uint32_t>(), dord.as<uint32_t>(), nn, d_tot, dseg.as<uint32_t>());
    MRGFE_TRY(exclusive_scan(ctx, dflush.as<uint32_t>(), dfpos.as<uint32_t>(), ds.as<Slice>(), tab, dblk.as<uint32_t>(), d_tot + 1));
    hipLaunchKernelGGL(avg_entry_ranks_kernel, dim3(1), dim3(512), 0, st, sk, nn, drank.as<uint32_t>());
    hipLaunchKernelGGL(avg_emit_kernel, g256, b256, 0, st, d_in, sk, sv, nn, dseg.as<uint32_t>(), d_tot, dfpos.as<uint32_t>(), drank.as<uint32_t>(), d_out);
    MRGFE_HIP_CHECK(hipGetLastError());
    uint32_t runs = 0;
    MRGFE_HIP_CHECK(hipMemcpyAsync(&runs, d_tot, 4, hipMemcpyDeviceToHost, st));
    MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    *out_n = runs;
    return MRGFE_OK;
}

// ---- radius outlier removal ------------------------------------------------------------------------------------
int filter_radius_outlier_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, double radius, int min_neighbors, float4* d_out, size_t* out_n)
{
    *out_n = 0;
    if (n == 0) return MRGFE_OK;
    NnGrid& grid = ctx_tmp_grid(ctx);
    int st = grid.build(ctx, d_in, n, static_cast<float>(radius), NnGrid::kCrowding1nn, 1);
    if (st == MRGFE_OK) {
        DevBuf& dfl = ctx->scratch[7];
        st = dfl.ensure(n * 4);
        // inlier iff #{q: (double)sqdist <= radius*radius} >= min_neighbors + 1 (the point itself counts)
        if (st == MRGFE_OK) st = grid.radius_count_flags(ctx, d_in, n, radius * radius, min_neighbors + 1, dfl.as<uint32_t>());
        uint32_t kept = 0;
        if (st == MRGFE_OK) st = compact_by_flags(ctx, d_in, static_cast<uint32_t>(n), dfl.as<uint32_t>(), d_out, &kept);
        *out_n = kept;
    }
    return st;
}

// ---- statistical outlier removal -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sor_mean_dist_kernel(const float* __restrict__ sqd, uint32_t n, int k1, float* __restrict__ dist, uint32_t* __restrict__ valid)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* row = sqd + size_t(i) * k1;
    float  d = 0.0f;
    uint32_t ok = 0;
    if (row[k1 - 1] >= 0.0f) {  // all mean_k + 1 neighbours found
        double sum = 0.0;
        for (int j = 1; j < k1; ++j) sum += static_cast<double>(sqrtf(row[j]));  // k = 0 is the query point
        d = static_cast<float>(sum / static_cast<double>(k1 - 1));
        ok = 1;
    }
    dist[i] = d;
    valid[i] = ok;
}

__global__ __launch_bounds__(256) void sor_flags_kernel(const float* __restrict__ dist, uint32_t n, double thr, uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flags[i] = (static_cast<double>(dist[i]) > thr) ? 0u : 1u;
}

int filter_statistical_outlier_device(mrgfe_ctx* ctx, const float4* d_in, size_t n, int mean_k, double stddev_mul, float4* d_out, size_t* out_n)
{
    *out_n = 0;
    if (n == 0) return MRGFE_OK;
    hipStream_t    st = ctx->stream;
    const uint32_t nn = static_cast<uint32_t>(n);
    const int      k1 = mean_k + 1;
    NnGrid& grid = ctx_tmp_grid(ctx);
    MRGFE_TRY(grid.build(ctx, d_in, n, 1.0f, NnGrid::kCrowdingKnn));
    DevBuf ddist, knn_d, knn_i;  // (per-call buffers, freed at the return, `knn_i` first)
    MRGFE_TRY(knn_i.ensure(n * k1 * 4));
    MRGFE_TRY(knn_d.ensure(n * k1 * 4));
    MRGFE_TRY(ddist.ensure(n * 8));
    MRGFE_TRY(grid.knn_device(ctx, d_in, n, k1, knn_i.as<int32_t>(), knn_d.as<float>()));
    float*    d_dist = ddist.as<float>();
    uint32_t* d_valid = reinterpret_cast<uint32_t*>(d_dist + n);
    hipLaunchKernelGGL(sor_mean_dist_kernel, dim3((nn + 255) / 256), dim3(256), 0, st, knn_d.as<float>(), nn, k1, d_dist, d_valid);
    // PCL's mean / variance: sequential f64 sums over the float distances (float square) - done on the host in that order
    std::vector<float>    h_dist(n);
    std::vector<uint32_t> h_valid(n);
    if (hipMemcpyAsync(h_dist.data(), d_dist, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(h_valid.data(), d_valid, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        set_error("statistical outlier: device to host copy failed");
        return MRGFE_ERR_HIP;
    }
    const double thr = sor::sequential<false>(h_dist.data(), h_valid.data(), n, stddev_mul).thr;  // (sor_threshold.h: the loop and the mean / variance / threshold tail)
    DevBuf& dfl = ctx->scratch[7];
    MRGFE_TRY(dfl.ensure(n * 4));
    hipLaunchKernelGGL(sor_flags_kernel, dim3((nn + 255) / 256), dim3(256), 0, st, d_dist, nn, thr, dfl.as<uint32_t>());
    uint32_t kept = 0;
    const int rc = compact_by_flags(ctx, d_in, nn, dfl.as<uint32_t>(), d_out, &kept);
    *out_n = kept;
    return rc;
}

// ---- host-pointer wrappers (the C ABI) -------------------------------------------------------------------------
template <class F>
static int host_wrap(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float* out, size_t* out_n, F&& f)
{
    *out_n = 0;
    if (n == 0) return MRGFE_OK;
    DevBuf dout, din;  // per-call buffers (the scratch slots are all in use by the algorithms), freed at the return, `din` first
    MRGFE_TRY(din.ensure(n * 16));
    MRGFE_TRY(dout.ensure(n * 16));
    MRGFE_TRY(upload_cloud(ctx, xyzi, n, stride, din.p));
    size_t m = 0;
    MRGFE_TRY(f(din.as<float4>(), dout.as<float4>(), &m));
    MRGFE_TRY(download(ctx, dout.p, m, out));
    *out_n = m;
    return MRGFE_OK;
}

// ---- the chain with its counts on the device (round 4) --------------------------------------------------------------------------------
// distance filter -> VoxelGrid -> RadiusOutlierRemoval used to hand every intermediate point COUNT to the host, which sized the next stage's
// tables: 8 host waits and ~18 small copies per scan for 0.45 ms of kernel time (CHANGELOG.md (rounds 1 - 4 notes, §10.6): 1.0 - 1.16 ms per 132k-point scan).  Here
// the counts stay where they are produced: the slices, voxel parameters and leaf slices the batched primitives read are members of ONE state
// record in device memory (PfState), rewritten between the stages by single-thread kernels that repeat the host's arithmetic float for float;
// every launch is sized for the input size and skips what lies beyond the device-side count; the radius filter's grid sizes itself
// (nn_build_device_driven).  The host waits once, reads five counts and an anomaly word from pinned memory, and only then learns how many
// points came out.  Anything unusual (no finite point, PCL's "leaf size too small" pass-through, a grid beyond its table) sets a bit in that
// word and the call is repeated through the host-driven chain below: same kernels for the arithmetic, so the outputs are the same bits
// either way (tests/test_gpu_filters.py holds the two against each other and the oracle).
// The same chain serves distance filter -> VoxelGrid -> StatisticalOutlierRemoval, the reference's code default: behind the voxel grid's compaction
// the k-NN mean distances on a grid that sizes itself (nn_knn_mean_device_driven) and PCL's threshold from certified tree sums (sor_threshold.h)
// take the radius filter's place (tests/test_gpu_prefilter_statistical.py).
// The chain is three stages (pf_stage_head / _downsample / _outlier below), so the other chains the parameters express are served the same way: the
// approximate grid's passes over the live count or no downsample at all in the middle, the radius filter or only a finish at the end
// (tests/test_gpu_prefilter_chains.py); the downsample stage alone serves the odometry frame (downsample_device_driven).
struct PfState {
    const float4* cp[2];  // cloud read by the downsample stage / by the outlier stage
    Slice       sl_in;    // points after the distance filter
    Slice       sl_vox;   // voxel runs (their centroids are compacted by the min-points flags)
    Slice       sl_rad;   // points after the downsample stage
    uint32_t    nv, pad0;
    VoxelParams vp;
    LeafSlice   ls;
    // after the distance filter, finite among them, voxels, after the downsample stage (APPROX_VOXELGRID: both the emitted centroids; no downsample: both
    // counts[0]), after the outlier filter (none: counts[3])
    uint32_t    counts[6];
    uint32_t    anomaly;
    uint32_t    pad1;
    uint32_t    bb_n[2];    // partial bounding boxes (one per tile the producer left) of the cloud the downsample stage / the outlier stage reads
    sor::Result sor;        // StatisticalOutlierRemoval: the sums, the threshold and their certificate (sor_finish_kernel)
};
constexpr uint32_t kPfAnomalyEmpty = 1u, kPfAnomalyOverflow = 2u, kPfAnomalyNoVoxel = 4u;
constexpr uint32_t kPfAnomalyCertificate = 8u;  // a tree sum of the statistical filter is not certified to be the sequential one (sor_threshold.h)
constexpr uint32_t kPfAnomalyRecheck = 16u;     // set by the HOST behind the wait: its own build of the threshold's tail gives other bits than the device's
constexpr uint32_t kPfAnomalyNonFinite = 32u;   // a non-finite point reached the outlier stage (distance filter off and no VoxelGrid in front of it)
// the pinned status record the host reads behind its one wait: words 0..4 the stage counts, 5 the anomaly word, 6 the completion mark; the box of the
// voxel centroids at word 8 (28 bytes); the statistical filter's result at byte 64
// and behind it what nn_build_device_sized chose for that filter's k-NN grid (NnSizedStatus)
constexpr size_t kPfStatusSorOffset = 64, kPfStatusGridOffset = (kPfStatusSorOffset + sizeof(sor::Result) + 7) & ~size_t(7);
constexpr size_t kPfStatusBytes = kPfStatusGridOffset + sizeof(NnSizedStatus);
static_assert(32 + sizeof(BBox) <= kPfStatusSorOffset, "the box ends before the statistical filter's record");

__device__ __forceinline__ Slice pf_slice(uint32_t n)
{
    Slice s;
    s.n = n; s.off = 0; s.blk_off = 0; s.nblk = (n + kTile - 1) / kTile;
    return s;
}
__device__ __forceinline__ void pf_state_init(PfState* __restrict__ st, const float4* cp0, const float4* cp1, uint32_t n_in)
{
    PfState s;
    memset(&s, 0, sizeof(s));
    s.cp[0] = cp0;
    s.cp[1] = cp1;
    s.sl_in = pf_slice(n_in);
    s.counts[0] = n_in;
    s.bb_n[0] = s.sl_in.nblk;
    *st = s;
}
__global__ void pf_init_kernel(PfState* __restrict__ st, const float4* cp0, const float4* cp1, uint32_t n_in)
{
    if (threadIdx.x || blockIdx.x) return;
    pf_state_init(st, cp0, cp1, n_in);
}
// The distance filter of the chain: flags of a tile of 2048 points and the tile's count of kept points (what scan_tile_sum_kernel would
// count in a launch of its own); workgroup 0 starts the chain's state first.
__global__ __launch_bounds__(256) void pf_distance_tiles_kernel(const float4* __restrict__ in, uint32_t n, double near_t, double far_t, uint32_t* __restrict__ flags,
                                                                 uint32_t* __restrict__ blk, PfState* __restrict__ st, const float4* cp0, const float4* cp1)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) pf_state_init(st, cp0, cp1, n);
    const uint32_t base = blockIdx.x * kTile;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const uint32_t f = distance_keep(in[i], near_t, far_t);
            flags[i] = f;
            cnt += f;
        }
    }
    __shared__ uint32_t sw[4];
    cnt = wave_sum(cnt);
    if (lane_id() == 0) sw[wave_id()] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}
// The scan head: PrefilteringComponent::cloud_callback up to its distance test (apps/prefiltering_component.cpp:119-149) in one pass over the wire
// records of a scan.  Per point: the strided record is read (pcl::fromROSMsg), deskewed (kDeskew), transformed into base_link_frame (kTransform) —
// scan_point.h, the bodies of gather_points_kernel, deskew_kernel and transform_cloud_kernel — and stored as the packed float4 the chain reads; with
// kFlags the kernel is also the chain's distance filter (pf_distance_tiles_kernel's flags, tile counts and first state).  Same tile shape as that
// kernel: one workgroup per 2048 points.  The three switches are compile-time: a variant carries only the registers of what it does.
struct ScanHeadArgs {
    const uint8_t* raw;
    float4*        out;
    uint32_t       n, width, row_step, point_step, ox, oy, oz;
    int32_t        oi;
    float          av[3];  // negated angular velocity
    double         scan_period;
    float          T[12];
    double         near_t, far_t;
    uint32_t*      flags;
    uint32_t*      blk;
    PfState*       st;
    const float4  *cp0, *cp1;
};
// kBytes: the layout is not a strict one (ingest.h layout_is_strict) and the record's fields are put together from aligned words.
template <bool kDeskew, bool kTransform, bool kFlags, bool kBytes = false>
__global__ __launch_bounds__(256) void scan_head_kernel(const ScanHeadArgs a)
{
    if (kFlags && blockIdx.x == 0 && threadIdx.x == 0) pf_state_init(a.st, a.cp0, a.cp1, a.n);
    const uint32_t base = blockIdx.x * kTile;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        if (i < a.n) {
            float4 p = load_point_record_as<kBytes>(a.raw, i, a.width, a.row_step, a.point_step, a.ox, a.oy, a.oz, a.oi);
            if (kDeskew) p = deskew_point(p, i, a.n, a.av[0], a.av[1], a.av[2], a.scan_period);
            if (kTransform) p = transform_finite_point(a.T, p);
            a.out[i] = p;
            if (kFlags) {
                const uint32_t f = distance_keep(p, a.near_t, a.far_t);
                a.flags[i] = f;
                cnt += f;
            }
        }
    }
    if (!kFlags) return;
    __shared__ uint32_t sw[4];
    cnt = wave_sum(cnt);
    if (lane_id() == 0) sw[wave_id()] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.blk[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}
// What the head needs besides the scan when it is also the chain's distance filter
struct ScanHeadFlags {
    double        near_t, far_t;
    uint32_t*     flags;
    uint32_t*     blk;
    PfState*      st;
    const float4 *cp0, *cp1;
};
static int launch_scan_head(mrgfe_ctx* ctx, const ScanHead& h, const void* d_raw, float4* d_out, const ScanHeadFlags* fl)
{
    ScanHeadArgs a;
    std::memset(&a, 0, sizeof(a));
    a.raw = static_cast<const uint8_t*>(d_raw);
    a.out = d_out;
    a.n = h.width * h.height;
    a.width = h.width; a.row_step = h.row_step; a.point_step = h.point_step;
    a.ox = h.off_x; a.oy = h.off_y; a.oz = h.off_z; a.oi = h.off_intensity;
    for (int k = 0; k < 3; ++k) a.av[k] = h.ang_v[k] * -1.0f;  // ang_v *= -1 (:275), as deskew_device does
    a.scan_period = h.scan_period;
    std::memcpy(a.T, h.T, sizeof(a.T));
    if (fl) { a.near_t = fl->near_t; a.far_t = fl->far_t; a.flags = fl->flags; a.blk = fl->blk; a.st = fl->st; a.cp0 = fl->cp0; a.cp1 = fl->cp1; }
    using Kernel = void (*)(const ScanHeadArgs);
    static const Kernel variants[8] = {scan_head_kernel<false, false, false>, scan_head_kernel<false, false, true>, scan_head_kernel<false, true, false>,
                                       scan_head_kernel<false, true, true>,   scan_head_kernel<true, false, false>, scan_head_kernel<true, false, true>,
                                       scan_head_kernel<true, true, false>,   scan_head_kernel<true, true, true>};
    static const Kernel byte_variants[8] = {scan_head_kernel<false, false, false, true>, scan_head_kernel<false, false, true, true>, scan_head_kernel<false, true, false, true>,
                                            scan_head_kernel<false, true, true, true>,   scan_head_kernel<true, false, false, true>, scan_head_kernel<true, false, true, true>,
                                            scan_head_kernel<true, true, false, true>,   scan_head_kernel<true, true, true, true>};
    const bool   strict = layout_is_strict(h.point_step, h.row_step, h.off_x, h.off_y, h.off_z, h.off_intensity);
    const Kernel kern = (strict ? variants : byte_variants)[(h.deskew ? 4 : 0) | (h.transform ? 2 : 0) | (fl ? 1 : 0)];
    hipLaunchKernelGGL(kern, dim3((a.n + kTile - 1) / kTile), dim3(256), 0, ctx->stream, a);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}
// Order-preserving compaction of the chain in ONE launch behind the tile counts: a workgroup adds up the counts of the tiles before its own
// (and of all tiles) itself, ranks its tile's kept elements by ballots and moves them; workgroup 0 records the kept count in the chain's state, and (kWhich 0 and 1) every workgroup leaves the bounding box of what it kept for the stage that reads the output — the
// exclusive scan (three launches), the compaction, the count and the bounding-box pass were six launches.
//   kWhich 0: the distance filter (n known to the host)      -> sl_in,  counts[0], boxes for the voxel grid
//   kWhich 1: the voxel grid's centroids (n = sl_vox.n)       -> sl_rad, counts[3], boxes for the radius filter's grid
//   kWhich 2: the outlier filter, radius or statistical (n = sl_rad.n) -> counts[4] and the host's status words
template <int kWhich>
__global__ __launch_bounds__(256) void pf_compact_kernel(const float4* __restrict__ in, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ blk, uint32_t n_host,
                                                          float4* __restrict__ out, PfState* st, uint32_t* __restrict__ h_status, BBox* __restrict__ partial)
{
    const uint32_t n = kWhich == 0 ? n_host : (kWhich == 1 ? st->sl_vox.n : st->sl_rad.n);
    const uint32_t nblk = (n + kTile - 1) / kTile;
    if (blockIdx.x >= nblk && blockIdx.x != 0) return;  // (workgroup 0 reports the count of an empty input too)
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
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (kWhich == 0) { st->sl_in = pf_slice(total); st->counts[0] = total; st->bb_n[0] = nblk; }
        else if (kWhich == 1) { st->sl_rad = pf_slice(total); st->counts[3] = total; st->bb_n[1] = nblk; }
        else {
            st->counts[4] = total;
            for (int k = 0; k < 5; ++k) h_status[k] = st->counts[k];
            h_status[5] = st->anomaly;
            __threadfence_system();
            h_status[6] = 0x600df00du;  // written last: the record is complete (the host reads it behind its one wait for the stream)
        }
    }
    if (blockIdx.x >= nblk) return;
    // rank of a kept element = kept elements of earlier rounds and wavefronts of the tile + kept lanes below its own
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
    BoxAcc acc;
    acc.init();
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        if (f[k]) {
            const float4 p = in[base + k * 256 + threadIdx.x];
            out[before + s_off[k][w] + lr[k]] = p;
            if (kWhich != 2) acc.add(p);
        }
    }
    if (kWhich != 2) {
        const BBox b = block_merge_box(acc);
        if (threadIdx.x == 0) partial[blockIdx.x] = b;
    }
}
// voxel_params_from_bbox (ndt_engine.cpp) on the device, float for float
__global__ __launch_bounds__(256) void pf_voxel_params_kernel(PfState* __restrict__ st, const BBox* __restrict__ partial, float leaf)
{
#pragma clang fp contract(off)
    const BBox bb = block_merge_partials(partial, st->bb_n[0]);  // (the boxes the producer of the cloud left, one per tile of its input)
    if (threadIdx.x) return;
    st->counts[1] = bb.n_finite;
    VoxelParams vp;
    memset(&vp, 0, sizeof(vp));
    if (bb.n_finite == 0) { st->anomaly |= kPfAnomalyEmpty; st->sl_in = pf_slice(0); st->vp = vp; st->nv = 0; return; }
    const float   inv_leaf = 1.0f / leaf;
    const int64_t dx = static_cast<int64_t>((bb.mx[0] - bb.mn[0]) * inv_leaf) + 1;
    const int64_t dy = static_cast<int64_t>((bb.mx[1] - bb.mn[1]) * inv_leaf) + 1;
    const int64_t dz = static_cast<int64_t>((bb.mx[2] - bb.mn[2]) * inv_leaf) + 1;
    bool over = dx * dy * dz > static_cast<int64_t>(INT32_MAX);
    int32_t div_b[3] = {1, 1, 1};
    if (!over) {
        for (int a = 0; a < 3; ++a) {
            vp.min_b[a] = static_cast<int32_t>(floorf(bb.mn[a] * inv_leaf));
            div_b[a] = static_cast<int32_t>(floorf(bb.mx[a] * inv_leaf)) - vp.min_b[a] + 1;
        }
        vp.divb_mul[0] = 1;
        vp.divb_mul[1] = div_b[0];
        vp.divb_mul[2] = div_b[0] * div_b[1];
        vp.inv_leaf = inv_leaf;
        const int64_t cells = static_cast<int64_t>(div_b[0]) * div_b[1] * div_b[2];
        over = cells > static_cast<int64_t>(INT32_MAX);
        vp.n_cells = static_cast<uint32_t>(cells);
    }
    if (over) { st->anomaly |= kPfAnomalyOverflow; st->sl_in = pf_slice(0); memset(&vp, 0, sizeof(vp)); st->vp = vp; st->nv = 0; return; }
    st->vp = vp;
    st->nv = bb.n_finite;
}
// blk: the tiles' run-head counts (run_head_tile_counts) -> their exclusive prefix, in place (scan_tiles_kernel's work), and the run count into the state
__global__ __launch_bounds__(256) void pf_leaves_kernel(PfState* __restrict__ st, uint32_t* __restrict__ blk)
{
    __shared__ uint32_t lds[8];
    const uint32_t nblk = st->sl_in.nblk;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nblk ? blk[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<256>(v, lds, &total);
        if (b < nblk) blk[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x) return;
    const uint32_t V = st->anomaly ? 0u : carry;
    LeafSlice ls;
    memset(&ls, 0, sizeof(ls));
    ls.n_leaves = V;
    ls.n_valid = st->nv;
    st->ls = ls;
    st->sl_vox = pf_slice(V);
    st->counts[2] = V;
    if (V == 0) st->anomaly |= kPfAnomalyNoVoxel;
}
__global__ __launch_bounds__(256) void voxel_centroid_dd_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ sorted_vals, const uint32_t* __restrict__ seg_start,
                                                                 const Slice* __restrict__ runs, int min_pts, float4* __restrict__ centroids, uint32_t* __restrict__ keep)
{
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= runs->n) return;
    const uint32_t b = seg_start[s], e = seg_start[s + 1];
    float sx = 0, sy = 0, sz = 0, si = 0;
    // four indices, then their four points, in flight at a time (two dependent loads per point otherwise); the additions stay in point order
    for (uint32_t k = b; k < e; k += 4) {
        uint32_t id[4];
        float4   p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) id[u] = sorted_vals[min(k + u, e - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = pts[id[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k + u < e) { sx += p[u].x; sy += p[u].y; sz += p[u].z; si += p[u].w; }
    }
    const float cnt = static_cast<float>(e - b);
    centroids[s] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
    keep[s] = (e - b) >= static_cast<uint32_t>(min_pts) ? 1u : 0u;
}
// ---- the single-workgroup kernels between the stages of the chains without a VoxelGrid or without an outlier filter ----------------------------------
// downsample NONE: the outlier stage reads the cloud, the count and the boxes the head left
__global__ __launch_bounds__(256) void pf_no_downsample_kernel(PfState* __restrict__ st, const BBox* __restrict__ partial, int outlier_follows)
{
    const BBox bb = block_merge_partials(partial, st->bb_n[0]);
    if (threadIdx.x) return;
    const uint32_t n = st->sl_in.n;
    st->counts[1] = bb.n_finite;
    st->counts[2] = n;
    st->counts[3] = n;
    st->sl_rad = st->sl_in;
    st->bb_n[1] = st->bb_n[0];
    if (outlier_follows && n == 0) st->anomaly |= kPfAnomalyEmpty;
    if (outlier_follows && bb.n_finite != n) st->anomaly |= kPfAnomalyNonFinite;
}
// APPROX_VOXELGRID: the emitted centroids (totals[0], left by the scan of the stretch heads) become the outlier stage's count; their boxes follow
// (bounding_box_partials over sl_rad: one per tile of the OUTPUT)
__global__ __launch_bounds__(256) void pf_approx_done_kernel(PfState* __restrict__ st, const BBox* __restrict__ partial_in, const uint32_t* __restrict__ totals)
{
    const BBox bb = block_merge_partials(partial_in, st->bb_n[0]);
    if (threadIdx.x) return;
    const uint32_t runs = totals[0];
    st->counts[1] = bb.n_finite;
    st->counts[2] = runs;
    st->counts[3] = runs;
    st->sl_rad = pf_slice(runs);
    st->bb_n[1] = st->sl_rad.nblk;
    if (st->sl_in.n == 0) st->anomaly |= kPfAnomalyEmpty;
}
// the approximate grid's centroids are non-finite where its points were: the outlier stage hands such a cloud back
__global__ __launch_bounds__(256) void pf_finite_check_kernel(PfState* __restrict__ st, const BBox* __restrict__ partial)
{
    const BBox bb = block_merge_partials(partial, st->bb_n[1]);
    if (threadIdx.x == 0 && bb.n_finite != st->sl_rad.n) st->anomaly |= kPfAnomalyNonFinite;
}
// A chain without an outlier filter ends here: the count and the merged box of the downsample stage's output (nn_build_device_driven reports that box
// where an outlier filter follows) and the host's status words, as pf_compact_kernel<2> writes them.
__global__ __launch_bounds__(256) void pf_finish_kernel(PfState* __restrict__ st, const BBox* __restrict__ partial, uint32_t* __restrict__ h_status, BBox* __restrict__ h_box)
{
    const BBox bb = block_merge_partials(partial, st->bb_n[1]);
    if (threadIdx.x) return;
    st->counts[4] = st->counts[3];
    *h_box = bb;
    for (int k = 0; k < 5; ++k) h_status[k] = st->counts[k];
    h_status[5] = st->anomaly;
    __threadfence_system();
    h_status[6] = 0x600df00du;
}
// ---- the filtered scan as wire records (pcl::toROSMsg(*filtered, filtered_ros), apps/prefiltering_component.cpp:152-155) ------------------------------------
// Behind the chain's last stage and in front of its one wait: record i of the work buffer for i < counts[4], the count the last stage left in the state.
// The launch is sized for the input; a chain that reports an anomaly (the host-driven passes will make the cloud) writes nothing.  One 16-byte store per
// lane at point_step 16, two at 32 (record_store.h): a wavefront writes 1024 / 2048 contiguous bytes, into the caller's page-locked buffer or the
// context's pinned one.  i < counts[4] <= the input count, and `out` has room for the input count (RecordSink).
template <int kStep>
__global__ __launch_bounds__(256) void pf_records_dd_kernel(const float4* __restrict__ in, const PfState* __restrict__ st, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (st->anomaly != 0u || i >= st->counts[4]) return;
    store_record<kStep>(out, i, in[i], EgressOffsets{});
}
// the same with the count known to the host: behind the host-driven passes, and for any packed device cloud (mrgfe_cloud_records_device)
template <int kStep>
__global__ __launch_bounds__(256) void cloud_records_kernel(const float4* __restrict__ in, uint32_t n, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    store_record<kStep>(out, i, in[i], EgressOffsets{});
}
// two packed clouds in one launch (the keyframe callback's kept and removed points, mrgfe_keyframe_callback_records): thread i < na writes record i of the
// first, na <= i < na + nb record i - na of the second; launched with ceil((na + nb) / 256) workgroups, each output has room for its own count
template <int kStep>
__global__ __launch_bounds__(256) void cloud_pair_records_kernel(const float4* __restrict__ a, uint32_t na, float4* __restrict__ out_a, const float4* __restrict__ b, uint32_t nb,
                                                                  float4* __restrict__ out_b)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i < na) store_record<kStep>(out_a, i, a[i], EgressOffsets{});
    else if (i - na < nb) store_record<kStep>(out_b, i - na, b[i - na], EgressOffsets{});
}
// pcl::transformPointCloud(*cloud, *aligned, odom) and pcl::toROSMsg(*aligned, ...) in one pass (apps/scan_matching_odometry_component.cpp:341-347,
// mrgfe_odom_frame_records): transform_cloud_kernel's body (scan_point.h) feeding the record store, so the bits are those of the two launches
struct RecordTransform { float m[12]; };
template <int kStep>
__global__ __launch_bounds__(256) void transform_records_kernel(const float4* __restrict__ in, uint32_t n, RecordTransform T, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    store_record<kStep>(out, i, transform_finite_point(T.m, in[i]), EgressOffsets{});
}
// ---- prefiltering/colored_points (apps/prefiltering_component.cpp:239-257, mrgfe_scan_callback_outputs) -----------------------------------------------------
// The raw scan as the records of pcl::toROSMsg(*colored, ...): point i of the wire records, read as the scan head kernel reads it (load_point_record_as,
// kBytes chosen by the same rule), before deskewing, transform and filters.  [UPSTREAM-RECALL] pcl::PointXYZRGB in memory, 32 bytes, which toROSMsg copies
// as it is (fields x@0 y@4 z@8 rgb@16): x y z 1.0f | b g r a | 12 zero bytes — `colored->resize` leaves data[3] = 1 and a = 255, getVector4fMap copies
// the PointXYZI's own 1.0f (:249).  t = (double)i / n, r = 255 * t and b = 255 * (1 - t) converted to uint8_t (:248-252): f64, a real division, truncated;
// 255 * t < 255 and 255 * (1 - t) <= 255, so the conversion never wraps.  No arithmetic touches x, y, z: a NaN's payload survives.
struct ColoredArgs {
    const uint8_t* raw;
    float4*        out;  // room for n records of 32 bytes
    uint32_t       n, width, row_step, point_step, ox, oy, oz;
};
template <bool kBytes>
__global__ __launch_bounds__(256) void colored_records_kernel(const ColoredArgs a)
{
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const float4   p = load_point_record_as<kBytes>(a.raw, i, a.width, a.row_step, a.point_step, a.ox, a.oy, a.oz, -1);
    const double   t = static_cast<double>(i) / static_cast<double>(a.n);
    const uint32_t r = static_cast<uint32_t>(255.0 * t), b = static_cast<uint32_t>(255.0 * (1.0 - t));
    a.out[2 * size_t(i)] = make_float4(p.x, p.y, p.z, 1.0f);
    a.out[2 * size_t(i) + 1] = make_float4(__uint_as_float(b | (128u << 8) | (r << 16) | (255u << 24)), 0.0f, 0.0f, 0.0f);
}
// ---- StatisticalOutlierRemoval's threshold without a host round trip (sor_threshold.h) --------------------------------------------------------------
// The reference's two f64 sums are sequential over the points; a dependent chain of n additions on one lane would cost as much as the rest of the chain.
// They are added in a tree instead — per thread, per wavefront, per tile of 2048 points, over the tiles — together with the minimum lowest-bit exponent
// of the terms of either sum; sor::certified then says whether the order could have mattered.  When it could (it does not on scans: q is -24 .. -34 and
// the sums stay below 2^17 where 2^(q + 52) is 2^18 at the least), the finish sets kPfAnomalyCertificate and the host-driven passes add in the
// reference's order.
struct SorPartial {
    double   sum, sq_sum;
    uint32_t valid;
    int32_t  q_sum, q_sq;
    uint32_t pad;
};
__device__ __forceinline__ SorPartial sor_partial_zero()
{
    SorPartial a;
    a.sum = 0.0; a.sq_sum = 0.0; a.valid = 0u; a.q_sum = sor::kNoTerm; a.q_sq = sor::kNoTerm; a.pad = 0u;
    return a;
}
__device__ __forceinline__ void sor_partial_add(SorPartial& a, double sum, double sq_sum, uint32_t valid, int32_t q_sum, int32_t q_sq)
{
    a.sum += sum; a.sq_sum += sq_sum; a.valid += valid;
    a.q_sum = sor::min_exponent(a.q_sum, q_sum);
    a.q_sq = sor::min_exponent(a.q_sq, q_sq);
}
// the 256 threads' partials in a fixed tree (lane i + lane i + off for off = 32 .. 1, then the four wavefronts); the result is valid in thread 0
__device__ __forceinline__ SorPartial sor_block_merge(SorPartial a, SorPartial* lds)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
        sor_partial_add(a, __shfl_down(a.sum, off, kWave), __shfl_down(a.sq_sum, off, kWave), __shfl_down(a.valid, off, kWave), __shfl_down(a.q_sum, off, kWave),
                        __shfl_down(a.q_sq, off, kWave));
    if (lane_id() == 0) lds[wave_id()] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        SorPartial lo = lds[0], hi = lds[2];
        sor_partial_add(lo, lds[1].sum, lds[1].sq_sum, lds[1].valid, lds[1].q_sum, lds[1].q_sq);
        sor_partial_add(hi, lds[3].sum, lds[3].sq_sum, lds[3].valid, lds[3].q_sum, lds[3].q_sq);
        sor_partial_add(lo, hi.sum, hi.sq_sum, hi.valid, hi.q_sum, hi.q_sq);
        a = lo;
    }
    return a;
}
// one workgroup per tile of 2048 of the first *n_ptr distances; part[tile] = the tile's sums
__global__ __launch_bounds__(256) void sor_reduce_tiles_kernel(const float* __restrict__ dist, const uint32_t* __restrict__ valid, const uint32_t* __restrict__ n_ptr,
                                                                SorPartial* __restrict__ part)
{
    const uint32_t n = *n_ptr, base = blockIdx.x * kTile;
    if (base >= n) return;  // uniform
    __shared__ SorPartial lds[4];
    SorPartial a = sor_partial_zero();
#pragma unroll
    for (int k = 0; k < kTile / 256; ++k) {
        const uint32_t i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const float d = dist[i], d2 = sor::square_term(d);
            sor_partial_add(a, static_cast<double>(d), static_cast<double>(d2), valid[i], sor::low_bit_exponent(d), sor::low_bit_exponent(d2));
        }
    }
    a = sor_block_merge(a, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
// one workgroup: the tiles' sums in a tree, then ONE thread certifies them and evaluates the threshold — into *out (device memory: sor_flags_dd_kernel
// reads the threshold there), into the host's pinned record, and a failed certificate into the chain's anomaly word
__global__ __launch_bounds__(256) void sor_finish_kernel(const SorPartial* __restrict__ part, const uint32_t* __restrict__ n_ptr, double stddev_mul, sor::Result* __restrict__ out,
                                                          sor::Result* __restrict__ h_out, uint32_t* __restrict__ anomaly)
{
    const uint32_t n = *n_ptr, nblk = (n + kTile - 1) / kTile;
    __shared__ SorPartial lds[4];
    SorPartial a = sor_partial_zero();
    for (uint32_t b = threadIdx.x; b < nblk; b += 256) {
        const SorPartial t = part[b];
        sor_partial_add(a, t.sum, t.sq_sum, t.valid, t.q_sum, t.q_sq);
    }
    uint64_t valid = a.valid;  // (the tiles' counts fit 32 bits, their total need not in the diagnostic's arrays)
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) valid += __shfl_down(valid, off, kWave);
    __shared__ uint64_t s_valid[4];
    if (lane_id() == 0) s_valid[wave_id()] = valid;
    a = sor_block_merge(a, lds);  // (synchronises)
    if (threadIdx.x) return;
    sor::Result r;
    r.sum = a.sum;
    r.sq_sum = a.sq_sum;
    r.valid = (s_valid[0] + s_valid[1]) + (s_valid[2] + s_valid[3]);
    r.q_sum = a.q_sum;
    r.q_sq = a.q_sq;
    r.thr = sor::threshold(r.sum, r.sq_sum, r.valid, stddev_mul);
    r.certified = (sor::certified(r.sum, r.q_sum) && sor::certified(r.sq_sum, r.q_sq)) ? 1u : 0u;
    r.pad = 0u;
    *out = r;
    if (h_out) *h_out = r;  // (pinned host memory: read behind the caller's stream wait)
    if (anomaly && !r.certified) *anomaly |= kPfAnomalyCertificate;
}
// sor_flags_kernel with the count and the threshold read from device memory
__global__ __launch_bounds__(256) void sor_flags_dd_kernel(const float* __restrict__ dist, const uint32_t* __restrict__ n_ptr, const double* __restrict__ thr, uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < *n_ptr) flags[i] = (static_cast<double>(dist[i]) > *thr) ? 0u : 1u;
}
// enqueue the reduction and the finish over the first *d_n of d_dist / d_valid (n_cap >= *d_n sizes the launch); d_part: n_cap / 2048 + 1 partials
static int sor_threshold_launch(mrgfe_ctx* ctx, const float* d_dist, const uint32_t* d_valid, const uint32_t* d_n, uint32_t n_cap, double stddev_mul, SorPartial* d_part,
                                sor::Result* d_out, sor::Result* h_out, uint32_t* d_anomaly)
{
    const uint32_t tiles = (n_cap + kTile - 1) / kTile;
    if (tiles) hipLaunchKernelGGL(sor_reduce_tiles_kernel, dim3(tiles), dim3(256), 0, ctx->stream, d_dist, d_valid, d_n, d_part);
    hipLaunchKernelGGL(sor_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, d_part, d_n, stddev_mul, d_out, h_out, d_anomaly);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// mrgfe_dbg_sor_threshold: out = sum, sq_sum, valid, thr, certified, q of the `sum` terms — from the reference's sequential loop on the host, or from the
// chain's own reduction and finish kernels over the uploaded arrays
int sor_threshold_debug(mrgfe_ctx* ctx, const float* dist, const uint32_t* valid, size_t n, double stddev_mul, int on_device, double out[6])
{
    sor::Result r;
    if (!on_device) {
        r = sor::sequential(dist, valid, n, stddev_mul);
    } else {
        if (n > 0x7fffffffu) { set_error("mrgfe_dbg_sor_threshold: too many values"); return MRGFE_ERR_INVALID; }
        const uint32_t nn = static_cast<uint32_t>(n);
        DevBuf dres, dpart, din;  // (per-call buffers of a diagnostic, freed at the return)
        MRGFE_TRY(din.ensure(std::max<size_t>(n, 1) * 8));
        MRGFE_TRY(dpart.ensure(sizeof(SorPartial) * (size_t(nn) / kTile + 2)));
        MRGFE_TRY(dres.ensure(sizeof(sor::Result) + 8));
        float*    d_dist = din.as<float>();
        uint32_t* d_valid = reinterpret_cast<uint32_t*>(d_dist + std::max<size_t>(n, 1));
        uint32_t* d_n = reinterpret_cast<uint32_t*>(dres.as<char>() + sizeof(sor::Result));
        if (n) {
            MRGFE_HIP_CHECK(hipMemcpyAsync(d_dist, dist, n * 4, hipMemcpyHostToDevice, ctx->stream));
            MRGFE_HIP_CHECK(hipMemcpyAsync(d_valid, valid, n * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        MRGFE_HIP_CHECK(hipMemcpyAsync(d_n, &nn, 4, hipMemcpyHostToDevice, ctx->stream));
        MRGFE_TRY(sor_threshold_launch(ctx, d_dist, d_valid, d_n, nn, stddev_mul, dpart.as<SorPartial>(), dres.as<sor::Result>(), nullptr, nullptr));
        MRGFE_HIP_CHECK(hipMemcpyAsync(&r, dres.p, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
        MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    out[0] = r.sum; out[1] = r.sq_sum; out[2] = static_cast<double>(r.valid); out[3] = r.thr; out[4] = static_cast<double>(r.certified);
    out[5] = static_cast<double>(r.q_sum);
    return MRGFE_OK;
}

// 1 (default): the usual chain keeps its counts on the device; 0: always the host-driven chain of round 3 (MRGFE_PREFILTER_HOST_DRIVEN=1, tests)
static std::atomic<int> g_pf_device_driven{-1};
static int prefilter_device_driven_mode()
{
    int v = g_pf_device_driven.load(std::memory_order_relaxed);
    if (v < 0) { v = std::getenv("MRGFE_PREFILTER_HOST_DRIVEN") ? 0 : 1; g_pf_device_driven.store(v, std::memory_order_relaxed); }
    return v;
}
int prefilter_set_device_driven(int mode)
{
    if (mode == 0 || mode == 1) g_pf_device_driven.store(mode, std::memory_order_relaxed);
    return prefilter_device_driven_mode();
}

static NnDeviceDrivenGrid& pf_grid(mrgfe_ctx* ctx)
{
    if (!ctx->pf_grid) ctx->pf_grid.reset(new NnDeviceDrivenGrid());
    return *ctx->pf_grid;
}

// The chains the device-driven form serves (the others, and its anomalies, go through the host-driven passes): every [distance] -> downsample ->
// outlier chain the parameters express, except — unless the context has mrgfe_ctx_set_wide_statistical_chains on — mean_k beyond one list entry per lane
// (64..255: nn_knn_mean_dd_wide_kernel<R>) and — unless it has mrgfe_ctx_set_statistical_chains on — the
// statistical filter behind anything but a VoxelGrid: without a leaf there is no rule for the k-NN grid's cell edge that the host could know
// (sor_cell_edge), so with the switch on the device chooses the edge itself (nn_build_device_sized, sor_sized_grid).
static int  chain_downsample(const PrefilterChain& ch) { return ch.approx_voxelgrid ? 2 : (ch.voxelgrid ? 1 : 0); }
static bool sor_sized_grid(const mrgfe_ctx* ctx, const PrefilterChain& ch)
{
    return ch.outlier == 2 && chain_downsample(ch) != 1 && ctx->statistical_chains.load(std::memory_order_relaxed);
}
static bool device_driven_applies(const mrgfe_ctx* ctx, const PrefilterChain& ch, uint32_t n)
{
    if (!prefilter_device_driven_mode() || n == 0) return false;
    const int down = chain_downsample(ch);
    if (down != 0 && !(ch.leaf > 0)) return false;
    if (ch.outlier == 2) {  // (mean_k + 1 entries must fit a wavefront's list: one per lane, or up to four with the wide switch)
        const int most = ctx->wide_statistical_chains.load(std::memory_order_relaxed) ? 255 : 63;
        return (down == 1 || sor_sized_grid(ctx, ch)) && ch.mean_k >= 1 && ch.mean_k <= most;
    }
    return true;
}

// The cell edge of the statistical filter's k-NN grid.  Search results do not depend on it, only the time does, and the host cannot run NnGrid::build's
// adaptive halving (which counts the points per cell) without a wait — so the edge comes from what the host knows: the voxel grid that made the cloud
// leaves at most one centroid per leaf^3, a scan's surfaces therefore at most (edge / leaf)^2 per cell.  EIGHT leaves, measured (MI355X, leaf 0.1, k = 20
// and 30; profiles/prefilter_statistical_summary.md): the search is ONE level, so what sets its time is the sparse far rings of a scan, whose queries
// walk ring after ring of small cells — at 4 leaves the k-NN launch of a 26k-point VLP-16 scan took 0.14 - 0.17 ms, at 8 leaves 0.05 - 0.06 ms, while the
// denser 130k-point VLP-64 scan is flat from 4 to 10 leaves (0.07 - 0.10 ms) and loses from 16 on (0.12 - 0.15 ms: hundreds of candidates per cell).
// Never below 0.2 m: a leaf of a few centimetres must not cost a table of 10^8 cells.  A cloud whose box needs more than kSorCellsCap cells at this edge
// sets kNnAnomalyCells and is handed back; 8^3 leaves per cell and 2^24 cells put that beyond PCL's own limit of 2^31 leaves for every leaf >= 0.025 m.
// A second, coarser level for the far rings was not tried.
// mean_k 64..255 (mrgfe_ctx_set_wide_statistical_chains) keeps both rules, this one and the device-sized grid's below.  Behind the voxel grid no other
// number of leaves was measured for them: at eight the wide launch takes 0.09 / 0.12 / 0.39 ms (mean_k 64 / 100 / 255) on the VLP-16 scan's centroids
// and 0.15 / 0.18 / 0.44 ms on the VLP-64 scan's, 0.3 to 0.6 of the whole call.  Without a leaf the other rules were measured
// (profiles/prefilter_statistical_wide_summary.md, k-NN launch ms at mean_k 64 / 100 / 255): the VLP-16 scan at the 1 m the target of 128 keeps
// 0.14 / 0.17 / 0.39, at 0.5 m 0.16 / 0.22 / 0.61, at 2 m 0.19 / 0.22 / 0.49; the VLP-64 scan at the 0.25 m it is halved to 0.56 / 0.70 / 1.74, at
// 0.5 m (targets 256 and 512) 1.09 / 1.25 / 2.59, at 1 m (1024) 2.11 / 2.33 / 4.41 — four times the neighbours do not ask for larger cells: a cell of
// the default rule holds ~100 points of the VLP-16 scan, and the dense scan pays for every candidate it measures.  Edges below 0.25 m were not tried.
constexpr uint32_t kSorCellsCap = (1u << 24) - 1u;  // 24 key bits: three radix passes, as for the radius filter's 2^22 cells
#ifndef MRGFE_SOR_CELL_LEAVES
#define MRGFE_SOR_CELL_LEAVES 8.0f
#endif
static float sor_cell_edge(const PrefilterChain& ch) { return std::max(MRGFE_SOR_CELL_LEAVES * ch.leaf, 0.2f); }
// Without a VoxelGrid in front (downsample NONE or APPROX_VOXELGRID, context switch on) the device sizes the grid: NnGrid::build's halving rule from a start
// edge, in MRGFE_SOR_GRID_PASSES counting passes (nn_build_device_sized).  The defaults are measured (MI355X, raw 26k-point VLP-16 and 130k-point VLP-64
// scans, k = 20 and 30; profiles/prefilter_chains_summary.md).  The search is ONE level, so — as behind the voxel grid — the sparse far rings favour
// larger cells than NnGrid's pyramid does: at the host route's target of 32 (NnGrid::kCrowdingKnn) the device halved the VLP-16 scan to 0.25 m and its
// k-NN launch took 0.45 ms, at 128 it keeps 1 m and takes 0.08 ms; the VLP-64 scan goes to 0.25 m (0.31 ms; 0.43 ms at 0.125 m, 0.70 ms at 0.5 m) and its
// APPROX_VOXELGRID(0.1) centroids to 0.5 m.  A target of 64 still halves the VLP-64 scan once too often.  ONE counting pass: a second and a third chose the
// same edges on both scans and cost 6 - 27 us per call each (a clear, a count and a decision).  Start edge 1 m as on the host route: 2 m costs a halving more.
#ifndef MRGFE_SOR_GRID_START_EDGE
#define MRGFE_SOR_GRID_START_EDGE 1.0f
#endif
#ifndef MRGFE_SOR_GRID_CROWDING
#define MRGFE_SOR_GRID_CROWDING 128.0
#endif
#ifndef MRGFE_SOR_GRID_MAX_HALVINGS
#define MRGFE_SOR_GRID_MAX_HALVINGS 4
#endif
#ifndef MRGFE_SOR_GRID_PASSES
#define MRGFE_SOR_GRID_PASSES 1
#endif
static_assert(MRGFE_SOR_GRID_PASSES >= 1 && MRGFE_SOR_GRID_PASSES <= 3, "one to three counting passes");
// mrgfe_dbg_set_sor_grid_rule: the tests' overrides (0 = the default)
static std::atomic<float>  g_sor_start_edge{0.0f};
static std::atomic<double> g_sor_crowding{0.0};
static std::atomic<int>    g_sor_max_halvings{-1};
void prefilter_set_sor_grid_rule(float start_edge, double crowding_target, int max_halvings)
{
    const bool all_default = !(start_edge > 0.0f) && !(crowding_target > 0.0) && max_halvings == 0;
    g_sor_start_edge.store(start_edge > 0.0f ? start_edge : 0.0f);
    g_sor_crowding.store(crowding_target > 0.0 ? crowding_target : 0.0);
    g_sor_max_halvings.store(all_default ? -1 : std::max(max_halvings, 0));
}

// ---- where a call's records go (RecordSink, filters.h) ----------------------------------------------------------------------------------------------
// a sink resolved for one call: the record kernel's destination as the device sees it
struct RecordDest {
    const RecordSink* sink = nullptr;
    float4*           d_dst = nullptr;
    bool              direct = false;  // d_dst is the caller's buffer
    bool              second = false;  // the call's second sink: staged through rec_pin2, counted in eg2_stats
};
static PinBuf&          dest_pin(mrgfe_ctx* ctx, const RecordDest& d) { return d.second ? ctx->rec_pin2 : ctx->rec_pin; }
static ScanEgressStats& dest_stats(mrgfe_ctx* ctx, const RecordDest& d) { return d.second ? ctx->eg2_stats : ctx->eg_stats; }
static bool page_locked(const void* p)
{
    hipPointerAttribute_t a;
    return hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
}
static void egress_begin(mrgfe_ctx* ctx)
{
    ScanEgressStats& e = ctx->eg_stats;
    e.direct = e.launches = e.waits = e.bytes = e.copied = 0;
    e.calls += 1;
    ScanEgressStats& e2 = ctx->eg2_stats;  // (a call without a second sink reports none)
    e2.direct = e2.launches = e2.waits = e2.bytes = e2.copied = 0;
}
// a call's second sink, where it has one (behind egress_begin when the call has a first one too)
static void egress_second_begin(mrgfe_ctx* ctx)
{
    ScanEgressStats& e = ctx->eg2_stats;
    e.direct = e.launches = e.waits = e.bytes = e.copied = 0;
    e.calls += 1;
}
// n_in: the points the record kernel may write at the most.  allow_direct false: the context's pinned buffer whatever the caller's memory is.
static int record_dest_open(mrgfe_ctx* ctx, const RecordSink& s, size_t n_in, bool allow_direct, RecordDest* d, bool second = false)
{
    d->sink = &s;
    d->d_dst = nullptr;
    d->direct = false;
    d->second = second;
    char* first = static_cast<char*>(s.records);
    if (allow_direct && s.capacity && (reinterpret_cast<uintptr_t>(first) & 15u) == 0) {
        // BOTH ends of the range in page-locked memory, as upload_cloud asks of a cloud it reads in place
        void* dev = nullptr;
        if (page_locked(first) && page_locked(first + s.capacity - 1) && hipHostGetDevicePointer(&dev, s.records, 0) == hipSuccess && dev) {
            d->d_dst = static_cast<float4*>(dev);
            d->direct = true;
        }
        (void)hipGetLastError();  // (an unregistered pointer is an error to the query, not to us)
    }
    if (!d->direct) {
        PinBuf& pin = dest_pin(ctx, *d);
        MRGFE_TRY(pin.ensure(n_in * size_t(s.point_step)));
        d->d_dst = pin.as<float4>();
    }
    dest_stats(ctx, *d).direct = d->direct ? 1 : 0;
    return MRGFE_OK;
}
// behind the wait that covers the record kernel: the m records are in the destination; a staged destination is copied out
static void record_dest_close(mrgfe_ctx* ctx, const RecordDest& d, size_t m)
{
    const size_t     bytes = m * size_t(d.sink->point_step);
    ScanEgressStats& e = dest_stats(ctx, d);
    if (!d.direct && bytes) {
        std::memcpy(d.sink->records, dest_pin(ctx, d).p, bytes);
        e.copied = static_cast<int64_t>(bytes);
    }
    e.bytes = static_cast<int64_t>(bytes);
}
// the m packed points at d_in as records, the count known to the host: one launch, queued
static int launch_cloud_records(mrgfe_ctx* ctx, const float4* d_in, uint32_t m, const RecordDest& d)
{
    if (m == 0) return MRGFE_OK;
    const auto kern = d.sink->point_step == 16 ? cloud_records_kernel<16> : cloud_records_kernel<32>;
    hipLaunchKernelGGL(kern, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_in, m, d.d_dst);
    MRGFE_HIP_CHECK(hipGetLastError());
    ctx->eg_stats.launches += 1;
    return MRGFE_OK;
}
int cloud_records_device(mrgfe_ctx* ctx, const float4* d_xyzi, size_t n, const RecordSink& rec)
{
    egress_begin(ctx);
    if (n == 0) return MRGFE_OK;
    RecordDest d;
    MRGFE_TRY(record_dest_open(ctx, rec, n, true, &d));
    MRGFE_TRY(launch_cloud_records(ctx, d_xyzi, static_cast<uint32_t>(n), d));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->eg_stats.waits += 1;
    record_dest_close(ctx, d, n);
    return MRGFE_OK;
}
int transformed_records_device(mrgfe_ctx* ctx, const float4* d_xyzi, size_t n, const float T_rowmajor[16], const RecordSink& rec)
{
    egress_begin(ctx);
    if (n == 0) return MRGFE_OK;
    RecordDest d;
    MRGFE_TRY(record_dest_open(ctx, rec, n, true, &d));
    RecordTransform T;
    std::memcpy(T.m, T_rowmajor, sizeof(T.m));
    const uint32_t nn = static_cast<uint32_t>(n);
    hipLaunchKernelGGL(rec.point_step == 16 ? transform_records_kernel<16> : transform_records_kernel<32>, dim3((nn + 255) / 256), dim3(256), 0, ctx->stream, d_xyzi, nn, T, d.d_dst);
    MRGFE_HIP_CHECK(hipGetLastError());
    ctx->eg_stats.launches += 1;
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->eg_stats.waits += 1;
    record_dest_close(ctx, d, n);
    return MRGFE_OK;
}
int cloud_pair_records_device(mrgfe_ctx* ctx, const float4* d_first, size_t n_first, const RecordSink* first, const float4* d_second, size_t n_second, const RecordSink* second)
{
    egress_begin(ctx);
    if (second) egress_second_begin(ctx);
    const uint32_t na = first ? static_cast<uint32_t>(n_first) : 0u, nb = second ? static_cast<uint32_t>(n_second) : 0u;
    if (size_t(na) + nb == 0) return MRGFE_OK;
    RecordDest da, db;
    if (na) MRGFE_TRY(record_dest_open(ctx, *first, na, true, &da));
    if (nb) MRGFE_TRY(record_dest_open(ctx, *second, nb, true, &db, true));
    const int  step = na ? first->point_step : second->point_step;
    const auto kern = step == 16 ? cloud_pair_records_kernel<16> : cloud_pair_records_kernel<32>;
    const uint32_t blocks = static_cast<uint32_t>((uint64_t(na) + nb + 255) / 256);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, ctx->stream, d_first, na, da.d_dst, d_second, nb, db.d_dst);
    MRGFE_HIP_CHECK(hipGetLastError());
    if (na) ctx->eg_stats.launches += 1;
    if (nb) ctx->eg2_stats.launches += 1;  // (the one launch serves both sinks)
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (na) ctx->eg_stats.waits += 1;
    else ctx->eg2_stats.waits += 1;  // (the second sink adds a wait only where it is alone)
    if (na) record_dest_close(ctx, da, na);
    if (nb) record_dest_close(ctx, db, nb);
    return MRGFE_OK;
}
// the coloured records of a scan whose wire records are at d_raw: one launch, queued
static int launch_colored_records(mrgfe_ctx* ctx, const ScanHead& h, const void* d_raw, const RecordDest& d)
{
    ColoredArgs a;
    std::memset(&a, 0, sizeof(a));
    a.raw = static_cast<const uint8_t*>(d_raw);
    a.out = d.d_dst;
    a.n = h.width * h.height;
    a.width = h.width; a.row_step = h.row_step; a.point_step = h.point_step;
    a.ox = h.off_x; a.oy = h.off_y; a.oz = h.off_z;
    const bool strict = layout_is_strict(h.point_step, h.row_step, h.off_x, h.off_y, h.off_z, h.off_intensity);  // (the head kernel's choice)
    hipLaunchKernelGGL(strict ? colored_records_kernel<false> : colored_records_kernel<true>, dim3((a.n + 255) / 256), dim3(256), 0, ctx->stream, a);
    MRGFE_HIP_CHECK(hipGetLastError());
    ctx->eg2_stats.launches += 1;
    return MRGFE_OK;
}
static size_t scan_raw_bytes(const ScanHead& h) { return size_t(h.height - 1) * h.row_step + size_t(h.width) * h.point_step; }
int scan_colored_records(mrgfe_ctx* ctx, const ScanHead& head, const RecordSink& colored)
{
    egress_second_begin(ctx);
    const size_t n = size_t(head.width) * head.height;
    if (n == 0) return MRGFE_OK;
    if (n > 0x7fffffffu) { set_error("scan callback: cloud too large"); return MRGFE_ERR_INVALID; }
    RecordDest  d;
    const void* d_raw = nullptr;
    MRGFE_TRY(record_dest_open(ctx, colored, n, true, &d, true));
    MRGFE_TRY(upload_raw_records(ctx, head.data, scan_raw_bytes(head), &d_raw));
    MRGFE_TRY(launch_colored_records(ctx, head, d_raw, d));
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->eg2_stats.waits += 1;
    record_dest_close(ctx, d, n);
    return MRGFE_OK;
}

// ---- the chain as three stages ----------------------------------------------------------------------------------------------------------------------
// head / distance -> downsample (NONE, VOXELGRID, APPROX_VOXELGRID) -> outlier (NONE, RADIUS, STATISTICAL).  A stage hands the next one its live count
// (PfState::sl_in, then sl_rad), its cloud (cp[0], then cp[1]) and one box per tile of that cloud (bb_n[0], then bb_n[1] entries) — nothing through the
// host.  The last stage writes the pinned status record; pf_run_stages waits once behind it.
// Buffers: three besides the scratch slots — the packed input, the work buffer the caller gets the result in, and a third one.  Each stage writes where
// its reader expects it (s1_out: the downsample stage's input; s2_out: the outlier stage's input, the work buffer itself when no outlier filter follows).
struct PfRun {
    mrgfe_ctx*            ctx;
    const PrefilterChain* ch;
    int                   down;  // chain_downsample
    uint32_t              n;     // points of the input: every launch is sized for it
    SliceTable            tab;
    PfState*              d_st;
    uint32_t*             h_status;
    BBox*                 h_box;
    BBox*                 d_part;      // scratch for the per-tile boxes
    const BBox*           boxes_in;    // the boxes of the downsample stage's input: d_part, or the ones the caller's own head kernel left
    uint32_t*             d_blk;
    const float4*         s1_out;
    float4 *              s2_out, *d_work;
    dim3                  g256, gtiles;
};
// what the host reads behind the wait
struct PfReport {
    uint32_t counts[5];
    uint32_t anomaly;
    BBox     box;  // of the outlier stage's input, or (no outlier filter) of the output
};

// Stage 1.  The packed input is in d_in already, or — `head` and its uploaded records `d_raw` — the scan head kernel writes it there as the chain's first
// launch; `d_head_boxes`: the caller's own head kernel has left one box per tile of d_in (the odometry frame), no distance filter.
static int pf_stage_head(PfRun& r, const ScanHead* head, const void* d_raw, float4* d_in, const BBox* d_head_boxes)
{
    mrgfe_ctx*            ctx = r.ctx;
    const PrefilterChain& ch = *r.ch;
    hipStream_t           st = ctx->stream;
    const dim3            b256(256);
    uint32_t*             d_flags = ctx->scratch[7].as<uint32_t>();
    float4*               dist_out = const_cast<float4*>(r.s1_out);
    if (head) {  // (with the distance filter on, the head is pf_distance_tiles_kernel too)
        const ScanHeadFlags fl{ch.near_t, ch.far_t, d_flags, r.d_blk, r.d_st, r.s1_out, r.s2_out};
        MRGFE_TRY(launch_scan_head(ctx, *head, d_raw, d_in, ch.distance ? &fl : nullptr));
    }
    r.boxes_in = r.d_part;
    if (ch.distance) {
        // flags + tile counts (and the state's first values), compaction with the count and the kept points' boxes
        if (!head) hipLaunchKernelGGL(pf_distance_tiles_kernel, r.gtiles, b256, 0, st, d_in, r.n, ch.near_t, ch.far_t, d_flags, r.d_blk, r.d_st, r.s1_out, r.s2_out);
        hipLaunchKernelGGL(pf_compact_kernel<0>, r.gtiles, b256, 0, st, d_in, d_flags, r.d_blk, r.n, dist_out, r.d_st, r.h_status, r.d_part);
    } else {
        if (r.s1_out != d_in) MRGFE_HIP_CHECK(hipMemcpyAsync(dist_out, d_in, size_t(r.n) * 16, hipMemcpyDeviceToDevice, st));  // (no stage at all: the output is the input)
        hipLaunchKernelGGL(pf_init_kernel, dim3(1), dim3(1), 0, st, r.d_st, r.s1_out, r.s2_out, r.n);
        if (d_head_boxes) r.boxes_in = d_head_boxes;
        else MRGFE_TRY(bounding_box_partials(ctx, &r.d_st->cp[0], &r.d_st->sl_in, r.tab, r.d_part));
    }
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// Stage 2: sl_in points at cp[0] -> sl_rad points at cp[1] with bb_n[1] boxes in d_part
static int pf_stage_downsample(PfRun& r)
{
    mrgfe_ctx*            ctx = r.ctx;
    const PrefilterChain& ch = *r.ch;
    hipStream_t           st = ctx->stream;
    const dim3            b256(256);
    const uint32_t        n = r.n;
    PfState*              d_st = r.d_st;
    DevBuf &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6], &dseg = ctx->scratch[9], &dcent = ctx->scratch[10],
           &dkeep = ctx->scratch[11];
    uint32_t *sk, *sv;
    if (r.down == 0) {
        hipLaunchKernelGGL(pf_no_downsample_kernel, dim3(1), b256, 0, st, d_st, r.boxes_in, ch.outlier != 0 ? 1 : 0);
    } else if (r.down == 1) {
        // VoxelGrid: voxel parameters from the boxes (device), keys, stable sort (32 key bits: the host does not know the cell count), runs, centroids
        hipLaunchKernelGGL(pf_voxel_params_kernel, dim3(1), b256, 0, st, d_st, r.boxes_in, ch.leaf);
        MRGFE_TRY(ndt_launch_cellkeys(ctx, &d_st->cp[0], &d_st->sl_in, r.tab, &d_st->vp, dk.as<uint32_t>(), dh.as<uint32_t>()));
        MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), &d_st->sl_in, r.tab, 32, dh.as<uint32_t>(), &sk, &sv, true, true));
        MRGFE_TRY(run_head_tile_counts(ctx, sk, &d_st->sl_in, r.tab, &d_st->nv, r.d_blk));
        hipLaunchKernelGGL(pf_leaves_kernel, dim3(1), b256, 0, st, d_st, r.d_blk);
        uint32_t* d_seg = dseg.as<uint32_t>();
        int32_t*  d_segkey = reinterpret_cast<int32_t*>(d_seg + size_t(n) + 4);
        MRGFE_TRY(ndt_launch_segments(ctx, sk, &d_st->sl_in, r.tab, &d_st->nv, r.d_blk, &d_st->ls, d_seg, d_segkey));
        hipLaunchKernelGGL(voxel_centroid_dd_kernel, r.g256, b256, 0, st, r.s1_out, sv, d_seg, &d_st->sl_vox, ch.min_pts, dcent.as<float4>(), dkeep.as<uint32_t>());
        MRGFE_TRY(tile_sums(ctx, dkeep.as<uint32_t>(), &d_st->sl_vox, r.tab, r.d_blk));
        hipLaunchKernelGGL(pf_compact_kernel<1>, r.gtiles, b256, 0, st, dcent.as<float4>(), dkeep.as<uint32_t>(), r.d_blk, 0u, r.s2_out, d_st, r.h_status, r.d_part);
    } else {
        // ApproximateVoxelGrid (filter_approx_voxelgrid_device's passes over the live count): entry keys, 9-bit stable sort, stretch heads and flushing
        // points, their two scans, the entry ranks, one centroid per stretch at its place in the sequential loop's output
        DevBuf &dhead = ctx->scratch[7], &dfpos = dcent, &dflush = dkeep, &dord = ctx->scratch[12], &drank = ctx->scratch[14];
        const Slice* sl = &d_st->sl_in;
        const float  inv = 1.0f / ch.leaf;  // inverse_leaf_size_ = Array3f::Ones() / leaf_size_
        uint32_t*    d_tot = r.d_blk + r.tab.total_blks;  // [0] stretches, [1] flushing points
        hipLaunchKernelGGL(avg_keys_dd_kernel, r.g256, b256, 0, st, r.s1_out, sl, inv, dk.as<uint32_t>());
        MRGFE_TRY(radix_sort_pairs(ctx, dk.as<uint32_t>(), dv.as<uint32_t>(), dkt.as<uint32_t>(), dvt.as<uint32_t>(), sl, r.tab, 9, dh.as<uint32_t>(), &sk, &sv, true));
        MRGFE_HIP_CHECK(hipMemsetAsync(dflush.p, 0, size_t(n) * 4, st));
        hipLaunchKernelGGL(avg_heads_dd_kernel, r.g256, b256, 0, st, r.s1_out, sk, sv, sl, inv, dhead.as<uint32_t>(), dflush.as<uint32_t>());
        MRGFE_TRY(exclusive_scan(ctx, dhead.as<uint32_t>(), dord.as<uint32_t>(), sl, r.tab, r.d_blk, d_tot));
        hipLaunchKernelGGL(avg_segments_dd_kernel, r.g256, b256, 0, st, dhead.as<uint32_t>(), dord.as<uint32_t>(), sl, d_tot, dseg.as<uint32_t>());
        MRGFE_TRY(exclusive_scan(ctx, dflush.as<uint32_t>(), dfpos.as<uint32_t>(), sl, r.tab, r.d_blk, d_tot + 1));
        hipLaunchKernelGGL(avg_entry_ranks_dd_kernel, dim3(1), dim3(512), 0, st, sk, sl, drank.as<uint32_t>());
        hipLaunchKernelGGL(avg_emit_dd_kernel, r.g256, b256, 0, st, r.s1_out, sk, sv, sl, dseg.as<uint32_t>(), d_tot, dfpos.as<uint32_t>(), drank.as<uint32_t>(), r.s2_out);
        hipLaunchKernelGGL(pf_approx_done_kernel, dim3(1), b256, 0, st, d_st, r.boxes_in, d_tot);
        MRGFE_TRY(bounding_box_partials(ctx, &d_st->cp[1], &d_st->sl_rad, r.tab, r.d_part));
        if (ch.outlier != 0) hipLaunchKernelGGL(pf_finite_check_kernel, dim3(1), b256, 0, st, d_st, r.d_part);
    }
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// Stage 3: the outlier filter over sl_rad points at s2_out into the work buffer, or the finish of a chain without one; either writes the status record
static int pf_stage_outlier(PfRun& r)
{
    mrgfe_ctx*            ctx = r.ctx;
    const PrefilterChain& ch = *r.ch;
    hipStream_t           st = ctx->stream;
    const dim3            b256(256);
    const uint32_t        n = r.n;
    PfState*              d_st = r.d_st;
    if (ch.outlier == 0) {
        hipLaunchKernelGGL(pf_finish_kernel, dim3(1), b256, 0, st, d_st, r.d_part, r.h_status, r.h_box);
        MRGFE_HIP_CHECK(hipGetLastError());
        return MRGFE_OK;
    }
    // a grid that sizes itself (from the boxes of the stage's input), flags, compaction
    NnDeviceDrivenGrid& grid = pf_grid(ctx);
    uint32_t*           d_flags = ctx->scratch[7].as<uint32_t>();
    if (ch.outlier == 1) {
        // RadiusOutlierRemoval: inlier iff #{q: (double)sqdist <= radius*radius} >= min_neighbors + 1 (the point itself counts)
        const float cell = static_cast<float>(ch.radius);
        MRGFE_TRY(nn_build_device_driven(ctx, &d_st->cp[1], &d_st->sl_rad, n, r.d_part, &d_st->bb_n[1], cell, 1u << 22, grid, &d_st->anomaly, r.h_box));
        MRGFE_TRY(nn_radius_flags_device_driven(ctx, grid, r.s2_out, &d_st->sl_rad, n, ch.radius * ch.radius, ch.radius_min_neighbors + 1, cell, d_flags));
    } else {
        // StatisticalOutlierRemoval: mean distance to the mean_k nearest (the exact wave-per-query search, its lists consumed in registers), the threshold
        // from the certified tree sums, inlier iff (double)mean distance <= threshold
        float*       d_dist = ctx->scratch[12].as<float>();
        uint32_t*    d_valid = reinterpret_cast<uint32_t*>(d_dist + n);
        sor::Result* h_sor = reinterpret_cast<sor::Result*>(ctx->pf_status.as<char>() + kPfStatusSorOffset);
        if (sor_sized_grid(ctx, ch)) {  // no leaf to take the edge from: the device chooses it from the cloud's density
            const float  start = g_sor_start_edge.load(std::memory_order_relaxed);
            const double target = g_sor_crowding.load(std::memory_order_relaxed);
            const int    halvings = g_sor_max_halvings.load(std::memory_order_relaxed);
            MRGFE_TRY(nn_build_device_sized(ctx, &d_st->cp[1], &d_st->sl_rad, n, r.d_part, &d_st->bb_n[1], start > 0.0f ? start : MRGFE_SOR_GRID_START_EDGE,
                                            target > 0.0 ? target : MRGFE_SOR_GRID_CROWDING, halvings >= 0 ? halvings : MRGFE_SOR_GRID_MAX_HALVINGS, MRGFE_SOR_GRID_PASSES,
                                            kSorCellsCap, grid, &d_st->anomaly, r.h_box, reinterpret_cast<NnSizedStatus*>(ctx->pf_status.as<char>() + kPfStatusGridOffset)));
        } else {
            MRGFE_TRY(nn_build_device_driven(ctx, &d_st->cp[1], &d_st->sl_rad, n, r.d_part, &d_st->bb_n[1], sor_cell_edge(ch), kSorCellsCap, grid, &d_st->anomaly, r.h_box));
        }
        MRGFE_TRY(nn_knn_mean_device_driven(ctx, grid, r.s2_out, &d_st->sl_rad, n, ch.mean_k + 1, d_dist, d_valid));
        MRGFE_TRY(sor_threshold_launch(ctx, d_dist, d_valid, &d_st->sl_rad.n, n, ch.stddev_mul, ctx->scratch[14].as<SorPartial>(), &d_st->sor, h_sor, &d_st->anomaly));
        hipLaunchKernelGGL(sor_flags_dd_kernel, r.g256, b256, 0, st, d_dist, &d_st->sl_rad.n, &d_st->sor.thr, d_flags);
    }
    MRGFE_TRY(tile_sums(ctx, d_flags, &d_st->sl_rad, r.tab, r.d_blk));
    hipLaunchKernelGGL(pf_compact_kernel<2>, r.gtiles, b256, 0, st, r.s2_out, d_flags, r.d_blk, 0u, r.d_work, d_st, r.h_status, r.d_part);
    MRGFE_HIP_CHECK(hipGetLastError());
    return MRGFE_OK;
}

// The three stages and the chain's one wait.  d_work receives the result (capacity n); d_third: a buffer of n points wherever a stage needs one that is
// neither the input nor the work buffer (an outlier filter, or the distance filter in front of the approximate grid), else unused.  `rec`: the record kernel
// follows the last stage, in front of the wait.
static int pf_run_stages(mrgfe_ctx* ctx, const PrefilterChain& ch, const ScanHead* head, const void* d_raw, float4* d_in, uint32_t n, float4* d_work, float4* d_third,
                         const BBox* d_head_boxes, PfReport* rep, const RecordDest* rec = nullptr)
{
    PfRun r;
    r.ctx = ctx;
    r.ch = &ch;
    r.down = chain_downsample(ch);
    r.n = n;
    r.tab.build(&n, 1);
    MRGFE_TRY(ctx->pf_state.ensure(sizeof(PfState)));
    MRGFE_TRY(ctx->pf_status.ensure(kPfStatusBytes));
    r.d_st = ctx->pf_state.as<PfState>();
    r.h_status = ctx->pf_status.as<uint32_t>();
    r.h_status[6] = 0;
    r.h_box = reinterpret_cast<BBox*>(r.h_status + 8);
    const SliceTable& tab = r.tab;
    if (ch.outlier == 2) {  // the statistical filter's mean distances and flags of validity, its tiles' sums
        MRGFE_TRY(ctx->scratch[12].ensure(size_t(n) * 8));
        MRGFE_TRY(ctx->scratch[14].ensure(sizeof(SorPartial) * (size_t(tab.total_blks) + 1)));
    }
    if (r.down == 2) {
        // the approximate grid's stretch ordinals and its 512 entry ranks.  Behind it the statistical filter may use the same two slots: both sizes are ensured
        // here, before the first launch (grow-only buffers: the larger demand holds), and the approximate grid's last reader of either (avg_emit_dd_kernel) is
        // queued on the one stream in front of the statistical stage's first writer (nn_knn_mean_dd_kernel, sor_threshold_launch)
        MRGFE_TRY(ctx->scratch[12].ensure(size_t(n) * 4));
        MRGFE_TRY(ctx->scratch[14].ensure(sizeof(uint32_t) * 512));
    }
    DevBuf &dbb = ctx->scratch[1], &dk = ctx->scratch[2], &dv = ctx->scratch[3], &dkt = ctx->scratch[4], &dvt = ctx->scratch[5], &dh = ctx->scratch[6], &dfl = ctx->scratch[7],
           &dblk = ctx->scratch[8], &dseg = ctx->scratch[9], &dcent = ctx->scratch[10], &dkeep = ctx->scratch[11];
    MRGFE_TRY(dbb.ensure(sizeof(BBox) * (tab.total_blks + 2)));
    MRGFE_TRY(dk.ensure(size_t(n) * 4)); MRGFE_TRY(dv.ensure(size_t(n) * 4)); MRGFE_TRY(dkt.ensure(size_t(n) * 4)); MRGFE_TRY(dvt.ensure(size_t(n) * 4));
    MRGFE_TRY(dh.ensure(sizeof(uint32_t) * 256 * (tab.total_blks + 1)));
    MRGFE_TRY(dfl.ensure(size_t(n) * 4));
    MRGFE_TRY(dblk.ensure(sizeof(uint32_t) * (tab.total_blks + 8)));
    MRGFE_TRY(dseg.ensure(sizeof(uint32_t) * (size_t(n) + 4) + sizeof(int32_t) * size_t(n)));
    MRGFE_TRY(dcent.ensure(sizeof(float4) * size_t(n)));
    MRGFE_TRY(dkeep.ensure(sizeof(uint32_t) * size_t(n)));
    r.d_part = dbb.as<BBox>();
    r.d_blk = dblk.as<uint32_t>();
    r.g256 = dim3((n + 255) / 256);
    r.gtiles = dim3(std::max<uint32_t>(1, tab.total_blks));
    r.d_work = d_work;
    const bool outlier = ch.outlier != 0;
    if (r.down == 0) {  // the outlier filter reads what the head left; without one that is the result
        r.s1_out = outlier ? (ch.distance ? d_third : d_in) : d_work;
        r.s2_out = const_cast<float4*>(r.s1_out);
    } else {
        r.s2_out = outlier ? d_third : d_work;
        // (the voxel grid's centroids pass through a scratch slot: it may read the buffer its compaction writes; the approximate grid emits in place)
        if (!ch.distance) r.s1_out = d_in;
        else r.s1_out = (r.down == 2 && !outlier) ? d_third : d_work;
    }
    MRGFE_TRY(pf_stage_head(r, head, d_raw, d_in, d_head_boxes));
    MRGFE_TRY(pf_stage_downsample(r));
    MRGFE_TRY(pf_stage_outlier(r));
    if (rec) {
        const auto kern = rec->sink->point_step == 16 ? pf_records_dd_kernel<16> : pf_records_dd_kernel<32>;
        hipLaunchKernelGGL(kern, r.g256, dim3(256), 0, ctx->stream, r.d_work, r.d_st, rec->d_dst);
        MRGFE_HIP_CHECK(hipGetLastError());
        ctx->eg_stats.launches += 1;
    }
    MRGFE_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the chain's one wait
    if (r.h_status[6] != 0x600df00du) { set_error("prefilter: the device-driven chain did not report"); return MRGFE_ERR_HIP; }
    for (int k = 0; k < 5; ++k) rep->counts[k] = r.h_status[k];
    rep->anomaly = r.h_status[5];
    rep->box = *r.h_box;
    return MRGFE_OK;
}

// A chain the device-driven form serves (device_driven_applies).  Returns MRGFE_OK with *used = true when it produced the output, *used = false
// (an anomaly) when the caller has to run the host-driven passes over d_in.
static int filter_chain_device_driven(mrgfe_ctx* ctx, const PrefilterChain& ch, const ScanHead* head, const void* d_raw, float4* d_in, uint32_t n, float4* d_work, float4* d_final,
                                      size_t* out_n, bool* used, const RecordDest* rec)
{
    *used = false;
    PfReport rep;
    MRGFE_TRY(pf_run_stages(ctx, ch, head, d_raw, d_in, n, d_work, d_final, nullptr, &rep, rec));
    PrefilterStats& ps = ctx->pf_stats;
    ps.anomaly = rep.anomaly;
    for (int k = 0; k < 5; ++k) ps.counts[k] = rep.counts[k];
    if (ch.outlier == 2) {
        const sor::Result* h_sor = reinterpret_cast<const sor::Result*>(ctx->pf_status.as<char>() + kPfStatusSorOffset);
        ctx->knn_stats.queries = rep.counts[3];  // (the live count of the k-NN launch)
        // the host's own build of the threshold's tail on the reported sums: the result must not depend on how the device library rounds an f64 divide or
        // square root (it costs nothing here)
        if (!sor::same_bits(sor::threshold(h_sor->sum, h_sor->sq_sum, h_sor->valid, ch.stddev_mul), h_sor->thr)) ps.anomaly |= kPfAnomalyRecheck;
        if (sor_sized_grid(ctx, ch)) {  // what the device chose for the k-NN grid (mrgfe_ctx_sor_grid_stats)
            const NnSizedStatus* g = reinterpret_cast<const NnSizedStatus*>(ctx->pf_status.as<char>() + kPfStatusGridOffset);
            SorGridStats&        s = ctx->sor_grid;
            s.sized = true;
            s.start = g->start;
            s.edge = g->edge;
            s.halvings = g->halvings;
            s.crowding = (g->measured && g->n_finite) ? 1.0 + 2.0 * double(g->crowd_sum) / double(g->n_finite) : 0.0;
            s.cells = g->n_cells;
        }
    }
    if (ps.anomaly != 0) return MRGFE_OK;  // something unusual: the host-driven chain decides what the reference does with it
    *out_n = rep.counts[4];
    *used = true;
    // remembered for mrgfe_reg_set_source_from_prefilter (filter_chain says whether d_work is the caller's buffer): behind an outlier filter the box of its
    // input, which encloses what it keeps; else the output's own box, which must not leave a non-finite point out
    const bool boxed = rep.box.n_finite > 0 && *out_n > 0 && (ch.outlier != 0 || rep.box.n_finite == *out_n);
    if (boxed) {
        for (int a = 0; a < 3; ++a) { ctx->pf_out_box[a] = rep.box.mn[a]; ctx->pf_out_box[3 + a] = rep.box.mx[a]; }
        ctx->pf_out_ptr = d_work;
        ctx->pf_out_n = *out_n;
        ctx->pf_out_valid = true;
    }
    return MRGFE_OK;  // the result is in d_work
}

// The downsample stage alone behind a caller's own head kernel (the odometry frame): VoxelGrid (method 1) or ApproximateVoxelGrid (2) of the n points at
// d_in into d_out (capacity n), one wait.  `d_tile_boxes`: one box per 2048-point tile of d_in as the caller's head left them, or NULL (a pass over d_in
// makes them).  rep->route: 0 the switch is off, 1 served (rep->kept points, their exact box and finite count), 2 an anomaly (rep->anomaly: no finite
// point, PCL's "leaf size too small" pass-through, no voxel) — on 0 and 2 the caller runs filter_[approx_]voxelgrid_device.  Leaves the chain's
// statistics and remembered output (mrgfe_ctx_prefilter_stats, mrgfe_reg_set_source_from_prefilter) alone: those describe chain calls.
int downsample_device_driven(mrgfe_ctx* ctx, int method, const float4* d_in, size_t n, const BBox* d_tile_boxes, float leaf, int min_pts, float4* d_out, DownsampleReport* rep)
{
    std::memset(rep, 0, sizeof(*rep));
    if (!prefilter_device_driven_mode() || n == 0 || n > 0x7fffffffu || !(leaf > 0) || (method != 1 && method != 2)) return MRGFE_OK;
    PrefilterChain ch;
    ch.distance = false;
    ch.voxelgrid = method == 1;
    ch.approx_voxelgrid = method == 2;
    ch.leaf = leaf;
    ch.min_pts = min_pts;
    ch.outlier = 0;
    PfReport pr;
    MRGFE_TRY(pf_run_stages(ctx, ch, nullptr, nullptr, const_cast<float4*>(d_in), static_cast<uint32_t>(n), d_out, nullptr, d_tile_boxes, &pr));
    rep->anomaly = pr.anomaly;
    rep->route = pr.anomaly ? 2 : 1;
    rep->n_finite_in = pr.counts[1];
    if (pr.anomaly) return MRGFE_OK;
    rep->kept = pr.counts[4];
    rep->kept_finite = pr.box.n_finite;
    for (int a = 0; a < 3; ++a) { rep->box[a] = pr.box.mn[a]; rep->box[3 + a] = pr.box.mx[a]; }
    return MRGFE_OK;
}

// Where the chain's packed input comes from — the only difference between the two entry families: a host cloud in one of the C ABI's layouts
// (upload_cloud puts it into the first buffer), or the wire records of a scan (they go up as they are and the scan head kernel writes the buffer).
struct ChainInput {
    const float*    xyzi = nullptr;
    size_t          stride = 16;
    const ScanHead* head = nullptr;
};

static int filter_chain_from(mrgfe_ctx* ctx, const PrefilterChain& ch, const ChainInput& in, size_t n, void* out, size_t* out_n, bool out_on_device, const RecordSink* rec,
                             const RecordSink* col = nullptr)
{
    *out_n = 0;
    if (rec) egress_begin(ctx);
    if (col) egress_second_begin(ctx);
    ctx->pf_out_valid = false;
    PrefilterStats& ps = ctx->pf_stats;  // (mrgfe_ctx_prefilter_stats: which route serves this call)
    ps.route = 0;
    ps.anomaly = 0;
    for (uint32_t& c : ps.counts) c = 0;
    ps.out_n = 0;
    ps.calls += 1;
    ctx->sor_grid = SorGridStats{};
    if (n == 0) return MRGFE_OK;
    if (n > 0x7fffffffu) { set_error("prefilter: cloud too large"); return MRGFE_ERR_INVALID; }
    DevBuf &a = ctx->pf_buf[0], &b = ctx->pf_buf[1];  // ping-pong, kept between calls (grow-only: a hipMalloc / hipFree pair per scan is a device-wide wait)
    const void* d_raw = nullptr;
    const bool  device_driven = device_driven_applies(ctx, ch, static_cast<uint32_t>(n));
    // The records of a device-driven STATISTICAL chain are staged whatever the caller's memory is: the host re-checks that chain's threshold behind the wait
    // (kPfAnomalyRecheck) and may hand the call back after the record kernel has run, and a caller's buffer must never hold a record beyond *out_n.
    RecordDest dest;
    int rc = rec ? record_dest_open(ctx, *rec, n, !(device_driven && ch.outlier == 2), &dest) : MRGFE_OK;
    if (rc == MRGFE_OK) rc = a.ensure(n * 16);
    if (rc == MRGFE_OK) rc = b.ensure(n * 16);
    if (rc == MRGFE_OK && !in.head) rc = upload_cloud(ctx, in.xyzi, n, in.stride, a.p);
    if (rc == MRGFE_OK && in.head) rc = upload_raw_records(ctx, in.head->data, size_t(in.head->height - 1) * in.head->row_step + size_t(in.head->width) * in.head->point_step, &d_raw);
    // The coloured records (col: only with a scan's wire records) are queued here, in front of the chain: the device-driven chain's one wait covers the kernel;
    // behind the host-driven passes colored_done waits for it.  They do not depend on the chain, so a chain that is handed back leaves them valid, and a direct
    // destination is final.  After a failure nothing may still write the caller's buffer: colored_done waits then, too.
    RecordDest cdest;
    bool       colored_queued = false;
    if (rc == MRGFE_OK && col) rc = record_dest_open(ctx, *col, n, true, &cdest, true);
    if (rc == MRGFE_OK && col) { rc = launch_colored_records(ctx, *in.head, d_raw, cdest); colored_queued = rc == MRGFE_OK; }
    auto colored_done = [&](int rc_in, bool waited) -> int {
        if (!colored_queued) return rc_in;
        if (rc_in != MRGFE_OK) { (void)hipStreamSynchronize(ctx->stream); return rc_in; }
        if (!waited) {
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("prefilter: the colour kernel failed"); return MRGFE_ERR_HIP; }
            ctx->eg2_stats.waits += 1;
        }
        record_dest_close(ctx, cdest, n);
        return MRGFE_OK;
    };
    if (rc == MRGFE_OK && in.head && !device_driven) rc = launch_scan_head(ctx, *in.head, d_raw, a.as<float4>(), nullptr);  // (the device-driven chain launches it itself)
    if (rc == MRGFE_OK && device_driven) {
        // the usual chain with its counts on the device: input a, work buffer = the caller's device buffer (capacity n) or b, result in the work buffer
        bool   used = false;
        size_t m = 0;
        float4* work = out_on_device ? static_cast<float4*>(out) : b.as<float4>();
        float4* final_buf = out_on_device ? b.as<float4>() : nullptr;
        DevBuf& c = ctx->scratch[13];
        if (!out_on_device) { rc = c.ensure(n * 16); final_buf = c.as<float4>(); }
        if (rc == MRGFE_OK) rc = filter_chain_device_driven(ctx, ch, in.head, d_raw, a.as<float4>(), static_cast<uint32_t>(n), work, final_buf, &m, &used, rec ? &dest : nullptr);
        if (rc != MRGFE_OK) return colored_done(rc, false);
        ps.route = used ? 1 : 2;
        if (used) {
            if (!out_on_device) ctx->pf_out_valid = false;  // (the cloud went to the host: nothing of the caller's stays on the device)
            if (rec) record_dest_close(ctx, dest, m);  // (the record kernel ran in front of the chain's wait)
            else if (!out_on_device) rc = download(ctx, work, m, static_cast<float*>(out));
            rc = colored_done(rc, true);  // (the colour kernel ran in front of the chain's wait, too)
            if (rc == MRGFE_OK) { *out_n = m; ps.out_n = m; ps.served += 1; }
            return rc;
        }
    }
    float4 *cur = a.as<float4>(), *nxt = b.as<float4>();
    size_t  m = n;
    auto pass = [&](auto&& f) {
        if (rc != MRGFE_OK || m == 0) return;
        size_t k = 0;
        rc = f(cur, m, nxt, &k);
        if (rc == MRGFE_OK) { std::swap(cur, nxt); m = k; }
    };
    if (ch.distance) pass([&](const float4* i, size_t ni, float4* o, size_t* k) { return filter_distance_device(ctx, i, ni, ch.near_t, ch.far_t, o, k); });
    if (ch.approx_voxelgrid) pass([&](const float4* i, size_t ni, float4* o, size_t* k) { return filter_approx_voxelgrid_device(ctx, i, ni, ch.leaf, o, k); });
    else if (ch.voxelgrid) pass([&](const float4* i, size_t ni, float4* o, size_t* k) { int overflow = 0; return filter_voxelgrid_device(ctx, i, ni, ch.leaf, ch.min_pts, o, k, &overflow); });
    if (ch.outlier == 1) pass([&](const float4* i, size_t ni, float4* o, size_t* k) { return filter_radius_outlier_device(ctx, i, ni, ch.radius, ch.radius_min_neighbors, o, k); });
    if (ch.outlier == 2) pass([&](const float4* i, size_t ni, float4* o, size_t* k) { return filter_statistical_outlier_device(ctx, i, ni, ch.mean_k, ch.stddev_mul, o, k); });
    if (rc == MRGFE_OK && rec) {
        // the host-driven passes made the cloud: its records with the host's count, the caller's device copy beside them, one more wait
        rc = launch_cloud_records(ctx, cur, static_cast<uint32_t>(m), dest);
        if (rc == MRGFE_OK && m && (out_on_device && hipMemcpyAsync(out, cur, m * 16, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)) { set_error("prefilter: device copy failed"); rc = MRGFE_ERR_HIP; }
        if (rc == MRGFE_OK && m) {
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("prefilter: the record kernel failed"); rc = MRGFE_ERR_HIP; }
            ctx->eg_stats.waits += 1;
        }
        if (rc == MRGFE_OK) record_dest_close(ctx, dest, m);
    } else if (rc == MRGFE_OK) {
        if (!out_on_device) {
            rc = download(ctx, cur, m, static_cast<float*>(out));
        } else if (m && (hipMemcpyAsync(out, cur, m * 16, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)) {
            set_error("prefilter: device copy failed");
            rc = MRGFE_ERR_HIP;
        }
    }
    rc = colored_done(rc, false);
    if (rc == MRGFE_OK) { *out_n = m; ps.out_n = m; }
    return rc;
}

int filter_chain(mrgfe_ctx* ctx, const PrefilterChain& ch, const float* xyzi, size_t n, size_t stride, void* out, size_t* out_n, bool out_on_device, const RecordSink* rec)
{
    ChainInput in;
    in.xyzi = xyzi;
    in.stride = stride;
    return filter_chain_from(ctx, ch, in, n, out, out_n, out_on_device, rec);
}
int scan_chain(mrgfe_ctx* ctx, const PrefilterChain& ch, const ScanHead& head, void* out, size_t* out_n, bool out_on_device, const RecordSink* rec, const RecordSink* colored)
{
    ChainInput in;
    in.head = &head;
    return filter_chain_from(ctx, ch, in, size_t(head.width) * head.height, out, out_n, out_on_device, rec, colored);
}

int filter_distance(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double near_t, double far_t, float* out, size_t* out_n)
{
    return host_wrap(ctx, xyzi, n, stride, out, out_n, [&](const float4* i, float4* o, size_t* m) { return filter_distance_device(ctx, i, n, near_t, far_t, o, m); });
}
int filter_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float leaf, int min_pts, float* out, size_t* out_n, int* overflow)
{
    return host_wrap(ctx, xyzi, n, stride, out, out_n, [&](const float4* i, float4* o, size_t* m) { return filter_voxelgrid_device(ctx, i, n, leaf, min_pts, o, m, overflow); });
}
int filter_approx_voxelgrid(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, float leaf, float* out, size_t* out_n)
{
    return host_wrap(ctx, xyzi, n, stride, out, out_n, [&](const float4* i, float4* o, size_t* m) { return filter_approx_voxelgrid_device(ctx, i, n, leaf, o, m); });
}
int filter_radius_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, double radius, int min_neighbors, float* out, size_t* out_n)
{
    return host_wrap(ctx, xyzi, n, stride, out, out_n, [&](const float4* i, float4* o, size_t* m) { return filter_radius_outlier_device(ctx, i, n, radius, min_neighbors, o, m); });
}
int filter_statistical_outlier(mrgfe_ctx* ctx, const float* xyzi, size_t n, size_t stride, int mean_k, double stddev_mul, float* out, size_t* out_n)
{
    return host_wrap(ctx, xyzi, n, stride, out, out_n, [&](const float4* i, float4* o, size_t* m) { return filter_statistical_outlier_device(ctx, i, n, mean_k, stddev_mul, o, m); });
}

}  // namespace mrgfe
