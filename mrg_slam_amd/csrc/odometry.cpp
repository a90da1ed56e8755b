// csrc/odometry.cpp — the odometry frame in one call (include/mrgfe.h mrgfe_odom_*): ScanMatchingOdometryComponent::cloud_callback -> matching()
// (apps/scan_matching_odometry_component.cpp:138-150, 195-350) over one registration.  The decisions live in OdomController (odom_ctl.h, host only); this
// file stages the frame's cloud, hands it to the registration and drives the controller.
//
// Where a frame's cloud lives.  The handle keeps ONE spare device buffer.  A frame's cloud is written into the spare (by the head kernel of odom_head.hip,
// by a device-to-device copy, or by the downsample filter), and the spare is then SWAPPED with the registration's own source buffer (first frame: target
// buffer) — the buffer mrgfe_reg_set_source / _set_target upload into, so the swaps of mrgfe_reg_source_becomes_target / mrgfe_reg_set_target keep working
// unchanged and no cloud is copied.  The buffer that comes back holds the source before this one (or nothing the registration still reads): it is what a
// failing frame swaps back, and what the next frame overwrites.  The registration so owns every cloud it keeps, none aliases caller memory.
//
// Order of effects.  The controller is stepped on a COPY, and the copy replaces the handle's controller as the call's last act: whatever fails before —
// the alignment, the status pass, the target build of a keyframe switch, the download of the aligned cloud — leaves the state as it was, and the
// registration's source and target are put back (the engines recompute lazily what they had derived from them).
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "api_internal.h"
#include "cellsort.h"
#include "common.h"
#include "filters.h"
#include "ingest.h"
#include "mapcloud.h"
#include "odom_ctl.h"
#include "odom_head.h"

using namespace mrgfe;

static_assert(sizeof(mrgfe_odom_params) == 72, "mrgfe_odom_params: the layout the bindings mirror");
static_assert(sizeof(mrgfe_odom_result) == 368, "mrgfe_odom_result: the layout the bindings mirror");
static_assert(sizeof(mrgfe_dbg_odom_state) == 160 && sizeof(OdomCtlState) == sizeof(mrgfe_dbg_odom_state), "mrgfe_dbg_odom_state mirrors OdomCtlState");
static_assert(int(MRGFE_ODOM_FIRST_FRAME) == int(ODOM_FIRST_FRAME) && int(MRGFE_ODOM_ACCEPTED) == int(ODOM_ACCEPTED) && int(MRGFE_ODOM_NOT_CONVERGED) == int(ODOM_NOT_CONVERGED) &&
                  int(MRGFE_ODOM_REJECTED) == int(ODOM_REJECTED) && int(MRGFE_ODOM_REJECTED_RESET) == int(ODOM_REJECTED_RESET),
              "enum mrgfe_odom_outcome mirrors OdomOutcome");

struct mrgfe_odom {
    mrgfe_reg*        reg = nullptr;
    mrgfe_ctx*        ctx = nullptr;
    mrgfe_odom_params p;
    OdomController    ctl;
    DevBuf            spare;  // the next frame's cloud is written here (see above)
    DevBuf            box;    // the head kernel's partial boxes, then the merged one
    PinBuf            h_box;  // ... which the host reads at the frame's first wait
    // what the last successful frame handed over (mrgfe_dbg_odom_source)
    const void*       last_cloud = nullptr;
    size_t            last_n = 0;
    float             last_box[6] = {0, 0, 0, 0, 0, 0};
    uint32_t          last_n_finite = 0xffffffffu;
    // mrgfe_odom_stats: the downsample route and anomaly word of the last completed frame, its points in and handed on, whether the source grid got a box,
    // frames whose downsample was served device-driven
    int64_t           stats[6] = {0, 0, 0, 0, 0, 0};
};
struct mrgfe_dbg_odom_ctl { OdomController c; };

namespace {

int check_odom_params(const mrgfe_odom_params* p, const char* fn)
{
    if (!p) { set_error("%s: NULL params", fn); return MRGFE_ERR_INVALID; }
    if (p->downsample_method < 0 || p->downsample_method > 2) { set_error("%s: unknown downsample_method %d (0 NONE, 1 VOXELGRID, 2 APPROX_VOXELGRID)", fn, p->downsample_method); return MRGFE_ERR_INVALID; }
    if (p->downsample_method != 0 && !(p->downsample_resolution > 0.0f)) { set_error("%s: downsample_resolution must be > 0", fn); return MRGFE_ERR_INVALID; }
    if (p->enable_transform_thresholding && p->max_consecutive_rejections < 1) { set_error("%s: max_consecutive_rejections must be >= 1", fn); return MRGFE_ERR_INVALID; }
    return MRGFE_OK;
}
OdomCtlParams ctl_params_from(const mrgfe_odom_params& p)
{
    OdomCtlParams c;
    c.keyframe_delta_translation = p.keyframe_delta_translation;
    c.keyframe_delta_angle = p.keyframe_delta_angle;
    c.keyframe_delta_time = p.keyframe_delta_time;
    c.enable_transform_thresholding = p.enable_transform_thresholding;
    c.max_consecutive_rejections = p.max_consecutive_rejections;
    c.max_acceptable_translation = p.max_acceptable_translation;
    c.max_acceptable_angle = p.max_acceptable_angle;
    return c;
}
void fill_result(const OdomDecision& d, mrgfe_odom_result* out)
{
    std::memset(out, 0, sizeof(*out));
    out->outcome = d.outcome;
    out->new_keyframe = d.new_keyframe;
    out->consecutive_rejections = d.consecutive_rejections;
    std::memcpy(out->odom, d.odom, sizeof(out->odom));
    std::memcpy(out->keyframe_pose, d.keyframe_pose, sizeof(out->keyframe_pose));
    std::memcpy(out->trans, d.trans, sizeof(out->trans));
}
// a rollback calls entry points that may set the thread's message: the failure's own message is put back behind them
struct KeepError {
    std::string msg;
    KeepError() : msg(mrgfe_last_error()) {}
    ~KeepError() { set_error("%s", msg.c_str()); }
};

// one frame's cloud, either form
struct FrameInput {
    bool                  device = false;
    mrgfe_keyframe_params lay{};        // message form (row_step filled in)
    const void*           data = nullptr;
    size_t                raw_bytes = 0;
    const void*           d_xyzi = nullptr;  // device form
    size_t                n = 0;             // points of the input cloud, > 0
};

// aligned_rec (the record forms): the aligned cloud as records instead of packed points, *n_aligned their count
int odom_frame_impl(const char* fn, mrgfe_odom* o, const FrameInput& in, double stamp, const float* msf_delta, int want_status, float* aligned_xyzi, mrgfe_odom_result* out,
                    const RecordSink* aligned_rec = nullptr, size_t* n_aligned = nullptr)
{
    mrgfe_reg* reg = o->reg;
    mrgfe_ctx* ctx = o->ctx;
    MRGFE_LOCK(ctx);
    MRGFE_TRY(ctx->bind());
    TraceRange tr(fn);
    hipStream_t  st = ctx->stream;
    const size_t n = in.n;
    const bool   downsample = o->p.downsample_method != 0;
    const bool   first = !o->ctl.has_keyframe();
    // a box serves the source grid of the engines that compute k-NN covariances (GicpEngine::compute_covariances); NDT and ICP_HIP build none.  Without a
    // downsample it is the head kernel's (wants_box: read at a wait of its own), with one the device-driven downsample stage reports the kept points'
    const bool   takes_box = !first && reg->gicp && keeps_covariances(reg->params);
    const bool   wants_box = takes_box && !downsample;

    // ---- 1. the frame's cloud into the spare buffer (nothing of the registration is touched yet) ----
    MRGFE_TRY(o->spare.ensure(n * 16));
    float4*       d_stage = o->spare.as<float4>();
    const float4* d_whole = nullptr;  // the whole input cloud, before the downsample (:342 transforms *cloud)
    float         hint[6];
    const float*  box_hint = nullptr;
    float         head_box[6] = {0, 0, 0, 0, 0, 0};
    uint32_t      head_finite = 0xffffffffu;
    size_t        m = n;  // points handed to the registration
    if (!in.device) {
        const uint32_t nblk = odom_head_tiles(static_cast<uint32_t>(n));
        MRGFE_TRY(o->box.ensure(sizeof(BBox) * (nblk + 1)));
        MRGFE_TRY(o->h_box.ensure(sizeof(BBox)));
        float4* d_gather = d_stage;
        if (downsample) { MRGFE_TRY(ctx->up_out.ensure(n * 16)); d_gather = ctx->up_out.as<float4>(); }  // (where mrgfe_ingest_pointcloud2 leaves its cloud)
        const void* d_raw = nullptr;
        MRGFE_TRY(upload_raw_records(ctx, in.data, in.raw_bytes, &d_raw));
        MRGFE_TRY(launch_odom_head(ctx, d_raw, in.lay, d_gather, o->box.as<BBox>(), o->box.as<BBox>() + nblk));
        MRGFE_HIP_CHECK(hipMemcpyAsync(o->h_box.p, o->box.as<BBox>() + nblk, sizeof(BBox), hipMemcpyDeviceToHost, st));
        d_whole = d_gather;
    } else {
        d_whole = static_cast<const float4*>(in.d_xyzi);
        if (!downsample) {
            MRGFE_HIP_CHECK(hipMemcpyAsync(d_stage, in.d_xyzi, n * 16, hipMemcpyDeviceToDevice, st));
            if (ctx->pf_out_valid && ctx->pf_out_ptr == in.d_xyzi && ctx->pf_out_n == n) {  // the rule of mrgfe_reg_set_source_from_prefilter
                std::memcpy(hint, ctx->pf_out_box, sizeof(hint));
                box_hint = hint;
            }
        }
    }
    DownsampleReport ds;
    std::memset(&ds, 0, sizeof(ds));
    if (downsample) {
        // the prefilter chain's downsample stage directly behind the head kernel, whose per-tile boxes give it the voxel parameters (device form: a pass
        // over the cloud makes them): ONE wait brings down the kept count, the kept points' exact box, the finite count and the anomaly word
        MRGFE_TRY(downsample_device_driven(ctx, o->p.downsample_method, d_whole, n, in.device ? nullptr : o->box.as<BBox>(), o->p.downsample_resolution,
                                           o->p.downsample_min_points_per_voxel, d_stage, &ds));
        if (ds.route == 1) {
            m = ds.kept;
            if (takes_box && m > 0 && ds.kept_finite == m) {  // (a voxel grid's centroids always are; the approximate grid's where its points were)
                std::memcpy(hint, ds.box, sizeof(hint));
                box_hint = hint;
            }
        }
    }
    if (downsample && ds.route != 1) {  // the switch is off, or an anomaly (PCL's pass-through, no finite point, no voxel): the host-driven filter decides
        if (o->p.downsample_method == 1) MRGFE_TRY(filter_voxelgrid_device(ctx, d_whole, n, o->p.downsample_resolution, o->p.downsample_min_points_per_voxel, d_stage, &m, nullptr));  // (waits)
        else MRGFE_TRY(filter_approx_voxelgrid_device(ctx, d_whole, n, o->p.downsample_resolution, d_stage, &m));  // (waits)
    } else if (!downsample && !in.device && wants_box) {
        MRGFE_HIP_CHECK(hipStreamSynchronize(st));  // the frame's first wait: the box is on the host
    }
    // (otherwise the box is not needed before the call's next wait — the downsample's, the alignment's or the first frame's — and is read behind it)
    auto read_head_box = [&]() {
        const BBox hb = *o->h_box.as<BBox>();
        for (int a = 0; a < 3; ++a) { head_box[a] = hb.mn[a]; head_box[3 + a] = hb.mx[a]; }
        head_finite = hb.n_finite;
    };
    if (!in.device && wants_box) {
        read_head_box();
        if (head_finite == n) {  // the exact box of a cloud whose points are all finite: what NnGrid::build's known_box asks for
            std::memcpy(hint, head_box, sizeof(hint));
            box_hint = hint;
        }
    }
    if (m == 0) { set_error("%s: no point is left after the downsample", fn); return MRGFE_ERR_EMPTY; }

    OdomController trial = o->ctl;  // stepped here, committed at the end
    float          guess[16];
    trial.begin_frame(stamp, msf_delta, guess);
    OdomDecision          d;
    mrgfe_matching_status status{};
    int                   has_status = 0;

    if (first) {
        // ---- 2a. :197-205: the cloud becomes the target, as mrgfe_reg_set_target places it ----
        const void*  old_tgt = reg->d_tgt;
        const size_t old_n = reg->n_tgt;
        const bool   had_target = reg->has_target;
        if (reg->d_src == reg->tgt.p && reg->tgt.p != nullptr) std::swap(reg->src, reg->tgt);  // (a source living in the target's buffer keeps it: mrgfe_reg_set_target)
        std::swap(reg->tgt, o->spare);
        int rc = mrgfe_reg_set_target_device(reg, reg->tgt.p, m);
        if (rc == MRGFE_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("%s: waiting for the stream failed", fn); rc = MRGFE_ERR_HIP; }  // (a device-form copy may still run)
        if (rc != MRGFE_OK) {
            KeepError keep;
            (void)hipStreamSynchronize(st);
            std::swap(reg->tgt, o->spare);
            if (had_target) (void)mrgfe_reg_set_target_device(reg, old_tgt, old_n);
            else { reg->d_tgt = old_tgt; reg->n_tgt = old_n; reg->has_target = false; }
            return rc;
        }
        d = trial.end_frame(false, nullptr);
        fill_result(d, out);
    } else {
        // ---- 2b. :207-268: the cloud becomes the source, align from the controller's guess, the status when asked ----
        const void*  old_src = reg->d_src;
        const size_t old_n = reg->n_src;
        const bool   had_source = reg->has_source;
        auto put_source_back = [&]() {
            (void)hipStreamSynchronize(st);
            std::swap(reg->src, o->spare);
            reg->d_src = old_src;
            reg->n_src = old_n;
            reg->has_source = had_source;
            if (reg->gicp) (void)reg->gicp->set_source(old_src, old_n);
        };
        std::swap(reg->src, o->spare);
        reg->d_src = reg->src.p;
        reg->n_src = m;
        reg->has_source = true;
        int rc = reg->gicp ? reg->gicp->set_source(reg->d_src, reg->n_src, box_hint) : MRGFE_OK;
        if (rc == MRGFE_OK) rc = mrgfe_reg_align(reg, guess, nullptr);
        if (rc == MRGFE_OK && want_status) {
            rc = mrgfe_reg_matching_status(reg, o->p.status_max_correspondence_dist, msf_delta, &status);  // :268, before every decision
            has_status = rc == MRGFE_OK;
        }
        if (rc != MRGFE_OK) {
            KeepError keep;
            put_source_back();
            return rc;
        }
        float final_cm[16];
        row2col(reg->final_rm, final_cm);
        d = trial.end_frame(reg->converged, final_cm);  // :270-339
        if (d.new_keyframe) {
            // ---- 3. :294-295, :332-333: the hand-over of mrgfe_reg_source_becomes_target ----
            const void*  old_tgt = reg->d_tgt;
            const size_t old_nt = reg->n_tgt;
            const bool   swaps = reg->d_src == reg->src.p && reg->src.p != nullptr;
            rc = mrgfe_reg_source_becomes_target(reg);
            if (rc != MRGFE_OK) {
                KeepError keep;
                (void)hipStreamSynchronize(st);
                if (swaps && reg->d_src == reg->tgt.p) std::swap(reg->src, reg->tgt);
                (void)mrgfe_reg_set_target_device(reg, old_tgt, old_nt);
                put_source_back();
                return rc;
            }
        }
        fill_result(d, out);
        out->converged = reg->converged ? 1 : 0;
        out->iterations = reg->iterations;
        out->has_status = has_status;
        if (has_status) out->status = status;
    }
    out->n_source = static_cast<uint32_t>(m);

    // ---- 4. :341-343: transformPointCloud(*cloud, *aligned, odom) on the paths that reach it ----
    if (aligned_xyzi && d.outcome == ODOM_ACCEPTED) {
        float odom_rm[16];
        col2row(d.odom, odom_rm);
        MRGFE_TRY(o->spare.ensure(n * 16));  // (the buffer that came back: nothing reads it any more)
        MRGFE_TRY(transform_cloud_device(ctx, d_whole, n, odom_rm, o->spare.as<float4>()));
        MRGFE_HIP_CHECK(hipMemcpyAsync(aligned_xyzi, o->spare.p, n * 16, hipMemcpyDeviceToHost, st));
        MRGFE_HIP_CHECK(hipStreamSynchronize(st));
    }
    if (aligned_rec && d.outcome == ODOM_ACCEPTED) {
        // :341-347 in one pass over the input cloud: transform and record in one kernel, into the caller's page-locked buffer or the context's pinned one
        float odom_rm[16];
        col2row(d.odom, odom_rm);
        MRGFE_TRY(transformed_records_device(ctx, d_whole, n, odom_rm, *aligned_rec));  // (the one wait of the aligned_xyzi path)
        *n_aligned = n;
    }
    if (!in.device && !wants_box) read_head_box();  // (at least one wait lies behind the copy by now)
    o->ctl = trial;
    o->last_cloud = first ? reg->d_tgt : reg->d_src;
    o->last_n = m;
    std::memcpy(o->last_box, head_box, sizeof(o->last_box));
    o->last_n_finite = head_finite;
    o->stats[0] = ds.route;
    o->stats[1] = ds.anomaly;
    o->stats[2] = static_cast<int64_t>(n);
    o->stats[3] = static_cast<int64_t>(m);
    o->stats[4] = (!first && reg->gicp && box_hint) ? 1 : 0;
    o->stats[5] += ds.route == 1 ? 1 : 0;
    return MRGFE_OK;
}

}  // namespace

extern "C" {

void mrgfe_odom_default_params(mrgfe_odom_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->downsample_method = 0;               // config/mrg_slam.yaml:95 (NONE)
    p->downsample_resolution = 0.1f;        // :94
    p->downsample_min_points_per_voxel = 1;
    p->keyframe_delta_translation = 1.0;    // :77-79
    p->keyframe_delta_angle = 0.5236;
    p->keyframe_delta_time = 10000.0;
    p->enable_transform_thresholding = 0;   // :82-86
    p->max_consecutive_rejections = 5;
    p->max_acceptable_translation = 1.0;
    p->max_acceptable_angle = 1.0;
    p->status_max_correspondence_dist = 0.5;  // scan_matching_odometry_component.cpp:413
}
size_t mrgfe_odom_params_size(void) { return sizeof(mrgfe_odom_params); }
size_t mrgfe_odom_result_size(void) { return sizeof(mrgfe_odom_result); }

int mrgfe_odom_create(mrgfe_reg* reg, const mrgfe_odom_params* params, mrgfe_odom** out)
{
    return abi_guard("mrgfe_odom_create", [&]() -> int {
        if (!reg || !out) { set_error("mrgfe_odom_create: NULL argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        MRGFE_TRY(check_odom_params(params, "mrgfe_odom_create"));
        mrgfe_odom* o = new (std::nothrow) mrgfe_odom();
        if (!o) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        o->reg = reg;
        o->ctx = reg->ctx;
        o->p = *params;
        o->ctl = OdomController(ctl_params_from(*params));
        *out = o;
        return MRGFE_OK;
    });
}

void mrgfe_odom_destroy(mrgfe_odom* o)
{
    if (!o) return;
    MRGFE_LOCK(o->ctx);
    (void)hipSetDevice(o->ctx->device);
    delete o;
}

int mrgfe_odom_reset(mrgfe_odom* o)
{
    if (!o) { set_error("mrgfe_odom_reset: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(o->ctx);
    o->ctl.reset();
    return MRGFE_OK;
}

int mrgfe_odom_stats(const mrgfe_odom* o, int64_t out[6])
{
    if (!o || !out) { set_error("mrgfe_odom_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(o->ctx);
    std::memcpy(out, o->stats, sizeof(o->stats));
    return MRGFE_OK;
}

int mrgfe_odom_frame(mrgfe_odom* o, const mrgfe_keyframe_params* lay, const void* data, size_t data_bytes, double stamp, const float* msf_delta, int want_status,
                     float* aligned_xyzi, mrgfe_odom_result* out)
{
    static const char* fn = "mrgfe_odom_frame";
    return abi_guard(fn, [&]() -> int {
        if (!o || !lay || !data || !out) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        FrameInput in;
        in.lay = *lay;
        MRGFE_TRY(check_pointcloud2_layout(o->ctx, fn, in.lay.width, in.lay.height, in.lay.point_step, &in.lay.row_step, in.lay.off_x, in.lay.off_y, in.lay.off_z, in.lay.off_intensity));
        in.n = size_t(in.lay.width) * in.lay.height;
        if (in.n == 0) { set_error("%s: an empty message", fn); return MRGFE_ERR_INVALID; }
        in.raw_bytes = size_t(in.lay.height - 1) * in.lay.row_step + size_t(in.lay.width) * in.lay.point_step;
        if (data_bytes < in.raw_bytes) { set_error("%s: the payload has %zu bytes, the layout needs %zu", fn, data_bytes, in.raw_bytes); return MRGFE_ERR_INVALID; }
        in.data = data;
        return odom_frame_impl(fn, o, in, stamp, msf_delta, want_status, aligned_xyzi, out);
    });
}

int mrgfe_odom_frame_device(mrgfe_odom* o, const void* d_xyzi, size_t n, double stamp, const float* msf_delta, int want_status, float* aligned_xyzi, mrgfe_odom_result* out)
{
    static const char* fn = "mrgfe_odom_frame_device";
    return abi_guard(fn, [&]() -> int {
        if (!o || !d_xyzi || !out) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        MRGFE_TRY(check_count(n, fn));
        if (n == 0) { set_error("%s: an empty cloud", fn); return MRGFE_ERR_INVALID; }
        FrameInput in;
        in.device = true;
        in.d_xyzi = d_xyzi;
        in.n = n;
        return odom_frame_impl(fn, o, in, stamp, msf_delta, want_status, aligned_xyzi, out);
    });
}

// what the record forms refuse before the frame is looked at: a NULL destination or count, a point_step other than the two of record_store.h, no room for one
// record per input point
static int check_aligned_sink(const char* fn, int point_step, void* records, size_t capacity_bytes, size_t* n_aligned, size_t n, RecordSink* sink)
{
    if (!records || !n_aligned) { set_error("%s: NULL aligned_records / n_aligned", fn); return MRGFE_ERR_INVALID; }
    *n_aligned = 0;
    if (point_step != 16 && point_step != 32) { set_error("%s: point_step %d (16: x y z intensity, 32: pcl::PointXYZI)", fn, point_step); return MRGFE_ERR_INVALID; }
    if (capacity_bytes / size_t(point_step) < n) { set_error("%s: capacity_bytes %zu, %zu input points of %d bytes need room", fn, capacity_bytes, n, point_step); return MRGFE_ERR_INVALID; }
    sink->point_step = point_step;
    sink->records = records;
    sink->capacity = capacity_bytes;
    return MRGFE_OK;
}

int mrgfe_odom_frame_records(mrgfe_odom* o, const mrgfe_keyframe_params* lay, const void* data, size_t data_bytes, double stamp, const float* msf_delta, int want_status,
                             int point_step, void* aligned_records, size_t capacity_bytes, size_t* n_aligned, mrgfe_odom_result* out)
{
    static const char* fn = "mrgfe_odom_frame_records";
    return abi_guard(fn, [&]() -> int {
        if (!o || !lay || !data || !out) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        FrameInput in;
        in.lay = *lay;
        MRGFE_TRY(check_pointcloud2_layout(o->ctx, fn, in.lay.width, in.lay.height, in.lay.point_step, &in.lay.row_step, in.lay.off_x, in.lay.off_y, in.lay.off_z, in.lay.off_intensity));
        in.n = size_t(in.lay.width) * in.lay.height;
        RecordSink sink;
        MRGFE_TRY(check_aligned_sink(fn, point_step, aligned_records, capacity_bytes, n_aligned, in.n, &sink));
        if (in.n == 0) { set_error("%s: an empty message", fn); return MRGFE_ERR_INVALID; }
        in.raw_bytes = size_t(in.lay.height - 1) * in.lay.row_step + size_t(in.lay.width) * in.lay.point_step;
        if (data_bytes < in.raw_bytes) { set_error("%s: the payload has %zu bytes, the layout needs %zu", fn, data_bytes, in.raw_bytes); return MRGFE_ERR_INVALID; }
        in.data = data;
        return odom_frame_impl(fn, o, in, stamp, msf_delta, want_status, nullptr, out, &sink, n_aligned);
    });
}

int mrgfe_odom_frame_records_device(mrgfe_odom* o, const void* d_xyzi, size_t n, double stamp, const float* msf_delta, int want_status, int point_step, void* aligned_records,
                                    size_t capacity_bytes, size_t* n_aligned, mrgfe_odom_result* out)
{
    static const char* fn = "mrgfe_odom_frame_records_device";
    return abi_guard(fn, [&]() -> int {
        if (!o || !d_xyzi || !out) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        MRGFE_TRY(check_count(n, fn));
        RecordSink sink;
        MRGFE_TRY(check_aligned_sink(fn, point_step, aligned_records, capacity_bytes, n_aligned, n, &sink));
        if (n == 0) { set_error("%s: an empty cloud", fn); return MRGFE_ERR_INVALID; }
        FrameInput in;
        in.device = true;
        in.d_xyzi = d_xyzi;
        in.n = n;
        return odom_frame_impl(fn, o, in, stamp, msf_delta, want_status, nullptr, out, &sink, n_aligned);
    });
}

// ---- diagnostic entry points (include/mrgfe_debug.h) ----
int mrgfe_dbg_odom_ctl_create(const mrgfe_odom_params* params, mrgfe_dbg_odom_ctl** out)
{
    return abi_guard("mrgfe_dbg_odom_ctl_create", [&]() -> int {
        if (!out) { set_error("mrgfe_dbg_odom_ctl_create: NULL argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        MRGFE_TRY(check_odom_params(params, "mrgfe_dbg_odom_ctl_create"));
        mrgfe_dbg_odom_ctl* h = new (std::nothrow) mrgfe_dbg_odom_ctl();
        if (!h) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        h->c = OdomController(ctl_params_from(*params));
        *out = h;
        return MRGFE_OK;
    });
}
void mrgfe_dbg_odom_ctl_destroy(mrgfe_dbg_odom_ctl* h) { delete h; }
int mrgfe_dbg_odom_ctl_begin(mrgfe_dbg_odom_ctl* h, double stamp, const float* msf_delta, int* aligns, float guess[16])
{
    if (!h || !aligns || !guess) { set_error("mrgfe_dbg_odom_ctl_begin: NULL argument"); return MRGFE_ERR_INVALID; }
    *aligns = h->c.begin_frame(stamp, msf_delta, guess) ? 1 : 0;
    return MRGFE_OK;
}
int mrgfe_dbg_odom_ctl_end(mrgfe_dbg_odom_ctl* h, int converged, const float* final_transformation, mrgfe_odom_result* out)
{
    if (!h || !out) { set_error("mrgfe_dbg_odom_ctl_end: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!h->c.pending()) { set_error("mrgfe_dbg_odom_ctl_end: no frame was begun"); return MRGFE_ERR_STATE; }
    if (h->c.has_keyframe() && !final_transformation) { set_error("mrgfe_dbg_odom_ctl_end: NULL final transformation"); return MRGFE_ERR_INVALID; }
    const bool first = !h->c.has_keyframe();
    const OdomDecision d = h->c.end_frame(converged != 0, final_transformation);
    fill_result(d, out);
    out->converged = (!first && converged) ? 1 : 0;
    return MRGFE_OK;
}
int mrgfe_dbg_odom_ctl_state(const mrgfe_dbg_odom_ctl* h, mrgfe_dbg_odom_state* out)
{
    if (!h || !out) { set_error("mrgfe_dbg_odom_ctl_state: NULL argument"); return MRGFE_ERR_INVALID; }
    std::memcpy(out, &h->c.state(), sizeof(*out));
    return MRGFE_OK;
}
int mrgfe_dbg_odom_state_of(const mrgfe_odom* o, mrgfe_dbg_odom_state* out)
{
    if (!o || !out) { set_error("mrgfe_dbg_odom_state_of: NULL argument"); return MRGFE_ERR_INVALID; }
    std::memcpy(out, &o->ctl.state(), sizeof(*out));
    return MRGFE_OK;
}
int mrgfe_dbg_odom_source(mrgfe_odom* o, float* out_xyzi, size_t* n, float box[6], uint32_t* n_finite)
{
    if (!o || !n) { set_error("mrgfe_dbg_odom_source: NULL argument"); return MRGFE_ERR_INVALID; }
    if (!o->last_cloud) { set_error("mrgfe_dbg_odom_source: no frame yet"); return MRGFE_ERR_STATE; }
    *n = o->last_n;
    if (box) std::memcpy(box, o->last_box, sizeof(o->last_box));
    if (n_finite) *n_finite = o->last_n_finite;
    if (!out_xyzi) return MRGFE_OK;
    MRGFE_LOCK(o->ctx);
    MRGFE_TRY(o->ctx->bind());
    MRGFE_HIP_CHECK(hipMemcpyAsync(out_xyzi, o->last_cloud, o->last_n * 16, hipMemcpyDeviceToHost, o->ctx->stream));
    MRGFE_HIP_CHECK(hipStreamSynchronize(o->ctx->stream));
    return MRGFE_OK;
}

}  // extern "C"
