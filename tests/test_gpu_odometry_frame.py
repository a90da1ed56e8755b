"""GPU: the odometry frame in one call (mrgfe_odom_frame / mrgfe_odom_frame_device; ScanMatchingOdometryComponent::cloud_callback -> matching(),
apps/scan_matching_odometry_component.cpp:138-150, 195-350).

1. The head kernel (csrc/odom_head.hip): for eight point counts around the 2048-point tile and four message layouts, the cloud the registration receives
   has the bytes of mrgfe_ingest_pointcloud2, and the box and finite count equal numpy's over the finite points, bit for bit.
2. One call against the composed calls, bit for bit: ingest -> downsample or none -> mrgfe_reg_set_source_device -> mrgfe_reg_align ->
   mrgfe_reg_matching_status -> mrgfe_reg_source_becomes_target with the guesses of a second controller stepped through mrgfe_dbg_odom_ctl_*; every field
   of mrgfe_odom_result, the status bytes, the aligned cloud, and afterwards getFitnessScore and the 1-NN search of both registrations.
3. GICP_HIP / SMALL_GICP_HIP against ScanMatchingOdometry over the CPU oracle's class: same keyframes, every trans within 1e-4 m / 1e-4 rad.
4. Failures and lifecycle.
Everything is drawn from fixed seeds; the frames are 8 prefiltered VLP-16 scans of the synthetic street, 1 m and 1.5 degrees apart."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
CLASSES = ["NdtHip", "PclNdtHip", "GicpHip", "SmallGicpHip", "VgicpHip", "IcpHip", "PclGicpHip"]
N_FRAMES = 8
# keyframe_delta_translation 1.5 m: at 1 m per frame every second frame becomes the keyframe, and no frame's motion is near the threshold
PARAMS = {"keyframe_delta_translation": 1.5, "keyframe_delta_angle": 0.5236, "keyframe_delta_time": 10000.0}
# thresholding on: a jump of several metres is rejected, the second rejection in a row resets
JUMP_PARAMS = dict(PARAMS, enable_transform_thresholding=1, max_acceptable_translation=1.8, max_acceptable_angle=1.0, max_consecutive_rejections=2)
JUMP_ORDER = [0, 1, 5, 6, 7]  # frame indices in the order they arrive: 1 m, then 4 m at once
JUMP_PRED_FROM = [None, 0, 1, 1, 6]  # the prediction is taken against prev_trans, which a rejected frame does not advance: the last accepted frame
PREFILTER = {"downsample_resolution": 0.25}
TOL_T, TOL_R = 1e-4, 1e-4  # the bar tests/test_gpu_gicp.py holds the GICP family to against the oracle

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
SIZES = [0, 1, 255, 256, 2047, 2048, 2049, 4097]
LAYOUTS = ["packed", "pcl32", "rows48", "no_intensity"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def refusal(fn):
    """(status, message) of the MrgfeError `fn` raises.  No exception object outlives this frame: kept in a test's frame (as `pytest.raises(...) as e` keeps it)
    it ties that frame — with its context, registration and odometry handle — into a reference cycle through its traceback, and the collector finalises the
    members of a cycle in no particular order, the context possibly before the handles that borrow it."""
    from mrg_slam_amd import MrgfeError

    try:
        fn()
    except MrgfeError as ex:
        return ex.status, str(ex)
    raise AssertionError("the call did not fail")


def message(cloud, layout):
    """The cloud as a PointCloud2 dict in one of the four layouts of tests/test_gpu_store_many.py, and the packed cloud the message stands for."""
    c = np.ascontiguousarray(cloud, dtype=np.float32)
    n = len(c)
    if layout == "packed":
        return {"data": c.tobytes(), "width": n, "height": 1, "point_step": 16, "fields": FIELDS, "row_step": 0}, c
    if layout == "pcl32":  # pcl::PointXYZI in memory: 32 bytes, intensity at byte 16, padding filled with NaN bit patterns
        rec = np.full((n, 8), np.nan, dtype=np.float32)
        rec[:, :3], rec[:, 4] = c[:, :3], c[:, 3]
        return {"data": rec.tobytes(), "width": n, "height": 1, "point_step": 32, "fields": {"x": 0, "y": 4, "z": 8, "intensity": 16}, "row_step": 0}, c
    if layout == "rows48":  # 48-byte records (x y z at 16, intensity at 36), height 2, every row padded by 80 bytes the message does not describe
        h, w = 2, (n + 1) // 2
        full = np.full((h * w, 4), 7.0, dtype=np.float32)  # (an odd count is padded to 2 x w points: the message stands for the padded cloud)
        full[:n] = c
        rec = np.full((h * w, 12), np.nan, dtype=np.float32)
        rec[:, 4:7], rec[:, 9] = full[:, :3], full[:, 3]
        rows = np.full((h, w * 48 + 80), 0xFF, dtype=np.uint8)
        rows[:, : w * 48] = rec.view(np.uint8).reshape(h, w * 48)
        return {"data": rows.tobytes(), "width": w, "height": h, "point_step": 48, "fields": {"x": 16, "y": 20, "z": 24, "intensity": 36}, "row_step": w * 48 + 80}, full
    if layout == "no_intensity":  # off_intensity < 0: the intensity is 0
        c0 = c.copy()
        c0[:, 3] = 0.0
        rec = np.full((n, 5), np.nan, dtype=np.float32)
        rec[:, 1:4] = c[:, :3]
        return {"data": rec.tobytes(), "width": n, "height": 1, "point_step": 20, "fields": {"x": 4, "y": 8, "z": 12}, "row_step": 0}, c0
    raise ValueError(layout)


def head_cloud(n, kind, seed=0):
    """Seeded random; `kind`: "mixed" a few non-finite points anywhere, "edges" non-finite points first and last in every 2048-point tile,
    "none_finite" no finite point at all (x, y or z non-finite in every point)"""
    rng = np.random.default_rng(9000 + 17 * n + seed)
    c = rng.normal(0, 5, (n, 4)).astype(np.float32)
    c[c == 0] = 1.0  # (a +-0 coordinate would make min / max a matter of operand order)
    if kind == "mixed" and n >= 8:
        c[n // 7, 0] = np.nan
        c[n // 3, 1] = np.inf
        c[n // 2] = np.nan
    elif kind == "edges":
        for i in sorted({0, n - 1} | {t for t in range(0, n, 2048)} | {t - 1 for t in range(2048, n + 1, 2048)}):
            if 0 <= i < n:
                c[i, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    elif kind == "none_finite":
        c[np.arange(n), np.arange(n) % 3] = np.nan
        c[::2, 3] = np.inf  # (a non-finite intensity alone does not make a point non-finite)
    return c


def numpy_box(cloud):
    fin = np.isfinite(cloud[:, :3]).all(axis=1)
    pts = cloud[fin, :3]
    if len(pts) == 0:
        return np.array([np.inf] * 3 + [-np.inf] * 3, dtype=np.float32), 0
    return np.concatenate([pts.min(axis=0), pts.max(axis=0)]).astype(np.float32), int(fin.sum())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_head_kernel_gathers_like_ingest_and_finds_the_exact_box(layout):
    from mrg_slam_amd import Context, HipOdometry, IcpHip, _lib
    from mrg_slam_amd.io import ingest_pointcloud2

    ctx = Context()
    reg = IcpHip(ctx=ctx)  # (a target is only kept, nothing is built for it: clouds without a finite point are fine)
    odo = HipOdometry(reg)
    cases = [(n, "mixed") for n in SIZES] + [(4097, "edges"), (2048, "edges"), (300, "none_finite"), (2050, "none_finite")]  # (even counts: the two-row layout pads an odd one with a finite point)
    for n, kind in cases:
        msg, cloud = message(head_cloud(n, kind), layout)
        if msg["width"] * msg["height"] == 0:
            assert refusal(lambda: odo.frame(msg, 1.0))[0] == _lib.ERR_INVALID  # an empty message is no frame
            continue
        odo.reset()
        r = odo.frame(msg, 1.0)
        assert r.outcome == "first_frame" and r.new_keyframe and r.n_source == len(cloud), (n, kind)
        got, box, n_finite = odo.source()
        want = ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ctx=ctx)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(cloud)), (n, kind)
        want_box, want_finite = numpy_box(cloud)
        assert n_finite == want_finite, (n, kind)
        assert np.array_equal(bits(box), bits(want_box)), (n, kind, box, want_box)
        if kind == "none_finite":
            assert n_finite == 0


# ---- the frames and the two routes -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    from mrg_slam_amd import Context, prefilter, synth

    ctx = Context()
    scene = synth.street_scene()
    poses = synth.arc_trajectory(N_FRAMES)
    raw = [synth.synth_lidar(scene, poses[k], "VLP16", synth.BASE_SEED + k) for k in range(N_FRAMES)]
    clouds = [prefilter(r, PREFILTER, ctx=ctx) for r in raw]
    assert all(1500 < len(c) < 12000 for c in clouds), [len(c) for c in clouds]
    return {"poses": poses, "raw": raw, "clouds": clouds, "stamps": [100.0 + 0.1 * k for k in range(N_FRAMES)]}


def predictions(frames, order, pred_from=None, null_at=()):
    """msf_delta per arriving frame: the true motion since frame pred_from[j] (default: the frame that arrived before it), slightly off; None (the identity
    of :211) on the first frame and at the positions `null_at`."""
    from mrg_slam_amd import synth

    pred_from = pred_from or [None] + order[:-1]
    out = []
    for j, (a, b) in enumerate(zip(pred_from, order)):
        out.append(None if a is None or j in null_at else synth.warm_guess(synth.rel_pose(frames["poses"][a], frames["poses"][b]), 10 + b).astype(np.float32))
    return out


def plain_predictions(cls_name, frames):
    """the plain sequence: frame 3 (right after a keyframe switch) comes without a prediction for the GICP family and ICP — it starts 1 m off; NDT's 1 m
    voxels are given one on every frame"""
    return predictions(frames, list(range(N_FRAMES)), null_at=() if "Ndt" in cls_name else (3,))


class Composed:
    """The composed route over one registration: the calls an integrator makes today, with the guesses of a controller stepped by hand."""

    def __init__(self, cls_name, ctx, params, downsample=None):
        import mrg_slam_amd as M
        from mrg_slam_amd import _lib

        self.L = _lib.lib()
        self.ctx = ctx
        self.reg = getattr(M, cls_name)(transformation_epsilon=0.01, ctx=ctx)
        self.downsample = downsample
        p = _lib.OdomParams()
        self.L.mrgfe_odom_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        self.status_dist = p.status_max_correspondence_dist
        self.h = C.c_void_p()
        assert self.L.mrgfe_dbg_odom_ctl_create(C.byref(p), C.byref(self.h)) == 0
        self.keep = []  # the device clouds the registration borrows

    def __del__(self):
        self.L.mrgfe_dbg_odom_ctl_destroy(self.h)

    def frame(self, msg, stamp, msf_delta, want_status, want_aligned):
        import torch

        from mrg_slam_amd import _lib, filters
        from mrg_slam_amd.io import ingest_pointcloud2
        from mrg_slam_amd.map_cloud import transform_cloud

        whole = ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ctx=self.ctx)
        cloud = whole
        if self.downsample is not None:
            f = filters.VoxelGrid(self.ctx) if self.downsample[0] == "VOXELGRID" else filters.ApproximateVoxelGrid(self.ctx)
            f.setLeafSize(self.downsample[1])
            if self.downsample[0] == "VOXELGRID":
                f.setMinimumPointsNumberPerVoxel(self.downsample[2])
            f.setInputCloud(whole)
            cloud = f.filter()
        dev = torch.from_numpy(np.ascontiguousarray(cloud)).to("cuda:0")
        torch.cuda.synchronize()
        self.keep = self.keep[-3:] + [dev]
        guess, aligns = np.zeros(16, dtype=np.float32), C.c_int(-1)
        d = None if msf_delta is None else np.ascontiguousarray(np.asarray(msf_delta, dtype=np.float32).T)
        dptr = None if d is None else d.ctypes.data_as(FP)
        assert self.L.mrgfe_dbg_odom_ctl_begin(self.h, stamp, dptr, C.byref(aligns), guess.ctypes.data_as(FP)) == 0
        out = _lib.OdomResult()
        status = _lib.MatchingStatus()
        if not aligns.value:
            self.reg.setInputTargetDevice(dev.data_ptr(), len(cloud))
            assert self.L.mrgfe_dbg_odom_ctl_end(self.h, 0, None, C.byref(out)) == 0
        else:
            self.reg.setInputSourceDevice(dev.data_ptr(), len(cloud))
            _lib.check(self.L.mrgfe_reg_align(self.reg._h, guess.ctypes.data_as(FP), None))
            if want_status:
                _lib.check(self.L.mrgfe_reg_matching_status(self.reg._h, self.status_dist, dptr, C.byref(status)))
            final = np.zeros(16, dtype=np.float32)
            _lib.check(self.L.mrgfe_reg_final_transformation(self.reg._h, final.ctypes.data_as(FP)))
            assert self.L.mrgfe_dbg_odom_ctl_end(self.h, self.L.mrgfe_reg_has_converged(self.reg._h), final.ctypes.data_as(FP), C.byref(out)) == 0
            if out.new_keyframe:
                assert self.reg.sourceBecomesTarget() == 0
            out.iterations = self.L.mrgfe_reg_iterations(self.reg._h)
            out.has_status = int(bool(want_status))
            if want_status:
                out.status = status
        out.n_source = len(cloud)
        aligned = None
        if want_aligned and out.outcome == _lib.ODOM_ACCEPTED:
            aligned = transform_cloud(whole, np.array(out.odom, dtype=np.float32).reshape(4, 4).T, ctx=self.ctx)
        return bytes(out), aligned


def run_sequence(route, frames, order, preds, layout="packed"):
    """-> per frame (result bytes, aligned cloud or None, the result record); `route` is a HipOdometry or a Composed"""
    from mrg_slam_amd import _lib

    rows = []
    for j, k in enumerate(order):
        msg, _ = message(frames["clouds"][k], layout)
        want_status, want_aligned = j % 2 == 1 or j == 2, j != 4
        if isinstance(route, Composed):
            raw, aligned = route.frame(msg, frames["stamps"][k], preds[j], want_status, want_aligned)
        else:
            r = route.frame(msg, frames["stamps"][k], preds[j], want_status, want_aligned)
            raw, aligned = bytes(r.raw), r.aligned
        rows.append((raw, aligned, _lib.OdomResult.from_buffer_copy(raw)))
    return rows


def same_rows(got, want, what):
    for j, (g, w) in enumerate(zip(got, want)):
        if g[0] != w[0]:
            raise AssertionError((what, j, "fields that differ", _differing_fields(g[2], w[2])))
        assert (g[1] is None) == (w[1] is None), (what, j)
        if g[1] is not None:
            assert np.array_equal(bits(g[1]), bits(w[1])), (what, j, "aligned cloud")
    assert len(got) == len(want)


def _differing_fields(a, b):
    out = []
    for name, _ in a._fields_:
        x, y = getattr(a, name), getattr(b, name)
        if (bytes(x) if hasattr(x, "_fields_") or hasattr(x, "_length_") else x) != (bytes(y) if hasattr(y, "_fields_") or hasattr(y, "_length_") else y):
            out.append(name)
    return out


def same_registration(a, b, frames, what):
    q = frames["clouds"][3][:400]
    assert a.getFitnessScore() == b.getFitnessScore(), what
    ia, da = a.nearestKSearch1(q)
    ib, db = b.nearestKSearch1(q)
    assert np.array_equal(ia, ib) and np.array_equal(bits(da), bits(db)), what


_ALONE = {}


def one_call_alone(cls_name, frames):
    """the plain sequence through the one call on a context of its own (memoised: items 2 and 4 compare against it)"""
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry

    if cls_name not in _ALONE:
        ctx = Context()
        reg = getattr(M, cls_name)(transformation_epsilon=0.01, ctx=ctx)
        odo = HipOdometry(reg, PARAMS)
        _ALONE[cls_name] = (run_sequence(odo, frames, list(range(N_FRAMES)), plain_predictions(cls_name, frames)), reg, odo, ctx)
    return _ALONE[cls_name]


@pytest.mark.parametrize("cls_name", CLASSES)
def test_one_call_equals_the_composed_calls(cls_name, frames):
    from mrg_slam_amd import _lib

    got, reg, _, ctx = one_call_alone(cls_name, frames)
    comp = Composed(cls_name, ctx, PARAMS)
    want = run_sequence(comp, frames, list(range(N_FRAMES)), plain_predictions(cls_name, frames))
    same_rows(got, want, cls_name)
    same_registration(reg, comp.reg, frames, cls_name)
    outcomes = [r[2].outcome for r in got]
    assert outcomes[0] == _lib.ODOM_FIRST_FRAME and all(o == _lib.ODOM_ACCEPTED for o in outcomes[1:]), outcomes
    assert sum(r[2].new_keyframe for r in got[1:]) >= 2, [r[2].new_keyframe for r in got]
    assert any(r[2].has_status for r in got) and any(r[1] is not None for r in got)


@pytest.mark.parametrize("cls_name", CLASSES)
def test_a_jump_is_rejected_then_accepted_by_the_reset(cls_name, frames):
    """thresholding on: the frame 4 m further is rejected, the next one is the second rejection in a row and becomes the keyframe; one call == composed"""
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry, _lib

    ctx = Context()
    reg = getattr(M, cls_name)(transformation_epsilon=0.01, ctx=ctx)
    preds = predictions(frames, JUMP_ORDER, JUMP_PRED_FROM)
    got = run_sequence(HipOdometry(reg, JUMP_PARAMS), frames, JUMP_ORDER, preds, layout="pcl32")
    comp = Composed(cls_name, ctx, JUMP_PARAMS)
    want = run_sequence(comp, frames, JUMP_ORDER, preds, layout="pcl32")
    same_rows(got, want, cls_name)
    same_registration(reg, comp.reg, frames, cls_name)
    outcomes = [r[2].outcome for r in got]
    assert outcomes[:4] == [_lib.ODOM_FIRST_FRAME, _lib.ODOM_ACCEPTED, _lib.ODOM_REJECTED, _lib.ODOM_REJECTED_RESET], outcomes
    assert got[2][2].consecutive_rejections == 1 and got[3][2].consecutive_rejections == 0 and got[3][2].new_keyframe == 1
    assert got[2][1] is None and got[3][1] is None  # the aligned cloud is written on ACCEPTED only


@pytest.mark.parametrize("cls_name", ["GicpHip", "NdtHip"])
@pytest.mark.parametrize("downsample", [("VOXELGRID", 0.25, 1), ("VOXELGRID", 0.5, 2), ("APPROX_VOXELGRID", 0.4, 1)])
def test_one_call_equals_the_composed_calls_with_a_downsample(cls_name, downsample, frames):
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry

    ctx = Context()
    reg = getattr(M, cls_name)(transformation_epsilon=0.01, ctx=ctx)
    params = dict(PARAMS, downsample_method=downsample[0], downsample_resolution=downsample[1], downsample_min_points_per_voxel=downsample[2])
    order, layout = list(range(5)), "rows48" if cls_name == "GicpHip" else "no_intensity"
    preds = predictions(frames, order)
    got = run_sequence(HipOdometry(reg, params), frames, order, preds, layout)
    comp = Composed(cls_name, ctx, PARAMS, downsample)
    want = run_sequence(comp, frames, order, preds, layout)
    same_rows(got, want, (cls_name, downsample))
    same_registration(reg, comp.reg, frames, (cls_name, downsample))
    sizes = [(r[2].n_source, len(message(frames["clouds"][k], layout)[1])) for k, r in zip(order, got)]
    assert all(a <= b for a, b in sizes), sizes
    if downsample[1] > PREFILTER["downsample_resolution"]:  # (the frames come out of a 0.25 m voxel grid: the same grid again keeps every point)
        assert any(a < b for a, b in sizes), sizes


@pytest.mark.parametrize("cls_name", ["NdtHip", "GicpHip", "SmallGicpHip", "IcpHip"])
def test_device_form_fed_by_the_scan_callback(cls_name, frames):
    """mrgfe_scan_callback_device leaves the prefiltered scan in the caller's buffer, mrgfe_odom_frame_device takes it from there (the GICP family builds the
    source grid in the chain's box); the buffer is overwritten with garbage between frames.  Same results as the message form over the same clouds."""
    import torch

    import mrg_slam_amd as M
    from mrg_slam_amd import HipOdometry
    from mrg_slam_amd.filters import scan_callback_to_device
    from mrg_slam_amd.io import pointcloud2_from_xyzi

    want, _, _, ctx = one_call_alone(cls_name, frames)
    reg = getattr(M, cls_name)(transformation_epsilon=0.01, ctx=ctx)
    odo = HipOdometry(reg, PARAMS)
    cap = max(len(r) for r in frames["raw"]) + 16
    buf = torch.empty((cap, 4), dtype=torch.float32, device="cuda:0")
    preds = plain_predictions(cls_name, frames)
    got = []
    for k in range(N_FRAMES):
        m = pointcloud2_from_xyzi(frames["raw"][k])
        n = scan_callback_to_device(m["data"], m["width"], m["height"], m["point_step"], m["fields"], buf.data_ptr(), cap, params=PREFILTER, ctx=ctx)
        assert n == len(frames["clouds"][k])
        r = odo.frame_device(buf.data_ptr(), n, frames["stamps"][k], preds[k], k % 2 == 1 or k == 2, k != 4)
        buf.fill_(float("nan"))  # the caller reuses its buffer: a keyframe never aliases it
        torch.cuda.synchronize()
        got.append((bytes(r.raw), r.aligned, r.raw))
    same_rows(got, want, cls_name)
    same_registration(reg, one_call_alone(cls_name, frames)[1], frames, cls_name)


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name,oracle_name,threads", [("GicpHip", "FastGicp", 4), ("SmallGicpHip", "SmallGicp", 1)])
def test_one_call_against_the_mirror_over_the_oracle(cls_name, oracle_name, threads, frames):
    from mrg_slam_amd import ScanMatchingOdometry, synth
    from oracle import oracle as orc

    got, _, _, _ = one_call_alone(cls_name, frames)
    o = getattr(orc, oracle_name)(transformation_epsilon=0.01, num_threads=threads)
    mirror = ScanMatchingOdometry(o, PARAMS)
    preds = plain_predictions(cls_name, frames)
    for k in range(N_FRAMES):
        before = mirror.keyframes
        mirror.matching(frames["stamps"][k], frames["clouds"][k], preds[k])
        r = got[k][2]
        assert bool(r.new_keyframe) == (mirror.keyframes > before), k
        if k == 0:
            continue
        To = np.asarray(o.getFinalTransformation())
        Tg = np.array(r.trans, dtype=np.float32).reshape(4, 4).T
        assert bool(r.converged) == bool(o.hasConverged()), k
        dt, dr = np.linalg.norm(Tg[:3, 3].astype(np.float64) - To[:3, 3]), synth.rotation_angle(Tg[:3, :3], To[:3, :3])
        print(f"{cls_name} frame {k}: |dt| {dt:.3e} m, angle {dr:.3e} rad")
        assert dt <= TOL_T and dr <= TOL_R, (k, dt, dr)


# ---- 4. failures and lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_failures_give_the_documented_codes_and_leave_the_sequence_undisturbed(frames):
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry, _lib

    want, _, _, _ = one_call_alone("SmallGicpHip", frames)
    ctx = Context()
    reg = M.SmallGicpHip(transformation_epsilon=0.01, ctx=ctx)
    odo = HipOdometry(reg, PARAMS)
    preds = plain_predictions("SmallGicpHip", frames)
    L = _lib.lib()

    def refused(msg, status=_lib.ERR_INVALID):
        state = bytes(odo.state())
        assert refusal(lambda: odo.frame(msg, 777.0, want_status=True, want_aligned=True))[0] == status and bytes(odo.state()) == state

    got = []
    for k in range(N_FRAMES):
        good, _ = message(frames["clouds"][k], "packed")
        if k in (0, 3, 6):  # before the first frame, after a keyframe switch and after a plain frame
            refused(dict(good, data=good["data"][:-4]))                                   # a short payload
            refused(dict(good, fields=dict(FIELDS, y=6)))                                 # an offset that is no multiple of 4
            refused(dict(good, point_step=12))                                            # fields outside the record
            refused(dict(good, data=b"", width=0))                                        # an empty message
            out = _lib.OdomResult()
            lay = _lib.KeyframeParams()
            assert L.mrgfe_odom_frame(None, C.byref(lay), None, 0, 0.0, None, 0, None, C.byref(out)) == _lib.ERR_INVALID       # NULL handle
            assert L.mrgfe_odom_frame(odo._h, C.byref(lay), None, 0, 0.0, None, 0, None, C.byref(out)) == _lib.ERR_INVALID     # NULL data
            assert L.mrgfe_odom_frame_device(odo._h, None, 5, 0.0, None, 0, None, C.byref(out)) == _lib.ERR_INVALID           # NULL cloud
            assert L.mrgfe_odom_frame_device(odo._h, C.c_void_p(256), 0, 0.0, None, 0, None, C.byref(out)) == _lib.ERR_INVALID  # no point
        r = odo.frame(good, frames["stamps"][k], preds[k], k % 2 == 1 or k == 2, k != 4)
        got.append((bytes(r.raw), r.aligned, r.raw))
    same_rows(got, want, "with failed frames in between")
    closed = HipOdometry(reg, PARAMS)
    closed.close()
    assert refusal(lambda: closed.frame(frames["clouds"][0], 1.0))[0] == _lib.ERR_INVALID
    assert L.mrgfe_odom_reset(None) == _lib.ERR_INVALID
    h = C.c_void_p()
    p = _lib.OdomParams()
    L.mrgfe_odom_default_params(C.byref(p))
    p.downsample_method = 7
    assert L.mrgfe_odom_create(reg._h, C.byref(p), C.byref(h)) == _lib.ERR_INVALID and not h.value
    assert L.mrgfe_odom_create(None, C.byref(p), C.byref(h)) == _lib.ERR_INVALID


def test_a_failed_target_build_puts_the_target_back_and_reset_starts_over(frames):
    """NDT: a first frame whose voxel grid would overflow int32 fails with MRGFE_ERR_OVERFLOW like mrgfe_reg_set_target; the registration's target is the
    keyframe again, the controller still has no keyframe, and the frames after it give what they give without the failed call.  reset(): the next
    frame is a first frame."""
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry, _lib

    overflow = frames["clouds"][2][:100].copy()
    overflow[0, :3] = (2e5, 2e5, 2e3)  # more than INT32_MAX voxels of 1 m in its bounding box
    rows = {}
    preds = predictions(frames, list(range(N_FRAMES)))
    for how in ("plain", "disturbed"):
        ctx = Context()
        reg = M.NdtHip(transformation_epsilon=0.01, ctx=ctx)
        odo = HipOdometry(reg, PARAMS)
        out = []
        for k in range(6):
            if k == 3:
                odo.reset()
                assert not odo.state().has_keyframe
                if how == "disturbed":
                    fitness = reg.getFitnessScore()
                    status, text = refusal(lambda: odo.frame(overflow, 55.0))
                    assert status == _lib.ERR_OVERFLOW and "Leaf size is too small" in text
                    assert not odo.state().has_keyframe and reg.getFitnessScore() == fitness
            r = odo.frame(frames["clouds"][k], frames["stamps"][k], None if k in (0, 3) else preds[k], True, True)
            out.append((bytes(r.raw), r.aligned, r.raw))
        rows[how] = out
        assert [r[2].outcome for r in out][0] == _lib.ODOM_FIRST_FRAME and out[3][2].outcome == _lib.ODOM_FIRST_FRAME
        assert np.array_equal(np.array(out[3][2].odom), np.eye(4, dtype=np.float32).reshape(16))
    same_rows(rows["disturbed"], rows["plain"], "after a failed first frame")


def test_two_handles_on_one_context_answer_as_they_do_alone(frames):
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry

    ctx = Context()
    names = ["GicpHip", "NdtHip"]
    regs = [getattr(M, n)(transformation_epsilon=0.01, ctx=ctx) for n in names]
    odos = [HipOdometry(r, PARAMS) for r in regs]
    preds = [plain_predictions(n, frames) for n in names]
    got = [[], []]
    for k in range(N_FRAMES):
        msg, _ = message(frames["clouds"][k], "packed")
        for i in (0, 1) if k % 2 == 0 else (1, 0):
            r = odos[i].frame(msg, frames["stamps"][k], preds[i][k], k % 2 == 1 or k == 2, k != 4)
            got[i].append((bytes(r.raw), r.aligned, r.raw))
    for i, n in enumerate(names):
        same_rows(got[i], one_call_alone(n, frames)[0], n)
