"""GPU: mrgfe_scan_callback[_device] — PointCloud2 bytes to the filtered scan in one call — against the separate calls it stands for
(mrgfe_ingest_pointcloud2 -> mrgfe_deskew -> mrgfe_transform_cloud -> mrgfe_prefilter[_device]) and against the CPU oracle's chain.  Every
comparison is bit for bit and in order; every compared output has more than 100 points unless the case is a degenerate one on purpose."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1
FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
DEFAULT = ("VOXELGRID", "RADIUS", True)
# (downsample_method, outlier_removal_method, enable_distance_filter, deskew, transform): every value of every axis, the default chain with all four
# deskew / transform settings
CHAINS = [DEFAULT + (False, False), DEFAULT + (True, False), DEFAULT + (False, True), DEFAULT + (True, True),
          ("APPROX_VOXELGRID", "RADIUS", True, True, True), ("NONE", "RADIUS", True, False, True), ("VOXELGRID", "STATISTICAL", True, True, False),
          ("VOXELGRID", "NONE", False, True, True), ("APPROX_VOXELGRID", "STATISTICAL", False, False, False), ("NONE", "NONE", True, True, True),
          ("VOXELGRID", "RADIUS", False, True, True), ("NONE", "STATISTICAL", False, False, True), ("APPROX_VOXELGRID", "NONE", True, False, True)]


def base_link():
    from mrg_slam_amd import synth

    return synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)


def chain_params(down, outlier, distance, **more):
    p = {"downsample_method": down, "outlier_removal_method": outlier, "enable_distance_filter": distance}
    p.update(more)
    return p


def packed(cloud):
    c = np.ascontiguousarray(cloud, dtype=np.float32)
    return {"data": memoryview(c).cast("B") if len(c) else b"", "width": len(c), "height": 1, "point_step": 16, "fields": FIELDS, "row_step": 0}


def oracle_chain(cloud, ang_v, T, params):
    """deskewing -> transformPointCloud (non-finite points stay as they are) -> the three filters, by the CPU oracle."""
    from mrg_slam_amd.prefiltering import DEFAULTS, OracleOps
    from oracle import oracle as orc

    c = np.ascontiguousarray(cloud, dtype=np.float32)
    if ang_v is not None:
        c = orc.deskew(c, ang_v, PERIOD)
    if T is not None:
        c = c.copy()
        fin = np.isfinite(c[:, :3]).all(1)
        if fin.any():
            c[fin] = orc.transform_points(T, np.ascontiguousarray(c[fin]))
    p = dict(DEFAULTS)
    p.update(params)
    return OracleOps(orc).filters(c, p)


def separate_calls(msg, ang_v, T, params, ctx=None):
    """The route the one call replaces: four entry points, the cloud through host memory between them."""
    from mrg_slam_amd import deskew, prefilter, transform_cloud
    from mrg_slam_amd.io import ingest_pointcloud2

    c = ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ctx=ctx)
    if ang_v is not None:
        c = deskew(c, ang_v, PERIOD, ctx=ctx)
    if T is not None:
        c = transform_cloud(c, T, ctx=ctx)
    return prefilter(c, params, ctx=ctx)


def one_call(msg, ang_v, T, params, ctx=None):
    from mrg_slam_amd import scan_callback

    return scan_callback(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ang_v, PERIOD, T, params, ctx=ctx)


def one_call_device(msg, ang_v, T, params, ctx=None):
    import torch

    from mrg_slam_amd import scan_callback_to_device

    n = msg["width"] * msg["height"]
    buf = torch.empty((max(n, 1), 4), dtype=torch.float32, device="cuda:0")
    m = scan_callback_to_device(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], buf.data_ptr(), n, msg["row_step"], ang_v, PERIOD, T, params, ctx=ctx)
    return buf[:m].cpu().numpy()


def with_nonfinite(cloud):
    c = cloud.copy()
    c[::97, 1] = np.nan  # fromROSMsg keeps NaN returns: they pass the transform untouched and the distance filter drops them
    c[5::389, 2] = np.inf
    return c


def vlp64_scan():
    from mrg_slam_amd import synth

    return synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED + 77)


def check(msg, cloud, ang_v, T, params, degenerate=False, ctx=None):
    got = one_call(msg, ang_v, T, params, ctx=ctx)
    print(f"scan_callback: {msg['width']} x {msg['height']} step {msg['point_step']} -> {len(got)} points  {params}")
    np.testing.assert_array_equal(got, separate_calls(msg, ang_v, T, params, ctx=ctx))
    np.testing.assert_array_equal(one_call_device(msg, ang_v, T, params, ctx=ctx), got)
    if cloud is not None:
        np.testing.assert_array_equal(got, oracle_chain(cloud, ang_v, T, params))
    assert degenerate or len(got) > 100
    return got


@pytest.mark.parametrize("which", range(len(CHAINS)))
def test_scan_callback_equals_the_separate_calls_and_the_oracle(street_pair_vlp16, which):
    down, outlier, distance, deskew, transform = CHAINS[which]
    cloud = street_pair_vlp16[which % 2]
    check(packed(cloud), cloud, ANG_V if deskew else None, base_link() if transform else None, chain_params(down, outlier, distance))


@pytest.mark.parametrize("device_driven", [1, 0])
@pytest.mark.parametrize("deskew,transform", [(False, False), (True, False), (False, True), (True, True)])
def test_default_chain_in_both_settings_of_the_device_driven_switch(street_pair_vlp16, device_driven, deskew, transform):
    from mrg_slam_amd._lib import lib

    cloud = street_pair_vlp16[1]
    try:
        assert lib().mrgfe_dbg_set_prefilter_device_driven(device_driven) == device_driven
        check(packed(cloud), cloud, ANG_V if deskew else None, base_link() if transform else None, {})
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)


@pytest.mark.parametrize("deskew,transform", [(True, True), (False, True)])
def test_default_chain_on_a_vlp64_scan(deskew, transform):
    cloud = vlp64_scan()
    assert len(cloud) > 100000
    check(packed(cloud), cloud, ANG_V if deskew else None, base_link() if transform else None, {})


def test_layouts_give_the_output_of_the_packed_layout(street_pair_vlp16):
    from mrg_slam_amd.io import pcl_xyzi_records

    cloud = np.ascontiguousarray(street_pair_vlp16[0][: (len(street_pair_vlp16[0]) // 16) * 16])
    n, T = len(cloud), base_link()
    ref = check(packed(cloud), cloud, ANG_V, T, {})
    # the reference's in-memory pcl::PointXYZI records
    pcl = {"data": pcl_xyzi_records(cloud).tobytes(), "width": n, "height": 1, "point_step": 32, "fields": {"x": 0, "y": 4, "z": 8, "intensity": 16}, "row_step": 0}
    np.testing.assert_array_equal(check(pcl, cloud, ANG_V, T, {}), ref)
    # an organised cloud: 16 rows, each padded by 48 bytes the message does not describe (filled with NaN bit patterns: they must not be read)
    w = n // 16
    rows = np.full((16, w * 16 + 48), 0xFF, dtype=np.uint8)
    rows[:, : w * 16] = cloud.view(np.uint8).reshape(16, w * 16)
    org = {"data": rows.tobytes(), "width": w, "height": 16, "point_step": 16, "fields": FIELDS, "row_step": w * 16 + 48}
    np.testing.assert_array_equal(check(org, cloud, ANG_V, T, {}), ref)
    # no intensity field: 12-byte x, y, z records; the packed cloud of the same points has intensity 0
    xyz0 = cloud.copy()
    xyz0[:, 3] = 0.0
    noi = {"data": np.ascontiguousarray(cloud[:, :3]).tobytes(), "width": n, "height": 1, "point_step": 12, "fields": {"x": 0, "y": 4, "z": 8}, "row_step": 0}
    np.testing.assert_array_equal(check(noi, xyz0, ANG_V, T, {}), check(packed(xyz0), xyz0, ANG_V, T, {}))
    # fields in another order inside a wider record
    rec = np.zeros((n, 6), dtype=np.float32)
    rec[:, 0], rec[:, 2], rec[:, 3], rec[:, 5] = cloud[:, 3], cloud[:, 2], cloud[:, 0], cloud[:, 1]
    mixed = {"data": rec.tobytes(), "width": n, "height": 1, "point_step": 24, "fields": {"x": 12, "y": 20, "z": 8, "intensity": 0}, "row_step": 0}
    np.testing.assert_array_equal(check(mixed, cloud, ANG_V, T, {}), ref)


@pytest.mark.parametrize("distance", [True, False])
def test_nan_and_inf_returns(street_pair_vlp16, distance):
    cloud = with_nonfinite(street_pair_vlp16[1])
    assert not np.isfinite(cloud).all()
    check(packed(cloud), cloud, ANG_V, base_link(), {"enable_distance_filter": distance})
    check(packed(cloud), cloud, None, base_link(), {"enable_distance_filter": distance, "downsample_resolution": 0.3})


def test_degenerate_scans_behave_like_the_separate_calls(street_pair_vlp16):
    from oracle.replay import small_cloud

    cloud, T = street_pair_vlp16[0], base_link()
    # an empty message: MRGFE_OK and no points, where the reference returns early
    assert check(packed(cloud[:0]), None, ANG_V, T, {}, degenerate=True).shape == (0, 4)
    # every point beyond distance_far_thresh
    assert len(check(packed(cloud), cloud, ANG_V, T, {"distance_near_thresh": 500.0, "distance_far_thresh": 600.0}, degenerate=True)) == 0
    # pcl::VoxelGrid's "leaf size is too small": the cloud passes through the voxel grid (0.01 m leaves over 60 km)
    spread = small_cloud(3000, 3, extent=(30000.0, 30000.0, 30000.0))
    p = {"downsample_resolution": 0.01, "distance_far_thresh": 1e9}
    check(packed(spread), spread, ANG_V, T, p, degenerate=True)
    assert len(check(packed(spread), spread, ANG_V, T, dict(p, outlier_removal_method="NONE"))) == len(spread)
    # one single point, kept by the distance filter and dropped by the radius filter / kept without it
    assert len(check(packed(cloud[:1]), cloud[:1], ANG_V, T, {}, degenerate=True)) == 0
    assert len(check(packed(cloud[:1]), cloud[:1], ANG_V, T, {"outlier_removal_method": "NONE"}, degenerate=True)) == 1
    # nothing but non-finite points
    nan = np.full((50, 4), np.nan, dtype=np.float32)
    assert len(check(packed(nan), nan, ANG_V, T, {}, degenerate=True)) == 0


@pytest.mark.parametrize("cls_name", ["NdtHip", "SmallGicpHip"])
def test_device_form_hands_over_to_the_registration_like_prefilter_device(street_pair_vlp16, cls_name):
    import torch

    import mrg_slam_amd as M
    from mrg_slam_amd import Context, deskew, prefilter, prefilter_to_device, scan_callback_to_device, synth, transform_cloud

    ctx = Context()
    tgt_raw, src_raw, rel = street_pair_vlp16
    T = base_link()
    tgt = prefilter(transform_cloud(tgt_raw, T, ctx=ctx), ctx=ctx)
    guess = synth.warm_guess(rel, 0)
    buf = torch.empty((len(src_raw), 4), dtype=torch.float32, device="cuda:0")
    res, clouds = {}, {}
    for how in ("prefilter_device", "scan_callback_device"):
        reg = getattr(M, cls_name)(transformation_epsilon=0.01, ctx=ctx)
        reg.setInputTarget(tgt)
        buf.zero_()
        torch.cuda.synchronize()
        if how == "prefilter_device":
            m = prefilter_to_device(transform_cloud(deskew(src_raw, ANG_V, PERIOD, ctx=ctx), T, ctx=ctx), buf.data_ptr(), buf.shape[0], ctx=ctx)
        else:
            msg = packed(src_raw)
            m = scan_callback_to_device(msg["data"], msg["width"], 1, 16, FIELDS, buf.data_ptr(), buf.shape[0], 0, ANG_V, PERIOD, T, ctx=ctx)
        reg.setInputSourceFromPrefilter(buf.data_ptr(), m)
        reg.align(guess)
        clouds[how] = buf[:m].cpu().numpy()
        res[how] = (reg.getFinalTransformation().copy(), reg.hasConverged(), reg.getFinalNumIteration(), reg.getFitnessScore())
    np.testing.assert_array_equal(clouds["scan_callback_device"], clouds["prefilter_device"])
    assert len(clouds["scan_callback_device"]) > 100
    np.testing.assert_array_equal(res["scan_callback_device"][0], res["prefilter_device"][0])
    assert res["scan_callback_device"][1:] == res["prefilter_device"][1:]
    assert res["scan_callback_device"][2] >= 1  # (an alignment took place)


def test_results_do_not_depend_on_what_the_context_did_before(street_pair_vlp16):
    from mrg_slam_amd import Context

    a, b = street_pair_vlp16[0], street_pair_vlp16[1]
    T = base_link()
    scans = [a, np.concatenate([a, b, a[::2]]), b[:5000], with_nonfinite(b), a[:2048], a[:2049]]  # larger, then smaller; tile boundaries
    settings = [(ANG_V, T, {}), (None, T, {}), (ANG_V, None, {"downsample_method": "APPROX_VOXELGRID"}), (ANG_V, T, {"enable_distance_filter": False}), (ANG_V, T, {}), (None, None, {})]
    used = Context()
    for k, (s, (av, tf, p)) in enumerate(zip(scans, settings)):
        fresh = one_call(packed(s), av, tf, p, ctx=Context())
        form = (one_call, one_call_device)[k % 2]
        np.testing.assert_array_equal(form(packed(s), av, tf, p, ctx=used), fresh, err_msg=f"scan {k}")
        np.testing.assert_array_equal((one_call_device, one_call)[k % 2](packed(s), av, tf, p, ctx=used), fresh, err_msg=f"scan {k}, the other form")
        np.testing.assert_array_equal(fresh, oracle_chain(s, av, tf, p))
        assert len(fresh) > 100


def test_bad_arguments_are_refused_and_the_context_stays_usable(street_pair_vlp16):
    import torch

    from mrg_slam_amd import Context, _lib

    L = _lib.lib()
    ctx = Context()
    cloud = np.ascontiguousarray(street_pair_vlp16[0])
    n = len(cloud)
    data = cloud.view(np.uint8).reshape(-1).ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.empty((n, 4), dtype=np.float32)
    outp = out.ctypes.data_as(C.POINTER(C.c_float))
    dbuf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    m = C.c_size_t(123)

    def params(**kw):
        p = _lib.ScanParams()
        L.mrgfe_scan_default_params(C.byref(p))
        p.width = n
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    ok = params()
    bad = [(ctx._h, None, data, outp, C.byref(m)), (ctx._h, C.byref(ok), None, outp, C.byref(m)), (ctx._h, C.byref(ok), data, None, C.byref(m)),
           (ctx._h, C.byref(ok), data, outp, None), (None, C.byref(ok), data, outp, C.byref(m))]
    for layout in (params(off_y=6), params(off_intensity=14), params(off_z=16), params(off_intensity=13, point_step=20), params(point_step=18),
                   params(row_step=16 * n - 4), params(point_step=32, row_step=16 * n), params(width=0x10000, height=0x10000)):
        bad.append((ctx._h, C.byref(layout), data, outp, C.byref(m)))
    unknown = params()
    unknown.filters.downsample_method = 7
    bad.append((ctx._h, C.byref(unknown), data, outp, C.byref(m)))
    for args in bad:
        assert L.mrgfe_scan_callback(*args) == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_scan_callback:")
        dev_args = args[:3] + (C.c_void_p(dbuf.data_ptr()) if args[3] is not None else None,) + args[4:]
        assert L.mrgfe_scan_callback_device(*dev_args) == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_scan_callback_device:")
    # a good call afterwards, on the same context
    assert L.mrgfe_scan_callback(ctx._h, C.byref(ok), data, outp, C.byref(m)) == 0
    np.testing.assert_array_equal(out[: m.value], oracle_chain(cloud, None, None, {}))
    assert m.value > 100
