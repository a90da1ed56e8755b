"""CPU: the scan callback's C structure and defaults (no GPU is needed to fill them), and the component's routing — point operations that
offer ``scan`` get exactly one call per scan, with the IMU queue consumed as on the three-call route."""
import ctypes as C

import numpy as np


def test_scan_default_params_and_struct_size():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    assert C.sizeof(_lib.ScanParams) == L.mrgfe_scan_params_size() == 200
    assert _lib.ScanParams.filters.offset == 128 and _lib.ScanParams.scan_period.offset == 48 and _lib.ScanParams.T.offset == 60
    p = _lib.ScanParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    L.mrgfe_scan_default_params(C.byref(p))
    # the packed 16-byte layout of the replay scripts, one row; the caller fills in the width
    assert (p.width, p.height, p.point_step, p.row_step) == (0, 1, 16, 0)
    assert (p.off_x, p.off_y, p.off_z, p.off_intensity) == (0, 4, 8, 12)
    # no deskewing, no transform
    assert p.deskew == 0 and list(p.ang_v) == [0.0, 0.0, 0.0] and p.scan_period == 0.1
    assert p.transform == 0 and list(p.T) == list(np.eye(4, dtype=np.float32).reshape(16))
    # mrgfe_prefilter_default_params
    q = _lib.PrefilterParams()
    L.mrgfe_prefilter_default_params(C.byref(q))
    assert bytes(p.filters) == bytes(q)
    f = p.filters
    assert (f.enable_distance_filter, f.distance_near_thresh, f.distance_far_thresh) == (1, 0.1, 35.0)
    assert (f.downsample_method, f.downsample_resolution, f.downsample_min_points_per_voxel) == (1, 0.1, 1)
    assert (f.outlier_removal_method, f.radius_radius, f.radius_min_neighbors, f.statistical_mean_k, f.statistical_stddev) == (1, 0.5, 2, 30, 1.2)
    L.mrgfe_scan_default_params(None)  # a NULL pointer is ignored, like its neighbours


def test_scan_wrappers_refuse_a_short_payload_before_the_library_sees_it():
    import pytest

    from mrg_slam_amd import scan_callback, scan_callback_to_device

    class NoCtx:  # the check comes first: nothing of the context is touched
        pass

    fields = {"x": 0, "y": 4, "z": 8, "intensity": 12}
    with pytest.raises(ValueError, match="payload has 160 bytes"):
        scan_callback(bytes(160), 11, 1, 16, fields, ctx=NoCtx())
    with pytest.raises(ValueError, match="payload has 160 bytes"):
        scan_callback_to_device(bytes(160), 4, 3, 16, fields, 0x1000, 12, row_step=80, ctx=NoCtx())
    with pytest.raises(ValueError, match="device buffer too small"):
        scan_callback_to_device(bytes(160), 10, 1, 16, fields, 0x1000, 9, ctx=NoCtx())


def _scan(n, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), dtype=np.float32)
    c[:, :3] = rng.normal(0, 8.0, (n, 3)) * [1.0, 1.0, 0.15]
    c[:, 3] = rng.uniform(0, 255, n)
    return c


def test_component_makes_one_scan_call_per_scan_and_consumes_the_imu_queue_identically():
    from mrg_slam_amd import synth
    from mrg_slam_amd.prefiltering import OracleOps, PrefilteringComponent
    from oracle import oracle as orc

    calls = []

    class Recording(OracleOps):
        def deskew(self, cloud, ang_v, scan_period):
            calls.append("deskew")
            return super().deskew(cloud, ang_v, scan_period)

        def transform(self, cloud, T):
            calls.append("transform")
            return super().transform(cloud, T)

        def filters(self, cloud, p):
            calls.append("filters")
            return super().filters(cloud, p)

    class Fused(Recording):
        """The whole callback as one operation, made of the oracle's steps."""

        def scan(self, cloud, ang_v, scan_period, T, p):
            calls.append(("scan", None if ang_v is None else np.asarray(ang_v).copy()))
            c = cloud if ang_v is None else OracleOps.deskew(self, cloud, ang_v, scan_period)
            c = c if T is None else OracleOps.transform(self, c, T)
            return OracleOps.filters(self, c, p)

    T = synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)
    scans = [_scan(3000, 1), _scan(4000, 2), _scan(2500, 3)]
    params = {"enable_deskewing": True, "downsample_resolution": 0.2}

    def drive(ops):
        calls.clear()
        c = PrefilteringComponent(params, ops=ops, lookup_transform=lambda a, b: T)
        outs, queues = [], []
        outs.append(c.cloud_callback(scans[0], stamp=0.05, frame_id="velodyne"))  # no IMU message yet: not deskewed
        queues.append([s for s, _ in c.imu_queue])
        for k in range(6):
            c.imu_callback(0.5 + 0.2 * k, [0.1 * k, -0.2, 0.3])  # stamps 0.5 ... 1.5
        outs.append(c.cloud_callback(scans[1], stamp=1.0, frame_id="velodyne"))  # the message of stamp 1.1; the three before it leave
        queues.append([s for s, _ in c.imu_queue])
        outs.append(c.cloud_callback(scans[2], stamp=9.0, frame_id="velodyne"))  # none newer: the last one, the queue is emptied
        queues.append([s for s, _ in c.imu_queue])
        return outs, queues, list(calls)

    three_out, three_q, three_calls = drive(Recording(orc))
    one_out, one_q, one_calls = drive(Fused(orc))
    assert three_calls == ["transform", "filters", "deskew", "transform", "filters", "deskew", "transform", "filters"]
    assert [c[0] for c in one_calls] == ["scan", "scan", "scan"]  # one call per scan, none of the separate ones
    assert one_calls[0][1] is None and one_calls[1][1][0] == np.float32(0.3) and one_calls[2][1][0] == np.float32(0.5)
    assert one_q == three_q and three_q[1] == [0.5 + 0.2 * k for k in (3, 4, 5)] and three_q[2] == []
    for a, b in zip(one_out, three_out):
        np.testing.assert_array_equal(a, b)
        assert len(a) > 100

    # the early returns are the same on both routes, and the IMU queue is consumed before the transform is looked up (:125 before :129-138)
    def no_tf(target, source):
        raise RuntimeError("no transform")

    for ops in (Recording(orc), Fused(orc)):
        calls.clear()
        c = PrefilteringComponent(params, ops=ops, lookup_transform=no_tf)
        assert c.cloud_callback(np.zeros((0, 4), np.float32)) is None and calls == []
        c.imu_callback(0.1, [0, 0, 1])
        c.imu_callback(0.3, [0, 0, 2])
        assert c.cloud_callback(scans[0], stamp=0.2, frame_id="velodyne") is None
        assert [s for s, _ in c.imu_queue] == [0.3] and "filters" not in calls and not [x for x in calls if x[0] == "scan"]
