"""GPU: the scan callback to its publish — ``mrgfe_scan_callback_records`` / ``mrgfe_prefilter_records`` / ``mrgfe_cloud_records_device`` (csrc/filters.hip:
pf_records_dd_kernel behind the chain's last stage, in front of its one wait).  The expectation is built here from the existing call,
``pack(scan_callback(...), step)`` with numpy, and every comparison is bit for bit on a uint32 view: the records hold the points, the order and the bits
of ``mrgfe_scan_callback`` for the same inputs.  Destinations are filled with a sentinel and have room for 64 records more than the input has points:
every byte at and beyond ``out_n * step`` is still the sentinel afterwards, in pageable and in page-locked memory."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1
FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
BASE = {"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "downsample_method": "NONE", "downsample_resolution": 0.1,
        "downsample_min_points_per_voxel": 1, "outlier_removal_method": "NONE", "radius_radius": 0.5, "radius_min_neighbors": 2, "statistical_mean_k": 20,
        "statistical_stddev": 1.0}
SENTINEL = 0xA5
SLACK = 64  # records of room beyond the input's point count


def params(**more):
    p = dict(BASE)
    p.update(more)
    return p


def chains(leaf_a=0.1, leaf_b=0.3):
    """the served chains of tests/test_gpu_prefilter_chains.py, and the two with a VOXELGRID in front of an outlier filter"""
    return [("distance filter only", params()),
            ("VOXELGRID", params(downsample_method="VOXELGRID", downsample_resolution=leaf_a)),
            ("VOXELGRID min 2", params(downsample_method="VOXELGRID", downsample_resolution=leaf_b, downsample_min_points_per_voxel=2)),
            ("NONE + RADIUS", params(outlier_removal_method="RADIUS")),
            ("APPROX", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=leaf_a)),
            ("APPROX + RADIUS", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=leaf_a, outlier_removal_method="RADIUS")),
            ("APPROX coarse + RADIUS", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=leaf_b, outlier_removal_method="RADIUS")),
            ("VOXELGRID + RADIUS", params(downsample_method="VOXELGRID", downsample_resolution=leaf_a, outlier_removal_method="RADIUS")),
            ("VOXELGRID + STATISTICAL", params(downsample_method="VOXELGRID", downsample_resolution=leaf_a, outlier_removal_method="STATISTICAL"))]


def pack(cloud, step):
    """the records of a packed cloud, as bytes: 16: the points; 32: x, y, z, 1.0f, intensity, 0, 0, 0 (the pcl::PointXYZI in memory)"""
    c = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4).view(np.uint32)
    if step == 16:
        return c.copy().view(np.uint8).reshape(-1)
    r = np.zeros((len(c), 8), dtype=np.uint32)
    r[:, :3] = c[:, :3]
    r[:, 3] = np.float32(1.0).view(np.uint32)
    r[:, 4] = c[:, 3]
    return r.view(np.uint8).reshape(-1)


def same_records(got, cloud, step, what):
    exp = pack(cloud, step)
    assert got.dtype == np.uint8 and got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), what


class Destination:
    """A sentinel-filled buffer for n_in + SLACK records, pageable or page-locked (mrgfe_pin_host_buffer; unpinned in close())."""

    def __init__(self, ctx, n_in, step, pinned):
        from mrg_slam_amd._lib import lib

        self.ctx, self.step, self.pinned = ctx, step, False
        self.buf = np.full((n_in + SLACK) * step, SENTINEL, dtype=np.uint8)
        assert self.buf.ctypes.data % 16 == 0
        if pinned:
            assert lib().mrgfe_pin_host_buffer(ctx._h, self.buf.ctypes.data_as(C.c_void_p), self.buf.nbytes) == 0
            self.pinned = True

    def untouched_beyond(self, n_bytes):
        return bool((self.buf[n_bytes:] == SENTINEL).all())

    def close(self):
        from mrg_slam_amd._lib import lib

        if self.pinned:
            assert lib().mrgfe_unpin_host_buffer(self.ctx._h, self.buf.ctypes.data_as(C.c_void_p)) == 0
            self.pinned = False


def payload(cloud):
    return memoryview(np.ascontiguousarray(cloud, dtype=np.float32)).cast("B")


def records_of_scan(ctx, cloud, p, step, pinned, dev_ptr=0, ang_v=None, T=None):
    """scan_callback_records of a packed scan into a fresh Destination: (records, prefilter stats, egress stats); the tail is checked here"""
    from mrg_slam_amd import scan_callback_records

    dst = Destination(ctx, len(cloud), step, pinned)
    try:
        got = scan_callback_records(payload(cloud), len(cloud), 1, 16, FIELDS, step, dst.buf, dev_ptr, 0, ang_v, PERIOD, T, p, ctx=ctx)
        ps, es = ctx.prefilter_stats(), ctx.egress_stats()
        assert len(got) == ps["points_out"] * step == es["bytes"], (ps, es, len(got))
        assert dst.untouched_beyond(len(got)), "bytes at or beyond out_n * point_step were written"
        assert es["direct"] == (es["copied"] == 0) or len(got) == 0, es
        return got.copy(), ps, es
    finally:
        dst.close()


@pytest.fixture(scope="module")
def ctx():
    from mrg_slam_amd import Context

    return Context()


@pytest.fixture(scope="module")
def quarter_scan():
    from mrg_slam_amd import synth

    scan = synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 4711)
    return np.ascontiguousarray(scan[::4])


SCAN_CASES = [(f"{name}, distance filter {'on' if dist else 'off'}", dict(p, enable_distance_filter=dist)) for name, p in chains() for dist in (True, False)]


@pytest.fixture(scope="module")
def scan_expected(quarter_scan, ctx):
    """the existing call, once per chain"""
    from mrg_slam_amd import scan_callback

    out = []
    for _, p in SCAN_CASES:
        out.append(scan_callback(payload(quarter_scan), len(quarter_scan), 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx))
        assert ctx.prefilter_stats()["route"] == 1
    return out


def test_a_fresh_context_has_no_egress_statistics():
    from mrg_slam_amd import Context

    assert Context().egress_stats() == {"direct": False, "launches": 0, "waits": 0, "bytes": 0, "copied": 0, "calls": 0}


@pytest.mark.parametrize("which", range(len(SCAN_CASES)), ids=[n for n, _ in SCAN_CASES])
def test_served_chains_write_the_records_inside_their_one_wait(quarter_scan, scan_expected, ctx, which):
    (name, p), exp = SCAN_CASES[which], scan_expected[which]
    assert len(quarter_scan) == 6488 and 0 < len(exp) <= len(quarter_scan)
    for step in (16, 32):
        for pinned in (False, True):
            what = (name, step, pinned)
            calls = ctx.egress_stats()["calls"]
            got, ps, es = records_of_scan(ctx, quarter_scan, p, step, pinned)
            print(what, "out_n", ps["points_out"], es)
            same_records(got, exp, step, what)
            assert ps["points_out"] == len(exp) and ps["route"] == 1 and ps["anomaly"] == 0, (what, ps)
            assert es["waits"] == 0 and es["launches"] == 1 and es["calls"] == calls + 1, (what, es)
            # the caller's page-locked buffer is written by the kernel itself — except behind STATISTICAL, whose records are staged (include/mrgfe.h)
            assert es["direct"] == (pinned and p["outlier_removal_method"] != "STATISTICAL"), (what, es)
            assert es["copied"] == (0 if es["direct"] else len(got)), (what, es)


def remembered(ctx):
    from mrg_slam_amd._lib import lib

    flag, n, box = C.c_int(-1), C.c_size_t(0), np.zeros(6, dtype=np.float32)
    assert lib().mrgfe_dbg_prefilter_output(ctx._h, C.byref(flag), C.byref(n), box.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return bool(flag.value), n.value, box.copy()


@pytest.mark.parametrize("name", ["VOXELGRID + RADIUS", "APPROX", "VOXELGRID + STATISTICAL"])
def test_the_device_cloud_is_what_the_device_form_leaves(quarter_scan, ctx, name):
    """with dev_ptr: the same packed scan as scan_callback_to_device, the same remembered output, and a registration takes it over the same way"""
    import torch

    from mrg_slam_amd import GicpHip, scan_callback, scan_callback_to_device

    p = dict(chains())[name]
    n = len(quarter_scan)
    exp = scan_callback(payload(quarter_scan), n, 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
    guess = np.eye(4, dtype=np.float32)
    guess[0, 3] = 0.05
    res = {}
    for how in ("device", "records", "records pinned"):
        buf = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda:0")
        if how == "device":
            m = scan_callback_to_device(payload(quarter_scan), n, 1, 16, FIELDS, buf.data_ptr(), n, 0, None, PERIOD, None, p, ctx=ctx)
        else:
            got, ps, es = records_of_scan(ctx, quarter_scan, p, 32, how.endswith("pinned"), dev_ptr=buf.data_ptr())
            same_records(got, exp, 32, (name, how))
            assert ps["route"] == 1 and es["waits"] == 0, (ps, es)
            m = ps["points_out"]
        rem = remembered(ctx)
        cloud = buf.cpu().numpy()
        reg = GicpHip(transformation_epsilon=0.01, ctx=ctx)
        reg.setInputTarget(exp)
        reg.setInputSourceFromPrefilter(buf.data_ptr(), m)
        reg.align(guess)
        res[how] = (m, cloud.view(np.uint32).copy(), rem, reg.getFinalTransformation().copy(), reg.hasConverged(), reg.getFinalNumIteration())
    dev = res["device"]
    assert dev[0] == len(exp) and np.array_equal(dev[1][: dev[0]], exp.view(np.uint32)) and dev[2][0] and dev[2][1] == dev[0]
    for how in ("records", "records pinned"):
        r = res[how]
        assert r[0] == dev[0] and np.array_equal(r[1][: r[0]], dev[1][: dev[0]]), how
        assert r[2][0] == dev[2][0] and r[2][1] == dev[2][1] and np.array_equal(r[2][2], dev[2][2]), (how, r[2], dev[2])
        np.testing.assert_array_equal(r[3], dev[3])
        assert r[4:] == dev[4:] and dev[5] >= 1
    # without dev_ptr nothing is remembered
    records_of_scan(ctx, quarter_scan, p, 32, False)
    assert not remembered(ctx)[0]


def test_deskewing_and_a_transform(quarter_scan, ctx):
    from mrg_slam_amd import scan_callback, synth

    T = synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)
    p = dict(chains())["APPROX + RADIUS"]
    exp = scan_callback(payload(quarter_scan), len(quarter_scan), 1, 16, FIELDS, 0, ANG_V, PERIOD, T, p, ctx=ctx)
    assert len(exp) > 500
    for step, pinned in ((32, True), (16, False)):
        got, ps, es = records_of_scan(ctx, quarter_scan, p, step, pinned, ang_v=ANG_V, T=T)
        same_records(got, exp, step, (step, pinned))
        assert ps["route"] == 1 and es["waits"] == 0 and es["direct"] == pinned, (ps, es)


def test_prefilter_records(quarter_scan, ctx):
    import torch

    from mrg_slam_amd import prefilter, prefilter_records

    p = dict(chains())["VOXELGRID + RADIUS"]
    exp = prefilter(quarter_scan, p, ctx=ctx)
    n = len(quarter_scan)
    buf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    for step, pinned, dev in ((32, False, 0), (16, True, buf.data_ptr())):
        dst = Destination(ctx, n, step, pinned)
        try:
            got = prefilter_records(quarter_scan, step, dst.buf, dev, p, ctx=ctx)
            ps, es = ctx.prefilter_stats(), ctx.egress_stats()
            same_records(got, exp, step, (step, pinned))
            assert dst.untouched_beyond(len(got)) and ps["route"] == 1 and ps["points_out"] == len(exp), ps
            assert es["waits"] == 0 and es["direct"] == pinned and es["bytes"] == len(got), es
        finally:
            dst.close()
    assert np.array_equal(buf[: len(exp)].cpu().numpy().view(np.uint32), exp.view(np.uint32)) and remembered(ctx)[0]
    fresh = prefilter_records(quarter_scan, 32, None, 0, p, ctx=ctx)  # (a buffer of the binding's own)
    same_records(fresh, exp, 32, "fresh")


def test_a_byte_aligned_22_byte_layout(quarter_scan):
    """Velodyne's XYZIRT records (x@0 y@4 z@8 intensity@12, ring@16 UINT16, time@18 FLOAT32) on a context with byte layouts on"""
    from mrg_slam_amd import Context, scan_callback, scan_callback_records

    c22 = Context()
    c22.set_byte_layouts(True)
    cloud = quarter_scan[:3001]
    rec = np.zeros(len(cloud), dtype={"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"],
                                      "offsets": [0, 4, 8, 12, 16, 18], "itemsize": 22})
    for k, f in enumerate(("x", "y", "z", "intensity")):
        rec[f] = cloud[:, k]
    rec["ring"], rec["time"] = np.arange(len(cloud)) % 16, np.linspace(0, 0.1, len(cloud), dtype=np.float32)
    data = memoryview(rec.tobytes())
    p = dict(chains())["VOXELGRID + RADIUS"]
    exp = scan_callback(data, len(cloud), 1, 22, FIELDS, 0, ANG_V, PERIOD, None, p, ctx=c22)
    assert len(exp) > 300
    for step, pinned in ((32, True), (16, False)):
        dst = Destination(c22, len(cloud), step, pinned)
        try:
            got = scan_callback_records(data, len(cloud), 1, 22, FIELDS, step, dst.buf, 0, 0, ANG_V, PERIOD, None, p, ctx=c22)
            same_records(got, exp, step, (step, pinned))
            es = c22.egress_stats()
            assert dst.untouched_beyond(len(got)) and c22.prefilter_stats()["route"] == 1 and es["waits"] == 0 and es["direct"] == pinned, es
        finally:
            dst.close()


SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]  # one thread, one block of the record kernel +- 1, a chain tile (2048) +- 1, more than two tiles


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_block_and_a_tile(ctx, n):
    """distance filter off and no other stage: every point comes back, so the LAST record of every size is written and checked; then a chain that drops some"""
    from mrg_slam_amd import scan_callback

    rng = np.random.default_rng(20261020 + n)
    cloud = rng.uniform(-3.0, 3.0, (n, 4)).astype(np.float32)
    for p in (params(enable_distance_filter=False), params(distance_near_thresh=2.0), params(downsample_method="VOXELGRID", downsample_resolution=0.5)):
        exp = scan_callback(payload(cloud), n, 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
        if not p["enable_distance_filter"]:
            assert len(exp) == n
        for step in (16, 32):
            for pinned in (False, True):
                got, ps, es = records_of_scan(ctx, cloud, p, step, pinned)
                same_records(got, exp, step, (n, step, pinned))
                assert ps["route"] == 1 and es["waits"] == 0 and (es["direct"] == pinned or len(exp) == 0), (n, ps, es)


def test_route_0_statistical_behind_none(quarter_scan, ctx):
    from mrg_slam_amd import scan_callback

    cloud = quarter_scan[::2]
    p = params(outlier_removal_method="STATISTICAL")
    exp = scan_callback(payload(cloud), len(cloud), 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 0 and 0 < len(exp) < len(cloud)
    for step, pinned in ((32, False), (32, True), (16, True)):
        got, ps, es = records_of_scan(ctx, cloud, p, step, pinned)
        same_records(got, exp, step, (step, pinned))
        assert ps["route"] == 0 and es["waits"] >= 1 and es["launches"] == 1 and es["direct"] == pinned, (ps, es)


def test_route_2_a_nan_in_front_of_the_radius_filter(ctx):
    import torch

    from mrg_slam_amd import _lib, scan_callback

    rng = np.random.default_rng(7)
    cloud = rng.uniform(-3.0, 3.0, (3000, 4)).astype(np.float32)
    cloud[1234, 1] = np.nan
    p = params(enable_distance_filter=False, outlier_removal_method="RADIUS")
    exp = scan_callback(payload(cloud), len(cloud), 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
    st = ctx.prefilter_stats()
    assert st["route"] == 2 and st["anomaly"] & _lib.PF_ANOMALY_NON_FINITE and 0 < len(exp) < len(cloud), st
    buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
    for step, pinned, dev in ((32, True, 0), (16, False, buf.data_ptr())):
        got, ps, es = records_of_scan(ctx, cloud, p, step, pinned, dev_ptr=dev)
        same_records(got, exp, step, (step, pinned))
        # the device-driven record launch found the anomaly word set and wrote nothing; the one behind the host-driven passes wrote the records
        assert ps["route"] == 2 and ps["anomaly"] & _lib.PF_ANOMALY_NON_FINITE and es["waits"] >= 1 and es["launches"] == 2 and es["direct"] == pinned, (ps, es)
    assert np.array_equal(buf[: len(exp)].cpu().numpy().view(np.uint32), exp.view(np.uint32)) and not remembered(ctx)[0]


def test_an_empty_result_and_an_empty_message(ctx):
    from mrg_slam_amd import scan_callback_records

    cloud = np.full((700, 4), 100.0, dtype=np.float32)  # every point beyond distance_far_thresh
    for p in (params(), params(downsample_method="VOXELGRID", outlier_removal_method="RADIUS")):
        for step, pinned in ((32, True), (16, False)):
            got, ps, es = records_of_scan(ctx, cloud, p, step, pinned)
            assert len(got) == 0 and ps["points_out"] == 0 and es["bytes"] == 0 and es["copied"] == 0, (ps, es)  # (nothing written: records_of_scan's tail check)
    for pinned in (False, True):
        dst = Destination(ctx, 0, 32, pinned)
        try:
            calls = ctx.prefilter_stats()["calls"]
            got = scan_callback_records(memoryview(b""), 0, 1, 16, FIELDS, 32, dst.buf, 0, 0, None, PERIOD, None, params(), ctx=ctx)
            assert len(got) == 0 and dst.untouched_beyond(0) and ctx.prefilter_stats()["calls"] == calls  # (the reference returns early: no chain call)
        finally:
            dst.close()


def test_nan_payload_bits_survive(ctx):
    """no outlier filter, distance filter off: the record kernel copies bits — quiet and signalling NaN payloads, in coordinates and intensity"""
    from mrg_slam_amd import scan_callback

    rng = np.random.default_rng(11)
    cloud = rng.uniform(-3.0, 3.0, (600, 4)).astype(np.float32)
    u = cloud.view(np.uint32)
    u[5, 0], u[17, 3], u[300, 2], u[599, 3] = 0x7FC12345, 0xFFC00001, 0x7F800123, 0x7FABCDEF
    p = params(enable_distance_filter=False)
    exp = scan_callback(payload(cloud), len(cloud), 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
    assert np.array_equal(exp.view(np.uint32), u)  # (the existing call keeps them: the expectation holds the payloads)
    for step in (16, 32):
        for pinned in (False, True):
            got, ps, es = records_of_scan(ctx, cloud, p, step, pinned)
            same_records(got, exp, step, (step, pinned))
            assert ps["route"] == 1 and es["waits"] == 0, (ps, es)
    r32 = pack(exp, 32).view(np.uint32).reshape(-1, 8)
    assert r32[5, 0] == 0x7FC12345 and r32[17, 4] == 0xFFC00001 and r32[300, 2] == 0x7F800123 and r32[599, 4] == 0x7FABCDEF


def test_cloud_records_from_device(quarter_scan, ctx):
    import torch

    from mrg_slam_amd import MrgfeError, cloud_records_from_device, scan_callback, scan_callback_to_device

    p = dict(chains())["VOXELGRID + RADIUS"]
    n = len(quarter_scan)
    exp = scan_callback(payload(quarter_scan), n, 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
    buf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    m = scan_callback_to_device(payload(quarter_scan), n, 1, 16, FIELDS, buf.data_ptr(), n, 0, None, PERIOD, None, p, ctx=ctx)
    assert m == len(exp)
    for step in (16, 32):
        for pinned in (False, True):
            dst = Destination(ctx, m, step, pinned)
            try:
                got = cloud_records_from_device(buf.data_ptr(), m, step, dst.buf, ctx=ctx)
                es = ctx.egress_stats()
                same_records(got, exp, step, (step, pinned))
                assert dst.untouched_beyond(len(got)), (step, pinned)
                assert es == {"direct": pinned, "launches": 1, "waits": 1, "bytes": m * step, "copied": 0 if pinned else m * step, "calls": es["calls"]}, es
            finally:
                dst.close()
    # a host pointer is refused unread, the destination untouched
    host = np.ascontiguousarray(exp)
    dst = Destination(ctx, m, 32, False)
    try:
        with pytest.raises(MrgfeError, match="not in the memory of device") as e:
            cloud_records_from_device(host.ctypes.data, m, 32, dst.buf, ctx=ctx)
        assert e.value.status == -1 and dst.untouched_beyond(0)
    finally:
        dst.close()
    assert len(cloud_records_from_device(buf.data_ptr(), 0, 32, ctx=ctx)) == 0


def test_the_component_returns_the_message(quarter_scan, ctx):
    from mrg_slam_amd.io import xyzi_from_pointcloud2
    from mrg_slam_amd.prefiltering import HipOps, PrefilteringComponent

    comp = PrefilteringComponent({"downsample_resolution": 0.2}, ops=HipOps(ctx), lookup_transform=lambda a, b: np.eye(4, dtype=np.float32))
    cloud = comp.pointcloud2_callback(payload(quarter_scan), len(quarter_scan), 1, 16, FIELDS)  # the default: the packed cloud, as before
    assert isinstance(cloud, np.ndarray) and cloud.shape[1] == 4 and len(cloud) > 100
    for step, off in ((32, 16), (16, 12)):
        msg = comp.pointcloud2_callback(payload(quarter_scan), len(quarter_scan), 1, 16, FIELDS, records=step)
        assert (msg["width"], msg["height"], msg["point_step"], msg["row_step"]) == (len(cloud), 1, step, len(cloud) * step)
        assert msg["fields"] == {"x": 0, "y": 4, "z": 8, "intensity": off} and msg["is_dense"] is False and msg["is_bigendian"] is False
        same_records(msg["data"], cloud, step, step)
        assert np.array_equal(xyzi_from_pointcloud2(msg["data"], msg["width"], 1, step, msg["fields"]).view(np.uint32), cloud.view(np.uint32))
