"""GPU: ``prefiltering/colored_points`` written on the device — ``mrgfe_scan_callback_outputs`` (csrc/filters.hip colored_records_kernel, queued in front
of the chain).  The yardstick is the numpy model of tests/colored_model.py (held by tests/test_colored_model_cpu.py): f64 ``i / n``, ``np.trunc`` and the
byte layout of the ``pcl::PointXYZRGB`` record; every byte of every record is compared.  Destinations are filled with a sentinel and have room for 64
records more than the input has points."""
import ctypes as C

import numpy as np
import pytest

import colored_model as cm

pytestmark = pytest.mark.gpu

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
BASE = {"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "downsample_method": "NONE", "downsample_resolution": 0.1,
        "downsample_min_points_per_voxel": 1, "outlier_removal_method": "NONE", "radius_radius": 0.5, "radius_min_neighbors": 2, "statistical_mean_k": 20,
        "statistical_stddev": 1.0}
VG_RADIUS = dict(BASE, downsample_method="VOXELGRID", outlier_removal_method="RADIUS")
VG_STATISTICAL = dict(BASE, downsample_method="VOXELGRID", outlier_removal_method="STATISTICAL")
NONE_STATISTICAL = dict(BASE, outlier_removal_method="STATISTICAL")  # host-driven passes (route 0) on a context without the statistical-chains switch
SENTINEL = 0xA5
SLACK = 64
SPECIAL = np.array([0x7FC12345, 0x7F812345, 0xFFC00001, 0x7F800000, 0xFF800000], dtype=np.uint32)  # NaNs with payloads (quiet, signalling), +-inf
ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)


def scan_of(n, seed=0):
    """n points a few metres out, with non-finite coordinates written into some of them"""
    rng = np.random.default_rng(100 + seed + n)
    c = np.ascontiguousarray(rng.uniform(-20.0, 20.0, (n, 4)).astype(np.float32))
    u = c.view(np.uint32)
    for k, s in enumerate(SPECIAL):
        if n > 8:
            u[(3 + k * 29) % n, k % 3] = s
    if n == 2:
        u[1, 2] = SPECIAL[0]
    return c


def payload(cloud):
    return memoryview(np.ascontiguousarray(cloud, dtype=np.float32)).cast("B")


def sentinel_buffer(ctx, n, step, pinned):
    from mrg_slam_amd._lib import lib

    buf = np.full((n + SLACK) * step, SENTINEL, dtype=np.uint8)
    assert buf.ctypes.data % 16 == 0
    if pinned:
        assert lib().mrgfe_pin_host_buffer(ctx._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    return buf


def release(ctx, buf, pinned):
    from mrg_slam_amd._lib import lib

    if pinned:
        assert lib().mrgfe_unpin_host_buffer(ctx._h, buf.ctypes.data_as(C.c_void_p)) == 0


def outputs(ctx, data, w, h, step, fields, p, row_step=0, pinned=False, record_step=32, ang_v=None, T=None, records=True):
    """scan_callback_outputs into fresh sentinel buffers: (filtered records, coloured records, prefilter stats, egress stats, second egress stats)"""
    from mrg_slam_amd import scan_callback_outputs

    n = w * h
    out, col = sentinel_buffer(ctx, n, record_step, pinned), sentinel_buffer(ctx, n, 32, pinned)
    try:
        rec, crec, m = scan_callback_outputs(data, w, h, step, fields, record_step, out, col, 0, row_step, ang_v, 0.1, T, p, records=records, ctx=ctx)
        ps, es, e2 = ctx.prefilter_stats(), ctx.egress_stats(), ctx.second_egress_stats()
        assert len(crec) == 32 * n == e2["bytes"], (len(crec), n, e2)
        assert (col[32 * n:] == SENTINEL).all(), "coloured bytes beyond the n records were written"
        if records:
            assert len(rec) == m * record_step and (out[len(rec):] == SENTINEL).all()
        else:
            assert rec is None and (out == SENTINEL).all()
        return (None if rec is None else rec.copy()), crec.copy(), ps, es, e2
    finally:
        release(ctx, out, pinned)
        release(ctx, col, pinned)


def same_bytes(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, "first differing byte", int(bad[0]), "record", int(bad[0]) // 32, "of", bad.size)


@pytest.fixture(scope="module")
def ctx():
    from mrg_slam_amd import Context

    return Context()


@pytest.fixture(scope="module")
def quarter_scan():
    from mrg_slam_amd import synth

    scan = synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 4711)
    return np.ascontiguousarray(scan[::4])


@pytest.mark.parametrize("n", cm.SIZES)
def test_every_byte_of_every_record(ctx, n):
    """a plain 16-byte layout with NaN / Inf points, deskewing and a transform on: the colours are those of the cloud as it was unpacked"""
    from mrg_slam_amd import scan_callback_records

    cloud = scan_of(n)
    exp = cm.colored_records(cloud.view(np.uint32)[:, :3])
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.5, -1.0, 0.25]
    filtered = scan_callback_records(payload(cloud), n, 1, 16, FIELDS, 32, None, 0, 0, ANG_V, 0.1, T, BASE, ctx=ctx).copy()
    for pinned in (False, True):
        rec, crec, ps, es, e2 = outputs(ctx, payload(cloud), n, 1, 16, FIELDS, BASE, pinned=pinned, ang_v=ANG_V, T=T)
        same_bytes(crec, exp, (n, pinned))
        assert np.array_equal(rec, filtered), (n, pinned)
        assert ps["route"] == 1 and es["waits"] == 0 and e2["waits"] == 0 and e2["launches"] == 1 and e2["direct"] == pinned, (ps, es, e2)
        assert e2["copied"] == (0 if pinned else 32 * n)


def test_organised_message_with_padded_rows(ctx):
    w, h, row_step = 301, 2, 301 * 16 + 16
    cloud = scan_of(w * h, seed=1)
    data = np.random.default_rng(5).integers(0, 256, row_step + w * 16, dtype=np.uint8)
    for r in range(h):
        data[r * row_step: r * row_step + w * 16] = cloud[r * w: (r + 1) * w].view(np.uint8).reshape(-1)
    _, crec, ps, _, e2 = outputs(ctx, data.tobytes(), w, h, 16, FIELDS, BASE, row_step=row_step)
    same_bytes(crec, cm.colored_records(cloud.view(np.uint32)[:, :3]), "height 2")
    assert ps["route"] == 1 and e2["waits"] == 0


def test_byte_aligned_xyzirt_records():
    """Velodyne's 22-byte points on a context with byte layouts on: the colour kernel reads them as the scan's head kernel does"""
    from mrg_slam_amd import Context

    c = Context()
    c.set_byte_layouts(True)
    n = 777
    cloud = scan_of(n, seed=2)
    rec_t = np.dtype({"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"], "offsets": [0, 4, 8, 12, 16, 18], "itemsize": 22})
    data = np.random.default_rng(6).integers(0, 256, n * 22, dtype=np.uint8)
    rows = data.view(rec_t)
    for k, f in enumerate(("x", "y", "z", "intensity")):
        rows[f] = cloud[:, k]
    fields = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1), ("ring", 16, 4, 1), ("time", 18, 7, 1)]
    _, crec, ps, _, e2 = outputs(c, data.tobytes(), n, 1, 22, fields, BASE)
    same_bytes(crec, cm.colored_records(cloud.view(np.uint32)[:, :3]), "22-byte records")
    assert ps["route"] == 1 and e2["waits"] == 0


def test_without_colored_records_the_call_is_scan_callback_records(quarter_scan):
    """two fresh contexts, the same input: output, prefilter statistics and egress statistics are equal"""
    from mrg_slam_amd import Context, scan_callback_outputs, scan_callback_records

    n = len(quarter_scan)
    for p in (VG_RADIUS, VG_STATISTICAL, NONE_STATISTICAL):
        a, b = Context(), Context()
        ra = scan_callback_records(payload(quarter_scan), n, 1, 16, FIELDS, 32, None, 0, 0, ANG_V, 0.1, None, p, ctx=a)
        rb, col, m = scan_callback_outputs(payload(quarter_scan), n, 1, 16, FIELDS, 32, None, None, 0, 0, ANG_V, 0.1, None, p, colored=False, ctx=b)
        assert col is None and m * 32 == len(rb) and np.array_equal(ra, rb)
        assert a.prefilter_stats() == b.prefilter_stats() and a.egress_stats() == b.egress_stats()
        assert b.second_egress_stats() == {"direct": False, "launches": 0, "waits": 0, "bytes": 0, "copied": 0, "calls": 0}


@pytest.mark.parametrize("name, p, route", [("VOXELGRID + RADIUS", VG_RADIUS, 1), ("VOXELGRID + STATISTICAL", VG_STATISTICAL, 1), ("NONE + STATISTICAL", NONE_STATISTICAL, 0)])
def test_colouring_leaves_the_filtered_records_and_the_waits_alone(ctx, quarter_scan, name, p, route):
    from mrg_slam_amd import scan_callback_records

    n = len(quarter_scan)
    exp_col = cm.colored_records(quarter_scan.view(np.uint32)[:, :3])
    filtered = scan_callback_records(payload(quarter_scan), n, 1, 16, FIELDS, 32, None, 0, 0, ANG_V, 0.1, None, p, ctx=ctx).copy()
    es0 = ctx.egress_stats()
    assert ctx.prefilter_stats()["route"] == route and 0 < len(filtered) < 32 * n
    got = {}
    for pinned in (False, True):
        rec, crec, ps, es, e2 = outputs(ctx, payload(quarter_scan), n, 1, 16, FIELDS, p, pinned=pinned, ang_v=ANG_V)
        print(name, "pinned" if pinned else "pageable", ps, es, e2)
        assert np.array_equal(rec, filtered) and ps["points_out"] * 32 == len(filtered) and ps["route"] == route, (name, pinned, ps)
        same_bytes(crec, exp_col, (name, pinned))
        # the filtered records' stage is the one of the call without colours (a route-1 STATISTICAL chain's stay staged through the first pinned buffer)
        assert (es["waits"], es["launches"]) == (es0["waits"], es0["launches"]), (es, es0)
        assert es["direct"] == (pinned and not (route == 1 and p["outlier_removal_method"] == "STATISTICAL")), es
        # the colour stage: its own destination, and on the one-wait route no wait of its own — the call's stream waits are still 1
        assert e2["direct"] == pinned and e2["launches"] == 1 and e2["waits"] == (0 if route == 1 else 1), e2
        got[pinned] = crec
    assert np.array_equal(got[False], got[True])


def test_coloured_records_alone_and_beside_a_device_cloud(ctx, quarter_scan):
    import torch

    from mrg_slam_amd import scan_callback_outputs, scan_callback_to_device

    n = len(quarter_scan)
    exp_col = cm.colored_records(quarter_scan.view(np.uint32)[:, :3])
    before = ctx.prefilter_stats()
    rec, crec, ps, _, e2 = outputs(ctx, payload(quarter_scan), n, 1, 16, FIELDS, VG_RADIUS, records=False)
    same_bytes(crec, exp_col, "alone")
    assert ps == before and e2["waits"] == 1  # (no chain ran)
    a = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda:0")
    b = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda:0")
    m = scan_callback_to_device(payload(quarter_scan), n, 1, 16, FIELDS, a.data_ptr(), n, 0, None, 0.1, None, VG_RADIUS, ctx=ctx)
    _, crec, mb = scan_callback_outputs(payload(quarter_scan), n, 1, 16, FIELDS, 32, None, None, b.data_ptr(), 0, None, 0.1, None, VG_RADIUS, records=False, ctx=ctx)
    same_bytes(crec, exp_col, "beside the device cloud")
    assert mb == m and torch.equal(a[:m].view(torch.int32), b[:m].view(torch.int32)) and ctx.second_egress_stats()["waits"] == 0


def raw_call(ctx, cloud, w, outs):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.filters import _scan_params

    q = _scan_params(w, 1, 16, FIELDS, 0, None, 0.1, None, BASE, ctx)
    m, mc = C.c_size_t(99), C.c_size_t(99)
    data = np.frombuffer(payload(cloud), dtype=np.uint8) if len(cloud) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().mrgfe_scan_callback_outputs(ctx._h, C.byref(q), data.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(outs) if outs is not None else None, C.byref(m), C.byref(mc))
    return rc, m.value, mc.value


def test_refusals_write_nothing(ctx):
    from mrg_slam_amd import _lib

    n = 300
    cloud = scan_of(n)
    rec, col = np.full(n * 32, SENTINEL, dtype=np.uint8), np.full(n * 32, SENTINEL, dtype=np.uint8)
    calls = ctx.prefilter_stats()["calls"]

    def outs(**kw):
        o = _lib.ScanOutputs()
        o.point_step, o.records, o.capacity_bytes, o.colored_records, o.colored_capacity_bytes = 32, rec.ctypes.data, rec.nbytes, col.ctypes.data, col.nbytes
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = {"coloured capacity one byte short": outs(colored_capacity_bytes=32 * n - 1),
             "neither records nor coloured records": outs(records=None, colored_records=None),
             "a refusal of scan_callback_records: point_step 24": outs(point_step=24),
             "a refusal of scan_callback_records: capacity short": outs(capacity_bytes=32 * n - 1)}
    for what, o in cases.items():
        rc, m, mc = raw_call(ctx, cloud, n, o)
        assert rc == _lib.ERR_INVALID and mc == 0, (what, rc, _lib.last_error())
        assert (rec == SENTINEL).all() and (col == SENTINEL).all(), what
    assert raw_call(ctx, cloud, n, None)[0] == _lib.ERR_INVALID
    assert ctx.prefilter_stats()["calls"] == calls  # nothing was launched
    rc, m, mc = raw_call(ctx, cloud, n, outs())  # and the same buffers are accepted as they are
    assert rc == 0 and mc == n and 0 < m <= n


def test_an_empty_message(ctx):
    from mrg_slam_amd import _lib

    rec, col = np.full(64, SENTINEL, dtype=np.uint8), np.full(64, SENTINEL, dtype=np.uint8)
    o = _lib.ScanOutputs()
    o.point_step, o.records, o.capacity_bytes, o.colored_records, o.colored_capacity_bytes = 32, rec.ctypes.data, rec.nbytes, col.ctypes.data, col.nbytes
    rc, m, mc = raw_call(ctx, np.zeros((0, 4), dtype=np.float32), 0, o)
    assert (rc, m, mc) == (0, 0, 0) and (rec == SENTINEL).all() and (col == SENTINEL).all()
