"""GPU: ``mrgfe_floor_callback`` — FloorDetectionComponent::cloud_callback (apps/floor_detection_component.cpp:69-93) in one call on the bytes of the
sensor_msgs/PointCloud2 — against the composed route on the same context: ``mrgfe_ingest_pointcloud2`` into a device buffer, then
``mrgfe_floor_detect_device``.  Result record, floor_filtered_points and floor_points are compared as bytes; every ``reason`` is reached once on both
routes; the accepted plane is also held against the restatement of detect() in tests/floor_reference.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import floor_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
U16, F32 = 4, 7  # sensor_msgs/PointField datatypes
PACKED = {"x": 0, "y": 4, "z": 8, "intensity": 12}
V22 = [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1), ("ring", 16, U16, 1), ("time", 18, F32, 1)]  # the Velodyne driver's XYZIRT
T18 = [("ring", 0, U16, 1), ("x", 2, F32, 1), ("y", 6, F32, 1), ("z", 10, F32, 1), ("intensity", 14, F32, 1)]  # every field straddles; the intensity ends the record
THRESH = 64  # floor_pts_thresh of every case here: the clouds are small
_fp = C.POINTER(C.c_float)


def floor_cloud(n, seed, walls=True):
    """A seeded synthetic floor seen from a sensor 2 m above it: a plane with 1 cm noise and, with ``walls``, two walls (a fifth of the points) that
    reach through the height band.  A few records have NaN coordinates."""
    rng = np.random.default_rng(seed)
    m = n - n // 5 if walls and n >= 10 else n
    c = np.zeros((n, 4), f32)
    c[:m, 0], c[:m, 1] = rng.uniform(-8, 8, m), rng.uniform(-8, 8, m)
    c[:m, 2] = -2.0 + rng.normal(scale=0.01, size=m)
    w = n - m
    if w:
        half = w // 2
        c[m: m + half, 0], c[m: m + half, 1] = 8.0 + rng.normal(scale=0.01, size=half), rng.uniform(-8, 8, half)
        c[m + half:, 0], c[m + half:, 1] = rng.uniform(-8, 8, w - half), -8.0 + rng.normal(scale=0.01, size=w - half)
        c[m:, 2] = rng.uniform(-2.0, 0.5, w)
    c[:, 3] = rng.uniform(0, 255, n)
    c = c[rng.permutation(n)]
    if n > 16:
        c[5, 0] = c[11, 2] = c[n - 2, 1] = np.nan
    return c


def records(cloud, fields, point_step, width=None, row_step=0, seed=0):
    """The cloud as a PointCloud2 message (dict) of the given FLOAT32 field offsets: ``fields`` a {name: offset} dict or a PointField list; every byte
    the fields do not cover is random."""
    n = len(cloud)
    w = n if width is None else width
    h = n // w if w else 1
    assert w * h == n
    rs = row_step or w * point_step
    raw = ((h - 1) * rs + w * point_step) if n else 0
    data = np.random.default_rng(1000 + seed + n).integers(0, 256, raw, dtype=np.uint8)
    offs = fields if isinstance(fields, dict) else {f[0]: f[1] for f in fields if f[2] == F32 and f[0] in PACKED}
    src = cloud.view(np.uint8).reshape(n, 16)
    for i in range(n):
        at = (i // w) * rs + (i % w) * point_step
        for k, name in enumerate(("x", "y", "z", "intensity")):
            if offs.get(name) is not None:
                data[at + offs[name]: at + offs[name] + 4] = src[i, 4 * k: 4 * k + 4]
    return {"data": data.tobytes(), "width": w, "height": h, "point_step": point_step, "row_step": row_step, "fields": fields}


def pcl32(cloud):
    from mrg_slam_amd.io import pcl_xyzi_records

    return {"data": pcl_xyzi_records(cloud).tobytes(), "width": len(cloud), "height": 1, "point_step": 32, "row_step": 0, "fields": {"x": 0, "y": 4, "z": 8, "intensity": 16}}


def both_routes(ctx, msg, **params):
    """(one call on the bytes, ingest to the device followed by detect_device) on the same context: two FloorRecords with the raw result records and
    the two wait counts."""
    import torch

    from mrg_slam_amd import FloorDetection
    from mrg_slam_amd.io import ingest_pointcloud2

    params.setdefault("floor_pts_thresh", THRESH)
    n = msg["width"] * msg["height"]
    one, two = FloorDetection(ctx=ctx, **params), FloorDetection(ctx=ctx, **params)
    one.detect_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"])
    waits_one = one.stage_times()["host_waits"]
    buf = torch.empty((max(n, 1), 4), dtype=torch.float32, device="cuda")
    if n:
        ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ctx=ctx, dev_ptr=buf.data_ptr())
    two.detect_device(buf.data_ptr(), n)
    waits_two = two.stage_times()["host_waits"]
    return one.last, two.last, waits_one, waits_two


def assert_same(a, b, what=""):
    for f in ("found", "reason", "n_clipped", "n_filtered", "n_inliers", "iterations", "skipped"):
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))
    assert (a.coeffs is None) == (b.coeffs is None) and (a.coeffs is None or a.coeffs.tobytes() == b.coeffs.tobytes()), what
    assert a.filtered.shape == b.filtered.shape and a.filtered.tobytes() == b.filtered.tobytes(), what
    assert (a.inliers is None) == (b.inliers is None) and (a.inliers is None or a.inliers.tobytes() == b.inliers.tobytes()), what


@pytest.fixture(scope="module")
def ctx():
    from mrg_slam_amd import Context

    return Context()


@pytest.fixture(scope="module")
def ctx_bytes():
    from mrg_slam_amd import Context

    c = Context()
    c.set_byte_layouts(True)
    return c


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049])
def test_bit_equal_at_the_workgroup_edges(ctx, n):
    cloud = floor_cloud(n, seed=n)
    for name, msg in (("packed", records(cloud, PACKED, 16)), ("pcl32", pcl32(cloud)), ("no intensity", records(cloud, {"x": 4, "y": 8, "z": 0}, 12, seed=3))):
        a, b, wa, wb = both_routes(ctx, msg)
        assert_same(a, b, (name, n))
        assert wa == wb >= 1, (name, n, wa, wb)  # the upload adds no wait
        assert a.reason == ("found" if n >= 255 else "too_few_filtered"), (name, n, a.reason)
    # the raw result record, reserved word included
    import torch

    from mrg_slam_amd import _lib
    from mrg_slam_amd.floor_detection import _params

    msg = records(cloud, PACKED, 16)
    q, r1, r2 = _params(dict(_defaults(), floor_pts_thresh=THRESH)), _lib.FloorResult(), _lib.FloorResult()
    lay = _layout(msg, ctx)
    buf = np.frombuffer(msg["data"], dtype=np.uint8)
    _lib.check(_lib.lib().mrgfe_floor_callback(ctx._h, C.byref(q), C.byref(lay), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(r1), None, None))  # NULL outputs are accepted
    dev = torch.from_numpy(cloud.copy()).cuda()
    _lib.check(_lib.lib().mrgfe_floor_detect_device(ctx._h, C.byref(q), C.c_void_p(dev.data_ptr()), n, C.byref(r2), None, None))
    assert bytes(r1) == bytes(r2)


def _defaults():
    from mrg_slam_amd.floor_detection import DEFAULTS

    return dict(DEFAULTS)


def _layout(msg, ctx):
    from mrg_slam_amd.io import layout_from_fields

    lay, _ = layout_from_fields(msg["fields"], msg["width"], msg["height"], msg["point_step"], msg["row_step"], ctx=ctx)
    return lay


def test_organised_message_with_padded_rows(ctx):
    cloud = floor_cloud(4 * 600, seed=21)
    msg = records(cloud, {"x": 0, "y": 4, "z": 8, "intensity": 16}, 20, width=600, row_step=600 * 20 + 12)
    a, b, wa, wb = both_routes(ctx, msg)
    assert_same(a, b)
    assert a.found and wa == wb
    # ... and the cloud the message stands for gives the same through the packed layout
    c, _, _, _ = both_routes(ctx, records(cloud, PACKED, 16))
    assert_same(a, c)


@pytest.mark.parametrize("fields,step", [(V22, 22), (T18, 18)], ids=["V22", "T18"])
@pytest.mark.parametrize("n", [3, 257])
def test_byte_aligned_records(ctx, ctx_bytes, fields, step, n):
    """22-byte XYZIRT records (every other record starts 2 bytes into a word) and 18-byte records whose last field straddles the payload's last word: the
    reader takes that word and nothing behind it."""
    from mrg_slam_amd import MrgfeError

    cloud = floor_cloud(n, seed=30 + n)
    msg = records(cloud, fields, step, seed=step)
    a, b, wa, wb = both_routes(ctx_bytes, msg)
    assert_same(a, b, (step, n))
    assert wa == wb and a.reason == ("found" if n >= 255 else "too_few_filtered")
    c, _, _, _ = both_routes(ctx_bytes, records(cloud, PACKED, 16))  # the strict instantiation on the same cloud
    assert_same(a, c, (step, n))
    # with byte layouts off the layout is refused (a {name: offset} dict switches nothing)
    from mrg_slam_amd import FloorDetection

    offs = {f[0]: f[1] for f in fields if f[0] in PACKED}
    with pytest.raises(MrgfeError, match="mrgfe_floor_callback") as e:
        FloorDetection(ctx=ctx).detect_pointcloud2(msg["data"], n, 1, step, offs)
    assert e.value.status == -1


@pytest.fixture(scope="module")
def street_floor():
    return floor_cloud(3750, seed=20251019)  # 3000 floor points and two walls


def tilted(cloud, deg):
    """The scan as a sensor pitched by ``deg`` sees it: rows R^T p, as tests/test_gpu_floor.py builds it."""
    R, _ = fr.tilt_rotations(deg)
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ R.astype(np.float64)).astype(f32)
    return out


def _plane_close(a, b, deg=0.5, dist=0.02):  # the tolerance of tests/test_gpu_floor.py::_plane_close
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ang = math.degrees(math.acos(min(1.0, abs(float(np.dot(a[:3], b[:3])) / (np.linalg.norm(a[:3]) * np.linalg.norm(b[:3]))))))
    return ang <= deg and abs(a[3] - b[3]) <= dist


@pytest.mark.parametrize("tilt", [0.0, 5.0])
def test_found_on_both_routes_and_against_the_restatement(ctx, street_floor, tilt):
    cloud = tilted(street_floor, tilt) if tilt else street_floor
    a, b, wa, wb = both_routes(ctx, pcl32(cloud), tilt_deg=tilt)
    assert_same(a, b)
    assert a.reason == "found" and wa == wb >= 3
    ref = fr.detect(cloud, {"tilt_deg": tilt, "floor_pts_thresh": THRESH})
    assert ref["found"] and _plane_close(a.coeffs, ref["coeffs"]), (a.coeffs, ref["coeffs"])
    # records with NaN coordinates are dropped by the band on both routes
    assert np.isnan(cloud[:, :3]).any() and a.n_clipped == ref["n_clipped"] and np.isfinite(a.filtered).all()
    assert a.n_inliers >= 2500 and abs(float(a.coeffs[3]) - 2.0) < 0.05  # most of the 3000 floor points, 2 m under the sensor


def test_every_other_reason_once(ctx, street_floor):
    rng = np.random.default_rng(77)
    wall = np.zeros((800, 4), f32)
    wall[:, 0], wall[:, 1], wall[:, 2] = 5.0 + rng.normal(scale=0.01, size=800), rng.uniform(-6, 6, 800), rng.uniform(-2.9, -1.1, 800)
    scatter = np.zeros((300, 4), f32)
    scatter[:, :3] = rng.uniform([-20, -20, -4.9], [20, 20, 0.9], (300, 3))
    sky = street_floor.copy()
    sky[:, 2] += 10.0
    two = street_floor[np.abs(street_floor[:, 2] + 2.0) < 0.1][:2]  # two points of the floor
    cases = [
        ("empty_input", np.zeros((0, 4), f32), {}),
        ("none_after_clip", sky, {}),
        ("too_few_filtered", floor_cloud(50, seed=5, walls=False), {}),
        ("too_few_inliers", scatter, {"use_normal_filtering": False, "height_clip_range": 3.0}),
        ("not_vertical", wall, {"use_normal_filtering": False}),
        ("no_model", two, {"use_normal_filtering": False, "floor_pts_thresh": 1}),
    ]
    for reason, cloud, params in cases:
        a, b, wa, wb = both_routes(ctx, records(cloud, PACKED, 16), **params)
        assert_same(a, b, reason)
        assert a.reason == b.reason == reason and not a.found, (reason, a.reason, b.reason)
        assert wa == wb, (reason, wa, wb)
    # the empty message: no wait at all, and the component publishes nothing (:74-77)
    a, _, wa, _ = both_routes(ctx, records(np.zeros((0, 4), f32), PACKED, 16))
    assert wa == 0 and a.n_clipped == 0
    from mrg_slam_amd import FloorDetectionComponent

    comp = FloorDetectionComponent({"floor_pts_thresh": THRESH})
    assert comp.pointcloud2_callback(records(np.zeros((0, 4), f32), PACKED, 16)) is None
    assert comp.pointcloud2_callback(records(sky, PACKED, 16)) == []
    got = comp.pointcloud2_callback(pcl32(street_floor))
    assert len(got) == 4 and got == comp.cloud_callback(street_floor)


def test_refusals_leave_the_context_usable(ctx, street_floor):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.floor_detection import _params

    L = _lib.lib()
    good = pcl32(street_floor)
    want, _, _, _ = both_routes(ctx, good)
    q = _params(dict(_defaults(), floor_pts_thresh=THRESH))
    buf = np.frombuffer(good["data"], dtype=np.uint8)
    n = len(street_floor)

    def call(lay, data, nbytes):
        r = _lib.FloorResult()
        filt, inl = np.full((n, 4), 7.0, f32), np.full((n, 4), 7.0, f32)
        st = L.mrgfe_floor_callback(ctx._h, C.byref(q), C.byref(lay), data, nbytes, C.byref(r), filt.ctypes.data_as(_fp), inl.ctypes.data_as(_fp))
        return st, r, filt, inl

    lay = _layout(good, ctx)
    bad_row = _layout(good, ctx)
    bad_row.row_step = n * 32 - 4  # does not hold a row
    unaligned = _layout(good, ctx)
    unaligned.off_intensity = 17  # not a multiple of 4, byte layouts off on this context
    for what, args in (("short payload", (lay, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 1)), ("row_step", (bad_row, buf.ctypes.data_as(C.c_void_p), buf.nbytes)),
                       ("NULL data", (lay, None, buf.nbytes)), ("offset", (unaligned, buf.ctypes.data_as(C.c_void_p), buf.nbytes))):
        st, r, filt, inl = call(*args)
        assert st == -1 and "mrgfe_floor_callback" in _lib.last_error(), (what, st, _lib.last_error())
        assert (filt == 7.0).all() and (inl == 7.0).all(), what  # a failing call leaves nothing behind
        after, _, _, _ = both_routes(ctx, good)  # ... and the next good call on the context gives the right result
        assert_same(after, want, what)


def test_the_two_existing_entry_points_still_agree(ctx, street_floor):
    """The refactor's guard: mrgfe_floor_detect on the host cloud and mrgfe_floor_detect_device on the same cloud in device memory, against each other
    (as tests/test_gpu_floor.py::test_device_input_matches_host_input) and against the restatement's stage counts."""
    import torch

    from mrg_slam_amd import FloorDetection

    dev = torch.from_numpy(street_floor.copy()).cuda()
    a, b = FloorDetection(ctx=ctx, floor_pts_thresh=THRESH), FloorDetection(ctx=ctx, floor_pts_thresh=THRESH)
    ga, gb = a.detect_device(dev.data_ptr(), len(street_floor)), b.detect(street_floor)
    assert a.last.found and ga.tobytes() == gb.tobytes()
    assert_same(a.last, b.last)
    assert a.stage_times()["host_waits"] >= 3
    ref = fr.detect(street_floor, {"floor_pts_thresh": THRESH})
    assert a.last.n_clipped == ref["n_clipped"] and _plane_close(ga, ref["coeffs"])
