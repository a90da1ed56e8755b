"""CPU: what ``mrgfe_floor_callback`` and ``mrgfe_keyframe_callback_device`` refuse before they need a context, a store or a device, and the routing and
argument marshalling of their Python wrappers over recording fakes — the component mirrors make exactly one call per message or device cloud, with the
same decisions as their host-cloud / message forms."""
import ctypes as C

import numpy as np
import pytest

_fp = C.POINTER(C.c_float)
FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}


def _layout(width, height=1, point_step=16, row_step=0, offs=(0, 4, 8, 12)):
    from mrg_slam_amd import _lib

    return _lib.KeyframeParams(width, height, point_step, row_step, offs[0], offs[1], offs[2], offs[3])


def test_floor_callback_refusals_need_no_context():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    q, r = _lib.FloorParams(), _lib.FloorResult()
    L.mrgfe_floor_default_params(C.byref(q))
    data = np.zeros(160, dtype=np.uint8)
    vp = data.ctypes.data_as(C.c_void_p)

    def refused(lay, d, nbytes, says, params=q):
        st = L.mrgfe_floor_callback(None, C.byref(params) if params is not None else None, C.byref(lay) if lay is not None else None, d, nbytes, C.byref(r), None, None)
        assert st == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_floor_callback:") and says in _lib.last_error(), (st, _lib.last_error())

    refused(None, vp, 160, "NULL argument")
    refused(_layout(10), vp, 160, "NULL argument", params=None)
    refused(_layout(10, offs=(0, 4, 8, 14)), vp, 160, "offset 14")                  # a field that does not fit point_step
    refused(_layout(10, offs=(0, 6, 8, 12)), vp, 160, "multiples of 4")             # no context: the strict rules
    refused(_layout(10, point_step=22), data.ctypes.data_as(C.c_void_p), 220, "point_step 22")
    refused(_layout(5, 2, row_step=76), vp, 160, "row_step 76")                     # a row shorter than its points
    refused(_layout(10), vp, 159, "the payload has 159 bytes, the layout needs 160")
    refused(_layout(5, 2, row_step=96), vp, 160, "the layout needs 176")
    refused(_layout(10), None, 160, "NULL data")
    bad = _lib.FloorParams()
    L.mrgfe_floor_default_params(C.byref(bad))
    bad.tilt_deg = float("nan")
    refused(_layout(10), vp, 160, "non-finite", params=bad)
    # a message that passes is then refused for the missing context, an empty one too: nothing was touched
    refused(_layout(10), vp, 160, "NULL argument")
    refused(_layout(0), None, 0, "NULL argument")
    assert L.mrgfe_floor_callback(None, C.byref(q), C.byref(_layout(10)), vp, 160, None, None, None) == _lib.ERR_INVALID  # NULL result


def test_keyframe_callback_device_refusals_need_no_store():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    ctr = np.zeros((65, 3), dtype=np.float32)

    def refused(key, ptr, n, n_centres, says, centres=ctr):
        nk, nr = C.c_size_t(7), C.c_size_t(7)
        st = L.mrgfe_keyframe_callback_device(None, key, ptr, n, centres.ctypes.data_as(_fp) if centres is not None else None, n_centres, 4.0, None, C.byref(nk), None, C.byref(nr))
        assert st == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_keyframe_callback_device:") and says in _lib.last_error(), (st, _lib.last_error())
        assert nk.value == 0 and nr.value == 0  # both counts are zeroed

    somewhere = C.c_void_p(0x1000)  # never read: every call below is refused before the pointer is looked at
    refused(0, somewhere, 10, 2, "key 0")
    refused(1, somewhere, 10, 65, "65 centres")
    refused(1, somewhere, 10, -1, "-1 centres")
    refused(1, somewhere, 10, 2, "2 centres", centres=None)
    refused(1, somewhere, 1 << 31, 2, "more than 2^31 - 1")
    refused(1, None, 10, 2, "NULL cloud")
    refused(1, somewhere, 10, 2, "NULL argument")  # ... and then for the missing store
    refused(1, None, 0, 0, "NULL argument")
    assert L.mrgfe_keyframe_callback_device(None, 1, somewhere, 10, None, 0, 4.0, None, None, None, None) == _lib.ERR_INVALID  # NULL n_kept


class _FakeLib:
    """Stands in for libmrgfe behind a wrapper: records the arguments of the one entry point under test and writes a result."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)  # (the host-only helpers: default parameters, mrgfe_pointcloud2_layout)

    def mrgfe_floor_callback(self, ctx, params, layout, data, nbytes, result, filtered, inliers):
        p, lay, res = params._obj, layout._obj, result._obj
        self.calls.append(dict(ctx=ctx, tilt=p.tilt_deg, thresh=p.floor_pts_thresh, normals=p.use_normal_filtering,
                               layout=(lay.width, lay.height, lay.point_step, lay.row_step, lay.off_x, lay.off_y, lay.off_z, lay.off_intensity),
                               first=C.cast(data, C.POINTER(C.c_uint8))[0] if data else None, nbytes=nbytes, filtered=filtered is not None, inliers=inliers is not None))
        res.found, res.reason, res.n_clipped, res.n_filtered, res.n_inliers, res.iterations = 1, 0, 9, 2, 1, 5
        res.coeffs[:] = [0.0, 0.0, 1.0, 2.0]
        if filtered is not None:
            filtered[0], filtered[4] = 1.5, 2.5
        if inliers is not None:
            inliers[0] = 3.5
        return 0

    def mrgfe_keyframe_callback_device(self, store, key, d_xyzi, n, centres, n_centres, radius_sqr, kept, n_kept, removed, n_removed):
        self.calls.append(dict(store=store, key=key, ptr=d_xyzi.value if d_xyzi is not None else None, n=n, centres=[centres[i] for i in range(3 * n_centres)],
                               radius_sqr=radius_sqr, kept=kept is not None, removed=removed is not None))
        n_kept._obj.value, n_removed._obj.value = 2, 1
        if kept is not None:
            kept[0], kept[4] = 1.0, 2.0
        if removed is not None:
            removed[0] = 9.0
        return 0


class _Ctx:
    _h = 0xC0

    def __init__(self):
        self.switched = []

    def set_byte_layouts(self, on):
        self.switched.append(on)


def test_detect_pointcloud2_marshals_the_message(monkeypatch):
    from mrg_slam_amd import _lib, floor_detection

    fake = _FakeLib(_lib.lib())
    monkeypatch.setattr(floor_detection, "lib", lambda: fake)
    ctx = _Ctx()
    fd = floor_detection.FloorDetection(ctx=ctx, tilt_deg=3.0, floor_pts_thresh=64, enable_normal_filtering=False)
    data = bytes([7]) + bytes(2 * 120 + 100 - 1)
    got = fd.detect_pointcloud2(data, 5, 3, 20, {"x": 4, "y": 8, "z": 0, "intensity": 16}, row_step=120)
    assert got.tolist() == [0.0, 0.0, 1.0, 2.0] and len(fake.calls) == 1
    c = fake.calls[0]
    assert c["ctx"] == 0xC0 and (c["tilt"], c["thresh"], c["normals"]) == (3.0, 64, 0)
    assert c["layout"] == (5, 3, 20, 120, 4, 8, 0, 16) and (c["first"], c["nbytes"]) == (7, 340) and c["filtered"] and c["inliers"]
    assert fd.last.reason == "found" and (fd.last.n_clipped, fd.last.iterations) == (9, 5)
    assert fd.last.filtered.shape == (2, 4) and fd.last.filtered[:, 0].tolist() == [1.5, 2.5] and fd.last.inliers[:, 0].tolist() == [3.5]
    assert ctx.switched == []  # a {name: offset} dict switches nothing
    # the driver's field list of 22-byte records: no intensity match for a UINT8 field, the context is switched to byte layouts; no clouds wanted
    fields = [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 2, 1), ("time", 18, 7, 1)]
    fd.detect_pointcloud2(bytes(66), 3, 1, 22, fields, want_clouds=False)
    c = fake.calls[1]
    assert c["layout"] == (3, 1, 22, 0, 0, 4, 8, -1) and c["nbytes"] == 66 and not c["filtered"] and not c["inliers"] and ctx.switched == [True]
    assert fd.last.filtered is None and fd.last.inliers is None
    # an empty message goes down with no data; a short payload is refused before the library sees it
    fd.detect_pointcloud2(b"", 0, 1, 16, FIELDS)
    assert fake.calls[2]["first"] is None and fake.calls[2]["nbytes"] == 0
    with pytest.raises(ValueError, match="payload has 159 bytes"):
        fd.detect_pointcloud2(bytes(159), 10, 1, 16, FIELDS)
    assert len(fake.calls) == 3


def test_component_hands_the_message_over_in_one_call():
    from mrg_slam_amd import FloorDetectionComponent

    calls = []

    class Recording:
        def detect(self, cloud, p):
            calls.append(("detect", len(cloud)))
            return np.array([0, 0, 1, 2], np.float32)

        def detect_pointcloud2(self, msg, p):
            calls.append(("detect_pointcloud2", msg["width"] * msg["height"], p["floor_pts_thresh"]))
            return None if msg["width"] == 7 else np.array([0, 0, 1, 1.5], np.float32)

    comp = FloorDetectionComponent({"floor_pts_thresh": 99}, ops=Recording())
    msg = {"data": bytes(160), "width": 10, "height": 1, "point_step": 16, "fields": FIELDS}
    assert comp.pointcloud2_callback(msg) == [0.0, 0.0, 1.0, 1.5]
    assert comp.pointcloud2_callback(dict(msg, width=7)) == []          # no floor: FloorCoeffs with no coefficients (:85-92)
    assert comp.pointcloud2_callback(dict(msg, width=0)) is None        # an empty cloud: nothing is published (:74-77)
    assert comp.pointcloud2_callback(dict(msg, height=0)) is None
    assert calls == [("detect_pointcloud2", 10, 99), ("detect_pointcloud2", 7, 99)]


def test_keyframe_callback_device_marshals_the_cloud(monkeypatch):
    from mrg_slam_amd import _lib, map_cloud

    fake = _FakeLib(_lib.lib())
    monkeypatch.setattr(map_cloud, "lib", lambda: fake)
    store = map_cloud.MapCloudStore.__new__(map_cloud.MapCloudStore)  # (no context: only the handle is read)
    store._h = C.c_void_p(0x51)
    kept, removed = store.keyframe_callback_device(5, 0xABC000, 10, [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], radius=1.5, want_removed=True)
    c = fake.calls[0]
    assert (c["key"], c["ptr"], c["n"], c["centres"]) == (5, 0xABC000, 10, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) and c["radius_sqr"] == 2.25 and c["kept"] and c["removed"]
    assert kept.shape == (2, 4) and kept[:, 0].tolist() == [1.0, 2.0] and removed.shape == (1, 4) and removed[0, 0] == 9.0
    # no centres: nothing can be removed, no room is made for it; an empty cloud goes down without a pointer
    kept, removed = store.keyframe_callback_device(6, 0, 0, want_kept=False, want_removed=True)
    c = fake.calls[1]
    assert (c["key"], c["ptr"], c["n"], c["centres"]) == (6, None, 0, []) and not c["kept"] and not c["removed"]
    assert kept is None and removed.shape == (0, 4)
    store._h = None  # (nothing to destroy)


def test_cloud_callback_device_takes_the_decisions_of_cloud_callback():
    from mrg_slam_amd import synth
    from mrg_slam_amd.keyframes import KeyframeCallback

    class Recording:
        def __init__(self):
            self.calls = []

        def keyframe(self, key, msg, centres, radius, want_removed):
            self.calls.append((key, np.asarray(centres).copy(), radius, want_removed))
            return np.zeros((3, 4), np.float32), (np.zeros((1, 4), np.float32) if want_removed else None)

        def keyframe_device(self, key, dev_ptr, n, centres, radius, want_removed):
            assert (dev_ptr, n) == (0xD000, 1234)
            self.calls.append((key, np.asarray(centres).copy(), radius, want_removed))
            return np.zeros((3, 4), np.float32), (np.zeros((1, 4), np.float32) if want_removed else None)

    ops = [Recording(), Recording()]
    cbs = [KeyframeCallback({"robot_remove_points_radius": 1.25}, ops=o) for o in ops]
    rng = np.random.default_rng(5)
    odom, out = np.eye(4), [[], []]
    for step in range(12):
        odom = odom @ synth.make_pose([rng.uniform(0.2, 0.9), 0.0, 0.0], synth.rot_z(rng.normal(0, 0.1)))
        for cb in cbs:
            if step == 5:
                cb.others_odom_poses = {"b": odom[:3, 3] + [3.0, 1.0, 0.0]}
                cb.trans_odom2map = synth.make_pose([0.2, -0.1, 0.0], synth.rot_z(0.02))
        out[0].append(cbs[0].cloud_callback(odom, {"width": 1234}, removed_points_wanted=step % 2 == 0))
        out[1].append(cbs[1].cloud_callback_device(odom, 0xD000, 1234, removed_points_wanted=step % 2 == 0))
    assert [r is None for r in out[0]] == [r is None for r in out[1]] and 4 <= len(ops[1].calls) < 12
    assert len(ops[0].calls) == len(ops[1].calls)
    for a, b in zip(ops[0].calls, ops[1].calls):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] == 1.25 and a[3] == b[3]
    for a, b in zip(out[0], out[1]):
        if a is not None:
            assert (a.key, a.accum_distance) == (b.key, b.accum_distance) and (a.kept is None) == (b.kept is None) and (a.removed is None) == (b.removed is None)
    assert any(len(c[1]) == 1 for c in ops[1].calls) and any(len(c[1]) == 0 for c in ops[1].calls)
    # a key of the caller's is passed through
    assert cbs[1].cloud_callback_device(odom @ synth.make_pose([5.0, 0, 0], np.eye(3)), 0xD000, 1234, key=77).key == 77
