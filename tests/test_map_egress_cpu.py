"""CPU: the host side of the map egress — the two records of ``mrgfe_map_store_publish`` against their ctypes mirrors, the message dict, and
``MapPublisher`` (update_map_cloud_msg, publish_map_service, save_map_service: apps/mrg_slam_component.cpp:712-740, 764-796, 1078-1144) over a stand-in
store that records its arguments."""
import ctypes as C
import os

import numpy as np

UTM, ENU = (364000.25, 5621000.5, 31.125), (-12.5, 7.75, 0.3)


def test_struct_sizes_and_defaults():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    assert C.sizeof(_lib.MapPublishParams) == 48 == L.mrgfe_map_publish_params_size()
    assert C.sizeof(_lib.MapPublishResult) == 32 == L.mrgfe_map_publish_result_size()
    p = _lib.MapPublishParams(9, 9, 9, 9, 9, 9)
    p.offsets[:] = [9.0] * 6
    L.mrgfe_map_publish_default_params(C.byref(p))
    # config/mrg_slam.yaml:235-237, the 32-byte records, no offsets
    assert (p.resolution, p.min_points_per_voxel, p.distance_far_thresh, p.skip_first_cloud, p.point_step, p.n_offsets) == (np.float32(0.1), 1, 10000.0, 0, 32, 0)
    assert list(p.offsets) == [0.0] * 6
    assert _lib.MapPublishParams.offsets.offset == 24 and _lib.MapPublishResult.point_step.offset == 24 and _lib.MapPublishResult.off_intensity.offset == 28


def test_message_dict_assembly():
    from mrg_slam_amd import _lib
    from mrg_slam_amd.io import pcl_xyzi_records, xyzi_from_pointcloud2
    from mrg_slam_amd.map_cloud import _map_message

    x = np.arange(20, dtype=np.float32).reshape(5, 4)
    for step, off in ((32, 16), (16, 12)):
        data = (pcl_xyzi_records(x) if step == 32 else x.view(np.uint8)).reshape(-1)
        msg = _map_message(data, _lib.MapPublishResult(5, 11, 5 * step, step, off))
        assert (msg["width"], msg["height"], msg["point_step"], msg["row_step"], msg["n_unfiltered"]) == (5, 1, step, 5 * step, 11)
        assert msg["fields"] == {"x": 0, "y": 4, "z": 8, "intensity": off} and msg["is_dense"] is False and msg["is_bigendian"] is False
        assert np.array_equal(xyzi_from_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"]), x)


class FakeStore:
    """Records every publish and answers with a message of ``width`` points (None: the reference's nullptr)."""

    def __init__(self, width=3):
        self.calls, self.width = [], width

    def publish(self, keys, poses, first_keyframe=None, **kw):
        self.calls.append(dict(keys=list(keys), poses=[np.asarray(T) for T in poses], first=list(first_keyframe), **kw))
        if self.width is None:
            return None
        step = kw.get("point_step", 32)
        data = (np.arange(self.width * step) % 251).astype(np.uint8)
        return {"height": 1, "width": self.width, "is_dense": False, "is_bigendian": False, "point_step": step, "row_step": self.width * step,
                "fields": {"x": 0, "y": 4, "z": 8, "intensity": 16 if step == 32 else 12}, "data": data, "n_unfiltered": self.width}


def snapshot(n=3):
    return [(k + 1, np.eye(4) * (k + 1), k == 0) for k in range(n)]


def publisher(store, **kw):
    from mrg_slam_amd import MapPublisher

    pub = MapPublisher(store, **kw)
    pub.set_snapshot(snapshot())
    return pub


def test_update_holds_the_flag():
    store = FakeStore()
    pub = publisher(store, map_cloud_resolution=0.1, map_cloud_min_points_per_voxel=1, map_cloud_distance_far_thresh=100.0, map_frame_id="world")
    first = pub.update()
    assert pub.updated and first["frame_id"] == "world" and len(store.calls) == 1
    c = store.calls[0]
    assert (c["keys"], c["first"]) == ([1, 2, 3], [True, False, False]) and np.array_equal(c["poses"][2], np.eye(4) * 3)
    # :727-729: the parameters as they are, skip_first_cloud false, toROSMsg records
    assert (c["resolution"], c["min_points_per_voxel"], c["distance_far_thresh"], c["skip_first_cloud"], c["point_step"]) == (0.1, 1, 100.0, False, 32)
    assert pub.update() is first and not pub.updated and len(store.calls) == 1  # not required: the cached message, no call
    pub.set_snapshot(snapshot(2))
    second = pub.update()
    assert second is not first and pub.updated and store.calls[1]["keys"] == [1, 2]
    # a generation that gives no cloud clears the flag and keeps the message (:724, :730-732)
    store.width = None
    pub.set_snapshot(snapshot(1))
    assert pub.update() is second and not pub.updated and len(store.calls) == 3
    assert pub.update() is second and len(store.calls) == 3


def test_request_defaults():
    from mrg_slam_amd import MapRequest

    store = FakeStore()
    pub = publisher(store, map_cloud_resolution=0.05, map_cloud_min_points_per_voxel=2, map_cloud_distance_far_thresh=10000.0)
    f32 = lambda v: float(np.float32(v))  # noqa: E731  (`float resolution = ...`, :774)
    msg = pub.publish_map(MapRequest())  # nothing set: the config
    c = store.calls[-1]
    assert (c["resolution"], c["min_points_per_voxel"], c["distance_far_thresh"], c["skip_first_cloud"], c["point_step"]) == (f32(0.05), 2, 10000.0, False, 32)
    assert msg["frame_id"] == "map"
    msg = pub.publish_map(MapRequest(resolution=0.2, min_points_per_voxel=0, distance_far_thresh=-1.0, skip_first_cloud=True, frame_id="odom"))
    c = store.calls[-1]  # min_points_per_voxel 0 is a value (only < 0 is "not set"); a negative threshold is one too (only 0 is not)
    assert (c["resolution"], c["min_points_per_voxel"], c["distance_far_thresh"], c["skip_first_cloud"]) == (f32(0.2), 0, -1.0, True)
    assert msg["frame_id"] == "odom"
    pub.publish_map(MapRequest(resolution=-1.0))  # a negative resolution is a value: the unfiltered union
    assert store.calls[-1]["resolution"] == -1.0
    assert pub.update_required  # the services leave the timer's flag alone
    store.width = None
    assert pub.publish_map() is None


def test_save_map_offsets_and_files(tmp_path):
    from mrg_slam_amd import MapRequest
    from mrg_slam_amd.io import read_pcd

    cases = [  # (zero_utm, zero_enu, req.utm) -> offsets, .utm file
        (None, None, True, [], False),
        (UTM, None, False, [], True),  # the file is written whenever zero_utm is set (:1121), the points move only on request
        (UTM, None, True, [UTM], True),
        (None, ENU, False, [ENU], False),  # ENU whenever set
        (UTM, ENU, True, [UTM, ENU], True),  # UTM first
        (UTM, ENU, False, [ENU], True),
    ]
    for i, (utm, enu, want_utm, offsets, utm_file) in enumerate(cases):
        store = FakeStore(width=4)
        pub = publisher(store, zero_utm=utm, zero_enu=enu)
        path = str(tmp_path / f"case{i}" / "deep" / "map.pcd")
        assert pub.save_map(MapRequest(resolution=0.3, utm=want_utm, skip_first_cloud=True), path)
        c = store.calls[-1]
        assert c["point_step"] == 16 and c["skip_first_cloud"] is True and c["resolution"] == float(np.float32(0.3)) and c["min_points_per_voxel"] == 2
        assert [tuple(o) for o in c["offsets"]] == offsets
        body = (np.arange(64) % 251).astype(np.uint8)
        raw = open(path, "rb").read()
        assert raw.endswith(body.tobytes()) and b"WIDTH 4\n" in raw and b"POINTS 4\n" in raw and b"DATA binary\n" in raw
        assert np.array_equal(read_pcd(path).view(np.uint8).reshape(-1), body)  # the records as they came down
        assert os.path.exists(path + ".utm") == utm_file
        if utm_file:
            assert open(path + ".utm").read() == "364000.250000 5621000.500000 31.125000\n"  # boost::format("%.6f %.6f %.6f"), :1123
    store = FakeStore(width=None)
    pub = publisher(store, zero_utm=UTM)
    path = str(tmp_path / "none" / "map.pcd")
    assert pub.save_map(MapRequest(), path) is False and not os.path.exists(path) and not os.path.exists(path + ".utm")  # :1099-1102
