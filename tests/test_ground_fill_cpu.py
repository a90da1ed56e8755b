"""CPU: the host side of the first-keyframe ground fill (src/mrg_slam/graph_database.cpp:114-129, src/pcl/fill_ground_plane.cpp) — the two loop counts of
mrgfe_ground_fill_counts against the model (tests/ground_fill_reference.py), the refusals that need no context, the record sizes, and the
graph_database.py mirror over a recording fake operation."""
import ctypes as C
import math

import numpy as np
import pytest

import ground_fill_reference as model

# (map_resolution, radius) -> rings x angles; r and angle are accumulated doubles
COUNTS = {(0.5, 2.0): (4, 26), (0.1, 0.3): (2, 19), (0.05, 1.0): (19, 126), (0.1, 0.7): (7, 44), (0.05, 7.5): (150, 943)}


def raw_counts(radius, resolution):
    from mrg_slam_amd import _lib

    p = _lib.GroundFillParams(radius, resolution, 0, 0)
    rings, angles = C.c_uint32(7), C.c_uint32(7)
    st = _lib.lib().mrgfe_ground_fill_counts(C.byref(p), C.byref(rings), C.byref(angles))
    return st, rings.value, angles.value


@pytest.mark.parametrize("params", sorted(COUNTS))
def test_counts_equal_the_model_and_the_table(params):
    resolution, radius = params
    assert model.counts(params) == COUNTS[params]
    assert raw_counts(radius, resolution) == (0,) + COUNTS[params]


def test_counts_accumulate_and_do_not_multiply():
    """0.1 + 0.1 + 0.1 > 0.3: two rings, where k * map_resolution would give three; 0.05 accumulated twenty times passes 1.0."""
    assert 0.1 + 0.1 + 0.1 > 0.3 and 3 * 0.1 > 0.3 and model.counts((0.1, 0.3))[0] == 2
    assert model.counts((0.05, 1.0))[0] == 19 and int(1.0 / 0.05) == 20
    # zero rings is a valid fill (radius < map_resolution); the angle loop still runs
    assert raw_counts(0.5, 1.0) == (0, 0, 4) and model.counts((1.0, 0.5)) == (0, 4)
    from mrg_slam_amd import ground_fill_counts

    assert ground_fill_counts(7.5, 0.05) == (150, 943)


def test_refusals_that_need_no_context():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    inf, nan = float("inf"), float("nan")
    for radius, resolution in ((0.0, 0.05), (-1.0, 0.05), (5.0, 0.0), (5.0, -0.05), (inf, 0.05), (5.0, inf), (nan, 0.05), (5.0, nan)):
        st, rings, angles = raw_counts(radius, resolution)
        assert st == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_ground_fill_counts:"), (radius, resolution, st)
    # more than 2^31 - 1 points: refused at once, not walked
    for radius, resolution in ((1000.0, 0.001), (1.0e9, 1.0e-9), (1.0e300, 1.0e-300)):
        st, rings, angles = raw_counts(radius, resolution)
        assert st == _lib.ERR_INVALID and "2^31" in _lib.last_error() and (rings, angles) == (0, 0)
    # the largest disc of the table's density that still fits: 18000 rings x 113098 angles = 2035764000 <= 2^31 - 1
    st, rings, angles = raw_counts(18000.0, 1.0)
    assert st == 0 and rings == 18000 and angles == math.ceil(2 * math.pi * 18000) and rings * angles <= 2**31 - 1
    st, rings, angles = raw_counts(19000.0, 1.0)  # 19000 x 119381 > 2^31 - 1
    assert st == _lib.ERR_INVALID
    p = _lib.GroundFillParams(5.0, 0.05, 0, 0)
    n = C.c_uint32(0)
    assert L.mrgfe_ground_fill_counts(None, C.byref(n), C.byref(n)) == _lib.ERR_INVALID
    assert L.mrgfe_ground_fill_counts(C.byref(p), None, C.byref(n)) == _lib.ERR_INVALID
    assert L.mrgfe_ground_fill_counts(C.byref(p), C.byref(n), None) == _lib.ERR_INVALID
    # the two entry points check their parameters before they touch the context or the store (NULL here)
    r = _lib.GroundFillResult()
    out = np.zeros((4, 4), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    bad = _lib.GroundFillParams(-5.0, 0.05, 0, 0)
    assert L.mrgfe_fill_ground_plane(None, C.byref(bad), None, fp, 0, 16, fp, 4, C.byref(r)) == _lib.ERR_INVALID and "finite and > 0" in _lib.last_error()
    assert L.mrgfe_map_store_fill_ground(None, 1, 2, C.byref(bad), None, None, 0, C.byref(r)) == _lib.ERR_INVALID and "finite and > 0" in _lib.last_error()
    simple = _lib.GroundFillParams(5.0, 0.05, 1, 0)
    assert L.mrgfe_fill_ground_plane(None, C.byref(simple), None, fp, 0, 16, fp, 4, C.byref(r)) == _lib.ERR_INVALID and "estimate" in _lib.last_error()
    assert L.mrgfe_map_store_fill_ground(None, 1, 2, C.byref(simple), None, None, 0, C.byref(r)) == _lib.ERR_INVALID and "estimate" in _lib.last_error()
    assert L.mrgfe_fill_ground_plane(None, C.byref(p), None, fp, 0, 16, fp, 4, None) == _lib.ERR_INVALID
    assert L.mrgfe_fill_ground_plane(None, C.byref(p), None, fp, 0, 16, fp, 4, C.byref(r)) == _lib.ERR_INVALID  # no context
    assert L.mrgfe_map_store_fill_ground(None, 1, 2, C.byref(p), None, None, 0, C.byref(r)) == _lib.ERR_INVALID  # no store


def test_records_and_defaults():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    assert L.mrgfe_ground_fill_params_size() == C.sizeof(_lib.GroundFillParams) == 24
    assert L.mrgfe_ground_fill_result_size() == C.sizeof(_lib.GroundFillResult) == 40
    p = _lib.GroundFillParams(1.0, 1.0, 1, 1)
    L.mrgfe_ground_fill_default_params(C.byref(p))
    assert (p.radius, p.map_resolution, p.simple, p.pad) == (5.0, 0.05, 0, 0)  # apps/mrg_slam_component.cpp:271, :245, :272
    L.mrgfe_ground_fill_default_params(None)


def test_model_lies_on_its_plane():
    """The model against first principles (not against the product): with a unit normal every generated point lies on the plane and on its ring."""
    n = np.array([0.1, -0.2, 1.0])
    n /= np.linalg.norm(n)
    d = 1.7
    pts = model.disc(n, d, 2.0, 0.5).astype(np.float64)
    assert pts.shape == (4 * 26, 4) and (pts[:, 3] == 0).all()
    assert np.abs(pts[:, :3] @ n + d).max() <= 1e-6
    for k, r in enumerate((0.5, 1.0, 1.5, 2.0)):
        s = np.array(model.ring_sample(r, tuple(n), d))
        ring = pts[26 * k: 26 * (k + 1), :3]
        foot = ring - np.outer(ring @ n, n)
        assert np.abs(np.linalg.norm(foot, axis=1) - np.linalg.norm(s - (s @ n) * n)).max() <= 1e-6
    cloud = np.arange(12, dtype=np.float32).reshape(3, 4)
    filled = model.fill(cloud, n, d, 2.0, 0.5)
    assert filled[:3].tobytes() == cloud.tobytes() and filled[3:].tobytes() == model.disc(n, d, 2.0, 0.5).tobytes()


# ---- the graph_database.py mirror -----------------------------------------------------------------------------------------------------------------
class Kf:
    def __init__(self, key, x):
        self.key = key
        self.odom = np.eye(4)
        self.odom[0, 3] = x


class NoEdgeOps:
    def information_matrices(self, edges):
        return np.zeros((len(edges), 6, 6)), np.zeros(len(edges))


class RecordingFill:
    def __init__(self):
        self.calls = []

    def fill_first_cloud(self, keyframe, radius, map_resolution, simple, estimate):
        self.calls.append((keyframe.key, radius, map_resolution, simple, None if estimate is None else np.array(estimate)))
        keyframe.key = keyframe.key + 1000  # the filled cloud's key, as HipGroundFillOps renames it


def test_mirror_fills_only_the_first_keyframe_of_an_empty_graph():
    from mrg_slam_amd.graph_database import GraphDatabaseEdges

    fill = RecordingFill()
    db = GraphDatabaseEdges({"enable_fill_first_cloud": True, "fill_first_cloud_radius": 7.5, "map_cloud_resolution": 0.05}, ops=NoEdgeOps(), fill_ops=fill)
    for i in range(4):
        db.add_odom_keyframe(Kf(1 + i, float(i)))
    edges = db.flush_keyframe_queue()
    # once, for keyframe 1, RANSAC variant: the estimate is not passed
    assert len(fill.calls) == 1 and fill.calls[0][:4] == (1, 7.5, 0.05, False) and fill.calls[0][4] is None
    # ... and BEFORE the edges were made: they name the filled cloud
    assert [e.keyed()[:2] for e in edges] == [(2, 1001), (3, 2), (4, 3)]
    # a second flush before insert_loops: keyframes_ is still empty but new_keyframes_ is not (:79)
    db.add_odom_keyframe(Kf(5, 4.0))
    db.flush_keyframe_queue()
    assert len(fill.calls) == 1
    db.insert_loops([])
    # keyframes_ is non-empty now
    db.add_odom_keyframe(Kf(6, 5.0))
    db.flush_keyframe_queue()
    assert len(fill.calls) == 1 and db.flush_keyframe_queue() is None


def test_mirror_simple_variant_passes_the_estimate_and_disabled_calls_nothing():
    from mrg_slam_amd.graph_database import DEFAULTS, GraphDatabaseEdges

    assert DEFAULTS["enable_fill_first_cloud"] is False and DEFAULTS["fill_first_cloud_radius"] == 5.0 and DEFAULTS["fill_first_cloud_simple"] is False
    assert DEFAULTS["map_cloud_resolution"] == 0.05
    fill = RecordingFill()
    db = GraphDatabaseEdges({"enable_fill_first_cloud": True, "fill_first_cloud_simple": True}, ops=NoEdgeOps(), fill_ops=fill)
    db.add_odom_keyframe(Kf(1, 2.0))
    odom2map = np.eye(4)
    odom2map[1, 3] = -3.0
    db.flush_keyframe_queue(odom2map)
    assert len(fill.calls) == 1 and fill.calls[0][:4] == (1, 5.0, 0.05, True)
    expect = np.eye(4)
    expect[0, 3], expect[1, 3] = 2.0, -3.0  # odom2map * keyframe->odom (:73-74)
    assert np.array_equal(fill.calls[0][4], expect)
    # disabled (the default): today's behaviour, the operation is never called and need not exist
    off_fill = RecordingFill()
    for db in (GraphDatabaseEdges(ops=NoEdgeOps(), fill_ops=off_fill), GraphDatabaseEdges(ops=NoEdgeOps())):
        db.add_odom_keyframe(Kf(1, 0.0))
        db.add_odom_keyframe(Kf(2, 1.0))
        assert [e.keyed()[:2] for e in db.flush_keyframe_queue()] == [(2, 1)]
    assert off_fill.calls == []
    with pytest.raises(ValueError, match="fill_ops"):
        GraphDatabaseEdges({"enable_fill_first_cloud": True}, ops=NoEdgeOps())


def test_hip_fill_ops_rename_the_keyframe_over_a_fake_store():
    from mrg_slam_amd.graph_database import HipGroundFillOps

    class FakeStore:
        def __init__(self, has_model):
            self.has_model, self.calls = has_model, []

        def fill_ground(self, src_key, dst_key, radius, map_resolution, simple=False, estimate=None, want_cloud=True):
            self.calls.append((src_key, dst_key, radius, map_resolution, simple, want_cloud))
            return (np.zeros((5, 4), np.float32) if self.has_model and want_cloud else None), {"has_model": self.has_model}

    kf = Kf(3, 0.0)
    kf.cloud = np.zeros((2, 4), np.float32)
    store = FakeStore(True)
    HipGroundFillOps(store, lambda k: k.key + 100).fill_first_cloud(kf, 7.5, 0.05, False, None)
    assert store.calls == [(3, 103, 7.5, 0.05, False, True)] and kf.key == 103 and len(kf.cloud) == 5
    kf = Kf(3, 0.0)
    kf.cloud = np.zeros((2, 4), np.float32)
    HipGroundFillOps(FakeStore(False), lambda k: k.key + 100).fill_first_cloud(kf, 7.5, 0.05, False, None)
    assert kf.key == 3 and len(kf.cloud) == 2  # no model: nothing changes
