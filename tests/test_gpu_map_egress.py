"""GPU: ``mrgfe_map_store_publish`` / ``_publish_device`` / ``_read`` — the map as the records its three callers send or save, and stored keyframes read
back — against the CPU oracle's MapCloudGenerator and against ``mrgfe_map_store_generate`` (unchanged, the second yardstick), bit for bit.

A few thousand points per case: tile edges (255 / 256 / 257 / 513 points, an empty keyframe, a single point), not map sizes.  The base input is held to the
oracle's counts first, so that a change of the generator cannot hollow the cases out: 1312 voxels at resolution 0.5, 400 of them fed by two or more
keyframes, and 140 output rows whose bits change when the keyframes are summed in the reverse order."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [257, 0, 1, 255, 256, 513, 1000]
KEYS = list(range(1, len(SIZES) + 1))
FIRST = [1] + [0] * (len(SIZES) - 1)
# (resolution, min_points_per_voxel, distance_far_thresh, skip_first_cloud) -> the oracle's point count
PARAMS = [((0.5, 1, 10000.0, False), 1312), ((0.5, 3, 6.0, False), 234), ((0.0, 1, 5.0, True), 1995), ((0.5, 1, -1.0, True), 1191)]
UTM, ENU = (364000.25, 5621000.5, 31.125), (-12.5, 7.75, 0.3)
INVALID = -1


def pose(k):
    T = np.eye(4)
    c, s = np.cos(0.1 * k), np.sin(0.1 * k)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = (0.4 * k, -0.3 * k, 0.05 * k)
    return T


def cloud_of(rng, n, sigma=1.5):
    c = rng.normal(0, sigma, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    return c


def records(x, step):
    """The expected bytes of a cloud: ``io.pcl_xyzi_records`` or the packed points."""
    from mrg_slam_amd.io import pcl_xyzi_records

    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 4)
    return (pcl_xyzi_records(x) if step == 32 else x.view(np.uint8).reshape(len(x), 16)).reshape(-1)


def same_bytes(got, want, what=""):
    got, want = np.asarray(got, dtype=np.uint8).reshape(-1), np.asarray(want, dtype=np.uint8).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def add_offsets(x, offsets):
    """(x + o1) + o2 in f32, intensity untouched."""
    y = np.array(x, dtype=np.float32, copy=True)
    for o in offsets:
        y[:, :3] = y[:, :3] + np.asarray(o, dtype=np.float64).astype(np.float32)
    return y


@pytest.fixture(scope="module")
def world():
    """The base input in a store, and the oracle's map for every parameter set (computed once, never changed)."""
    from mrg_slam_amd import Context, MapCloudStore
    from oracle import oracle as orc

    rng = np.random.default_rng(20261020)
    clouds = [cloud_of(rng, n) for n in SIZES]
    poses = [pose(k) for k in range(len(SIZES))]
    ctx = Context()
    store = MapCloudStore(ctx)
    for key, c in zip(KEYS, clouds):
        store.add(key, c)
    oracle = {p: orc.map_cloud_generate(clouds, poses, FIRST, *p)[0] for p, _ in PARAMS}
    unfiltered = {p: len(orc.map_cloud_generate(clouds, poses, FIRST, 0.0, 1, p[2], p[3])[0]) for p, _ in PARAMS}
    return {"ctx": ctx, "store": store, "clouds": clouds, "poses": poses, "oracle": oracle, "unfiltered": unfiltered, "orc": orc}


def kw_of(p):
    return dict(resolution=p[0], min_points_per_voxel=p[1], distance_far_thresh=p[2], skip_first_cloud=p[3])


def raw_publish(store, keys, poses, first, data, capacity, **fields):
    """mrgfe_map_store_publish as it is: (status, result)."""
    from mrg_slam_amd import _lib

    p = _lib.MapPublishParams()
    _lib.lib().mrgfe_map_publish_default_params(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    ks = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
    P = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float64).T.reshape(16) for T in poses])) if len(keys) else np.zeros((0, 16))
    fk = np.ascontiguousarray(np.asarray(first, dtype=np.uint8))
    r = _lib.MapPublishResult()
    st = _lib.lib().mrgfe_map_store_publish(store._h, len(keys), ks.ctypes.data_as(C.POINTER(C.c_uint64)), P.ctypes.data_as(C.POINTER(C.c_double)),
                                            fk.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(p), data.ctypes.data_as(C.c_void_p) if data is not None else None, capacity, C.byref(r))
    return st, r


def test_the_base_input_is_what_the_oracle_was_held_to(world):
    orc, clouds, poses = world["orc"], world["clouds"], world["poses"]
    for p, count in PARAMS:
        assert len(world["oracle"][p]) == count, p
    x = world["oracle"][PARAMS[0][0]]
    back = orc.map_cloud_generate(clouds[::-1], poses[::-1], FIRST[::-1], *PARAMS[0][0])[0]
    assert back.shape == x.shape and int((back.view(np.uint32) != x.view(np.uint32)).any(axis=1).sum()) == 140  # a wrong summation order shows
    u = orc.map_cloud_generate(clouds, poses, FIRST, 0.0, 1, 10000.0, False)[0]  # (input order: the keyframe of every row is known)
    kf = np.concatenate([np.full(len(c), k) for k, c in enumerate(clouds)])
    cell = np.floor(u[:, :3] * (np.float32(1.0) / np.float32(0.5))).astype(np.int64)
    seen = {}
    for c, k in zip(map(tuple, cell), kf):
        seen.setdefault(c, set()).add(int(k))
    assert len(seen) == 1312 and sum(1 for v in seen.values() if len(v) >= 2) == 400


@pytest.mark.parametrize("step", [32, 16])
@pytest.mark.parametrize("which", range(len(PARAMS)))
def test_same_points_as_the_generators(world, which, step):
    from mrg_slam_amd.io import layout_from_fields, xyzi_from_pointcloud2

    p, count = PARAMS[which]
    store, x = world["store"], world["oracle"][p]
    msg = store.publish(KEYS, world["poses"], FIRST, point_step=step, **kw_of(p))
    same_bytes(msg["data"], records(x, step), "oracle")
    same_bytes(msg["data"], records(store.generate(KEYS, world["poses"], FIRST, **kw_of(p)), step), "generate")
    assert msg["n_unfiltered"] == world["unfiltered"][p]
    assert (msg["width"], msg["height"], msg["point_step"], msg["row_step"]) == (count, 1, step, count * step) and not msg["is_dense"] and not msg["is_bigendian"]
    assert msg["fields"] == {"x": 0, "y": 4, "z": 8, "intensity": 16 if step == 32 else 12}
    # the message goes back in through the readers of PointCloud2 bytes
    back = xyzi_from_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"])
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
    lay, needs = layout_from_fields(msg["fields"], msg["width"], msg["height"], msg["point_step"], msg["row_step"])
    assert (lay.point_step, lay.off_intensity, needs) == (step, msg["fields"]["intensity"], False)
    st = store.egress_stats()
    assert st["bytes_down"] == msg["row_step"]


@pytest.mark.parametrize("step", [32, 16])
@pytest.mark.parametrize("offsets", [(UTM,), (UTM, ENU), (ENU, UTM)])
def test_offsets_are_separate_f32_additions_behind_the_filter(world, offsets, step):
    for p in (PARAMS[0][0], PARAMS[2][0]):  # behind the voxel filter, and on the unfiltered union
        msg = world["store"].publish(KEYS, world["poses"], FIRST, point_step=step, offsets=offsets, **kw_of(p))
        same_bytes(msg["data"], records(add_offsets(world["oracle"][p], offsets), step), p)  # (intensity and the padding words: untouched)
    x = world["oracle"][PARAMS[0][0]]
    if len(offsets) == 2:  # the two additions are not one: some row rounds differently when the offsets are added up first
        both = np.asarray(offsets[0], np.float64).astype(np.float32) + np.asarray(offsets[1], np.float64).astype(np.float32)
        assert not np.array_equal(add_offsets(x, offsets), add_offsets(x, (both,)))


def test_wide_keys_take_the_second_radix_pass(world):
    from mrg_slam_amd import MapCloudStore

    rng = np.random.default_rng(20261021)
    a = np.empty((600, 4), dtype=np.float32)
    a[:, 0], a[:, 2] = rng.uniform(-2, 2, 600), rng.uniform(-2, 2, 600)
    a[:, 1] = rng.uniform(-150, 150, 600)
    a[:, 3] = rng.uniform(0, 1, 600)
    a[:50] = a[50:100]
    b = a[::-1].copy()
    far = np.eye(4)
    far[0, 3] = 1e5
    poses, first = [np.eye(4), far], [1, 0]
    x = world["orc"].map_cloud_generate([a, b], poses, first, 0.05, 1, 10000.0, False)[0]
    assert len(x) == 1100
    # 21 + 13 + 7 = 41 key bits (+ 1 for the non-finite points): more than one 32-bit sort
    span = np.floor(x[:, :3].max(0) / np.float32(0.05)) - np.floor(x[:, :3].min(0) / np.float32(0.05))
    assert [int(s).bit_length() for s in span] == [21, 13, 7]
    store = MapCloudStore(world["ctx"])
    store.add(1, a)
    store.add(2, b)
    for step in (32, 16):
        msg = store.publish([1, 2], poses, first, resolution=0.05, point_step=step)
        same_bytes(msg["data"], records(x, step), step)


def test_non_finite_points_follow_generate(world):
    from mrg_slam_amd import MapCloudStore

    c = cloud_of(np.random.default_rng(5), 700)
    c[3, 0], c[300, 1], c[301, 2], c[699, 0], c[512] = np.nan, np.inf, -np.inf, np.nan, np.nan
    store = MapCloudStore(world["ctx"])
    store.add(1, c)
    store.add(2, world["clouds"][0])
    poses = [pose(1), pose(2)]
    for kw in (dict(resolution=0.5), dict(resolution=0.0, distance_far_thresh=-1.0), dict(resolution=0.0, distance_far_thresh=4.0), dict(resolution=0.5, distance_far_thresh=4.0)):
        g = store.generate([1, 2], poses, None, **kw)
        for step in (32, 16):
            same_bytes(store.publish([1, 2], poses, None, point_step=step, **kw)["data"], records(g, step), (kw, step))


def test_emptiness_and_refusals(world):
    from mrg_slam_amd import MrgfeError

    store, poses = world["store"], world["poses"]
    assert store.publish([], [], []) is None  # no keyframes
    assert store.publish(KEYS[:2], poses[:2], FIRST[:2], distance_far_thresh=1e-6) is None  # nothing left before the filter, two keyframes
    one = store.publish(KEYS[:1], poses[:1], [0], distance_far_thresh=1e-6)  # ... one keyframe: an empty map, MRGFE_OK
    assert one is not None and (one["width"], one["row_step"], len(one["data"]), one["n_unfiltered"]) == (0, 0, 0, 0)
    none = store.publish(KEYS, poses, FIRST, resolution=0.5, min_points_per_voxel=10000)  # the count threshold above every voxel
    assert none is not None and none["width"] == 0 and none["n_unfiltered"] == sum(SIZES)
    before = store.egress_stats()
    for bad in (dict(keys=[1, 99]), dict(point_step=24), dict(point_step=0), dict(offsets=(UTM, ENU, UTM))):
        keys = bad.pop("keys", KEYS[:2])
        with pytest.raises(MrgfeError) as e:
            store.publish(keys, poses[:2], FIRST[:2], **bad)
        assert e.value.status == INVALID
    st, _ = raw_publish(store, KEYS[:2], poses[:2], FIRST[:2], np.zeros(16, np.uint8), 16, n_offsets=-1)
    assert st == INVALID
    assert store.egress_stats() == before  # refused before any launch: nothing ran
    # capacity one byte short: the needed size comes back and the buffer is not touched
    p, count = PARAMS[0]
    for step in (32, 16):
        data = np.full(count * step, 0xA5, dtype=np.uint8)
        st, r = raw_publish(store, KEYS, poses, FIRST, data, count * step - 1, resolution=p[0], point_step=step)
        assert st == INVALID and (r.n_points, r.data_bytes, r.point_step) == (count, count * step, step)
        assert (data == 0xA5).all()
        st, r = raw_publish(store, KEYS, poses, FIRST, data, count * step, resolution=p[0], point_step=step)
        assert st == 0 and r.off_intensity == (16 if step == 32 else 12)
        same_bytes(data, records(world["oracle"][p], step))


def test_the_workspace_grows_once_and_the_store_is_only_read(world):
    from mrg_slam_amd import Context, MapCloudStore

    ctx = Context()  # (a context of its own: its scratch buffers have not served another test)
    store = MapCloudStore(ctx)
    for key, c in zip(KEYS, world["clouds"]):
        store.add(key, c)
    contents = (store.bytes(), [store.has(k) for k in KEYS], [r.copy() for r in store.read(KEYS, 16)])
    large, small = PARAMS[0][0], PARAMS[1][0]
    grown = []
    for p, keys in ((large, KEYS), (small, KEYS[:3]), (large, KEYS)):
        k = len(keys)
        msg = store.publish(keys, world["poses"][:k], FIRST[:k], **kw_of(p))
        st = store.egress_stats()
        want = world["oracle"][p] if k == len(KEYS) else world["orc"].map_cloud_generate(world["clouds"][:k], world["poses"][:k], FIRST[:k], *p)[0]
        same_bytes(msg["data"], records(want, 32), (p, k))
        assert st["bytes_down"] == msg["row_step"] and st["host_waits"] >= 1 and st["launches"] >= 1
        grown.append(st["workspace_grown"])
    assert grown[0] > 0 and grown[1:] == [0, 0], grown
    after = (store.bytes(), [store.has(k) for k in KEYS], store.read(KEYS, 16))
    assert after[:2] == contents[:2]
    for a, b in zip(after[2], contents[2]):
        same_bytes(a, b)


def test_the_device_form_feeds_the_keyframe_callback(world):
    from mrg_slam_amd import MapCloudStore

    store = MapCloudStore(world["ctx"])
    for key, c in zip(KEYS, world["clouds"]):
        store.add(key, c)
    p = PARAMS[1][0]
    host = store.publish(KEYS, world["poses"], FIRST, point_step=16, offsets=(ENU,), **kw_of(p))
    dev = store.publish_device(KEYS, world["poses"], FIRST, point_step=16, offsets=(ENU,), **kw_of(p))
    assert dev["data"] is None and dev["dev_ptr"] and dev["width"] == host["width"] == PARAMS[1][1] and dev["row_step"] == host["row_step"]
    kept, _ = store.keyframe_callback_device(100, dev["dev_ptr"], dev["width"])  # point_step 16, no centres: a gather out of the workspace into the store
    same_bytes(kept.view(np.uint8), host["data"])
    same_bytes(store.read([100], 16)[0], host["data"])
    same_bytes(host["data"], records(add_offsets(world["oracle"][p], (ENU,)), 16))
    empty = store.publish_device(KEYS[:1], world["poses"][:1], [0], distance_far_thresh=1e-6)
    assert empty["width"] == 0 and empty["dev_ptr"] == 0


@pytest.mark.parametrize("offsets", [(), (UTM,), (UTM, ENU)])
@pytest.mark.parametrize("step", [16, 32])
def test_the_device_form_of_the_unfiltered_map_is_complete_on_return(world, step, offsets):
    """Resolution 0 without a far cut: no compaction, the record kernel is the copy and nothing behind it needs the host — the call still waits for it, so a
    reader on another stream (here: another context's store) finds whole records."""
    from mrg_slam_amd import Context, MapCloudStore

    kw = dict(resolution=0.0, distance_far_thresh=-1.0, point_step=step, offsets=offsets)
    store, poses = world["store"], world["poses"]
    want = records(add_offsets(world["orc"].map_cloud_generate(world["clouds"], poses, FIRST, 0.0, 1, -1.0, False)[0], offsets), step)
    dev = store.publish_device(KEYS, poses, FIRST, **kw)
    st = store.egress_stats()
    assert dev["width"] == sum(SIZES) == dev["n_unfiltered"] and dev["dev_ptr"]
    assert (st["launches"], st["host_waits"], st["bytes_down"]) == (1, 2, 0)  # the wait for uploads in flight, and the one behind the record kernel
    other = MapCloudStore(Context())  # a stream of its own
    n16 = dev["row_step"] // 16  # (32-byte records read as pairs of packed points: the bytes are what is compared)
    kept, _ = other.keyframe_callback_device(1, dev["dev_ptr"], n16)
    same_bytes(kept.view(np.uint8), want, "another stream")
    same_bytes(store.publish(KEYS, poses, FIRST, **kw)["data"], want, "host form")


def test_round_trip_through_the_keyframe_callback(world):
    from mrg_slam_amd import MapCloudStore

    store = MapCloudStore(world["ctx"])
    for key, c in zip(KEYS, world["clouds"]):
        store.add(key, c)
    msg = store.publish(KEYS, world["poses"], FIRST, resolution=0.5)  # the 32-byte form
    kept, _ = store.keyframe_callback(200, msg)
    assert np.array_equal(kept.view(np.uint32), world["oracle"][PARAMS[0][0]].view(np.uint32))
    same_bytes(store.read([200], 32)[0], msg["data"])


@pytest.fixture(scope="module")
def read_store(world):
    """Keyframes of the tile-edge sizes, one made by the keyframe callback with a removal sphere, one by the ground fill."""
    from mrg_slam_amd import MapCloudStore

    rng = np.random.default_rng(77)
    sizes = [0, 1, 255, 256, 257, 513]
    clouds = {10 + i: cloud_of(rng, n) for i, n in enumerate(sizes)}
    store = MapCloudStore(world["ctx"])
    for key, c in clouds.items():
        store.add(key, c)
    kept, removed = store.keyframe_callback(30, cloud_of(rng, 900), np.zeros((1, 3), np.float32), 1.5)
    assert len(kept) and len(removed)
    clouds[30] = kept
    filled, info = store.fill_ground(14, 31, radius=0.5, map_resolution=0.1, simple=True, estimate=np.eye(4))
    assert info["n_added"] > 0 and len(filled) == 257 + info["n_added"]
    clouds[31] = filled  # (exists nowhere else: the fill ran on the device)
    return store, clouds


@pytest.mark.parametrize("step", [32, 16])
def test_read_returns_what_went_in(read_store, step):
    store, clouds = read_store
    keys = [13, 10, 15, 31, 11, 13, 30, 12, 14]  # permuted, 13 twice, the empty keyframe in the middle
    out = store.read(keys, step)
    assert len(out) == len(keys)
    for k, r in zip(keys, out):
        assert r.shape == (len(clouds[k]), step) and r.dtype == np.uint8
        same_bytes(r, records(clouds[k], step), k)
    st = store.egress_stats()
    total = sum(len(clouds[k]) for k in keys) * step
    assert (st["launches"], st["host_waits"], st["bytes_down"]) == ((1 if step == 32 else 0), 1, total)  # the whole list: one launch at most, one wait
    assert store.read([], step) == [] and store.read([10], step)[0].shape == (0, step)


@pytest.mark.parametrize("step", [32, 16])
def test_read_refusals(read_store, step):
    from mrg_slam_amd import _lib

    store, clouds = read_store
    L = _lib.lib()

    def raw(keys, step, data, capacity, offs):
        ks = np.asarray(keys, dtype=np.uint64)
        return L.mrgfe_map_store_read(store._h, len(keys), ks.ctypes.data_as(C.POINTER(C.c_uint64)), step, data.ctypes.data_as(C.c_void_p), capacity,
                                      offs.ctypes.data_as(C.POINTER(C.c_uint64)))

    keys = [12, 999, 13]
    need = (255 + 256) * step
    data, offs = np.full(need + 256 * step, 0x5A, np.uint8), np.full(4, 7, np.uint64)
    assert raw(keys, step, data, len(data), offs) == INVALID and (data == 0x5A).all() and (offs == 7).all()  # unknown key: nothing written
    keys = [12, 13]
    offs = np.full(3, 7, np.uint64)
    assert raw(keys, step, data, need - 1, offs) == INVALID and (data == 0x5A).all()  # short capacity: the offsets say what is needed
    assert offs.tolist() == [0, 255 * step, need]
    assert raw(keys, 24, data, len(data), offs) == INVALID
    assert raw(keys, step, data, need, offs) == 0
    same_bytes(data[:need], np.concatenate([records(clouds[12], step), records(clouds[13], step)]))
    assert (data[need:] == 0x5A).all()


def test_map_publisher_over_the_real_store(world, tmp_path):
    from mrg_slam_amd import MapCloudStore, MapPublisher, MapRequest
    from mrg_slam_amd.io import read_pcd

    store = MapCloudStore(world["ctx"])
    for key, c in zip(KEYS, world["clouds"]):
        store.add(key, c)
    pub = MapPublisher(store, map_cloud_resolution=0.5, map_cloud_min_points_per_voxel=1, zero_utm=UTM, zero_enu=ENU)
    assert pub.update() is None and not pub.updated  # nothing to publish yet
    pub.set_snapshot(list(zip(KEYS, world["poses"], FIRST)))
    first = pub.update()
    assert pub.updated and first["frame_id"] == "map"
    same_bytes(first["data"], records(world["oracle"][PARAMS[0][0]], 32))
    stats = store.egress_stats()
    again = pub.update()
    assert again is first and not pub.updated and store.egress_stats() == stats  # the cached message, no call
    # save_map: generate plus the two offsets, as a PCD that reads back
    req = MapRequest(resolution=0.0, min_points_per_voxel=3, distance_far_thresh=6.0, utm=True)  # resolution 0: the config's 0.5
    path = str(tmp_path / "maps" / "map.pcd")
    assert pub.save_map(req, path)
    want = add_offsets(store.generate(KEYS, world["poses"], FIRST, resolution=0.5, min_points_per_voxel=3, distance_far_thresh=6.0), (UTM, ENU))
    got = read_pcd(path)
    assert len(got) == PARAMS[1][1] and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert open(path + ".utm").read() == "364000.250000 5621000.500000 31.125000\n"
    msg = pub.publish_map(MapRequest(resolution=0.5, min_points_per_voxel=1, distance_far_thresh=-1.0, skip_first_cloud=True, frame_id="odom"))
    assert msg["frame_id"] == "odom"
    same_bytes(msg["data"], records(world["oracle"][PARAMS[3][0]], 32))
