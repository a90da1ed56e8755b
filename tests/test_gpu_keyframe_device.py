"""GPU: ``mrgfe_keyframe_callback_device`` — the keyframe callback for a filtered scan that is already in HBM (all components in one container) — against
``mrgfe_keyframe_callback`` on the bytes of the same cloud in the packed layout: two stores per case, one fed by each form; kept and removed clouds, both
counts, the store's byte count and the stored cloud are compared bit for bit, the refusals status for status, and a batch that reads the two stores by
key gives the same 384-byte record."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
SIZES = [0, 1, 255, 2048, 2049]  # the tile (2048) edges of the partition, one workgroup short of full, the trivial ones
RADIUS = 1.5
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_small.npz"))
_fp = C.POINTER(C.c_float)


def cloud_of(n, seed=0):
    rng = np.random.default_rng(2000 + 7 * n + seed)
    c = rng.normal(0, 4, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    return c  # (finite points only: generate() multiplies by the pose and cuts by distance, which does not keep a NaN's payload or an infinity)


def centres_of(k, seed=0):
    return np.random.default_rng(70 + k + seed).normal(0, 3, (k, 3)).astype(np.float32)


def packed_msg(cloud):
    c = np.ascontiguousarray(cloud, dtype=np.float32)
    return {"data": c.tobytes(), "width": len(c), "height": 1, "point_step": 16, "fields": FIELDS, "row_step": 0}


def to_device(cloud, ctx=None):
    """The cloud in a torch buffer, put there by the library's own ingest (``mrgfe_ingest_pointcloud2`` with a device output)."""
    import torch

    from mrg_slam_amd.io import ingest_pointcloud2

    buf = torch.empty((max(len(cloud), 1), 4), dtype=torch.float32, device="cuda")
    if len(cloud):
        ingest_pointcloud2(np.ascontiguousarray(cloud).tobytes(), len(cloud), 1, 16, FIELDS, ctx=ctx, dev_ptr=buf.data_ptr())
    return buf


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def raw_device(store, key, ptr, n, centres, radius_sqr):
    """mrgfe_keyframe_callback_device as it is: (status, kept, removed)."""
    from mrg_slam_amd import _lib

    ctr = np.ascontiguousarray(np.asarray(centres, dtype=np.float32).reshape(-1, 3))
    cap = min(int(n), 1 << 20)
    kept, removed = np.empty((cap, 4), np.float32), np.empty((cap, 4), np.float32)
    nk, nr = C.c_size_t(99), C.c_size_t(99)
    st = _lib.lib().mrgfe_keyframe_callback_device(store._h, key, C.c_void_p(ptr) if ptr else None, n, ctr.ctypes.data_as(_fp) if len(ctr) else None, len(ctr), float(radius_sqr),
                                                   kept.ctypes.data_as(_fp), C.byref(nk), removed.ctypes.data_as(_fp), C.byref(nr))
    return st, kept[: nk.value], removed[: nr.value]


@pytest.mark.parametrize("n", SIZES)
def test_equals_the_bytes_form(n):
    from mrg_slam_amd import Context, MapCloudStore

    ctx = Context()
    by_bytes, by_device = MapCloudStore(ctx), MapCloudStore(ctx)
    cloud = cloud_of(n)
    dev = to_device(cloud, ctx)
    far = np.full((1, 3), 1000.0, np.float32)
    # (centres, radius): none, one, sixty-four; a radius that keeps nothing, one that removes nothing
    cases = [(centres_of(0), RADIUS), (centres_of(1), 3.0), (centres_of(64), RADIUS), (centres_of(1), 1e6), (centres_of(64), 1e6), (far, RADIUS), (centres_of(64) + 1000.0, RADIUS)]
    removed_some = 0
    for key, (centres, radius) in enumerate(cases, start=1):
        a_kept, a_removed = by_bytes.keyframe_callback(key, packed_msg(cloud), centres, radius, want_kept=True, want_removed=True)
        b_kept, b_removed = by_device.keyframe_callback_device(key, dev.data_ptr(), n, centres, radius, want_kept=True, want_removed=True)
        what = (n, len(centres), radius)
        same(a_kept, b_kept, what)
        same(a_removed, b_removed, what)
        assert len(b_kept) + len(b_removed) == n, what
        assert by_bytes.has(key) == by_device.has(key) == len(b_kept) and by_bytes.bytes() == by_device.bytes(), what
        same(by_bytes.generate([key], [np.eye(4)], None, 0.0), by_device.generate([key], [np.eye(4)], None, 0.0), what)
        same(by_device.generate([key], [np.eye(4)], None, 0.0), b_kept, what)
        if radius == 1e6:
            assert len(b_kept) == 0 and len(b_removed) == n, what
        if len(centres) == 0 or float(centres[0, 0]) > 500.0:
            assert len(b_removed) == 0, what
            same(b_kept, cloud, what)
        removed_some += 0 < len(b_removed) < n
    assert n < 255 or removed_some >= 2  # the split cases split
    # the caller's buffer was only read
    same(dev[:n].cpu().numpy(), cloud)
    # outputs that are not wanted: the same counts and the same stored cloud
    none_kept, none_removed = by_device.keyframe_callback_device(100, dev.data_ptr(), n, centres_of(64), RADIUS, want_kept=False, want_removed=False)
    assert none_kept is None and none_removed is None
    same(by_device.generate([100], [np.eye(4)], None, 0.0), by_device.generate([3], [np.eye(4)], None, 0.0))


def test_a_buffer_filled_by_the_scan_callback():
    """The one-container route: ``mrgfe_scan_callback_device`` leaves the filtered scan in the buffer, the keyframe callback reads it there."""
    import torch

    from mrg_slam_amd import MapCloudStore, scan_callback_to_device, synth

    raw = synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 7400)
    buf = torch.empty((len(raw), 4), dtype=torch.float32, device="cuda")
    n = scan_callback_to_device(np.ascontiguousarray(raw).tobytes(), len(raw), 1, 16, FIELDS, buf.data_ptr(), len(raw))
    assert 2049 < n < len(raw)
    filtered = buf[:n].cpu().numpy()
    centres = np.array([[4.0, 1.0, -1.0], [-6.0, -3.0, 0.0]], np.float32)
    by_bytes, by_device = MapCloudStore(), MapCloudStore()
    a = by_bytes.keyframe_callback(1, packed_msg(filtered), centres, 3.0, want_removed=True)
    b = by_device.keyframe_callback_device(1, buf.data_ptr(), n, centres, 3.0, want_removed=True)
    same(a[0], b[0])
    same(a[1], b[1])
    assert 0 < len(b[1]) < n and by_bytes.bytes() == by_device.bytes() == 16 * len(b[0])
    same(by_bytes.generate([1], [np.eye(4)], None, 0.0), by_device.generate([1], [np.eye(4)], None, 0.0))


def test_refusals_leave_the_store_unchanged():
    from mrg_slam_amd import MapCloudStore, _lib

    store = MapCloudStore()
    cloud = cloud_of(3000, 2)
    dev = to_device(cloud)
    ptr, n = dev.data_ptr(), len(cloud)
    centres = centres_of(2)
    st, kept0, removed0 = raw_device(store, 1, ptr, n, centres, 2.25)
    assert st == 0 and len(kept0) + len(removed0) == n
    state = (store.bytes(), store.has(1))

    def refused(status, key, p, count, ctr):
        st, kept, removed = raw_device(store, key, p, count, ctr, 2.25)
        assert st == status and _lib.last_error().startswith("mrgfe_keyframe_callback_device:"), (st, _lib.last_error())
        assert len(kept) == 0 and len(removed) == 0  # both counts are zeroed
        assert (store.bytes(), store.has(1)) == state and (key == 1 or store.has(key) is None)

    refused(_lib.ERR_INVALID, 2, ptr, n, centres_of(65))  # 65 centres
    refused(_lib.ERR_INVALID, 0, ptr, n, centres)         # key 0
    refused(_lib.ERR_STATE, 1, ptr, n, centres)           # a stored key
    refused(_lib.ERR_STATE, 1, ptr, 10, np.zeros((0, 3)))
    refused(_lib.ERR_INVALID, 2, 0, n, centres)           # a NULL pointer with points
    refused(_lib.ERR_INVALID, 2, ptr, 1 << 31, centres)   # more than 2^31 - 1 points
    host = cloud.copy()
    refused(_lib.ERR_INVALID, 2, host.ctypes.data, n, centres)           # host memory: refused, not read
    refused(_lib.ERR_INVALID, 2, host.ctypes.data, n, np.zeros((0, 3)))
    # a good call afterwards, under the key the refused calls named; an empty cloud needs no pointer
    st, kept, removed = raw_device(store, 2, ptr, n, centres, 2.25)
    assert st == 0 and store.has(2) == len(kept) and store.bytes() == state[0] + 16 * len(kept)
    same(kept, kept0)
    same(removed, removed0)
    st, kept, removed = raw_device(store, 3, 0, 0, centres, 2.25)
    assert st == 0 and store.has(3) == 0 and len(kept) == 0 and len(removed) == 0


def test_a_batch_reads_both_stores_alike():
    """One NDT_HIP record: the target and the pair named by key in a store filled by the bytes form and in one filled by the device form."""
    from mrg_slam_amd import BatchMatcher, MapCloudStore, _lib
    from mrg_slam_amd.registration import default_params

    prm = default_params(_lib.NDT_HIP)
    prm.transformation_epsilon = 0.01
    tgt, src = np.ascontiguousarray(G["tgt"]), np.ascontiguousarray(G["src"])
    by_bytes, by_device = MapCloudStore(), MapCloudStore()
    devs = [to_device(tgt), to_device(src)]
    for key, (cloud, dev) in enumerate(zip((tgt, src), devs), start=1):
        by_bytes.keyframe_callback(key, packed_msg(cloud), want_kept=False)
        by_device.keyframe_callback_device(key, dev.data_ptr(), len(cloud), want_kept=False)
    recs = []
    for store in (by_bytes, by_device):
        b = BatchMatcher(prm)
        t = b.add_target_from_store(store, 1)
        b.add_pair_from_store(t, store, 2, G["guess"])
        res = b.align(float("inf"))
        assert res["iterations"].max() >= 1 and np.isfinite(res["fitness"]).all()
        recs.append(np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=np.uint8).copy())
        del b  # (the batch goes before the store it reads)
    assert recs[0].shape == (384,) and np.array_equal(recs[0], recs[1])


def test_callback_mirror_on_device_clouds():
    """KeyframeCallback.cloud_callback_device over a short odometry sequence stores the same keys and clouds as cloud_callback on the messages: the same
    KeyframeUpdater decision, the same centres."""
    from mrg_slam_amd import MapCloudStore, synth
    from mrg_slam_amd.keyframes import KeyframeCallback
    from oracle.replay import small_cloud

    stores = [MapCloudStore(), MapCloudStore()]
    cbs = [KeyframeCallback(store=s) for s in stores]
    rng = np.random.default_rng(3)
    odom, results = np.eye(4), [[], []]
    for step in range(12):
        odom = odom @ synth.make_pose([rng.uniform(0.2, 0.9), 0.0, 0.0], synth.rot_z(rng.normal(0, 0.1)))
        cloud = small_cloud(2600 + 10 * step, 60 + step)
        dev = to_device(cloud)
        for cb in cbs:
            if step == 4:  # two other robots appear, one of them close
                cb.others_odom_poses = {"b": odom[:3, 3] + [3.0, 1.0, 0.0], "c": odom[:3, 3] + [-40.0, 5.0, 0.0]}
                cb.trans_odom2map = synth.make_pose([0.2, -0.1, 0.0], synth.rot_z(0.02))
        results[0].append(cbs[0].cloud_callback(odom, packed_msg(cloud), removed_points_wanted=(step % 2 == 0)))
        results[1].append(cbs[1].cloud_callback_device(odom, dev.data_ptr(), len(cloud), removed_points_wanted=(step % 2 == 0)))
    assert [r is None for r in results[0]] == [r is None for r in results[1]]
    taken = [(a, b) for a, b in zip(*results) if a is not None]
    assert 4 <= len(taken) < 12
    removed_seen = 0
    for a, b in taken:
        assert a.key == b.key and a.accum_distance == b.accum_distance
        np.testing.assert_array_equal(a.centres_sensor, b.centres_sensor)
        assert (a.kept is None) == (b.kept is None) and (a.removed is None) == (b.removed is None)
        if a.kept is not None:
            same(a.kept, b.kept)
        if a.removed is not None:
            same(a.removed, b.removed)
            removed_seen += len(a.removed)
        same(stores[0].generate([a.key], [np.eye(4)], None, 0.0), stores[1].generate([a.key], [np.eye(4)], None, 0.0))
    assert removed_seen > 0 and stores[0].bytes() == stores[1].bytes() > 0
