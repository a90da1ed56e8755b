"""GPU: mrgfe_map_store_add_keyframes — many PointCloud2 keyframe messages into the map store in one call (one arena block, one launch driven by a
tile table, one wait) — against mrgfe_keyframe_callback with 0 centres message by message: every stored cloud byte for byte, the byte count, the
known-key rules, failures that leave the store as it was, and a batch fed from a bulk-filled store."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
SIZES = [0, 1, 255, 2047, 2048, 2049, 4097]  # around the 2048-point tile: none, one partial, one full, one full + 1 point, two full + 1
LAYOUTS = ["packed", "pcl32", "rows48", "no_intensity"]


def cloud_of(n, seed=0):
    """Seeded random, with a few NaN / inf points (their bit patterns must arrive as they are)."""
    rng = np.random.default_rng(4000 + 13 * n + seed)
    c = rng.normal(0, 5, (n, 4)).astype(np.float32)
    if n >= 8:
        c[n // 7, 0] = np.nan
        c[n // 3, 1] = np.inf
        c[n - 1, 2] = -np.inf
        c[n // 2] = np.nan
    return c


def message(cloud, layout):
    """The cloud as a PointCloud2 dict in one of four layouts, and the packed cloud the message stands for."""
    c = np.ascontiguousarray(cloud, dtype=np.float32)
    n = len(c)
    if layout == "packed":
        return {"data": c.tobytes(), "width": n, "height": 1, "point_step": 16, "fields": FIELDS, "row_step": 0}, c
    if layout == "pcl32":  # pcl::PointXYZI in memory: 32 bytes, intensity at byte 16, padding filled with NaN bit patterns
        rec = np.full((n, 8), np.nan, dtype=np.float32)
        rec[:, :3], rec[:, 4] = c[:, :3], c[:, 3]
        return {"data": rec.tobytes(), "width": n, "height": 1, "point_step": 32, "fields": {"x": 0, "y": 4, "z": 8, "intensity": 16}, "row_step": 0}, c
    if layout == "rows48":  # 48-byte records (x y z at 16, intensity at 36), height 2, every row padded by 80 bytes the message does not describe
        h = 2
        w = (n + 1) // 2
        full = np.full((h * w, 4), 7.0, dtype=np.float32)  # (an odd count is padded to 2 x w points: the message stands for the padded cloud)
        full[:n] = c
        rec = np.full((h * w, 12), np.nan, dtype=np.float32)
        rec[:, 4:7], rec[:, 9] = full[:, :3], full[:, 3]
        rows = np.full((h, w * 48 + 80), 0xFF, dtype=np.uint8)
        rows[:, : w * 48] = rec.view(np.uint8).reshape(h, w * 48)
        return {"data": rows.tobytes(), "width": w, "height": h, "point_step": 48, "fields": {"x": 16, "y": 20, "z": 24, "intensity": 36}, "row_step": w * 48 + 80}, full
    if layout == "no_intensity":  # off_intensity < 0: the stored intensity is 0
        c0 = c.copy()
        c0[:, 3] = 0.0
        rec = np.full((n, 5), np.nan, dtype=np.float32)
        rec[:, 1:4] = c[:, :3]
        return {"data": rec.tobytes(), "width": n, "height": 1, "point_step": 20, "fields": {"x": 4, "y": 8, "z": 12}, "row_step": 0}, c0
    raise ValueError(layout)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def stored(store, key):
    """The stored cloud, read back through map generation with no voxel filter, no distance cut and the identity pose."""
    n = store.has(key)
    assert n is not None
    if n == 0:
        return np.zeros((0, 4), np.float32)
    return store.generate([key], [np.eye(4)], None, 0.0, distance_far_thresh=0.0)


def check_call(items, wants):
    """One bulk call into a fresh store against the callback, message by message, into another."""
    from mrg_slam_amd import MapCloudStore

    bulk, single = MapCloudStore(), MapCloudStore()
    before = bulk.bytes()
    added = bulk.add_keyframes(items)
    assert added.dtype == np.uint8 and list(added) == [1] * len(items)
    points = 0
    for (key, msg), want in zip(items, wants):
        single.keyframe_callback(key, msg, want_kept=False)
        assert bulk.has(key) == single.has(key) == len(want)
        got = stored(bulk, key)
        same(got, stored(single, key))
        # ... and the message's own points: the read-back multiplies by the identity pose, which leaves a finite point's bits alone (0 * inf is NaN)
        finite = np.isfinite(want[:, :3]).all(axis=1)
        same(got[finite], want[finite])
        assert np.isnan(got[~finite, :3]).any(axis=1).all() and np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32))
        points += len(want)
    assert bulk.bytes() - before == 16 * points == single.bytes()
    return bulk


def test_seven_sizes_with_mixed_layouts_in_one_call():
    items, wants = [], []
    for i, n in enumerate(SIZES):
        msg, want = message(cloud_of(n), LAYOUTS[i % 4])
        items.append((100 + i, msg))
        wants.append(want)
    check_call(items, wants)
    # the same sizes with the layouts rotated, largest first (tiles of a long message in front of the short ones)
    items, wants = [], []
    for i, n in enumerate(reversed(SIZES)):
        msg, want = message(cloud_of(n, 1), LAYOUTS[(i + 3) % 4])
        items.append((200 + i, msg))
        wants.append(want)
    check_call(items, wants)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_calls_of_one_message(layout):
    for n in SIZES:
        msg, want = message(cloud_of(n, 2), layout)
        check_call([(5, msg)], [want])


def test_three_hundred_small_keyframes_in_one_call():
    items, wants = [], []
    for i in range(300):
        msg, want = message(cloud_of(3, i), LAYOUTS[i % 4])
        items.append((1000 + i, msg))
        wants.append(want)
    bulk = check_call(items, wants)
    assert bulk.bytes() == 16 * sum(len(w) for w in wants)


def test_known_keys_are_skipped_and_another_count_is_refused():
    from mrg_slam_amd import MapCloudStore, MrgfeError, _lib

    store = MapCloudStore()
    a, b, c = (message(cloud_of(n, 3), lay) for n, lay in ((700, "packed"), (2049, "pcl32"), (300, "no_intensity")))
    store.keyframe_callback(1, a[0], want_kept=False)
    before = store.bytes()
    # key 1 is stored (same count: skipped), key 2 comes twice (the second is skipped, whatever its points are), key 3 is new
    b_other = message(cloud_of(2049, 99), "packed")
    added = store.add_keyframes([(1, a[0]), (2, b[0]), (3, c[0]), (2, b_other[0])])
    assert list(added) == [0, 1, 1, 0]
    assert store.bytes() - before == 16 * (2049 + 300)
    ref = MapCloudStore()
    for key, m in ((1, a), (2, b), (3, c)):
        ref.keyframe_callback(key, m[0], want_kept=False)
        same(stored(store, key), stored(ref, key))
    assert list(store.add_keyframes([(3, c[0]), (1, a[0])])) == [0, 0] and store.bytes() - before == 16 * (2049 + 300)
    assert len(store.add_keyframes([])) == 0
    state = (store.bytes(), store.has(1), store.has(2), store.has(3))
    for items in ([(9, a[0]), (2, message(cloud_of(10), "packed")[0])],                           # a stored key with another count
                  [(9, a[0]), (10, c[0]), (9, message(cloud_of(701), "packed")[0])]):            # a repeat inside the call with another count
        with pytest.raises(MrgfeError) as e:
            store.add_keyframes(items)
        assert e.value.status == _lib.ERR_STATE and "mrgfe_map_store_add_keyframes" in str(e.value)
        assert (store.bytes(), store.has(1), store.has(2), store.has(3)) == state and store.has(9) is None and store.has(10) is None
    with pytest.raises(MrgfeError) as e:
        store.add_keyframes([(9, a[0]), (0, c[0])])  # key 0
    assert e.value.status == _lib.ERR_INVALID and store.has(9) is None and store.bytes() == state[0]


def test_a_bad_message_among_seven_leaves_the_store_unchanged():
    from mrg_slam_amd import MapCloudStore, MrgfeError, _lib

    store = MapCloudStore()
    first, _ = message(cloud_of(500, 4), "packed")
    store.keyframe_callback(1, first, want_kept=False)
    state = (store.bytes(), store.has(1))
    msgs = [message(cloud_of(n, 5), LAYOUTS[i % 4]) for i, n in enumerate([2049, 1, 4097, 255, 2048, 0, 2047])]
    good = msgs[3][0]
    bad = [dict(good, data=good["data"][:-1]),                                                  # a short payload
           dict(good, fields={"x": 4, "y": 8, "z": 12, "intensity": 20}),                       # an offset outside point_step
           dict(good, fields={"x": 4, "y": 10, "z": 12}),                                       # ... not a multiple of 4
           dict(good, row_step=good["width"] * good["point_step"] - 4)]                         # a row shorter than its points
    for b in bad:
        items = [(10 + i, (b if i == 3 else m[0])) for i, m in enumerate(msgs)]  # message 4 of 7
        with pytest.raises(MrgfeError) as e:
            store.add_keyframes(items)
        assert e.value.status == _lib.ERR_INVALID
        assert (store.bytes(), store.has(1)) == state and all(store.has(10 + i) is None for i in range(7))
    # the same seven, all good, afterwards
    added = store.add_keyframes([(10 + i, m[0]) for i, m in enumerate(msgs)])
    assert list(added) == [1] * 7 and store.bytes() - state[0] == 16 * sum(len(m[1]) for m in msgs)
    ref = MapCloudStore()
    ref.keyframe_callback(1, first, want_kept=False)
    same(stored(store, 1), stored(ref, 1))
    for i, m in enumerate(msgs):
        ref.keyframe_callback(10 + i, m[0], want_kept=False)
        same(stored(store, 10 + i), stored(ref, 10 + i))


def test_the_added_flags_are_cleared_when_the_call_fails():
    from mrg_slam_amd import MapCloudStore, _lib
    from mrg_slam_amd.map_cloud import keyframe_params

    store = MapCloudStore()
    msg, _ = message(cloud_of(100, 6), "packed")
    buf = np.frombuffer(msg["data"], dtype=np.uint8)
    recs = (_lib.KeyframeMsg * 2)()
    for i, key in enumerate((4, 0)):  # the second message has key 0
        recs[i].key, recs[i].layout, recs[i].data, recs[i].data_bytes = key, keyframe_params(msg), buf.ctypes.data, buf.nbytes
    added = (C.c_uint8 * 2)(9, 9)
    assert _lib.lib().mrgfe_map_store_add_keyframes(store._h, 2, recs, added) == _lib.ERR_INVALID
    assert list(added) == [0, 0] and store.has(4) is None and store.bytes() == 0
    recs[1].key = 5
    assert _lib.lib().mrgfe_map_store_add_keyframes(store._h, 2, recs, None) == 0  # the flags are optional
    assert store.has(4) == store.has(5) == 100


def test_a_batch_from_a_bulk_filled_store_gives_the_same_records():
    """Two small NDT pairs named by key: a store filled by ONE bulk call against a store filled one callback at a time, raw 384-byte records."""
    from mrg_slam_amd import BatchMatcher, MapCloudStore, _lib, synth
    from mrg_slam_amd.registration import default_params
    from oracle.replay import small_cloud

    prm = default_params(_lib.NDT_HIP)
    prm.transformation_epsilon = 0.01
    world = small_cloud(6000, 21)
    clouds = {}
    for k in range(4):
        T = np.linalg.inv(synth.make_pose([0.3 * k, 0.1 * k, 0.0], synth.rot_z(0.02 * k)))
        c = world[np.sort(np.random.default_rng(60 + k).choice(len(world), 2500 + 100 * k, replace=False))].copy()
        c[:, :3] = (c[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        clouds[k + 1] = c
    bulk, single = MapCloudStore(), MapCloudStore()
    items = [(k, message(c, LAYOUTS[k % 2])[0]) for k, c in clouds.items()]
    assert list(bulk.add_keyframes(items)) == [1, 1, 1, 1]
    for k, m in items:
        single.keyframe_callback(k, m, want_kept=False)
    recs = []
    for store in (bulk, single):
        b = BatchMatcher(prm)
        for tgt, src in ((1, 2), (3, 4)):
            t = b.add_target_from_store(store, tgt)
            b.add_pair_from_store(t, store, src, np.eye(4))
        res = b.align(float("inf"))
        assert res["iterations"].max() >= 1 and np.isfinite(res["fitness"]).all()
        recs.append(np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=np.uint8).reshape(len(res), 384).copy())
        del b  # (the batch goes before the store it reads)
    assert recs[0].shape == (2, 384) and np.array_equal(recs[0], recs[1])
