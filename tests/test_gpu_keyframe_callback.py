"""GPU: mrgfe_keyframe_callback — PointCloud2 bytes to keyframe `key` of the map store in one call — against the route it stands for
(mrgfe_ingest_pointcloud2 -> mrgfe_remove_points_near), the CPU oracle's removal and a numpy restatement, bit for bit and in order; the state it
leaves in the store; and mrgfe_batch_add_target_from_store / _pair_from_store against the same batch fed from host pointers (raw 384-byte records)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 3 * 2048 + 5]  # the wave (64), workgroup (256) and tile (2048) edges
CENTRE_COUNTS = [0, 1, 2, 64]
RADIUS = 1.5
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_small.npz"))


def cloud_of(n, seed=0):
    rng = np.random.default_rng(1000 + 7 * n + seed)
    c = rng.normal(0, 4, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    return c


def centres_of(k, seed=0):
    return np.random.default_rng(50 + k + seed).normal(0, 3, (k, 3)).astype(np.float32)


def message(cloud, layout):
    """The cloud as a PointCloud2 in one of the four layouts, and the packed cloud the message stands for."""
    from mrg_slam_amd.io import pcl_xyzi_records

    c = np.ascontiguousarray(cloud, dtype=np.float32)
    n = len(c)
    if layout == "packed":
        return {"data": c.tobytes(), "width": n, "height": 1, "point_step": 16, "fields": FIELDS, "row_step": 0}, c
    if layout == "pcl32":  # the reference's in-memory pcl::PointXYZI records, intensity at byte 16
        return {"data": pcl_xyzi_records(c).tobytes(), "width": n, "height": 1, "point_step": 32, "fields": {"x": 0, "y": 4, "z": 8, "intensity": 16}, "row_step": 0}, c
    if layout == "organised":  # rows padded by 48 bytes the message does not describe (NaN bit patterns: they must not be read)
        h = next((f for f in (16, 5, 3, 2) if n and n % f == 0), 1)
        w = n // h
        rows = np.full((h, w * 16 + 48), 0xFF, dtype=np.uint8)
        rows[:, : w * 16] = c.view(np.uint8).reshape(h, w * 16)
        return {"data": rows.tobytes(), "width": w, "height": h, "point_step": 16, "fields": FIELDS, "row_step": w * 16 + 48}, c
    if layout == "no_intensity":  # 12-byte x, y, z records: the cloud has intensity 0
        c0 = c.copy()
        c0[:, 3] = 0.0
        return {"data": np.ascontiguousarray(c[:, :3]).tobytes(), "width": n, "height": 1, "point_step": 12, "fields": {"x": 0, "y": 4, "z": 8}, "row_step": 0}, c0
    raise ValueError(layout)


def numpy_split(cloud, centres, radius_sqr):
    """apps/mrg_slam_component.cpp:412-423 in float32: (p - c).squaredNorm() < radius_sqr, every operation rounded, no fusing."""
    gone = np.zeros(len(cloud), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in np.asarray(centres, dtype=np.float32).reshape(-1, 3):
            d = cloud[:, :3] - c
            s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            s = s + d[:, 2] * d[:, 2]
            gone |= s < np.float32(radius_sqr)
    return cloud[~gone], cloud[gone]


def composed(msg, centres, radius, ctx=None):
    """The route the one call replaces: pcl::fromROSMsg on the GPU, the cloud down, up again into the removal, kept and removed down."""
    from mrg_slam_amd import remove_points_near
    from mrg_slam_amd.io import ingest_pointcloud2

    c = ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"], ctx=ctx)
    return remove_points_near(c, centres, radius, ctx=ctx)


def same(a, b):
    """Bit-equal clouds (NaN payloads included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def raw_callback(store, key, msg, centres, radius_sqr, want_kept=True, want_removed=True):
    """mrgfe_keyframe_callback with radius_sqr given as it is: (status, kept, removed)."""
    from mrg_slam_amd import _lib
    from mrg_slam_amd.map_cloud import keyframe_params

    p = keyframe_params(msg)
    n = int(p.width) * int(p.height)
    buf = np.frombuffer(msg["data"], dtype=np.uint8)
    ctr = np.ascontiguousarray(np.asarray(centres, dtype=np.float32).reshape(-1, 3))
    kept, removed = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32)
    fp = C.POINTER(C.c_float)
    nk, nr = C.c_size_t(99), C.c_size_t(99)
    st = _lib.lib().mrgfe_keyframe_callback(store._h, key, C.byref(p), buf.ctypes.data_as(C.c_void_p) if len(buf) else None, buf.nbytes, ctr.ctypes.data_as(fp) if len(ctr) else None,
                                            len(ctr), float(radius_sqr), kept.ctypes.data_as(fp) if want_kept else None, C.byref(nk),
                                            removed.ctypes.data_as(fp) if want_removed else None, C.byref(nr))
    return st, kept[: nk.value], removed[: nr.value]


@pytest.mark.parametrize("layout", ["packed", "pcl32", "organised", "no_intensity"])
def test_equals_the_composed_route_the_oracle_and_numpy(layout):
    from mrg_slam_amd import Context, MapCloudStore
    from oracle import oracle as orc

    ctx = Context()
    store = MapCloudStore(ctx)
    key, some_removed, some_kept = 0, 0, 0
    for n in SIZES:
        cloud = cloud_of(n)
        msg, want_cloud = message(cloud, layout)
        for k in CENTRE_COUNTS:
            centres = centres_of(k)
            key += 1
            before = store.bytes()
            kept, removed = store.keyframe_callback(key, msg, centres, RADIUS)
            ckept, cremoved = composed(msg, centres, RADIUS, ctx=ctx)
            print(f"{layout}: n {n} K {k} -> kept {len(kept)} removed {len(removed)}")
            same(kept, ckept)
            same(removed, cremoved)
            okept, oremoved = orc.remove_points_near(want_cloud, centres, RADIUS)
            same(kept, okept)
            same(removed, oremoved)
            nkept, nremoved = numpy_split(want_cloud, centres, np.float32(RADIUS * RADIUS))
            same(kept, nkept)
            same(removed, nremoved)
            assert len(kept) + len(removed) == n
            assert store.has(key) == len(kept) and store.bytes() - before == 16 * len(kept)
            some_removed += len(removed) > 0
            some_kept += len(kept) > 0
    assert some_removed >= 20 and some_kept >= 40  # the cases are not degenerate


def test_larger_cloud_and_outputs_that_are_not_wanted():
    """A keyframe-sized cloud (many tiles), and the NULL outputs: counts and the stored cloud do not depend on what is downloaded."""
    from mrg_slam_amd import MapCloudStore

    store = MapCloudStore()
    cloud = cloud_of(60 * 2048 + 77, 3)
    centres = centres_of(2, 9)
    msg, _ = message(cloud, "pcl32")
    nkept, nremoved = numpy_split(cloud, centres, 4.0)
    assert len(nremoved) > 1000
    for key, (wk, wr) in enumerate([(True, True), (False, True), (True, False), (False, False)], start=1):
        st, kept, removed = raw_callback(store, key, msg, centres, 4.0, wk, wr)
        assert st == 0 and len(kept) == len(nkept) and len(removed) == len(nremoved)
        if wk:
            same(kept, nkept)
        if wr:
            same(removed, nremoved)
        same(store.generate([key], [np.eye(4)], None, 0.0), nkept)
    assert store.bytes() == 4 * 16 * len(nkept)


def test_constructed_points():
    from mrg_slam_amd import MapCloudStore

    store = MapCloudStore()
    origin = np.zeros((1, 3), np.float32)
    p345 = np.array([[3.0, 4.0, 0.0, 0.5]], np.float32)
    # |p|^2 = 25 exactly: not < 25 -> kept; < nextafter(25) -> removed
    st, kept, removed = raw_callback(store, 1, message(p345, "packed")[0], origin, 25.0)
    assert st == 0 and len(removed) == 0
    same(kept, p345)
    st, kept, removed = raw_callback(store, 2, message(p345, "packed")[0], origin, np.nextafter(np.float32(25.0), np.float32(np.inf)))
    assert st == 0 and len(kept) == 0 and store.has(2) == 0
    same(removed, p345)
    # a point inside two spheres is removed once; NaN and Inf points are kept
    pts = np.array([[0.1, 0.0, 0.0, 1.0], [np.nan, 0.0, 0.0, 2.0], [0.0, np.inf, 0.0, 3.0], [0.0, 0.0, -np.inf, 4.0], [9.0, 9.0, 9.0, 5.0], [0.0, 0.2, 0.0, 6.0], [np.nan, np.nan, np.nan, np.nan]],
                   np.float32)
    two = np.array([[0.0, 0.0, 0.0], [0.05, 0.05, 0.0]], np.float32)
    st, kept, removed = raw_callback(store, 3, message(pts, "pcl32")[0], two, 1.0)
    assert st == 0
    same(removed, pts[[0, 5]])
    same(kept, pts[[1, 2, 3, 4, 6]])
    # every point removed: the key is stored with 0 points; no point removed: the whole cloud
    cloud = cloud_of(5000, 1)
    before = store.bytes()
    st, kept, removed = raw_callback(store, 4, message(cloud, "packed")[0], origin, 1e12)
    assert st == 0 and len(kept) == 0 and store.has(4) == 0 and store.bytes() == before
    same(removed, cloud)
    assert len(store.generate([4], [np.eye(4)], None, 0.0)) == 0
    st, kept, removed = raw_callback(store, 5, message(cloud, "packed")[0], origin + 1000.0, 1.0)
    assert st == 0 and len(removed) == 0 and store.has(5) == 5000 and store.bytes() == before + 16 * 5000
    same(kept, cloud)


def test_store_state_after_the_callback():
    """What map generation and the edge information matrices read is the kept cloud: generate() with resolution <= 0 and the identity pose returns it
    exactly, and the information matrix between two keyframes equals the one between the same clouds entered by mrgfe_map_store_add."""
    from mrg_slam_amd import InformationMatrixCalculator, MapCloudStore, synth
    from oracle.replay import small_cloud

    a, b = small_cloud(5000, 31), small_cloud(4100, 32)
    centres = np.array([[2.0, 1.0, -1.0], [-6.0, -3.0, 0.0]], np.float32)
    one, two = MapCloudStore(), MapCloudStore()
    kept = {}
    for key, c in ((11, a), (12, b)):
        kept[key], removed = one.keyframe_callback(key, message(c, "pcl32")[0], centres, 4.0)
        assert len(removed) > 50 and len(kept[key]) > 3000
        assert one.has(key) == len(kept[key])
        same(one.generate([key], [np.eye(4)], None, 0.0), kept[key])
        two.add(key, kept[key])
    assert one.bytes() == two.bytes() == 16 * (len(kept[11]) + len(kept[12]))
    rel = synth.make_pose([0.3, -0.2, 0.05], synth.rot_xyz(0.01, -0.01, 0.05))
    calc = InformationMatrixCalculator()
    for k1, k2 in ((11, 12), (12, 11)):
        i1 = calc.calc_information_matrix_keyed(one, k1, k2, rel)
        f1 = calc.last_fitness_score
        i2 = calc.calc_information_matrix_keyed(two, k1, k2, rel)
        assert np.array_equal(i1, i2) and f1 == calc.last_fitness_score and np.isfinite(f1) and f1 > 0
    poses = [synth.make_pose([1.0, 2.0, 0.0], synth.rot_z(0.3)), synth.make_pose([-4.0, 0.5, 0.1], synth.rot_z(-1.0))]
    same(one.generate([11, 12], poses, [True, False], 0.2), two.generate([11, 12], poses, [True, False], 0.2))


def test_errors_leave_the_store_unchanged():
    from mrg_slam_amd import MapCloudStore, _lib

    store = MapCloudStore()
    cloud = cloud_of(3000, 2)
    msg, _ = message(cloud, "packed")
    centres = centres_of(2)
    st, kept0, _ = raw_callback(store, 1, msg, centres, 2.25)
    assert st == 0
    state = (store.bytes(), store.has(1))

    def refused(status, key, m, ctr, starts="mrgfe_keyframe_callback:"):
        st, kept, removed = raw_callback(store, key, m, ctr, 2.25)
        assert st == status and _lib.last_error().startswith(starts), (st, _lib.last_error())
        assert len(kept) == 0 and len(removed) == 0  # both counts are zeroed
        assert (store.bytes(), store.has(1)) == state and (key == 1 or store.has(key) is None)

    refused(_lib.ERR_INVALID, 2, msg, centres_of(65))               # 65 centres
    refused(_lib.ERR_STATE, 1, msg, centres)                        # a duplicate key
    refused(_lib.ERR_STATE, 1, message(cloud[:10], "packed")[0], np.zeros((0, 3)))
    refused(_lib.ERR_INVALID, 0, msg, centres)                      # key 0
    refused(_lib.ERR_INVALID, 2, dict(msg, data=msg["data"][:-1]), centres)          # a short payload
    refused(_lib.ERR_INVALID, 2, dict(msg, data=msg["data"][: 16 * 2999]), np.zeros((0, 3)))
    refused(_lib.ERR_INVALID, 2, dict(msg, fields={"x": 0, "y": 4, "z": 8, "intensity": 16}), centres)  # an offset outside point_step
    refused(_lib.ERR_INVALID, 2, dict(msg, fields={"x": 0, "y": 6, "z": 8, "intensity": 12}), centres)  # ... not a multiple of 4
    refused(_lib.ERR_INVALID, 2, dict(msg, row_step=16 * 3000 - 4), centres)         # a row shorter than its points
    # a good call afterwards, under the key the refused calls named
    st, kept, _ = raw_callback(store, 2, msg, centres, 2.25)
    assert st == 0 and store.has(2) == len(kept) and store.bytes() == state[0] + 16 * len(kept)
    same(kept, kept0)
    same(store.generate([1], [np.eye(4)], None, 0.0), kept0)


def test_callback_mirror_over_the_one_call_and_the_composed_ops():
    """KeyframeCallback (apps/mrg_slam_component.cpp:358-456) runs the SAME control flow over the one call and over the composed route
    (ingest -> removal -> map_store_add): same keyframes, same clouds, same store contents."""
    from mrg_slam_amd import MapCloudStore, remove_points_near, synth
    from mrg_slam_amd.io import ingest_pointcloud2
    from mrg_slam_amd.keyframes import KeyframeCallback
    from oracle.replay import small_cloud

    class ComposedOps:
        def __init__(self, store):
            self.store = store

        def keyframe(self, key, msg, centres, radius, want_removed):
            c = ingest_pointcloud2(msg["data"], msg["width"], msg["height"], msg["point_step"], msg["fields"], msg["row_step"])
            kept, removed = remove_points_near(c, centres, radius) if len(centres) else (c, None)
            self.store.add(key, kept)
            return kept, (removed if want_removed else None)

    stores = [MapCloudStore(), MapCloudStore()]
    cbs = [KeyframeCallback(store=stores[0]), KeyframeCallback(ops=ComposedOps(stores[1]))]
    rng = np.random.default_rng(3)
    odom, results = np.eye(4), [[], []]
    for step in range(12):
        odom = odom @ synth.make_pose([rng.uniform(0.2, 0.9), 0.0, 0.0], synth.rot_z(rng.normal(0, 0.1)))
        msg, _ = message(small_cloud(2600 + 10 * step, 60 + step), "pcl32")
        for cb, out in zip(cbs, results):
            if step == 4:  # two other robots appear, one of them close
                cb.others_odom_poses = {"b": odom[:3, 3] + [3.0, 1.0, 0.0], "c": odom[:3, 3] + [-40.0, 5.0, 0.0]}
                cb.trans_odom2map = synth.make_pose([0.2, -0.1, 0.0], synth.rot_z(0.02))
            out.append(cb.cloud_callback(odom, msg, removed_points_wanted=(step % 2 == 0)))
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


def records(res):
    return np.frombuffer(np.ascontiguousarray(res).tobytes(), dtype=np.uint8).reshape(len(res), 384)


@pytest.mark.parametrize("method", ["NDT_HIP", "GICP_HIP", "SMALL_GICP_HIP"])
def test_batch_from_the_store_gives_the_host_pointer_records(method):
    """One target and three candidates out of tests/golden/frontend_small.npz, named by key in a shared map store, against the same batch fed from
    host pointers: raw 384-byte records, with the fitness score, run twice (the second run of a GICP method uses the cached covariances)."""
    from mrg_slam_amd import BatchMatcher, MapCloudStore, MrgfeError, _lib, synth
    from mrg_slam_amd.registration import default_params

    prm = default_params(getattr(_lib, method))
    prm.transformation_epsilon = 0.01
    tgt = np.ascontiguousarray(G["tgt"])
    cands = {2: np.ascontiguousarray(G["src"]), 3: np.ascontiguousarray(G["voxel_out_0p1"]), 4: np.ascontiguousarray(G["sor_out"])}
    rng = np.random.default_rng(8)
    guesses = {2: G["guess"], 3: synth.perturb_pose(np.eye(4), rng), 4: synth.perturb_pose(np.eye(4), rng)}
    store = MapCloudStore()
    store.keyframe_callback(1, message(tgt, "pcl32")[0])  # through the callback ...
    store.keyframe_callback(2, message(cands[2], "packed")[0])
    store.add(3, cands[3])                                 # ... and through mrgfe_map_store_add, whose upload is asynchronous
    store.add(4, cands[4])
    host, keyed = BatchMatcher(prm), BatchMatcher(prm)
    assert keyed.store_bytes() == 0
    for run in range(2):
        host.clear()
        keyed.clear()
        th = host.add_target(tgt)
        tk = keyed.add_target_from_store(store, 1) if run == 0 else keyed.add_target(tgt)  # the target from the store / from the host
        for k in (2, 3, 4):
            assert host.add_pair(th, cands[k], guesses[k]) == keyed.add_pair_from_store(tk, store, k, guesses[k])
        # a key used for the target and for a pair, and one keyframe twice
        host.add_pair(th, tgt, np.eye(4))
        keyed.add_pair_from_store(tk, store, 1, np.eye(4))
        host.add_pair(th, cands[3], np.eye(4))
        keyed.add_pair_from_store(tk, store, 3, np.eye(4))
        res = host.align(float("inf"))
        a, b = records(res), records(keyed.align(float("inf")))
        assert a.shape == (5, 384) and np.array_equal(a, b), np.flatnonzero((a != b).any(1))
        assert res["iterations"].max() >= 1 and np.isfinite(res["fitness"]).all()  # (alignments took place, and were scored)
        if method == "NDT_HIP":
            assert keyed.store_bytes() == 0 and keyed.has_cloud(2) is None  # nothing is kept in the batch: the store has the clouds
        else:
            n_cov = len(tgt) + sum(len(c) for c in cands.values())
            assert 0 < keyed.store_bytes() and keyed.has_cloud(2) is None
            assert keyed.store_bytes() < 16 * n_cov + 48 * n_cov  # the covariances only, no cloud (a keyed pair keeps both)
    with pytest.raises(MrgfeError) as e:
        keyed.add_pair_from_store(0, store, 99, np.eye(4))  # a missing key
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(MrgfeError) as e:
        keyed.add_target_from_store(store, 99)
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(MrgfeError):
        keyed.add_pair_from_store(7, store, 2, np.eye(4))  # no such target
    if method != "NDT_HIP":
        with pytest.raises(MrgfeError) as e:
            keyed.forget(2)  # in use by the current batch
        assert e.value.status == _lib.ERR_STATE
    keyed.clear()
    keyed.forget()
    assert keyed.store_bytes() == 0
    del keyed, host  # (the batches go before the store they read)


def test_loop_detector_with_a_store_gives_the_same_loops():
    """Six keyframes, two per detect_batched call: with store= the keyframes are queued by key out of the shared store (targets and candidates), and the
    Loop list — keyframes and relative poses, bit for bit — is that of the same session fed from host memory."""
    from loop_session import run_session
    from mrg_slam_amd import BatchMatcher, MapCloudStore, synth
    from mrg_slam_amd.loop_detector import Edge, KeyFrame, LoopDetector
    from oracle.replay import small_cloud

    world = small_cloud(9000, 77)
    rng = np.random.default_rng(4)

    def session():
        kfs = []
        for k in range(6):
            T = synth.make_pose([0.8 * (k % 3), 0.3 * (k // 3), 0.0], synth.rot_z(0.03 * k))
            pick = np.sort(np.random.default_rng(100 + k).choice(len(world), 3500, replace=False))
            c = world[pick].copy()
            Ti = np.linalg.inv(T)
            c[:, :3] = (c[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
            drift = synth.make_pose(np.random.default_rng(200 + k).normal(0, 0.05, 3) * [1, 1, 0.1], synth.rot_z(np.random.default_rng(300 + k).normal(0, 0.005)))
            kf = KeyFrame(id=k + 1, cloud=c, estimate=T @ drift, accum_distance=20.0 * k, first_keyframe=(k == 0))
            if k:
                prev = kfs[-1]
                rel = np.linalg.inv(kf.estimate) @ prev.estimate
                kf.prev_edge = Edge(kf, prev, rel)
                prev.next_edge = Edge(kf, prev, rel)
                kf.connected.add(prev.id)
                prev.connected.add(kf.id)
            kfs.append(kf)
        return kfs

    del rng
    params = {"accum_distance_thresh_same_robot": 15.0, "loop_closure_consistency_max_delta_trans": 0.5, "loop_closure_consistency_max_delta_angle": 0.1}
    reg_kw = dict(resolution=1.0, transformation_epsilon=0.01, maximum_iterations=64)
    plain_kfs, store_kfs = session(), session()
    plain = LoopDetector(params, matcher=BatchMatcher(**reg_kw))
    store = MapCloudStore()
    for kf in store_kfs:
        store.keyframe_callback(kf.store_key(), kf.cloud, want_kept=False)
    with_store = LoopDetector(params, matcher=BatchMatcher(**reg_kw), store=store)
    a = run_session(plain, plain_kfs, list(range(6)), group=2, batched=True)
    b = run_session(with_store, store_kfs, list(range(6)), group=2, batched=True)
    assert len(a) >= 2
    assert [(lp.key1.id, lp.key2.id) for lp in a] == [(lp.key1.id, lp.key2.id) for lp in b]
    for la, lb in zip(a, b):
        assert np.array_equal(la.relative_pose.view(np.uint32), lb.relative_pose.view(np.uint32))
    assert plain.alignments == with_store.alignments > 0
    assert plain.matcher.store_bytes() > 0 and with_store.matcher.store_bytes() == 0  # nothing was copied into the batch: the store has the keyframes
