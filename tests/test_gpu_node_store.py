"""GPU: mrgfe_node_add_target_from_store / _add_pair_from_store, mrgfe_node_clear_pairs and mrgfe_node_store_stats — a node fed by map-store key.

Every expected record comes from ONE BatchMatcher fed by add_*_from_store from the same store (the existing single-batch route); the node must return
the same bytes for every member count, batch method and copy mode (mrgfe_dbg_node_set_store_copy: 0 reads the store in place on its device, 1 always
copies to a replica — the route a member on another device takes, exercised here on one card).  Workloads are those of tests/test_gpu_node.py: targets of
3800 - 5000 points, sources of 2400 + 170 k points."""
import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu

INF = float("inf")


def _params(method, eps=None):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    p = default_params(getattr(_lib, method))
    p.transformation_epsilon, p.maximum_iterations = (1e-4 if method == "PCL_NDT_HIP" else 0.01) if eps is None else eps, 64
    return p


class _Workload:
    """targets and (target index, source, guess) pairs, every cloud under a key of its own in `store`"""

    def __init__(self, store, base, n_targets, n_pairs, seed, sizes=(5000, 3800, 4400)):
        from mrg_slam_amd import synth
        from oracle import oracle as orc

        self.store = store
        self.targets = [small_cloud(sizes[k % len(sizes)], 300 + k) for k in range(n_targets)]
        self.tkeys = [base + 100 + k for k in range(n_targets)]
        rng = np.random.default_rng(seed)
        self.pairs, self.skeys = [], []
        for k in range(n_pairs):
            ti = min(n_targets - 1, k * n_targets // n_pairs)  # ordered by target, like the reference's list
            rel = synth.make_pose(rng.normal(0, 0.2, 3), synth.rot_xyz(*rng.normal(0, 0.02, 3)))
            src = orc.transform_points(np.linalg.inv(rel), self.targets[ti][: 2400 + 170 * k])
            self.pairs.append((ti, src, synth.perturb_pose(np.eye(4), rng)))
            self.skeys.append(base + k)
        for key, c in zip(self.tkeys + self.skeys, self.targets + [p[1] for p in self.pairs]):
            store.add(key, c)
        self._want = {}

    def feed(self, matcher, which=None):
        """the whole list (or the pairs `which`) by key; the targets are always all declared, in order"""
        tids = [matcher.add_target_from_store(self.store, k) for k in self.tkeys]
        for i in (range(len(self.pairs)) if which is None else which):
            ti, _, guess = self.pairs[i]
            matcher.add_pair_from_store(tids[ti], self.store, self.skeys[i], guess)

    def want(self, method, which=None, fit=INF):
        """the records of ONE batch fed from the store, computed once per (method, list) and left unchanged"""
        from mrg_slam_amd import BatchMatcher

        key = (method, None if which is None else tuple(which), fit)
        if key not in self._want:
            bm = BatchMatcher(_params(method))
            self.feed(bm, which)
            res = bm.align(fit)
            res["pair_id"] = np.arange(len(res))
            res.setflags(write=False)
            self._want[key] = res
        return self._want[key]

    def named(self, node, which=None):
        """(clouds, points) the members name in the node's last align: per block its distinct targets and its sources (every key is distinct)"""
        which = list(range(len(self.pairs))) if which is None else list(which)
        clouds = points = 0
        for m in range(node.n_members):
            first, count = node.shard(m)
            block = which[first:first + count]
            for ti in sorted({self.pairs[i][0] for i in block}):
                clouds, points = clouds + 1, points + len(self.targets[ti])
            clouds, points = clouds + len(block), points + sum(len(self.pairs[i][1]) for i in block)
        return clouds, points


@pytest.fixture(scope="module")
def world():
    from mrg_slam_amd import MapCloudStore

    store = MapCloudStore()
    return {"store": store, "full": _Workload(store, 1000, 3, 11, 5), "small": _Workload(store, 2000, 2, 5, 8)}


def _node(members, method, copy):
    from mrg_slam_amd import NodeMatcher

    node = NodeMatcher([0] * members if isinstance(members, int) else members, _params(method))
    node.set_store_copy(copy)
    return node


def _check_copy_modes(w, members, method):
    """both copy modes on one workload: records, mrgfe_node_store_stats and mrgfe_node_store_bytes"""
    want = w.want(method).tobytes()
    node0 = _node(members, method, 0)
    w.feed(node0)
    assert node0.align(INF).tobytes() == want
    clouds, points = w.named(node0)
    assert node0.store_stats() == (clouds, 0, 0, 0)
    node1 = _node(members, method, 1)
    assert node1.store_bytes() == 0
    for rep in range(2):  # the repeat of the same list finds every replica resident
        node1.clear()
        w.feed(node1)
        assert node1.align(INF).tobytes() == want, rep
        assert w.named(node1) == (clouds, points)
        assert node1.store_stats() == ((0, clouds, 16 * points, 0) if rep == 0 else (0, 0, 0, 0)), rep
        # 16 bytes per replicated point on top of what the in-place route keeps (the GICP family's covariances, cached under the same keys)
        assert node1.store_bytes() - node0.store_bytes() == 16 * points
    assert clouds > 0
    return node0, node1


# ---- 1. records ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 2, 3, 4])
def test_node_fed_by_key_equals_one_batch_fed_by_key(world, members):
    node0, _ = _check_copy_modes(world["full"], members, "NDT_HIP")
    assert node0.store_bytes() == 0  # NDT_HIP in place: nothing is kept anywhere but in the store
    if members == 1:
        assert node0.store_stats()[0] == 3 + 11


@pytest.mark.parametrize("method", ["GICP_HIP", "VGICP_HIP", "ICP_HIP", "PCL_NDT_HIP"])
def test_every_batch_method_both_copy_modes(world, method):
    node0, node1 = _check_copy_modes(world["small"], 2, method)
    if method in ("ICP_HIP", "PCL_NDT_HIP"):
        assert node0.store_bytes() == 0  # they cache nothing
    else:
        assert node0.store_bytes() >= 48 * sum(len(p[1]) for p in world["small"].pairs)  # the sources' covariances, under their keys, on both routes


# ---- 2. mixed lists --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copy", [0, 1])
def test_a_list_mixing_host_and_store_clouds_equals_the_same_list_on_one_batch(world, copy):
    from mrg_slam_amd import BatchMatcher

    w = world["full"]

    def feed(m, is_node):
        tids = [m.add_target(w.targets[0]), m.add_target_from_store(w.store, w.tkeys[1]),
                m.add_target(w.targets[2], key=777) if is_node else m.add_target(w.targets[2])]  # (a batch has no keyed target: the cloud is the same)
        for i, (ti, src, guess) in enumerate(w.pairs):
            if i % 3 == 0:
                m.add_pair(tids[ti], src, guess)
            elif i % 3 == 1:
                m.add_pair_from_store(tids[ti], w.store, w.skeys[i], guess)
            else:
                m.add_pair(tids[ti], src, guess, key=5000 + i)

    bm = BatchMatcher(_params("NDT_HIP"))
    feed(bm, False)
    want = bm.align(INF)
    want["pair_id"] = np.arange(len(want))
    assert want.tobytes() == w.want("NDT_HIP").tobytes()  # (the single-batch routes agree among themselves)
    node = _node(3, "NDT_HIP", copy)
    for rep in range(2):
        node.clear()
        feed(node, True)
        assert node.align(INF).tobytes() == want.tobytes(), rep
    st = node.store_stats()
    assert (st[0] > 0 and st[1] == 0) if copy == 0 else (st[0] == 0 and st[1] == 0)  # (second call, copy mode 1: the replicas were resident)


# ---- 3. clear_pairs --------------------------------------------------------------------------------------------------------------------------------
SECOND = [0, 1, 5, 4, 9, 10, 2]  # 7 pairs in blocks of 3 / 2 / 2 after 11 in blocks of 4 / 4 / 3: every member keeps one target and lacks one


@pytest.mark.parametrize("method", ["NDT_HIP", "GICP_HIP"])
@pytest.mark.parametrize("copy", [0, 1])
def test_clear_pairs_keeps_the_targets_and_gives_a_fresh_nodes_records(world, copy, method):
    w = world["full"]
    node = _node(3, method, copy)
    w.feed(node)
    assert node.align(INF).tobytes() == w.want(method).tobytes()
    node.clear_pairs()
    tids = [0, 1, 2]  # the declared targets keep their indices
    for i in SECOND:
        node.add_pair_from_store(tids[w.pairs[i][0]], w.store, w.skeys[i], w.pairs[i][2])
    got = node.align(INF)
    assert [node.shard(m)[1] for m in range(3)] == [3, 2, 2]
    st = node.store_stats()
    assert st[3] == 3 and st[3] > 0  # every member found the target of its old block built ...
    assert (st[0] if copy == 0 else st[1]) >= 3  # ... and added the one it lacked, with the sources it had not seen
    fresh = _node(3, method, copy)
    w.feed(fresh, SECOND)
    assert got.tobytes() == fresh.align(INF).tobytes()
    assert fresh.store_stats()[3] == 0
    assert got.tobytes() == w.want(method, SECOND).tobytes()
    # a third stage on the same targets, and a full clear after it: nothing stale is reused
    node.clear_pairs()
    for i in range(len(w.pairs)):
        node.add_pair_from_store(tids[w.pairs[i][0]], w.store, w.skeys[i], w.pairs[i][2])
    assert node.align(INF).tobytes() == w.want(method).tobytes() and node.store_stats()[3] > 0
    node.clear()
    w.feed(node, SECOND)
    assert node.align(INF).tobytes() == w.want(method, SECOND).tobytes() and node.store_stats()[3] == 0


@pytest.mark.parametrize("copy", [0, 1])
def test_align_best_then_clear_pairs_then_align_equals_the_batch_sequence(world, copy):
    from mrg_slam_amd import BatchMatcher

    w = world["full"]
    group = np.array([p[0] for p in w.pairs], dtype=np.int32)  # the candidates of one target are one group

    def run(m):
        m.clear()
        w.feed(m)
        first = m.align_best(INF, group, score_cap=1.25)
        m.clear_pairs()
        for i in SECOND:
            m.add_pair_from_store(w.pairs[i][0], w.store, w.skeys[i], w.pairs[i][2])
        second = m.align(-1.0)
        for rec in (first[0], second):
            rec["pair_id"] = np.arange(len(rec))
        return first, second

    want1, want2 = run(BatchMatcher(_params("NDT_HIP")))
    node = _node(3, "NDT_HIP", copy)
    got1, got2 = run(node)
    assert node.store_stats()[3] == 3
    for a, b in zip(got1, want1):
        assert a.tobytes() == b.tobytes()
    assert got2.tobytes() == want2.tobytes()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing(world):
    from mrg_slam_amd import MrgfeError, _lib

    w = world["small"]
    node = _node(2, "NDT_HIP", 0)
    t = node.add_target_from_store(w.store, w.tkeys[0])
    node.add_pair_from_store(t, w.store, w.skeys[0], np.eye(4))
    n_pairs = lambda: _lib.lib().mrgfe_node_num_pairs(node._h)  # noqa: E731
    assert n_pairs() == 1
    missing = 987654321
    with pytest.raises(MrgfeError, match=str(missing)):
        node.add_pair_from_store(t, w.store, missing, np.eye(4))
    with pytest.raises(MrgfeError, match=str(missing)):
        node.add_target_from_store(w.store, missing)
    with pytest.raises(MrgfeError, match="out of range"):
        node.add_pair_from_store(t + 1, w.store, w.skeys[1], np.eye(4))  # (the refused target above was not declared)
    with pytest.raises(MrgfeError, match="out of range"):
        node.add_pair_from_store(-1, w.store, w.skeys[1], np.eye(4))
    g = np.eye(4, dtype=np.float32)
    fp = g.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    assert _lib.lib().mrgfe_node_add_target_from_store(node._h, None, w.tkeys[0]) == _lib.ERR_INVALID
    assert _lib.lib().mrgfe_node_add_pair_from_store(node._h, t, None, w.skeys[0], fp) == _lib.ERR_INVALID
    assert _lib.lib().mrgfe_node_add_pair_from_store(node._h, t, w.store._h, w.skeys[0], None) == _lib.ERR_INVALID
    assert _lib.lib().mrgfe_node_add_target_from_store(None, w.store._h, w.tkeys[0]) == _lib.ERR_INVALID
    with pytest.raises(MrgfeError):
        node.set_store_copy(2)
    assert n_pairs() == 1
    assert len(node.align(INF)) == 1  # the node is still usable


# ---- 5. the replicas are bounded -------------------------------------------------------------------------------------------------------------------
def test_replicas_fall_under_the_members_cap_least_recently_named_first(world, monkeypatch):
    """the cap of test_member_target_store_is_bounded_lru (tests/test_gpu_node.py), over replicas: 1 MiB holds three 20000-point keyframes (0.32 MB each)"""
    from mrg_slam_amd import BatchMatcher, NodeMatcher

    store = world["store"]
    clouds = [small_cloud(20000, 900 + k) for k in range(6)]
    src = clouds[0][:3000].copy()
    keys, skey = [7000 + k for k in range(6)], 7100
    for k, c in zip(keys + [skey], clouds + [src]):
        store.add(k, c)
    monkeypatch.setenv("MRGFE_KEYFRAME_STORE_MB", "1")
    node = NodeMatcher([0], _params("NDT_HIP"))
    monkeypatch.delenv("MRGFE_KEYFRAME_STORE_MB")
    node.set_store_copy(1)
    big = _node(1, "NDT_HIP", 1)
    held = []
    for k in keys:  # one new keyframe per call, like matching()
        node.clear()
        node.add_pair_from_store(node.add_target_from_store(store, k), store, skey, np.eye(4))
        node.align()
        held.append(node.store_bytes())
    assert max(held) <= (1 << 20) + 20000 * 16 and held[-1] <= (1 << 20)
    assert node.store_stats()[1] == 1  # the source stayed (named by every call), the target was new
    # the most recently named replicas are still there, the oldest is gone and is copied again
    node.clear()
    node.add_pair_from_store(node.add_target_from_store(store, keys[5]), store, skey, np.eye(4))
    node.add_pair_from_store(node.add_target_from_store(store, keys[4]), store, skey, np.eye(4))
    assert len(node.align()) == 2 and node.store_stats()[1] == 0
    node.clear()
    node.add_pair_from_store(node.add_target_from_store(store, keys[0]), store, skey, np.eye(4))
    assert len(node.align()) == 1 and node.store_stats()[1:3] == (1, 20000 * 16)
    # a call whose own clouds exceed the cap keeps all of them, and the records are those of an unbounded node and of one batch
    bm = BatchMatcher(_params("NDT_HIP"))
    for m in (node, big, bm):
        m.clear()
        for k in keys:
            m.add_pair_from_store(m.add_target_from_store(store, k), store, skey, np.eye(4))
    want = bm.align(INF)
    want["pair_id"] = np.arange(len(want))
    assert node.align(INF).tobytes() == big.align(INF).tobytes() == want.tobytes()
    assert node.store_bytes() == big.store_bytes() == 16 * (6 * 20000 + 3000)


# ---- 6. forget -------------------------------------------------------------------------------------------------------------------------------------
def test_forget_drops_the_replicas_and_the_next_call_copies_again(world):
    w = world["small"]
    node = _node(2, "NDT_HIP", 1)
    w.feed(node)
    want = w.want("NDT_HIP").tobytes()
    assert node.align(INF).tobytes() == want
    first = node.store_stats()
    assert first[1] > 0 and node.store_bytes() == first[2]
    node.clear()
    assert node.store_bytes() == first[2]  # mrgfe_node_clear drops nothing resident
    node.forget(0)
    assert node.store_bytes() == 0
    w.feed(node)
    assert node.align(INF).tobytes() == want and node.store_stats() == first


# ---- 7. a member on another device than the store --------------------------------------------------------------------------------------------------
def test_a_member_on_another_device_reads_a_replica(world):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("this machine shows fewer than 2 devices: the cross-device copy needs a second one")
    w = world["full"]
    node = _node([0, 1], "NDT_HIP", 0)
    w.feed(node)
    assert node.align(INF).tobytes() == w.want("NDT_HIP").tobytes()
    st = node.store_stats()
    assert st[0] > 0 and st[1] > 0 and st[2] > 0  # member 0 in place, member 1 by replica
