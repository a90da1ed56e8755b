"""GPU: bounded best-candidate selection over a node (mrgfe_node_align_best / NodeMatcher.align_best) and on a batch's worker thread
(mrgfe_batch_align_best_async): records, states, winners, scores and intervals must be those of mrgfe_batch_align_best on ONE batch holding the whole
pair list — byte for byte, no tolerance — for any member count, also where a group straddles a block boundary, which is where a per-member selection
would prune less.  Members share the one card (at most four of them)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_gpu_select_best import BIG, _bits, _street_pairs, _wrong, check_against_full

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NDT_KW = dict(transformation_epsilon=0.01, maximum_iterations=64)


@pytest.fixture(scope="module")
def street():
    return _street_pairs()


def _same(a, b):
    """every array of two align_best results (or of two interval pairs), byte for byte"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and _bits(x).tobytes() == _bits(y).tobytes()


def _list1(street, sizes=(4, 4, 3)):
    """11 pairs over 3 targets, groups of 4, 4 and 3 (= the targets): the true candidate and wrong ones of several metres.  Blocks of 2 members: 6 + 5,
    of 4 members: 3 + 3 + 3 + 2 — a group straddles a boundary; of 3 members: 4 + 4 + 3 — none does."""
    offsets = (0.0, 3.0, 5.0, 8.0)
    targets = [s[0] for s in street[: len(sizes)]]
    pairs, group = [], []
    for k, n in enumerate(sizes):
        for dx in offsets[:n]:
            pairs.append((k, street[k][1], _wrong(street[k][3], dx)))
            group.append(k)
    return targets, pairs, np.array(group, dtype=np.int32)


def _queue(m, targets, pairs, keyed=False):
    """the same list on a BatchMatcher or a NodeMatcher"""
    m.clear()
    tids = [m.add_target(t) for t in targets]
    for i, (ti, src, guess) in enumerate(pairs):
        m.add_pair(tids[ti], src, guess, key=500 + i if keyed else 0)


def _one_batch(targets, pairs, group, max_range=INF, score_cap=None, params=None, **kw):
    """the reference: (align_best 4-tuple, intervals, full records) of ONE batch holding the whole list"""
    from mrg_slam_amd import BatchMatcher

    bm = BatchMatcher(params, **(kw or NDT_KW)) if params is None else BatchMatcher(params)
    _queue(bm, targets, pairs)
    got = bm.align_best(max_range, group, score_cap=score_cap)
    bounds = bm.fit_bounds()
    full = bm.align(max_range)
    return got, bounds, full


def _node(members, params=None, **kw):
    from mrg_slam_amd import NodeMatcher

    return NodeMatcher([0] * members, params, **(kw or NDT_KW))


def _node_best(node, targets, pairs, group, max_range=INF, score_cap=None, keyed=False):
    _queue(node, targets, pairs, keyed)
    got = node.align_best(max_range, group, score_cap=score_cap)
    return got, node.fit_bounds()


@pytest.fixture(scope="module")
def ref1(street):
    targets, pairs, group = _list1(street)
    return (targets, pairs, group) + _one_batch(targets, pairs, group)


# ---- 1. one batch equals the node
@pytest.mark.parametrize("members", [1, 2, 3, 4])
def test_node_equals_one_batch(ref1, members):
    targets, pairs, group, want, want_bounds, _ = ref1
    node = _node(members)
    got, bounds = _node_best(node, targets, pairs, group)
    _same(got, want)
    _same(bounds, want_bounds)
    assert (got[0]["pair_id"] == np.arange(len(pairs))).all()
    blocks = [node.shard(m) for m in range(members)]
    straddles = any(group[b[0] - 1] == group[b[0]] for b in blocks[1:] if 0 < b[0] < len(pairs))
    assert straddles == (members in (2, 4))
    st = node.select_stats()
    assert st["exact"] + st["pruned"] + st["above_cap"] + st["skipped"] == len(pairs)
    assert [st[k] for k in ("exact", "pruned", "above_cap", "skipped")] == [int((got[1] == s).sum()) for s in range(4)]
    _queue(node, targets, pairs)
    full = node.align(INF)
    check_against_full(full, *got, group, 3)


# ---- 2. pruning across members
def test_wrong_candidates_on_another_member_are_pruned(street):
    from mrg_slam_amd import _lib

    (tgt0, src0, _, g0), (tgt1, src1, _, g1) = street[0], street[1]
    # group 0: its true candidate is pair 0 (member 0's block), its wrong candidates are pairs 4 .. 7 (member 1's block)
    pairs = [(0, src0, g0), (1, src1, g1), (1, src1, _wrong(g1, 4.0)), (1, src1, _wrong(g1, 6.0))] + [(0, src0, _wrong(g0, dx)) for dx in (3.0, 5.0, 7.0, 9.0)]
    group = np.array([0, 1, 1, 1, 0, 0, 0, 0], dtype=np.int32)
    want, want_bounds, _ = _one_batch([tgt0, tgt1], pairs, group)
    pruned = np.flatnonzero(want[1] == _lib.FIT_PRUNED)
    assert (pruned >= 4).any(), "precondition: the one-batch path prunes a wrong candidate of group 0"
    node = _node(2)
    got, bounds = _node_best(node, [tgt0, tgt1], pairs, group)
    assert node.shard(0) == (0, 4) and node.shard(1) == (4, 4)
    assert (np.flatnonzero(got[1] == _lib.FIT_PRUNED) == pruned).all()
    _same(got, want)
    _same(bounds, want_bounds)


# ---- 3. the other methods, the cap, finite ranges (2 members)
@pytest.mark.parametrize("method", ["GICP_HIP", "ICP_HIP"])
def test_gicp_and_icp(street, method):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    targets = [s[0] for s in street[:3]]
    pairs = [(k, street[k][1], _wrong(street[k][3], dx)) for k in range(3) for dx in (0.0, 3.0, 8.0)]
    group = np.repeat(np.arange(3, dtype=np.int32), 3)
    want, want_bounds, full = _one_batch(targets, pairs, group, params=default_params(getattr(_lib, method)))
    got, bounds = _node_best(_node(2, default_params(getattr(_lib, method))), targets, pairs, group)
    _same(got, want)
    _same(bounds, want_bounds)
    check_against_full(full, *got, group, 3)


def test_score_cap(street):
    targets = [s[0] for s in street]
    pairs, group = [], []
    for k, (_, src, _, g) in enumerate(street):
        for dx in ((0.0, 5.0, 9.0) if k % 2 == 0 else (5.0, 9.0)):  # a true candidate among wrong ones in every other group
            pairs.append((k, src, _wrong(g, dx)))
            group.append(k)
    group = np.array(group, dtype=np.int32)
    want, want_bounds, full = _one_batch(targets, pairs, group, score_cap=1.25)
    got, bounds = _node_best(_node(2), targets, pairs, group, score_cap=1.25)
    assert (want[2] == -2).any() and (want[2] >= 0).any()
    assert ((got[2] == -2) == (want[2] == -2)).all()
    _same(got, want)
    _same(bounds, want_bounds)
    check_against_full(full, *got, group, len(street), cap=1.25)


@pytest.mark.parametrize("max_range", [1.0, 4.0])
def test_finite_range(street, max_range):
    targets, pairs, group = _list1(street)
    want, want_bounds, full = _one_batch(targets, pairs, group, max_range=max_range)
    got, bounds = _node_best(_node(2), targets, pairs, group, max_range=max_range)
    _same(got, want)
    _same(bounds, want_bounds)
    check_against_full(full, *got, group, 3)


# ---- 4. edges
def test_ungrouped_pairs_and_an_empty_group(street):
    targets, pairs, _ = _list1(street)
    group = np.array([0, 0, -1, 0, 1, 1, 1, -1, 3, 3, 3], dtype=np.int32)  # group 2 is empty
    want, want_bounds, full = _one_batch(targets, pairs, group)
    got, bounds = _node_best(_node(2), targets, pairs, group)
    _same(got, want)
    _same(bounds, want_bounds)
    assert got[2][2] == -1 and got[3][2] == BIG
    assert got[1][2] == 0 and got[1][7] == 0  # group -1: scored exactly
    check_against_full(full, *got, group, 4)


def test_a_group_of_non_converged_pairs_only(street):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    # (an NDT that stops at its iteration limit still reports convergence, as PCL's does; the LM loop of GICP does not)
    prm = default_params(_lib.GICP_HIP)
    prm.maximum_iterations = 1
    targets = [s[0] for s in street[:3]]
    pairs = [(k, street[k][1], _wrong(street[k][3], dx)) for k in range(3) for dx in (2.0, 4.0, 6.0)]
    group = np.repeat(np.arange(3, dtype=np.int32), 3)
    want, want_bounds, full = _one_batch(targets, pairs, group, params=prm)
    dead = [g for g in range(3) if (full["converged"][group == g] == 0).all()]
    assert dead, "precondition: with one iteration some group has no converged candidate"
    got, bounds = _node_best(_node(2, prm), targets, pairs, group)
    _same(got, want)
    _same(bounds, want_bounds)
    for g in dead:
        assert got[2][g] == -1 and got[3][g] == BIG and (got[1][group == g] == _lib.FIT_SKIPPED).all()


@pytest.mark.parametrize("n_pairs,members", [(3, 4), (1, 2)])
def test_fewer_pairs_than_members(street, n_pairs, members):
    targets, pairs, group = _list1(street, sizes=(n_pairs,))
    want, want_bounds, _ = _one_batch(targets, pairs, group)
    node = _node(members)
    got, bounds = _node_best(node, targets, pairs, group)
    _same(got, want)
    _same(bounds, want_bounds)
    assert node.shard(members - 1)[1] == 0  # an empty block


def _raw_best(node, n, max_range, cap, group, n_groups, res=None, state=None, best=None, score=None, null_best=False):
    """mrgfe_node_align_best with the arrays as given: the status"""
    from mrg_slam_amd import _lib

    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    grp = np.ascontiguousarray(group, dtype=np.int32)
    res = (_lib.PairResult * max(n, 1))() if res is None else res
    state = np.zeros(max(n, 1), dtype=np.int32) if state is None else state
    best = np.zeros(max(n_groups, 1), dtype=np.int32) if best is None else best
    score = np.zeros(max(n_groups, 1)) if score is None else score
    return _lib.lib().mrgfe_node_align_best(node._h, max_range, cap, grp.ctypes.data_as(ip) if grp.size else None, n_groups, res, state.ctypes.data_as(ip),
                                            None if null_best else best.ctypes.data_as(ip), score.ctypes.data_as(dp))


def test_no_pairs(street):
    from mrg_slam_amd import _lib

    node = _node(2)
    rec, state, best, score = node.align_best(INF, np.zeros(0, dtype=np.int32))
    assert len(rec) == len(state) == len(best) == len(score) == 0
    res = (_lib.PairResult * 1)()
    C.memset(res, 0x5A, C.sizeof(res))
    before = bytes(res)
    state, best, sc = np.full(1, 77, dtype=np.int32), np.full(1, 77, dtype=np.int32), np.full(1, 77.0)
    assert _raw_best(node, 0, INF, BIG, [], 0, res, state, best, sc) == _lib.MRGFE_OK
    assert bytes(res) == before and state[0] == 77 and best[0] == 77 and sc[0] == 77.0


# ---- 5. errors
def test_bad_arguments_are_refused_before_any_member_runs(street):
    from mrg_slam_amd import _lib

    targets, pairs, group = _list1(street)
    node = _node(2)
    _queue(node, targets, pairs)
    n = len(pairs)
    bad_high, bad_low = group.copy(), group.copy()
    bad_high[5], bad_low[5] = 3, -2
    for args in ((INF, BIG, bad_high, 3), (INF, BIG, bad_low, 3), (-1.0, BIG, group, 3), (float("nan"), BIG, group, 3), (INF, float("nan"), group, 3)):
        assert _raw_best(node, n, *args) == _lib.ERR_INVALID
        assert _lib.last_error().startswith("mrgfe_node_align_best")
    assert _raw_best(node, n, INF, BIG, group, 3, null_best=True) == _lib.ERR_INVALID
    assert node.shard(0) == (0, 0) and node.shard(1) == (0, 0)  # no block was cut, no member ran


def test_a_failing_second_member_is_named_and_the_node_stays_usable(ref1):
    from mrg_slam_amd import MrgfeError, _lib

    targets, pairs, group, want, want_bounds, _ = ref1
    node = _node(2)
    node.clear()
    tids = [node.add_target(t) for t in targets]
    for i, (ti, src, guess) in enumerate(pairs):
        if i == 8:  # in the second block (pairs 6 .. 10): a key that is resident nowhere, and no cloud
            node.add_pair(tids[ti], None, guess, key=777, n_points=len(src))
        else:
            node.add_pair(tids[ti], src, guess)
    with pytest.raises(MrgfeError) as e:  # member 0's first stage has succeeded by then (or is given up when it has)
        node.align_best(INF, group)
    assert e.value.status == _lib.ERR_INVALID and "mrgfe_node_align_best: member 1 " in str(e.value)
    with pytest.raises(MrgfeError) as e:
        node.fit_bounds()
    assert e.value.status == _lib.ERR_STATE
    got, bounds = _node_best(node, targets, pairs, group)
    _same(got, want)
    _same(bounds, want_bounds)


def test_fit_bounds_after_a_plain_align_is_a_state_error(ref1):
    from mrg_slam_amd import MrgfeError, _lib

    targets, pairs, group = ref1[:3]
    node = _node(2)
    _node_best(node, targets, pairs, group)
    _queue(node, targets, pairs)
    node.align(INF)
    _queue(node, targets, pairs)
    with pytest.raises(MrgfeError) as e:
        node.fit_bounds()
    assert e.value.status == _lib.ERR_STATE


# ---- 6. call sequences
@pytest.mark.parametrize("keyed", [False, True])
def test_call_sequences_match_fresh_nodes(ref1, keyed):
    targets, pairs, group = ref1[:3]

    def run(node, kind):
        _queue(node, targets, pairs, keyed)
        return (node.align(INF),) if kind == "full" else node.align_best(INF, group)

    fresh = {kind: run(_node(2), kind) for kind in ("best", "full")}
    node = _node(2)
    for kind in ("best", "full", "best"):
        _same(run(node, kind), fresh[kind])
    _same(fresh["best"], ref1[3])


# ---- 7. the asynchronous form of the batch call
def test_async_equals_sync(ref1):
    from mrg_slam_amd import BatchMatcher

    targets, pairs, group, want = ref1[:4]
    bm = BatchMatcher(**NDT_KW)
    _queue(bm, targets, pairs)
    bm.align_best_async(INF, group)
    _same(bm.wait(), want)
    _same(bm.fit_bounds(), ref1[4])
    bm.align_async(INF)  # wait() after a plain align_async: the records alone
    rec = bm.wait()
    assert isinstance(rec, np.ndarray) and _bits(rec).tobytes() == _bits(ref1[5]).tobytes()


def test_a_second_async_before_wait_is_refused(ref1):
    from mrg_slam_amd import BatchMatcher, MrgfeError, _lib

    targets, pairs, group, want = ref1[:4]
    bm = BatchMatcher(**NDT_KW)
    _queue(bm, targets, pairs)
    bm.align_best_async(INF, group)
    for again in (lambda: bm.align_best_async(INF, group), lambda: bm.align_async(INF)):
        with pytest.raises(MrgfeError) as e:
            again()
        assert e.value.status == _lib.ERR_STATE
    _same(bm.wait(), want)  # the running align's outputs are intact


def test_two_batches_in_flight(ref1, street):
    from mrg_slam_amd import BatchMatcher, Context

    targets, pairs, group, want = ref1[:4]
    targets2, pairs2, group2 = _list1(street[3:], sizes=(3, 2))
    want2 = _one_batch(targets2, pairs2, group2)[0]
    a, b = BatchMatcher(ctx=Context(0), **NDT_KW), BatchMatcher(ctx=Context(0), **NDT_KW)
    _queue(a, targets, pairs)
    a.align_best_async(INF, group)
    _queue(b, targets2, pairs2)
    b.align_best_async(INF, group2)
    _same(a.wait(), want)
    _same(b.wait(), want2)


def test_async_refuses_bad_arguments_itself(ref1):
    from mrg_slam_amd import BatchMatcher, MrgfeError, _lib

    targets, pairs, group = ref1[:3]
    bm = BatchMatcher(**NDT_KW)
    _queue(bm, targets, pairs)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    res = (_lib.PairResult * len(pairs))()
    state, best, score = np.zeros(len(pairs), dtype=np.int32), np.zeros(3, dtype=np.int32), np.zeros(3)
    bad = group.copy()
    bad[0] = 3

    def call(max_range, cap, grp, best_ptr):
        return _lib.lib().mrgfe_batch_align_best_async(bm._h, max_range, cap, grp.ctypes.data_as(ip), 3, res, state.ctypes.data_as(ip), best_ptr, score.ctypes.data_as(dp))

    for args in ((INF, BIG, bad, best.ctypes.data_as(ip)), (-1.0, BIG, group, best.ctypes.data_as(ip)), (INF, float("nan"), group, best.ctypes.data_as(ip)), (INF, BIG, group, None)):
        assert call(*args) == _lib.ERR_INVALID
        assert _lib.last_error().startswith("mrgfe_batch_align_best:")  # the synchronous call's text
    with pytest.raises(MrgfeError) as e:  # nothing was posted
        _lib.check(_lib.lib().mrgfe_batch_wait(bm._h))
    assert e.value.status == _lib.ERR_STATE


# ---- 8. the loop detector on a node
RING_KEYFRAMES = 16  # the smallest ring session on which the full path on one batch finds two loops or more (8, 10, 12 and 14 keyframes: none)


def test_loop_detector_bounded_on_a_node_equals_full_on_a_batch():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from loop_session import make_ring_session, run_session
    from mrg_slam_amd import BatchMatcher, NodeMatcher, prefilter
    from mrg_slam_amd.loop_detector import LoopDetector

    reg_kw = dict(resolution=1.0, transformation_epsilon=0.01, maximum_iterations=64)
    pf = lambda c: prefilter(c, {"downsample_resolution": 0.2})  # noqa: E731
    out = {}
    for mode, matcher in (("full", lambda: BatchMatcher(**reg_kw)), ("bounded", lambda: NodeMatcher([0, 0], **reg_kw))):
        kfs, order = make_ring_session(RING_KEYFRAMES, "VLP16", prefilter=pf)
        det = LoopDetector({"fitness_selection": mode}, matcher=matcher())
        out[mode] = run_session(det, kfs, order, group=6, batched=True)
    a, b = out["full"], out["bounded"]
    assert len(a) >= 2, "precondition: the full path on one batch finds at least two loops"
    assert [(lp.key1.slam_uuid, lp.key1.id, lp.key2.slam_uuid, lp.key2.id) for lp in a] == [(lp.key1.slam_uuid, lp.key1.id, lp.key2.slam_uuid, lp.key2.id) for lp in b]
    for x, y in zip(a, b):
        assert _bits(x.relative_pose).tobytes() == _bits(y.relative_pose).tobytes()
