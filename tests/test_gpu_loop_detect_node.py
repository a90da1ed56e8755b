"""GPU: LoopDetector::detect in one call over a NODE (mrgfe_loop_create_node, HipLoopDetector(matcher=<NodeMatcher>)) against the same detector over ONE
batch (mrgfe_loop_create) and the same store: the (key1, key2) list, relative_pose and score byte for byte, the LoopManager and the stats of every call.

Ring session sized like the `ring` fixture of tests/test_gpu_loop_detect.py (64 keyframes, 4 or 6 new ones per call; the scans are the cached ones).  The
single-batch detector alone must find at least 2 loops and turn at least one new keyframe that had candidates away (fitness gate or consistency check):
asserted on ITS result.  Small case: a call that validation refuses leaves the detector as it was."""
import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu


def _params(method):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    prm = default_params(getattr(_lib, method))
    prm.transformation_epsilon, prm.maximum_iterations = 0.01, 64
    if method == "NDT_HIP":
        prm.resolution = 1.0
    return prm


@pytest.fixture(scope="module")
def ring():
    from loop_session import make_ring_session
    from mrg_slam_amd import MapCloudStore, prefilter

    kfs, order = make_ring_session(64, "VLP64", prefilter=lambda c: prefilter(c, {"downsample_resolution": 0.2}))
    store = MapCloudStore()
    for kf in kfs:
        store.add(kf.store_key(), kf.cloud)
    return {"kfs": kfs, "order": order, "store": store, "connected": [set(k.connected) for k in kfs], "baseline": {}}


def _session(ring, det, group):
    """the keyframes `group` at a time; every loop becomes a graph edge.  Returns what the comparison is over."""
    kfs, order = ring["kfs"], ring["order"]
    for k, c in zip(kfs, ring["connected"]):
        k.connected = set(c)
    known, loops, calls = [], [], []
    for g0 in range(0, len(order), group):
        new = [kfs[i] for i in order[g0:g0 + group]]
        found = det.detect(known, new)
        for lp in found:
            lp.key1.connected.add(lp.key2.id)
            lp.key2.connected.add(lp.key1.id)
        loops += [(lp.key1.id, lp.key2.id, lp.relative_pose.tobytes(), lp.score) for lp in found]
        calls.append(det.stats())
        known += new
    return {"loops": loops, "calls": calls, "manager": det.loop_manager_entries(), "sizes": det.loop_candidates_sizes}


def _baseline(ring, method, selection, reuse, group):
    """HipLoopDetector over ONE BatchMatcher (with the same stage reuse: without it stats()["target_builds"] counts the targets of stage 2 again): computed
    once per configuration, shared, and held to what the session is meant to exercise"""
    from mrg_slam_amd import BatchMatcher, HipLoopDetector

    key = (method, selection, reuse, group)
    if key not in ring["baseline"]:
        det = HipLoopDetector({"fitness_selection": selection}, BatchMatcher(_params(method)), ring["store"])
        det.set_stage_reuse(reuse)
        want = _session(ring, det, group)
        assert len(want["loops"]) >= 2
        # a new keyframe that had candidates after the gates and closed no loop: its best match failed the fitness gate or the consistency check
        assert len(want["sizes"]) > len(want["loops"])
        assert any(c["consistency_pairs"] > 0 for c in want["calls"])
        ring["baseline"][key] = want
    return ring["baseline"][key]


# (method, members, fitness_selection, copy mode, stage reuse, new keyframes per call): every member count with both selections; both copy modes and
# stage reuse on and off with each of them; GICP_HIP at two members
CASES = [
    ("NDT_HIP", 1, "full", 0, True, 4),
    ("NDT_HIP", 1, "bounded", 1, False, 6),
    ("NDT_HIP", 2, "full", 0, False, 6),
    ("NDT_HIP", 2, "bounded", 1, True, 4),
    ("NDT_HIP", 3, "full", 1, True, 6),
    ("NDT_HIP", 3, "full", 1, False, 4),
    ("NDT_HIP", 3, "bounded", 0, True, 6),
    ("NDT_HIP", 3, "bounded", 0, False, 4),
    ("GICP_HIP", 2, "full", 1, True, 6),
    ("GICP_HIP", 2, "bounded", 0, False, 6),
]


@pytest.mark.parametrize("method,members,selection,copy,reuse,group", CASES)
def test_ring_session_over_a_node_equals_the_single_batch_detector(ring, method, members, selection, copy, reuse, group):
    from mrg_slam_amd import HipLoopDetector, NodeMatcher

    want = _baseline(ring, method, selection, reuse, group)
    node = NodeMatcher([0] * members, _params(method))
    node.set_store_copy(copy)
    hip = HipLoopDetector({"fitness_selection": selection}, node, ring["store"])
    assert hip.set_stage_reuse(reuse) is True
    got = _session(ring, hip, group)
    assert [lp[:2] for lp in got["loops"]] == [lp[:2] for lp in want["loops"]]
    assert got == want
    st = node.store_stats()  # of the last align the session ran
    assert (st[1] == 0 and st[2] == 0) if copy == 0 else st[0] == 0
    assert node.store_bytes() > 0 if (copy == 1 or method == "GICP_HIP") else node.store_bytes() == 0
    hip.close()


# ---- a failing call ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six():
    """six keyframes of about 2000 points on a line, 2 m apart, 20 m of driving between them; the last two arrive as new keyframes, one per call"""
    from mrg_slam_amd import MapCloudStore, synth
    from mrg_slam_amd.loop_detector import Edge, KeyFrame
    from oracle import oracle as orc

    base = small_cloud(2000, 77)
    kfs = []
    for i in range(6):
        est = synth.make_pose([2.0 * i, 0.0, 0.0], synth.rot_z(0.01 * i))
        cloud = orc.transform_points(np.linalg.inv(est), base)[: 2000 - 37 * i]
        kf = KeyFrame(id=i + 1, cloud=cloud, estimate=est, accum_distance=20.0 * i, first_keyframe=(i == 0))
        if 0 < i < 4:  # the new keyframes have no odometry edge to the others here: all but the first are their candidates
            rel = np.linalg.inv(est) @ kfs[-1].estimate
            kf.prev_edge = Edge(kf, kfs[-1], rel)
            kfs[-1].next_edge = Edge(kf, kfs[-1], rel)
        kfs.append(kf)
    store = MapCloudStore()
    for kf in kfs:
        store.add(kf.store_key(), kf.cloud)
    return kfs, store


def _state(hip):
    return hip.loop_manager_entries(), hip.stats(), hip.loop_candidates_sizes, hip.loop_detection_times


def _loops(found):
    return [(lp.key1.id, lp.key2.id, lp.relative_pose.tobytes(), lp.score) for lp in found]


@pytest.mark.parametrize("copy", [0, 1])
def test_a_refused_call_leaves_the_detector_as_it_was(six, copy):
    from mrg_slam_amd import BatchMatcher, HipLoopDetector, MrgfeError, NodeMatcher, _lib

    kfs, store = six
    calm = HipLoopDetector(None, BatchMatcher(_params("NDT_HIP")), store)  # the undisturbed detector, over one batch
    want = [_loops(calm.detect(kfs[:4], [kfs[4]])), _loops(calm.detect(kfs[:5], [kfs[5]]))]
    assert calm.stats()["superset_pairs"] >= 3
    node = NodeMatcher([0, 0], _params("NDT_HIP"))
    node.set_store_copy(copy)
    hip = HipLoopDetector(None, node, store)
    assert _loops(hip.detect(kfs[:4], [kfs[4]])) == want[0]
    before, pairs_before = _state(hip), _lib.lib().mrgfe_node_num_pairs(node._h)
    assert before[1]["superset_pairs"] == 3 and before[2] != []
    # keyframe 3 taken out of the caller's list: keyframe 2's next and keyframe 4's previous keyframe are in neither list, and validation refuses the call
    with pytest.raises(MrgfeError):
        hip.detect([kfs[0], kfs[1], kfs[3], kfs[4]], [kfs[5]])
    assert _state(hip) == before and _lib.lib().mrgfe_node_num_pairs(node._h) == pairs_before
    # a keyframe the store lacks: refused by name before anything is queued on the node
    from mrg_slam_amd.loop_detector import KeyFrame

    stranger = KeyFrame(id=99, cloud=small_cloud(1500, 5), estimate=kfs[5].estimate, accum_distance=kfs[5].accum_distance)
    with pytest.raises(MrgfeError, match=str(stranger.store_key())):
        hip.detect(kfs[:5], [stranger])
    assert _state(hip) == before and _lib.lib().mrgfe_node_num_pairs(node._h) == pairs_before
    assert _loops(hip.detect(kfs[:5], [kfs[5]])) == want[1]
    assert hip.loop_manager_entries() == calm.loop_manager_entries() and hip.stats() == calm.stats() and hip.loop_candidates_sizes == calm.loop_candidates_sizes
