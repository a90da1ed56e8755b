"""GPU: LoopDetector::detect in one call over the map store (mrgfe_loop_detect, HipLoopDetector) against the mirror's detect_batched over the same kind of
batch and the same store.

Ring session (tests/loop_session.py, built exactly as tests/test_gpu_loop_detector.py builds it, so the cached scans are reused): the keyframes sit in a
MapCloudStore, arrive 4 or 6 per call, and are matched with NDT_HIP, SMALL_GICP_HIP and ICP_HIP, fitness_selection full and bounded.  With the mirror's
normalize_estimate and _guess monkeypatched to the library's two helpers both routes align from the same float guesses: the same (key1, key2) list,
relative_pose and score bit for bit, the same last_batched counts in every call, target_builds = the new keyframes that had candidates (stage 2 runs on
the targets stage 1 built).  Against the unpatched mirror, and against the sequential detect() on a single registration, the key list is still equal.

Small cases (five keyframes of about 2000 points): a key the store lacks is refused with nothing queued and the batch still usable; a call without
candidates touches no GPU; two detectors share one store."""
import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu

METHODS = ["NDT_HIP", "SMALL_GICP_HIP", "ICP_HIP"]
REG_KW = dict(transformation_epsilon=0.01, maximum_iterations=64)


def _params(method):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    prm = default_params(getattr(_lib, method))
    prm.transformation_epsilon, prm.maximum_iterations = REG_KW["transformation_epsilon"], REG_KW["maximum_iterations"]
    if method == "NDT_HIP":
        prm.resolution = 1.0
    return prm


@pytest.fixture(scope="module")
def ring():
    """the session, its keyframes in a MapCloudStore, and the graph edges it starts with (run_session adds the loops' edges: restored before every run)"""
    from loop_session import make_ring_session
    from mrg_slam_amd import MapCloudStore, prefilter

    kfs, order = make_ring_session(64, "VLP64", prefilter=lambda c: prefilter(c, {"downsample_resolution": 0.2}))
    store = MapCloudStore()
    for kf in kfs:
        store.add(kf.store_key(), kf.cloud)
    return {"kfs": kfs, "order": order, "store": store, "connected": [set(k.connected) for k in kfs], "mirror": {}}


def _run(ring, detect, group):
    """run_session of tests/loop_session.py with a per-call hook: (loops, what `detect` returned per call)"""
    kfs, order = ring["kfs"], ring["order"]
    for k, c in zip(kfs, ring["connected"]):
        k.connected = set(c)
    known, loops, per_call = [], [], []
    for g0 in range(0, len(order), group):
        new = [kfs[i] for i in order[g0:g0 + group]]
        found, info = detect(known, new)
        for lp in found:
            lp.key1.connected.add(lp.key2.id)
            lp.key2.connected.add(lp.key1.id)
        loops += found
        per_call.append(info)
        known += new
    return loops, per_call


class _RecordingMatcher:
    """a BatchMatcher that remembers the fitness of every (target key, source key) pair it scored: the mirror's Loop carries no score"""

    def __init__(self, bm):
        self.bm, self.scores, self._targets, self._pairs = bm, {}, [], []

    def __getattr__(self, name):
        return getattr(self.bm, name)

    def clear(self):
        self._targets, self._pairs = [], []
        self.bm.clear()

    def add_target_from_store(self, store, key):
        self._targets.append(key)
        return self.bm.add_target_from_store(store, key)

    def add_pair_from_store(self, target, store, key, guess=None):
        self._pairs.append((self._targets[target], key))
        return self.bm.add_pair_from_store(target, store, key, guess)

    def _note(self, rec, want):
        if want:
            for pk, r in zip(self._pairs, rec):
                self.scores[pk] = float(r["fitness"])
        return rec

    def align(self, fitness_max_range=-1.0):
        return self._note(self.bm.align(fitness_max_range), fitness_max_range >= 0)

    def align_best(self, max_range, group, score_cap=None):
        out = self.bm.align_best(max_range, group, score_cap=score_cap)
        self._note(out[0], True)
        return out


def _mirror_session(ring, method, selection, group, patched, monkeypatch):
    """the mirror's detect_batched over a BatchMatcher and the store; patched: it aligns from the library's float guesses.  Computed once per
    configuration and shared."""
    from mrg_slam_amd import BatchMatcher, loop_detector as ld

    key = (method, selection, group, patched)
    if key not in ring["mirror"]:
        if patched:
            monkeypatch.setattr(ld, "normalize_estimate", ld.lib_normalize_estimate)
            monkeypatch.setattr(ld.LoopDetector, "_guess", lambda self, ne, kf: ld.lib_guess(ne, kf.estimate, self.p["use_planar_registration_guess"]))
        matcher = _RecordingMatcher(BatchMatcher(_params(method)))
        det = ld.LoopDetector({"fitness_selection": selection}, matcher=matcher, store=ring["store"])

        def detect(known, new):
            det.last_batched = None
            found = det.detect_batched(known, new)
            return found, det.last_batched

        loops, per_call = _run(ring, detect, group)
        ring["mirror"][key] = ([(lp.key1.id, lp.key2.id, lp.relative_pose.copy(), matcher.scores[(lp.key1.store_key(), lp.key2.store_key())]) for lp in loops], per_call,
                               list(det.loop_candidates_sizes))
        monkeypatch.undo()
    return ring["mirror"][key]


@pytest.mark.parametrize("group", [4, 6])
@pytest.mark.parametrize("selection", ["full", "bounded"])
@pytest.mark.parametrize("method", METHODS)
def test_ring_session_one_call_equals_detect_batched(ring, monkeypatch, method, selection, group):
    from mrg_slam_amd import BatchMatcher, HipLoopDetector

    want, want_calls, want_sizes = _mirror_session(ring, method, selection, group, True, monkeypatch)
    hip = HipLoopDetector({"fitness_selection": selection}, BatchMatcher(_params(method)), ring["store"])

    def detect(known, new):
        hip.last_batched = None
        found = hip.detect(known, new)
        st = hip.stats()
        if hip.last_batched is not None:
            # target_builds: the new keyframes that had candidates — not that number plus the targets of stage 2
            with_candidates = sum(1 for k in new if hip_probe.find_candidates(k, known, ignore_loop_manager=True))
            assert st["target_builds"] == with_candidates >= 1, (st, with_candidates)
        else:
            assert st["superset_pairs"] == 0 and st["target_builds"] == 0
        return found, hip.last_batched

    from mrg_slam_amd.loop_detector import LoopDetector

    hip_probe = LoopDetector(registration=object())  # find_candidates of the mirror, gates ignored: which new keyframes have candidates
    got, got_calls = _run(ring, detect, group)
    assert len(got) >= 2
    assert [(lp.key1.id, lp.key2.id) for lp in got] == [(a, b) for a, b, _, _ in want]
    for lp, (_, _, pose, score) in zip(got, want):
        assert lp.relative_pose.dtype == np.float32 and lp.relative_pose.tobytes() == pose.tobytes()
        assert lp.score == score
    assert got_calls == want_calls and any(c is not None and c["consistency_pairs"] > 0 for c in got_calls)
    assert any(c is not None and c["superset_pairs"] > c["sequential_pairs"] for c in got_calls)  # the gates pruned inside a call
    assert hip.loop_candidates_sizes == want_sizes


@pytest.mark.parametrize("method", METHODS)
def test_ring_session_key_list_equals_the_unpatched_mirror_and_the_sequential_loop(ring, monkeypatch, method):
    """from numpy's guesses (LAPACK's inverse: the last float bit of a guess may differ) and one registration at a time, the decisions are the same"""
    from mrg_slam_amd import IcpHip, NdtHip, SmallGicpHip
    from mrg_slam_amd.loop_detector import LoopDetector

    group = 6
    keys = [(a, b) for a, b, _, _ in _mirror_session(ring, method, "full", group, True, monkeypatch)[0]]
    assert [(a, b) for a, b, _, _ in _mirror_session(ring, method, "full", group, False, monkeypatch)[0]] == keys
    reg = {"NDT_HIP": lambda: NdtHip(resolution=1.0, **REG_KW), "SMALL_GICP_HIP": lambda: SmallGicpHip(**REG_KW), "ICP_HIP": lambda: IcpHip(**REG_KW)}[method]()
    seq = LoopDetector(registration=reg)
    loops, _ = _run(ring, lambda known, new: (seq.detect(known, new), None), group)
    assert [(lp.key1.id, lp.key2.id) for lp in loops] == keys and len(keys) >= 2


# ---- small cases ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five():
    """five keyframes of about 2000 points on a line, 2 m apart, 20 m of driving between them; the last one is the new keyframe"""
    from mrg_slam_amd import MapCloudStore, synth
    from mrg_slam_amd.loop_detector import Edge, KeyFrame
    from oracle import oracle as orc

    base = small_cloud(2000, 77)
    kfs = []
    for i in range(5):
        est = synth.make_pose([2.0 * i, 0.0, 0.0], synth.rot_z(0.01 * i))
        cloud = orc.transform_points(np.linalg.inv(est), base)[: 2000 - 37 * i]
        kf = KeyFrame(id=i + 1, cloud=cloud, estimate=est, accum_distance=20.0 * i, first_keyframe=(i == 0))
        if i:
            rel = np.linalg.inv(est) @ kfs[-1].estimate
            kf.prev_edge = Edge(kf, kfs[-1], rel)
            kfs[-1].next_edge = Edge(kf, kfs[-1], rel)
        kfs.append(kf)
    kfs[4].prev_edge = None  # the new keyframe has no odometry edge to the others here: they are all candidates but the first
    kfs[3].next_edge = None
    store = MapCloudStore()
    for kf in kfs:
        store.add(kf.store_key(), kf.cloud)
    return kfs, store


def test_a_key_the_store_lacks_is_refused_before_anything_is_queued(five):
    from mrg_slam_amd import BatchMatcher, HipLoopDetector, MapCloudStore, _lib

    kfs, store = five
    partial = MapCloudStore()
    for kf in kfs[:2] + kfs[3:]:
        partial.add(kf.store_key(), kf.cloud)  # keyframe 3 is missing: a candidate, and the neighbour of two more
    bm = BatchMatcher(_params("NDT_HIP"))
    t = bm.add_target_from_store(partial, kfs[4].store_key())  # something of the caller's is queued on the batch
    bm.add_pair_from_store(t, partial, kfs[1].store_key(), np.eye(4))
    hip = HipLoopDetector(None, bm, partial)
    with pytest.raises(_lib.MrgfeError, match=str(kfs[2].store_key())):
        hip.detect(kfs[:4], kfs[4:])
    assert _lib.lib().mrgfe_batch_num_pairs(bm._h) == 1  # nothing was cleared, nothing queued
    assert hip.loop_manager_entries() == [] and hip.loop_candidates_sizes == [] and hip.stats()["superset_pairs"] == 0
    rec = bm.align(float("inf"))  # ... and the batch is still usable
    assert len(rec) == 1
    # the same detector over a complete list works afterwards (keyframe 3 left out of the graph altogether)
    kfs[1].next_edge, keep_next = None, kfs[1].next_edge
    kfs[3].prev_edge, keep_prev = None, kfs[3].prev_edge
    try:
        loops = hip.detect([kfs[0], kfs[1], kfs[3]], kfs[4:])
    finally:
        kfs[1].next_edge, kfs[3].prev_edge = keep_next, keep_prev
    assert hip.stats()["superset_pairs"] == 2 and hip.stats()["target_builds"] == 1 and len(loops) <= 1


def test_a_call_without_candidates_touches_no_gpu(five):
    from mrg_slam_amd import BatchMatcher, HipLoopDetector

    kfs, store = five
    bm = BatchMatcher(_params("NDT_HIP"))
    hip = HipLoopDetector(None, bm, store)
    first = hip.detect(kfs[:4], kfs[4:])
    st = hip.stats()
    assert st["superset_pairs"] == 3 and st["new_keyframes"] == 1 and st["target_builds"] == 1
    rounds, pairs, timing = bm.rounds(), bm.timing(), hip.loop_candidates_sizes
    assert rounds > 0 and timing == [3]
    far = hip.detect(kfs[:4], [_moved(kfs[4], 500.0)])  # no keyframe within candidate_max_xy_distance
    assert far == [] and hip.detect(kfs[:4], []) == [] and hip.detect([], kfs[4:]) == []
    assert bm.rounds() == rounds and bm.timing() == pairs and hip.loop_candidates_sizes == [3]
    assert hip.stats() == {"superset_pairs": 0, "sequential_pairs": 0, "consistency_pairs": 0, "new_keyframes": 1, "target_builds": 0}
    assert [(lp.key1.id, lp.key2.id) for lp in first] == [(lp.key1.id, lp.key2.id) for lp in _fresh(five).detect(kfs[:4], kfs[4:])]


def _moved(kf, dx):
    from mrg_slam_amd.loop_detector import KeyFrame

    est = kf.estimate.copy()
    est[0, 3] += dx
    return KeyFrame(id=kf.id, cloud=kf.cloud, estimate=est, accum_distance=kf.accum_distance)


def _fresh(five, method="NDT_HIP"):
    from mrg_slam_amd import BatchMatcher, HipLoopDetector

    return HipLoopDetector(None, BatchMatcher(_params(method)), five[1])


def test_two_detectors_share_one_store(five):
    """two detectors (two batches, two methods) over one store: each gives what it gives alone, whatever the other did in between"""
    kfs, store = five
    alone = {m: _fresh(five, m).detect(kfs[:4], kfs[4:]) for m in ("NDT_HIP", "ICP_HIP")}
    a, b = _fresh(five, "NDT_HIP"), _fresh(five, "ICP_HIP")
    got_a1 = a.detect(kfs[:4], kfs[4:])
    got_b = b.detect(kfs[:4], kfs[4:])
    a.reset()
    got_a2 = a.detect(kfs[:4], kfs[4:])
    for got, want in ((got_a1, alone["NDT_HIP"]), (got_a2, alone["NDT_HIP"]), (got_b, alone["ICP_HIP"])):
        assert [(lp.key1.id, lp.key2.id) for lp in got] == [(lp.key1.id, lp.key2.id) for lp in want]
        for x, y in zip(got, want):
            assert x.relative_pose.tobytes() == y.relative_pose.tobytes() and x.score == y.score
    assert a.stats()["target_builds"] == b.stats()["target_builds"] == 1 and store.bytes() == sum(16 * len(k.cloud) for k in kfs)
