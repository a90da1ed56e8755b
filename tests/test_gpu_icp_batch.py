"""GPU: ICP_HIP in mrgfe_batch_* / mrgfe_node_* / the loop detector.  The pairs of a batch advance through pcl::IterativeClosestPoint's loop in lock
step (one correspondence + moment launch, one reduction and ONE host wait per round for all pairs still running), on the arithmetic of the single
registration: every record must equal a fresh IcpHip registration of the same pair bit for bit, and the CPU oracle within the bar of
tests/test_gpu_gicp.py (1e-4 m / 1e-4 rad, same convergence decision and iteration count)."""
import copy

import numpy as np
import pytest

from icp_cases import EPS, SIZES, batch_workload, icp_params, pose_errors

pytestmark = pytest.mark.gpu

POSE_FIELDS = ("T", "H", "trans_probability", "converged", "iterations", "evaluations", "pair_id")


def _single(params, target, src, guess):
    """(T, converged, iterations, evaluations, fitness) of a fresh single registration"""
    from mrg_slam_amd import IcpHip

    r = IcpHip(params.max_correspondence_distance, params.transformation_epsilon, params.maximum_iterations, bool(params.use_reciprocal_correspondences))
    r.setInputTarget(target)
    r.setInputSource(src)
    r.align(guess)
    fit = r.getFitnessScore() if len(target) and len(src) else None
    return r.getFinalTransformation(), r.hasConverged(), r.getFinalNumIteration(), r.evals, fit


def _batch(params, targets, pairs, fit=float("inf"), matcher=None):
    from mrg_slam_amd import BatchMatcher

    bm = matcher or BatchMatcher(params)
    bm.clear()
    tids = [bm.add_target(t) for t in targets]
    for ti, src, guess in pairs:
        bm.add_pair(tids[ti], src, guess)
    return bm, bm.align(fit)


def _same(a, b, fields=POSE_FIELDS + ("fitness",)):
    for f in fields:
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f


def _equals_single(params, targets, pairs, rec, singles=None):
    from mrg_slam_amd.registration import result_matrix

    for k, (ti, src, guess) in enumerate(pairs):
        T, conv, it, ev, fit = singles[k] if singles is not None else _single(params, targets[ti], src, guess)
        np.testing.assert_array_equal(result_matrix(rec[k]), T, err_msg=f"pair {k}")
        assert (bool(rec[k]["converged"]), int(rec[k]["iterations"]), int(rec[k]["evaluations"])) == (conv, it, ev), k
        assert not rec[k]["H"].any() and rec[k]["trans_probability"] == 0 and rec[k]["pair_id"] == k
        if fit is not None:
            assert rec[k]["fitness"] == pytest.approx(fit, rel=1e-12), k


@pytest.fixture(scope="module")
def workload():
    return batch_workload()


@pytest.fixture(scope="module")
def results(workload):
    """per mode: (single-engine results, batch matcher, batch records) — computed once, read by the tests below"""
    targets, pairs = workload
    out = {}
    for rec in (False, True):
        p = icp_params(rec)
        singles = [_single(p, targets[ti], src, guess) for ti, src, guess in pairs]
        bm, got = _batch(p, targets, pairs)
        out[rec] = (singles, bm, got)
    return out


@pytest.mark.parametrize("reciprocal", [False, True])
def test_batch_records_equal_single_registrations_and_the_oracle(workload, results, reciprocal):
    from mrg_slam_amd.registration import result_matrix
    from oracle import oracle as orc

    targets, pairs = workload
    singles, bm, got = results[reciprocal]
    p = icp_params(reciprocal)
    its = [s[2] for s in singles]
    print(f"reciprocal={reciprocal}: iterations {its}, rounds {bm.rounds()}")
    assert len(set(its)) >= 3 and all(s[1] for s in singles)  # the pairs leave the busy list in different rounds
    _equals_single(p, targets, pairs, got, singles)
    assert bm.rounds() == max(s[3] for s in singles)
    again = bm.align(float("inf"))  # a second align of the same batch: the working copies start from the sources again
    _same(again, got)
    for k, (ti, src, guess) in enumerate(pairs):
        o = orc.Icp(transformation_epsilon=EPS, use_reciprocal_correspondences=reciprocal)
        o.setInputTarget(targets[ti])
        o.setInputSource(src)
        o.align(guess)
        dt, dr = pose_errors(result_matrix(got[k]), o.getFinalTransformation())
        print(f"  pair {k}: {got[k]['iterations']} iterations (oracle {o.getFinalNumIteration()}), {dt:.3g} m, {dr:.3g} rad")
        assert bool(got[k]["converged"]) == o.hasConverged() and got[k]["iterations"] == o.getFinalNumIteration(), k
        assert dt <= 1e-4 and dr <= 1e-4, k
    if reciprocal:
        for k in range(len(pairs)):
            assert not np.array_equal(got[k]["T"], results[False][2][k]["T"]), k


def test_degenerate_pairs_beside_healthy_ones(workload, results):
    from mrg_slam_amd.registration import result_matrix

    targets, pairs = workload
    empty = np.zeros((0, 4), np.float32)
    healthy = pairs[:3]
    g = pairs[0][2]
    far = pairs[0][1] + np.float32([1000, 0, 0, 0])
    p = icp_params()
    # targets: 0, 1 as before, 2 empty
    extra = [(0, empty, g), (2, pairs[1][1], g), (0, far, g), (0, pairs[0][1][:2], g)]
    mixed = [healthy[0], extra[0], healthy[1], extra[1], extra[2], healthy[2], extra[3]]
    _, got = _batch(p, targets + [empty], mixed)
    for k in (1, 3, 4, 6):
        assert got[k]["converged"] == 0 and got[k]["iterations"] == 0 and got[k]["evaluations"] == 1, k
        np.testing.assert_array_equal(result_matrix(got[k]), np.asarray(g, dtype=np.float32))
        assert not got[k]["H"].any() and got[k]["pair_id"] == k
    _, alone = _batch(p, targets, healthy)
    for k_mixed, k_alone in ((0, 0), (2, 1), (5, 2)):
        _same(got[k_mixed], alone[k_alone], fields=("T", "H", "fitness", "trans_probability", "converged", "iterations", "evaluations"))
        _same(alone[k_alone], results[False][2][k_alone], fields=("T", "converged", "iterations", "evaluations"))
    # the iteration limit counts as converged
    _, one = _batch(icp_params(eps=1e-12, maximum_iterations=1), targets, healthy)
    assert all(r["converged"] == 1 and r["iterations"] == 1 and r["evaluations"] == 1 for r in one)
    _equals_single(icp_params(eps=1e-12, maximum_iterations=1), targets, healthy, one)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_identity_guess_beside_other_guesses(workload, reciprocal):
    targets, pairs = workload
    mixed = [(ti, src, np.eye(4) if k % 2 == 0 else guess) for k, (ti, src, guess) in enumerate(pairs[:4])]
    p = icp_params(reciprocal)
    _, got = _batch(p, targets, mixed)
    _equals_single(p, targets, mixed, got)


def test_keyed_store_fed_bounded_and_async(workload, results):
    from mrg_slam_amd import BatchMatcher, MapCloudStore

    targets, pairs = workload
    _, _, want = results[False]
    p = icp_params()
    # keyed pairs: the clouds stay in the batch's store, and cost 16 bytes per point — no covariances
    keyed = BatchMatcher(p)
    for rep in range(2):
        keyed.clear()
        tids = [keyed.add_target(t) for t in targets]
        for k, (ti, src, guess) in enumerate(pairs):
            keyed.add_pair(tids[ti], src if rep == 0 else None, guess, key=100 + k)
        _same(keyed.align(float("inf")), want)
        assert keyed.store_bytes() == 16 * sum(SIZES)
    # targets and pairs out of a map store: nothing is cached in the batch
    store = MapCloudStore()
    for k, t in enumerate(targets):
        store.add(1 + k, t)
    for k, (_, src, _) in enumerate(pairs):
        store.add(100 + k, src)
    fed = BatchMatcher(p)
    tids = [fed.add_target_from_store(store, 1 + k) for k in range(len(targets))]
    for k, (ti, _, guess) in enumerate(pairs):
        fed.add_pair_from_store(tids[ti], store, 100 + k, guess)
    _same(fed.align(float("inf")), want)
    assert fed.store_bytes() == 0
    # bounded selection over two groups (the candidates of target 0 / of target 1): the winners and scores of the full-fitness path
    group = np.array([ti for ti, _, _ in pairs], dtype=np.int32)
    bm, _ = _batch(p, targets, pairs)
    rec, state, best, best_score = bm.align_best(float("inf"), group)
    _same(rec, want, fields=POSE_FIELDS)
    for g in (0, 1):
        members = [k for k in range(len(pairs)) if group[k] == g and want[k]["converged"]]
        winner = max((k for k in members if want[k]["fitness"] == min(want[m]["fitness"] for m in members)))  # among equal scores the last wins
        assert best[g] == winner and best_score[g] == want[winner]["fitness"]
    # asynchronous align
    bm.align_async(float("inf"))
    _same(bm.wait(), want)


def test_node_members_give_the_records_of_one_batch(workload, results):
    from mrg_slam_amd import NodeMatcher

    targets, pairs = workload
    for reciprocal in (False, True):
        want = results[reciprocal][2]
        node = NodeMatcher([0, 0], icp_params(reciprocal))
        tids = [node.add_target(t) for t in targets]
        for ti, src, guess in pairs:
            node.add_pair(tids[ti], src, guess)
        assert node.align(float("inf")).tobytes() == want.tobytes()
        node.close()


def test_loop_detector_batched_equals_the_sequential_registration():
    """A 28-keyframe ring session (two robots), four new keyframes per call: detect_batched over an ICP BatchMatcher — full and bounded fitness selection —
    returns the Loop list of detect() with one IcpHip registration, loop for loop, with the same relative poses."""
    from loop_session import make_ring_session, run_session
    from mrg_slam_amd import BatchMatcher, IcpHip
    from mrg_slam_amd.loop_detector import LoopDetector
    from oracle import oracle as orc

    pf = lambda c: orc.voxelgrid(orc.distance_filter(c, 0.1, 35.0), 0.25, 1)[0]  # noqa: E731
    p = icp_params(eps=0.01)
    session = make_ring_session(28, "VLP16", prefilter=pf)
    out = {}
    for name in ("sequential", "batched", "bounded", "one_by_one"):
        kfs, order = copy.deepcopy(session)  # (run_session enters the loops it finds into the keyframes' graph)
        if name == "sequential":
            det = LoopDetector(registration=IcpHip(transformation_epsilon=0.01))
        else:
            det = LoopDetector({"fitness_selection": "bounded" if name == "bounded" else "full"}, matcher=BatchMatcher(p))
        if name == "one_by_one":
            out[name] = run_session(det, kfs, order, group=4)  # detect() with the matcher: the candidates of one new keyframe per batch
        else:
            out[name] = run_session(det, kfs, order, group=4, batched=(name != "sequential"))
    ref = out["sequential"]
    assert len(ref) >= 2
    for name in ("batched", "bounded", "one_by_one"):
        got = out[name]
        assert [(lp.key1.id, lp.key2.id) for lp in got] == [(lp.key1.id, lp.key2.id) for lp in ref], name
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a.relative_pose, b.relative_pose, err_msg=name)


def test_pcl_gicp_stays_refused():
    from mrg_slam_amd import BatchMatcher, MrgfeError, _lib  # noqa: F401
    from mrg_slam_amd.registration import default_params

    for method in (_lib.PCL_GICP_HIP, _lib.PCL_GICP_OMP_HIP):
        with pytest.raises(MrgfeError, match="single registrations only"):
            BatchMatcher(default_params(method))
