"""GPU: PCL_GICP_HIP / PCL_GICP_OMP_HIP in mrgfe_batch_* and the loop detector, behind Context.set_bfgs_batches.  The pairs of a batch advance
through pcl::GICP's BFGS in lock step (per round the searches of the pairs that begin an outer iteration, one cost / gradient launch, one sum launch
with ONE workgroup per pair, ONE host wait), on the arithmetic and the decisions of the single registration: every record must equal a fresh
PclGicpHip registration of the same pair bit for bit, and the CPU oracle within the bar of tests/test_gpu_gicp.py (1e-4 m / 1e-4 rad, same
convergence decision and iteration count).  Every test makes its own Context with the switch on; the default context keeps refusing."""
import copy

import numpy as np
import pytest

from pclgicp_cases import EPS, SIZES, batch_workload, oracle_results, pcl_params, pose_errors

pytestmark = pytest.mark.gpu

POSE_FIELDS = ("T", "H", "trans_probability", "converged", "iterations", "evaluations", "pair_id")
CONFIGS = {"serial": dict(omp=False), "omp8": dict(omp=True, num_threads=8), "omp1": dict(omp=True, num_threads=1)}


def _ctx():
    from mrg_slam_amd import Context

    c = Context()
    c.set_bfgs_batches(True)
    return c


def _single(params, target, src, guess, ctx):
    """(T, converged, iterations, evaluations, fitness) of a fresh single registration"""
    from mrg_slam_amd import PclGicpHip
    from mrg_slam_amd._lib import PCL_GICP_OMP_HIP

    r = PclGicpHip(params.correspondence_randomness, params.max_correspondence_distance, params.transformation_epsilon, params.rotation_epsilon, params.maximum_iterations,
                   params.max_optimizer_iterations, omp=params.method == PCL_GICP_OMP_HIP, num_threads=params.num_threads, ctx=ctx)
    r.setInputTarget(target)
    r.setInputSource(src)
    r.align(guess)
    fit = r.getFitnessScore() if len(target) and len(src) else None
    return r.getFinalTransformation(), r.hasConverged(), r.getFinalNumIteration(), r.evals, fit


def _batch(params, targets, pairs, ctx, fit=float("inf"), matcher=None):
    from mrg_slam_amd import BatchMatcher

    bm = matcher or BatchMatcher(params, ctx=ctx)
    bm.clear()
    tids = [bm.add_target(t) for t in targets]
    for ti, src, guess in pairs:
        bm.add_pair(tids[ti], src, guess)
    return bm, bm.align(fit)


def _same(a, b, fields=POSE_FIELDS + ("fitness",)):
    for f in fields:
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f


def _equals_single(params, targets, pairs, rec, ctx, singles=None):
    from mrg_slam_amd.registration import result_matrix

    for k, (ti, src, guess) in enumerate(pairs):
        T, conv, it, ev, fit = singles[k] if singles is not None else _single(params, targets[ti], src, guess, ctx)
        np.testing.assert_array_equal(result_matrix(rec[k]), T, err_msg=f"pair {k}")
        assert (bool(rec[k]["converged"]), int(rec[k]["iterations"]), int(rec[k]["evaluations"])) == (conv, it, ev), k
        assert not rec[k]["H"].any() and rec[k]["trans_probability"] == 0 and rec[k]["pair_id"] == k
        if fit is not None:
            assert rec[k]["fitness"] == pytest.approx(fit, rel=1e-12), k


@pytest.fixture(scope="module")
def workload():
    return batch_workload()


@pytest.fixture(scope="module")
def ctx():
    return _ctx()


@pytest.fixture(scope="module")
def results(workload, ctx):
    """per configuration: (single-engine results, batch matcher, batch records) — computed once, read by the tests below"""
    targets, pairs = workload
    out = {}
    for name, kw in CONFIGS.items():
        p = pcl_params(**kw)
        singles = [_single(p, targets[ti], src, guess, ctx) for ti, src, guess in pairs]
        bm, got = _batch(p, targets, pairs, ctx)
        out[name] = (singles, bm, got)
    return out


@pytest.mark.parametrize("config", list(CONFIGS))
def test_batch_records_equal_single_registrations_and_the_oracle(workload, results, ctx, config):
    from mrg_slam_amd.registration import result_matrix

    targets, pairs = workload
    singles, bm, got = results[config]
    p = pcl_params(**CONFIGS[config])
    evs = [s[3] for s in singles]
    print(f"{config}: evaluations {evs}, iterations {[s[2] for s in singles]}, rounds {bm.rounds()}")
    assert len(set(evs)) >= 3 and all(s[1] for s in singles)  # the pairs leave the busy list in different rounds
    _equals_single(p, targets, pairs, got, ctx, singles)
    assert 0 < bm.rounds() <= max(int(r["evaluations"]) for r in got)
    again = bm.align(float("inf"))  # a second align of the same batch: the working copies start from the sources again
    _same(again, got)
    for k, (To, conv, it, _) in enumerate(oracle_results(p, targets, pairs)):
        dt, dr = pose_errors(result_matrix(got[k]), To)
        print(f"  pair {k}: {got[k]['iterations']} iterations (oracle {it}), {got[k]['evaluations']} evaluations, {dt:.3g} m, {dr:.3g} rad")
        assert bool(got[k]["converged"]) == conv and got[k]["iterations"] == it, k
        assert dt <= 1e-4 and dr <= 1e-4, k


@pytest.mark.parametrize("config", ["serial", "omp8"])
def test_tree_mode_records_equal_single_registrations(workload, ctx, config):
    """mrgfe_dbg_set_pclgicp_reference_order(0): the sums of both routes come out of the block tree (the reduction of gicp_reduce_kernel, pair by pair)"""
    from mrg_slam_amd._lib import lib

    targets, pairs = workload
    p = pcl_params(**CONFIGS[config])
    try:
        assert lib().mrgfe_dbg_set_pclgicp_reference_order(0) == 0
        bm, got = _batch(p, targets, pairs, ctx)
        _equals_single(p, targets, pairs, got, ctx)
        assert 0 < bm.rounds() <= max(int(r["evaluations"]) for r in got)
    finally:
        lib().mrgfe_dbg_set_pclgicp_reference_order(1)


@pytest.mark.parametrize("config", ["serial", "omp8"])
def test_degenerate_pairs_beside_healthy_ones(workload, results, ctx, config):
    targets, pairs = workload
    empty = np.zeros((0, 4), np.float32)
    healthy = pairs[:3]
    g = pairs[0][2]
    far = pairs[0][1] + np.float32([1000, 0, 0, 0])
    p = pcl_params(**CONFIGS[config])
    # targets: 0, 1 as before, 2 empty.  An empty source, an empty target, fewer than four correspondences, a 3-point source
    extra = [(0, empty, g), (2, pairs[1][1], g), (0, far, g), (0, pairs[0][1][:3], g)]
    mixed = [healthy[0], extra[0], healthy[1], extra[1], extra[2], healthy[2], extra[3]]
    all_targets = targets + [empty]
    _, got = _batch(p, all_targets, mixed, ctx)
    _equals_single(p, all_targets, mixed, got, ctx)
    for k in (1, 3, 4):
        assert got[k]["converged"] == 0 and got[k]["iterations"] == 0, k
    for k_mixed, k_all in ((0, 0), (2, 1), (5, 2)):
        _same(got[k_mixed], results[config][2][k_all], fields=("T", "H", "trans_probability", "converged", "iterations", "evaluations"))


def test_iteration_limits(workload, ctx):
    targets, pairs = workload
    for kw in (dict(maximum_iterations=1, eps=1e-12), dict(max_optimizer_iterations=1), dict(max_optimizer_iterations=2), dict(omp=True, max_optimizer_iterations=2)):
        p = pcl_params(**kw)
        _, got = _batch(p, targets, pairs[:4], ctx)
        _equals_single(p, targets, pairs[:4], got, ctx)
        if "maximum_iterations" in kw:  # the iteration limit counts as converged
            assert all(r["converged"] == 1 and r["iterations"] == 1 for r in got)


@pytest.mark.parametrize("config", ["serial", "omp8"])
def test_keyed_store_fed_cleared_bounded_and_async(workload, results, ctx, config):
    from mrg_slam_amd import BatchMatcher, MapCloudStore

    targets, pairs = workload
    _, _, want = results[config]
    p = pcl_params(**CONFIGS[config])
    # keyed pairs: the clouds and their covariances (PCL's form) stay in the batch's store; the second time no cloud is handed over
    keyed = BatchMatcher(p, ctx=ctx)
    for rep in range(2):
        keyed.clear()
        tids = [keyed.add_target(t) for t in targets]
        for k, (ti, src, guess) in enumerate(pairs):
            keyed.add_pair(tids[ti], src if rep == 0 else None, guess, key=100 + k)
        _same(keyed.align(float("inf")), want)
    # targets and pairs out of a map store
    store = MapCloudStore(ctx)
    for k, t in enumerate(targets):
        store.add(1 + k, t)
    for k, (_, src, _) in enumerate(pairs):
        store.add(100 + k, src)
    fed = BatchMatcher(p, ctx=ctx)
    tids = [fed.add_target_from_store(store, 1 + k) for k in range(len(targets))]
    for k, (ti, _, guess) in enumerate(pairs):
        fed.add_pair_from_store(tids[ti], store, 100 + k, guess)
    _same(fed.align(float("inf")), want)
    # clear_pairs, then new pairs on the old targets: what was built for the targets is kept, the records are the same
    fed.clear_pairs()
    for k, (ti, _, guess) in enumerate(pairs):
        fed.add_pair_from_store(tids[ti], store, 100 + k, guess)
    _same(fed.align(float("inf")), want)
    # bounded selection over two groups (the candidates of target 0 / of target 1): the winners and scores of the full-fitness path
    group = np.array([ti for ti, _, _ in pairs], dtype=np.int32)
    bm, _ = _batch(p, targets, pairs, ctx)
    rec, state, best, best_score = bm.align_best(float("inf"), group)
    _same(rec, want, fields=POSE_FIELDS)
    for g in (0, 1):
        members = [k for k in range(len(pairs)) if group[k] == g and want[k]["converged"]]
        winner = max((k for k in members if want[k]["fitness"] == min(want[m]["fitness"] for m in members)))  # among equal scores the last wins
        assert best[g] == winner and best_score[g] == want[winner]["fitness"]
    # asynchronous align
    bm.align_async(float("inf"))
    _same(bm.wait(), want)


def test_loop_detectors_equal_the_sequential_registration(ctx, monkeypatch):
    """A 28-keyframe ring session (two robots), four new keyframes per call: detect_batched over a PCL_GICP_HIP BatchMatcher and the one-call
    HipLoopDetector over the same kind of batch and a MapCloudStore return the Loop list of detect() with one PclGicpHip registration, loop for loop,
    with the same relative poses.  (All three align from the library's float guesses, as tests/test_gpu_loop_detect.py arranges it.)"""
    from loop_session import make_ring_session, run_session
    from mrg_slam_amd import BatchMatcher, HipLoopDetector, MapCloudStore, PclGicpHip
    from mrg_slam_amd import loop_detector as ld
    from oracle import oracle as orc

    monkeypatch.setattr(ld, "normalize_estimate", ld.lib_normalize_estimate)
    monkeypatch.setattr(ld.LoopDetector, "_guess", lambda self, ne, kf: ld.lib_guess(ne, kf.estimate, self.p["use_planar_registration_guess"]))
    pf = lambda c: orc.voxelgrid(orc.distance_filter(c, 0.1, 35.0), 0.25, 1)[0]  # noqa: E731
    p = pcl_params()
    session = make_ring_session(28, "VLP16", prefilter=pf)
    out = {}
    for name in ("sequential", "batched", "one_call"):
        kfs, order = copy.deepcopy(session)  # (run_session enters the loops it finds into the keyframes' graph)
        if name == "sequential":
            det = ld.LoopDetector(registration=PclGicpHip(transformation_epsilon=EPS, ctx=ctx))
        elif name == "batched":
            det = ld.LoopDetector(matcher=BatchMatcher(p, ctx=ctx))
        else:
            store = MapCloudStore(ctx)
            for kf in kfs:
                store.add(kf.store_key(), kf.cloud)
            det = HipLoopDetector(None, BatchMatcher(p, ctx=ctx), store)
        out[name] = run_session(det, kfs, order, group=4, batched=(name == "batched"))
    ref = out["sequential"]
    assert len(ref) >= 2
    for name in ("batched", "one_call"):
        got = out[name]
        assert [(lp.key1.id, lp.key2.id) for lp in got] == [(lp.key1.id, lp.key2.id) for lp in ref], name
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a.relative_pose, b.relative_pose, err_msg=name)


def test_the_door_is_the_context_switch():
    from mrg_slam_amd import BatchMatcher, Context, MrgfeError, NodeMatcher, _lib
    from mrg_slam_amd.registration import default_params

    closed, opened = Context(), _ctx()
    for method in (_lib.PCL_GICP_HIP, _lib.PCL_GICP_OMP_HIP):
        with pytest.raises(MrgfeError, match="single registrations only"):
            BatchMatcher(default_params(method), ctx=closed)
        with pytest.raises(MrgfeError, match="single registrations only"):
            NodeMatcher([0], default_params(method))
        BatchMatcher(default_params(method), ctx=opened)
    # off again: refused again, with the code and the text of a context that never had it on
    opened.set_bfgs_batches(False)
    with pytest.raises(MrgfeError, match="single registrations only") as e:
        BatchMatcher(default_params(_lib.PCL_GICP_HIP), ctx=opened)
    assert e.value.status == _lib.ERR_INVALID
    assert _lib.lib().mrgfe_ctx_set_bfgs_batches(None, 1) == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_ctx_set_bfgs_batches:")
    assert SIZES[1] < 256  # (the workload keeps its one-tile pair)
