"""GPU: bounded best-candidate selection (mrgfe_batch_align_best / BatchMatcher.align_best, loop_detector.cpp:126-145 and :156-160) against
the full path (mrgfe_batch_align) on the same batch: the group winners and scores bit for bit, every EXACT record bit for bit, every PRUNED value a
lower bound above its group's best, and every certified interval around the full fitness."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.finfo(np.float64).max
POSE_FIELDS = ("T", "H", "trans_probability", "converged", "iterations", "evaluations", "pair_id")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _group_rule(rec, group, n_groups):
    """loop_closure.select_best per group on full records: (pair index or -1, score)"""
    from mrg_slam_amd.loop_closure import select_best

    out = []
    for g in range(n_groups):
        idx = np.flatnonzero(group == g)
        b, s = select_best(rec[idx])
        out.append((-1 if b is None else int(idx[b]), s))
    return out


def check_against_full(full, rec, state, best, score, group, n_groups, cap=None):
    from mrg_slam_amd import _lib

    for f in POSE_FIELDS:
        assert (_bits(rec[f]) == _bits(full[f])).all(), f
    ex = state == _lib.FIT_EXACT
    assert (_bits(rec["fitness"][ex]) == _bits(full["fitness"][ex])).all()
    assert (rec["fitness"][state == _lib.FIT_SKIPPED] == BIG).all()
    assert not ((state == _lib.FIT_SKIPPED) & (group >= 0) & (full["converged"] != 0) & (full["fitness"] != BIG)).any()
    want = _group_rule(full, group, n_groups)
    for g, (wb, ws) in enumerate(want):
        has = bool(((group == g) & (full["converged"] != 0)).any())
        if cap is not None and has and ws > cap:
            assert best[g] == -2 and score[g] > cap, (g, wb, ws, best[g], score[g])
            continue
        assert best[g] == wb and _bits(np.float64(score[g])) .tobytes() == _bits(np.float64(ws)).tobytes(), (g, wb, ws, best[g], score[g])
        pr = np.flatnonzero((group == g) & (state == _lib.FIT_PRUNED))
        assert (rec["fitness"][pr] <= full["fitness"][pr]).all() and (rec["fitness"][pr] > ws).all()
    # the unchanged host rule on the returned records, group by group
    got = _group_rule(rec, group, n_groups)
    for g, ((wb, ws), (gb, gs)) in enumerate(zip(want, got)):
        if cap is None or not ws > cap:
            assert (wb, ws) == (gb, gs), g
    return int((state == _lib.FIT_PRUNED).sum())


@pytest.fixture(scope="module")
def config3():
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from mrg_slam_amd import distance_filter

    raw, pairs = bench.make_loop_workload()
    scans = [distance_filter(s, 0.1, 35.0) for s in raw]
    dev = [torch.from_numpy(s).cuda() for s in scans]
    return scans, dev, pairs


def _queue_config3(bm, scans, dev, pairs, ids):
    targets = sorted({pairs[i][0] for i in ids})
    tpos = {a: k for k, a in enumerate(targets)}
    bm.add_device([dev[a].data_ptr() for a in targets], [len(scans[a]) for a in targets], np.array([tpos[pairs[i][0]] for i in ids], dtype=np.int32),
                  [dev[pairs[i][1]].data_ptr() for i in ids], [len(scans[pairs[i][1]]) for i in ids], np.stack([pairs[i][2] for i in ids]))


def test_config3_bounded_equals_full(config3):
    """256 loop-closure pairs, groups = new keyframes, max_range inf: winners, scores and EXACT records bit for bit; a share of the pairs pruned"""
    from mrg_slam_amd import BatchMatcher

    scans, dev, pairs = config3
    ids = list(range(len(pairs)))
    news = sorted({p[0] for p in pairs})
    group = np.array([news.index(p[0]) for p in pairs], dtype=np.int32)
    bm = BatchMatcher(transformation_epsilon=0.1, maximum_iterations=64)
    _queue_config3(bm, scans, dev, pairs, ids)
    full = bm.align(float("inf"))
    rec, state, best, score = bm.align_best(float("inf"), group)
    n_pruned = check_against_full(full, rec, state, best, score, group, len(news))
    st = bm.select_stats()
    print(f"config[3]: {n_pruned} of {len(pairs)} pairs pruned; stats {st}")
    assert n_pruned > 0
    assert st["pruned"] == n_pruned and st["exact"] + st["pruned"] + st["above_cap"] + st["skipped"] == len(pairs)


def _set_sweep(mode):
    from mrg_slam_amd._lib import lib

    return lib().mrgfe_dbg_set_fit_sweep(mode)


@pytest.fixture()
def sweep_mode():
    before = _set_sweep(-1)
    yield
    _set_sweep(before)


# sweep_off: MRGFE_FIT_SWEEP=0 — no seed, no sweep; the bounds come from the block pass alone and every queued contender takes the pyramid walk
@pytest.mark.parametrize("max_range,sweep_off", [(float("inf"), False), (1.0, False), (4.0, False), (float("inf"), True), (4.0, True)],
                         ids=["inf", "1.0", "4.0", "inf-sweep_off", "4.0-sweep_off"])
def test_bounds_hold_the_full_fitness(config3, sweep_mode, max_range, sweep_off):
    from mrg_slam_amd import BatchMatcher

    if sweep_off:
        assert _set_sweep(0) == 0
    scans, dev, pairs = config3
    ids = list(range(0, len(pairs), 2))
    news = sorted({pairs[i][0] for i in ids})
    group = np.array([news.index(pairs[i][0]) for i in ids], dtype=np.int32)
    bm = BatchMatcher(transformation_epsilon=0.1, maximum_iterations=64)
    _queue_config3(bm, scans, dev, pairs, ids)
    full = bm.align(max_range)
    rec, state, best, score = bm.align_best(max_range, group)
    lo, hi = bm.fit_bounds()
    conv = full["converged"] != 0
    assert (lo[conv] <= full["fitness"][conv]).all() and (full["fitness"][conv] <= hi[conv]).all()
    check_against_full(full, rec, state, best, score, group, len(news))


def _street_pairs(n=6):
    from mrg_slam_amd import prefilter, synth

    scene = synth.street_scene()
    out = []
    for k in range(n):
        tgt, src, rel = synth.scan_pair(k, "VLP16", scene)
        out.append((prefilter(tgt), prefilter(src), rel, synth.warm_guess(rel, k)))
    return out


@pytest.fixture(scope="module")
def street():
    return _street_pairs()


def _wrong(guess, dx):
    g = np.array(guess, dtype=np.float32, copy=True)
    g[0, 3] += dx
    return g


def test_duplicates_nonconverged_singletons_empty_groups_and_spans(street):
    from mrg_slam_amd import BatchMatcher

    tgt0, src0, _, g0 = street[0]
    tgt1, src1, _, g1 = street[1]
    for iters in (64, 1):
        bm = BatchMatcher(transformation_epsilon=0.01, maximum_iterations=iters)
        t0, t1 = bm.add_target(tgt0), bm.add_target(tgt1)
        plan = [  # (target, source, guess, group)
            (t0, src0, g0, 0), (t0, src0, g0, 0),            # duplicates: both exact, the last wins
            (t0, src1, _wrong(g0, 3.0), 0),
            (t1, src1, g1, 1),                               # a singleton group
            (t0, src0, _wrong(g0, 2.0), -1),                 # group -1 beside grouped pairs
            (t1, src0, _wrong(g1, 4.0), 3), (t0, src0, g0, 3),  # a group over two targets
            (t1, src1, _wrong(g1, 6.0), 0),
        ]                                                    # group 2: empty
        for t, s, g, _ in plan:
            bm.add_pair(t, s, g)
        group = np.array([p[3] for p in plan], dtype=np.int32)
        full = bm.align(float("inf"))
        rec, state, best, score = bm.align_best(float("inf"), group)
        check_against_full(full, rec, state, best, score, group, 4)
        assert best[2] == -1 and score[2] == BIG
        assert state[4] == 0
        from mrg_slam_amd import _lib

        if iters == 64:
            assert full["converged"][0] and full["converged"][1]
            assert state[0] == state[1] == _lib.FIT_EXACT and best[0] == 1
        nc = np.flatnonzero((full["converged"] == 0) & (group >= 0))
        assert (state[nc] == _lib.FIT_SKIPPED).all() and not np.isin(best, nc).any()


def test_score_cap_gives_minus_two_exactly_where_the_full_best_exceeds_it(street):
    from mrg_slam_amd import BatchMatcher

    bm = BatchMatcher(transformation_epsilon=0.01, maximum_iterations=64)
    group = []
    for k, (tgt, src, _, g) in enumerate(street):
        t = bm.add_target(tgt)
        if k % 2 == 0:  # a true candidate among wrong ones
            bm.add_pair(t, src, g)
            group.append(k)
        for dx in (5.0, 9.0):
            bm.add_pair(t, src, _wrong(g, dx))
            group.append(k)
    group = np.array(group, dtype=np.int32)
    full = bm.align(float("inf"))
    rec, state, best, score = bm.align_best(float("inf"), group, score_cap=1.25)
    check_against_full(full, rec, state, best, score, group, len(street), cap=1.25)
    assert (best == -2).any() and (best >= 0).any()


def test_gicp_batch_bounded_equals_full(street):
    from mrg_slam_amd import BatchMatcher
    from mrg_slam_amd._lib import GICP_HIP
    from mrg_slam_amd.registration import default_params

    bm = BatchMatcher(default_params(GICP_HIP))
    group = []
    for k, (tgt, src, _, g) in enumerate(street[:3]):
        t = bm.add_target(tgt)
        for dx in (0.0, 3.0, 8.0):
            bm.add_pair(t, src, _wrong(g, dx))
            group.append(k)
    group = np.array(group, dtype=np.int32)
    full = bm.align(float("inf"))
    rec, state, best, score = bm.align_best(float("inf"), group)
    check_against_full(full, rec, state, best, score, group, 3)


@pytest.mark.parametrize("keyed", [False, True])
def test_call_sequences_match_fresh_batches(street, keyed):
    from mrg_slam_amd import BatchMatcher

    def queue(bm):
        bm.clear()
        group = []
        for k, (tgt, src, _, g) in enumerate(street[:4]):
            t = bm.add_target(tgt)
            for j, dx in enumerate((0.0, 4.0)):
                key = 100 + 10 * k + j if keyed else 0
                bm.add_pair(t, None if keyed and bm.has_cloud(key) == len(src) else src, _wrong(g, dx), key=key)
                group.append(k)
        return np.array(group, dtype=np.int32)

    def fresh(kind):
        bm = BatchMatcher(transformation_epsilon=0.01, maximum_iterations=64)
        group = queue(bm)
        return bm.align(float("inf")) if kind == "full" else bm.align_best(float("inf"), group)

    ref_best, ref_full = fresh("best"), fresh("full")
    bm = BatchMatcher(transformation_epsilon=0.01, maximum_iterations=64)
    for kind in ("best", "full", "best"):
        group = queue(bm)
        got = bm.align(float("inf")) if kind == "full" else bm.align_best(float("inf"), group)
        if kind == "full":
            assert _bits(got).tobytes() == _bits(ref_full).tobytes()
        else:
            for a, b in zip(got, ref_best):
                assert _bits(a).tobytes() == _bits(b).tobytes()


def test_detect_batched_bounded_equals_full():
    """the ring session (two robots, the 15 m gates pruning inside calls) with six new keyframes per call: the same Loop list either way"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from loop_session import make_ring_session, run_session
    from mrg_slam_amd import BatchMatcher, prefilter
    from mrg_slam_amd.loop_detector import LoopDetector

    reg_kw = dict(resolution=1.0, transformation_epsilon=0.01, maximum_iterations=64)
    pf = lambda c: prefilter(c, {"downsample_resolution": 0.2})  # noqa: E731
    out = {}
    for mode in ("full", "bounded"):
        kfs, order = make_ring_session(64, "VLP64", prefilter=pf)
        det = LoopDetector({"fitness_selection": mode}, matcher=BatchMatcher(**reg_kw))
        out[mode] = run_session(det, kfs, order, group=6, batched=True)
    a, b = out["full"], out["bounded"]
    assert len(a) >= 3 and any(lp.key1.slam_uuid != lp.key2.slam_uuid for lp in a)
    assert [(lp.key1.id, lp.key2.id) for lp in a] == [(lp.key1.id, lp.key2.id) for lp in b]
    for x, y in zip(a, b):
        assert _bits(x.relative_pose).tobytes() == _bits(y.relative_pose).tobytes()


def test_match_candidates_bounded_equals_full(street):
    from mrg_slam_amd import BatchMatcher, loop_closure

    tgt = street[0][0]
    clouds = [s[1] for s in street]
    guesses = [_wrong(street[0][3], dx) for dx in (0.0, 2.0, 5.0, 0.0, 9.0, 1.0)]
    full = loop_closure.match_candidates(lambda: BatchMatcher(transformation_epsilon=0.01, maximum_iterations=64), tgt, clouds, guesses)
    bnd = loop_closure.match_candidates(lambda: BatchMatcher(transformation_epsilon=0.01, maximum_iterations=64), tgt, clouds, guesses, select="bounded")
    assert full[1] == bnd[1] and full[2] == bnd[2]
    for f in POSE_FIELDS:
        assert _bits(full[0][f]).tobytes() == _bits(bnd[0][f]).tobytes()
