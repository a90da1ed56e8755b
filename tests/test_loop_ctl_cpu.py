"""CPU: the one-call loop detector (mrgfe_loop_detect, csrc/loop_ctl.h + csrc/loop_detect.cpp) with a scripted aligner in place of both GPU batches
(mrgfe_dbg_loop_set_aligner), no GPU involved.

1. The twelve random two-robot sessions of tests/test_loop_detector_cpu.py (its `_random_session`, same seeds, arrival groups 1, 2, 5 and 8) against the
   mirror's SEQUENTIAL detect() over a ScriptedRegistration on the same table: same (key1, key2) list, relative_pose bit for bit (it is copied from the
   records), same loop_candidates_sizes, same final LoopManager entries; superset_pairs >= sequential_pairs with pruning seen for groups > 1; every
   alignment the sequential loop ran is among those the aligner was asked for.
2. Edge cases: empty lists, an unknown prev_key, key 0, a capacity too small, a failing aligner (state and counters unchanged), mrgfe_loop_reset.
3. mrgfe_loop_guess / mrgfe_loop_normalize_estimate against the mirror on 200 random poses."""
import ctypes as C

import numpy as np
import pytest

from mrg_slam_amd import _lib, synth
from mrg_slam_amd.loop_detector import HipLoopDetector, LoopDetector, lib_guess, lib_normalize_estimate, normalize_estimate
from test_loop_detector_cpu import ScriptedRegistration, _random_session

PRM = {"accum_distance_thresh_same_robot": 15.0, "accum_distance_thresh_other_robot": 5.0, "candidate_max_xy_distance": 6.0}


class TableAligner:
    """the aligner callback over a session's table: keys are store keys, the table is keyed by keyframe ids"""

    def __init__(self, table, kfs):
        self.table, self.calls, self.fail = table, [], False
        self.id_of = {kf.store_key(): kf.id for kf in kfs}

    def __call__(self, stage, target_keys, pair_target, source_keys, guesses, want_fitness):
        if self.fail:
            raise RuntimeError("scripted failure")
        out = []
        for t, s, g in zip(pair_target, source_keys, guesses):
            ids = (self.id_of[target_keys[t]], self.id_of[s])
            self.calls.append(ids)
            T, conv, score = self.table[ids]
            out.append((g if T is None else T, conv, score))
        return out


def _manager(det_seq, hip):
    """the mirror's LoopManager as (slam id, slam id, key1, key2) entries, ordered as mrgfe_dbg_loop_manager orders them"""
    out = []
    for a, inner in det_seq.loop_manager.loop_map.items():
        for b, lp in inner.items():
            out.append((hip.slam_id(a), hip.slam_id(b), lp.key1.store_key(), lp.key2.store_key()))
    return sorted(out)


@pytest.mark.parametrize("seed", range(12))
def test_one_call_detect_returns_the_sequential_loop_list(seed):
    rng = np.random.default_rng(1000 + seed)
    kfs, news, table = _random_session(rng)
    seq = LoopDetector(PRM, registration=ScriptedRegistration(table))
    aligner = TableAligner(table, kfs + news)
    hip = HipLoopDetector(PRM, aligner=aligner)
    group = [1, 2, 5, 8][seed % 4]
    n_loops, pruned = 0, 0
    for g0 in range(0, len(news), group):
        batch = news[g0:g0 + group]
        ls, lh = seq.detect(kfs, batch), hip.detect(kfs, batch)
        assert [(lp.key1.id, lp.key2.id) for lp in ls] == [(lp.key1.id, lp.key2.id) for lp in lh]
        for a, b in zip(ls, lh):
            assert a.key1 is b.key1 and a.key2 is b.key2
            assert a.relative_pose.dtype == b.relative_pose.dtype == np.float32 and a.relative_pose.tobytes() == b.relative_pose.tobytes()
            assert b.score == table[(a.key1.id, a.key2.id)][2]
        n_loops += len(ls)
        st = hip.stats()
        if st["superset_pairs"]:
            assert st["superset_pairs"] >= st["sequential_pairs"] and st["new_keyframes"] == len(batch)
            assert hip.last_batched == {k: st[k] for k in ("superset_pairs", "sequential_pairs", "consistency_pairs", "new_keyframes")}
            assert 1 <= st["target_builds"] <= len(batch)
            pruned += st["superset_pairs"] - st["sequential_pairs"]
    assert n_loops >= 2
    assert seq.loop_candidates_sizes == hip.loop_candidates_sizes and len(hip.loop_detection_times) == len(hip.loop_candidates_sizes)
    assert hip.average_time_per_candidate_us() is not None and all(t >= 0 for t in hip.loop_detection_times)
    if group > 1:
        assert pruned > 0, "the session never exercised the LoopManager gates inside a call"
    assert set(seq.registration.calls) <= set(aligner.calls)
    assert hip.loop_manager_entries() == _manager(seq, hip) and len(hip.loop_manager_entries()) >= 1


def test_bounded_selection_and_planar_guess_take_the_same_decisions():
    """fitness_selection only changes which GPU call stage 1 makes (the aligner sees the same pairs); the planar guess reaches the aligner with z = 0"""
    kfs, news, table = _random_session(np.random.default_rng(1003))
    seq = LoopDetector(dict(PRM, use_planar_registration_guess=True), registration=ScriptedRegistration(table))
    aligner = TableAligner(table, kfs + news)
    seen = []
    hip = HipLoopDetector(dict(PRM, fitness_selection="bounded", use_planar_registration_guess=True),
                          aligner=lambda stage, tk, pt, sk, g, wf: (seen.append((stage, g.copy(), wf)), aligner(stage, tk, pt, sk, g, wf))[1])
    for g0 in range(0, len(news), 4):
        a, b = seq.detect(kfs, news[g0:g0 + 4]), hip.detect(kfs, news[g0:g0 + 4])
        assert [(lp.key1.id, lp.key2.id) for lp in a] == [(lp.key1.id, lp.key2.id) for lp in b]
    assert {s for s, _, _ in seen} == {1, 2} and all(wf == (s == 1) for s, _, wf in seen)
    assert all((g[:, 2, 3] == 0).all() and (g[:, 3, :] == [0, 0, 0, 1]).all() for _, g, _ in seen)


def _raw(det, kfs, news, edges=(), capacity=None):
    """mrgfe_loop_detect itself: (status, n_loops, records)"""
    ek = (C.c_uint64 * max(2 * len(edges), 1))(*[k for e in edges for k in e])
    cap = len(news) if capacity is None else capacity
    out = (_lib.LoopResult * max(cap, 1))()
    n = C.c_int(-7)
    st = _lib.lib().mrgfe_loop_detect(det._h, len(kfs), det._records(kfs), len(news), det._records(news), len(edges), ek, out, cap, C.byref(n))
    return st, n.value, out


def test_edge_cases_leave_the_state_alone():
    kfs, news, table = _random_session(np.random.default_rng(1001))
    aligner = TableAligner(table, kfs + news)
    hip = HipLoopDetector(PRM, aligner=aligner)
    # empty lists: MRGFE_OK, no loops, the aligner is never asked
    assert hip.detect(kfs, []) == [] and hip.detect([], news) == [] and hip.detect([], []) == []
    assert aligner.calls == [] and hip.last_batched is None and hip.loop_candidates_sizes == []
    assert hip.stats() == {"superset_pairs": 0, "sequential_pairs": 0, "consistency_pairs": 0, "new_keyframes": 0, "target_builds": 0}
    # a first run that finds loops
    first = hip.detect(kfs, news[:8])
    assert len(first) >= 1
    state = (hip.loop_manager_entries(), hip.loop_candidates_sizes, hip.loop_detection_times, hip.stats())
    n_calls = len(aligner.calls)

    # an unknown prev_key
    rec = hip._records(kfs)
    rec[5].prev_key = 0x1234567
    n = C.c_int(0)
    out = (_lib.LoopResult * 8)()
    st = _lib.lib().mrgfe_loop_detect(hip._h, len(kfs), rec, 8, hip._records(news[8:16]), 0, None, out, 8, C.byref(n))
    assert st == _lib.ERR_INVALID and "neither list" in _lib.last_error() and str(0x1234567) in _lib.last_error() and n.value == 0
    # key 0, in either list
    rec = hip._records(kfs)
    rec[3].key = 0
    assert _lib.lib().mrgfe_loop_detect(hip._h, len(kfs), rec, 8, hip._records(news[8:16]), 0, None, out, 8, C.byref(n)) == _lib.ERR_INVALID and "key 0" in _lib.last_error()
    rec = hip._records(news[8:16])
    rec[0].key = 0
    assert _lib.lib().mrgfe_loop_detect(hip._h, len(kfs), hip._records(kfs), 8, rec, 0, None, out, 8, C.byref(n)) == _lib.ERR_INVALID and "key 0" in _lib.last_error()
    assert len(aligner.calls) == n_calls  # refused before anything was queued
    # capacity too small: the call says how many loops there are and changes nothing
    probe = HipLoopDetector(PRM, aligner=TableAligner(table, kfs + news))
    probe.detect(kfs, news[:8])
    expect = probe.detect(kfs, news[8:16])
    want = len(expect)
    assert want >= 1
    st, got, _ = _raw(hip, kfs, news[8:16], capacity=want - 1)
    assert st == _lib.ERR_INVALID and got == want and "room for" in _lib.last_error()
    # a failing aligner
    aligner.fail = True
    with pytest.raises(_lib.MrgfeError, match="aligner of stage 1"):
        hip.detect(kfs, news[8:16])
    aligner.fail = False
    assert (hip.loop_manager_entries(), hip.loop_candidates_sizes, hip.loop_detection_times, hip.stats()) == state
    # ... and the next good call gives what it would have given without the failed ones
    again = hip.detect(kfs, news[8:16])
    assert [(lp.key1.id, lp.key2.id) for lp in again] == [(lp.key1.id, lp.key2.id) for lp in expect]
    assert hip.loop_manager_entries() == probe.loop_manager_entries() and hip.loop_candidates_sizes == probe.loop_candidates_sizes
    # reset forgets the loops and the counters: the first call gives the first result again
    hip.reset()
    assert hip.loop_manager_entries() == [] and hip.loop_candidates_sizes == [] and hip.stats()["superset_pairs"] == 0
    assert [(lp.key1.id, lp.key2.id) for lp in hip.detect(kfs, news[:8])] == [(lp.key1.id, lp.key2.id) for lp in first]


def test_a_failing_second_stage_leaves_the_state_alone():
    kfs, news, table = _random_session(np.random.default_rng(1002))
    inner = TableAligner(table, kfs + news)

    def aligner(stage, tk, pt, sk, g, wf):
        if stage == 2 and aligner.fail:
            raise RuntimeError("scripted failure")
        return inner(stage, tk, pt, sk, g, wf)

    aligner.fail = False
    hip = HipLoopDetector(PRM, aligner=aligner)
    hip.detect(kfs, news[:5])
    state = (hip.loop_manager_entries(), hip.loop_candidates_sizes, hip.stats())
    aligner.fail = True
    with pytest.raises(_lib.MrgfeError, match="aligner of stage 2"):
        hip.detect(kfs, news[5:10])
    assert (hip.loop_manager_entries(), hip.loop_candidates_sizes, hip.stats()) == state


def test_create_refuses_bad_arguments_and_a_detector_without_an_aligner_refuses_to_detect():
    L = _lib.lib()
    p = _lib.LoopParams()
    L.mrgfe_loop_default_params(C.byref(p))
    from mrg_slam_amd.loop_detector import DEFAULTS

    assert (p.candidate_max_xy_distance, p.accum_distance_thresh_same_robot, p.accum_distance_thresh_other_robot, p.fitness_score_thresh) == tuple(
        DEFAULTS[k] for k in ("candidate_max_xy_distance", "accum_distance_thresh_same_robot", "accum_distance_thresh_other_robot", "fitness_score_thresh"))
    assert p.fitness_score_max_range == float("inf") and p.fitness_selection == 0 and p.use_planar_registration_guess == 0 and p.enable_loop_closure_consistency_check == 1
    assert (p.loop_closure_consistency_max_delta_trans, p.loop_closure_consistency_max_delta_angle) == (DEFAULTS["loop_closure_consistency_max_delta_trans"], DEFAULTS["loop_closure_consistency_max_delta_angle"])
    assert (L.mrgfe_loop_params_size(), L.mrgfe_loop_keyframe_size(), L.mrgfe_loop_result_size()) == (C.sizeof(_lib.LoopParams), C.sizeof(_lib.LoopKeyframe), C.sizeof(_lib.LoopResult)) == (72, 432, 88)
    h = C.c_void_p()
    p.fitness_selection = 2
    assert L.mrgfe_loop_create(None, None, C.byref(p), C.byref(h)) == _lib.ERR_INVALID and not h.value
    p.fitness_selection = 0
    assert L.mrgfe_loop_create(None, None, None, C.byref(h)) == _lib.ERR_INVALID
    assert L.mrgfe_loop_create(None, None, C.byref(p), C.byref(h)) == _lib.MRGFE_OK and h.value
    kfs, news, _ = _random_session(np.random.default_rng(7), n_known=12, n_new=2)
    det = HipLoopDetector.__new__(HipLoopDetector)
    det._h, det._slam_ids = h, {}
    st, n, _ = _raw(det, kfs, news)
    assert st == _lib.ERR_STATE and n == 0 and "aligner" in _lib.last_error()
    det.close()


def _random_pose(rng, scale):
    R = synth.rot_xyz(*rng.uniform(-np.pi, np.pi, size=3))
    return synth.make_pose(rng.uniform(-50, 50, size=3), R * scale)


def test_guess_and_normalize_estimate_follow_the_mirror():
    """200 random poses (rotations all over SO(3), slightly denormalised like an optimiser's output).  normalize_estimate is held to 16 eps per entry:
    the two differ in the order the quaternion's four squares are added for its norm alone (numpy's norm against one left-to-right sum), at most 1.5 eps relative
    on the sum, under 2 eps on every normalised component after the square root and the division; a rotation entry is a sum of two products of two components,
    each at most 1 in size and off by at most 4 eps plus its own rounding, so at most 10 eps — 16 eps leaves room for nothing but that.  The float guess: equal to
    within 1 ulp per entry, exactly equal for at least 95 % of the entries — the mirror inverts with LAPACK where the library forms the rigid inverse, a
    difference of a few double ulp that moves a float rounding only when the double value lies that close to a float tie."""
    rng = np.random.default_rng(20240)
    mirror = LoopDetector(registration=object())
    planar = LoopDetector({"use_planar_registration_guess": True}, registration=object())
    exact = total = 0
    for i in range(200):
        new, cand = _random_pose(rng, 1.0 + rng.uniform(-1e-6, 1e-6)), _random_pose(rng, 1.0 + rng.uniform(-1e-6, 1e-6))
        nn, nl = normalize_estimate(new), lib_normalize_estimate(new)
        assert np.abs(nn - nl).max() <= 16 * np.finfo(np.float64).eps and (nn[:, 3] == nl[:, 3]).all() and (nl[3] == [0, 0, 0, 1]).all()
        class K:  # noqa: E306  (the slice of KeyFrame _guess reads)
            estimate = cand
        for det, pl in ((mirror, False), (planar, True)):
            gm, gl = det._guess(nn, K), lib_guess(nn, cand, pl)
            assert gl.dtype == np.float32
            ulp = np.spacing(np.abs(gm).astype(np.float32))
            assert (np.abs(gm.astype(np.float64) - gl.astype(np.float64)) <= ulp).all(), (i, gm, gl)
            exact += int((gm == gl).sum())
            total += 16
            if pl:
                assert gl[2, 3] == 0.0
    assert exact >= 0.95 * total, (exact, total)
