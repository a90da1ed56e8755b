"""GPU: mrgfe_batch_clear_pairs — forget the pairs, keep the targets and everything built for them.  Two targets and five pairs are aligned, the pairs are
cleared, three OTHER pairs follow of which none names target 0: the records equal, byte for byte, those of a fresh batch holding the same two targets and
those three pairs — through align, align_best and align_async, for every batch method (a pair's sums depend on its own points and the round plan the PAIR list makes, DESIGN.md §9;
the target no pair names enters no launch and no NDT round plan)."""
import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu

METHODS = ["NDT_HIP", "PCL_NDT_HIP", "GICP_HIP", "SMALL_GICP_HIP", "VGICP_HIP", "ICP_HIP"]


@pytest.fixture(scope="module")
def case():
    """targets, the five pairs of the first align and the three of the second (target index, source, guess); computed once, left unchanged"""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    targets = [small_cloud(3000, 310), small_cloud(2900, 311)]
    rng = np.random.default_rng(31)

    def pair(ti, n):
        rel = synth.make_pose(rng.normal(0, 0.15, 3), synth.rot_xyz(*rng.normal(0, 0.015, 3)))
        return ti, orc.transform_points(np.linalg.inv(rel), targets[ti][:n]), synth.perturb_pose(np.eye(4), rng)

    first = [pair(k % 2, 2300 + 130 * k) for k in range(5)]
    second = [pair(1, 2450), pair(1, 2877), pair(1, 2001)]  # target 0 stays unused
    for c in targets + [p[1] for p in first + second]:
        c.setflags(write=False)
    return targets, first, second


def _matcher(method):
    from mrg_slam_amd import BatchMatcher, _lib
    from mrg_slam_amd.registration import default_params

    prm = default_params(getattr(_lib, method))
    prm.transformation_epsilon = 0.01
    return BatchMatcher(prm)


def _queue(bm, pairs, tids):
    for ti, src, guess in pairs:
        bm.add_pair(tids[ti], src, guess)


def _align(bm, how, n):
    if how == "align":
        return bm.align(float("inf"))
    if how == "align_async":
        bm.align_async(float("inf"))
        return bm.wait()
    group = np.zeros(n, dtype=np.int32)  # one group: the bounded selection prunes what cannot be the best
    rec, state, best, best_score = bm.align_best(float("inf"), group, score_cap=None)
    return rec, state, best, best_score


@pytest.mark.parametrize("how", ["align", "align_best", "align_async"])
@pytest.mark.parametrize("method", METHODS)
def test_pairs_after_clear_pairs_equal_a_fresh_batch(case, method, how):
    targets, first, second = case
    bm = _matcher(method)
    tids = [bm.add_target(t) for t in targets]
    _queue(bm, first, tids)
    _align(bm, how, len(first))
    rounds_before = bm.ndt_rounds() if "NDT" in method else None
    bm.clear_pairs()
    _queue(bm, second, tids)
    got = _align(bm, how, len(second))

    fresh = _matcher(method)
    ftids = [fresh.add_target(t) for t in targets]
    _queue(fresh, second, ftids)
    want = _align(fresh, how, len(second))
    if how == "align_best":
        for a, b in zip(got[1:], want[1:]):
            np.testing.assert_array_equal(a, b)
        got, want = got[0], want[0]
    assert len(got) == len(second) and got.tobytes() == want.tobytes()
    assert (got["converged"] == 1).any() and list(got["pair_id"]) == [0, 1, 2]
    if "NDT" in method:  # the round plan is that of the three pairs alone: the unused target and the forgotten pairs left no trace in it
        a, b = bm.ndt_rounds(), fresh.ndt_rounds()
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert a[0].sum() > 0 and a[0].max() <= len(second) < rounds_before[0].max()  # (never more than three pairs in a round; the first align had five)


def test_clear_pairs_on_an_empty_batch_and_an_out_of_range_target(case):
    from mrg_slam_amd import _lib

    targets, first, _ = case
    bm = _matcher("NDT_HIP")
    assert _lib.lib().mrgfe_batch_clear_pairs(bm._h) == _lib.MRGFE_OK  # nothing queued yet
    assert _lib.lib().mrgfe_batch_clear_pairs(None) == _lib.ERR_INVALID
    t0 = bm.add_target(targets[0])
    bm.add_pair(t0, first[0][1], first[0][2])
    bm.clear_pairs()
    assert _lib.lib().mrgfe_batch_num_pairs(bm._h) == 0
    with pytest.raises(_lib.MrgfeError, match="out of range"):
        bm.add_pair(t0 + 1, first[0][1], first[0][2])  # one target is kept: index 1 does not exist
    with pytest.raises(_lib.MrgfeError, match="out of range"):
        bm.add_pair(-1, first[0][1], first[0][2])
    assert len(bm.align(float("inf"))) == 0  # an empty pair list over a kept target aligns nothing
    bm.add_pair(t0, first[0][1], first[0][2])
    assert len(bm.align(float("inf"))) == 1
    bm.clear()  # a full clear forgets the target too
    with pytest.raises(_lib.MrgfeError, match="out of range"):
        bm.add_pair(t0, first[0][1], first[0][2])
