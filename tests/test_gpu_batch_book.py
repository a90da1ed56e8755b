"""GPU: the pair list of a batch (targets, pairs, guesses) for every method family a batch serves — NDT_HIP, GICP_HIP, VGICP_HIP and ICP_HIP.  What the
list promises and no other suite pins: a guess set after an align is read by the next one, a refused add or set_guess leaves the list as it was, host
and device adds give the same records, a cleared batch starts over, and the engine statistics of a batch without an NDT engine are zero by rule.
Two targets and four pairs per method, one of them with an empty source; records are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

from conftest import small_cloud
from icp_cases import batch_workload, icp_params

pytestmark = pytest.mark.gpu

INF = float("inf")
METHODS = ["NDT_HIP", "GICP_HIP", "VGICP_HIP", "ICP_HIP", "ICP_HIP_reciprocal"]
EMPTY = np.zeros((0, 4), np.float32)


def _params(name):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    if name.startswith("ICP_HIP"):
        return icp_params(name.endswith("reciprocal"))
    p = default_params(getattr(_lib, name))
    p.transformation_epsilon = 0.01
    return p


def _workload(name):
    """(targets, [(target index, source, guess)]): three healthy pairs over two targets and one empty source"""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    if name.startswith("ICP_HIP"):
        targets, pairs = batch_workload()
        pairs = pairs[:3]
    else:
        targets = [small_cloud(3000, 700), small_cloud(2500, 701)]
        rng = np.random.default_rng(71)
        pairs = []
        for k, n in enumerate((2049, 2500, 2817)):  # ragged last blocks, block counts that differ
            ti = k % 2
            rel = synth.make_pose(rng.normal(0, 0.15, 3), synth.rot_xyz(*rng.normal(0, 0.015, 3)))
            pairs.append((ti, orc.transform_points(np.linalg.inv(rel), targets[ti][:n]), synth.perturb_pose(np.eye(4), rng)))
    return targets, pairs[:2] + [(1, EMPTY, pairs[0][2])] + pairs[2:]


def _fill(bm, targets, pairs):
    tids = [bm.add_target(t) for t in targets]
    for ti, src, guess in pairs:
        bm.add_pair(tids[ti], src, guess)


def _fresh(name, targets, pairs):
    from mrg_slam_amd import BatchMatcher

    bm = BatchMatcher(_params(name))
    _fill(bm, targets, pairs)
    return bm, bm.align(INF)


def _num_pairs(bm):
    from mrg_slam_amd._lib import lib

    return lib().mrgfe_batch_num_pairs(bm._h)


def _same(got, want):
    assert len(got) == len(want)
    for f in want.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    assert got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def base():
    """per method: (targets, pairs, matcher, records of its first align) — computed once, the matcher is read only by the statistics test"""
    out = {}
    for name in METHODS:
        targets, pairs = _workload(name)
        out[name] = (targets, pairs) + _fresh(name, targets, pairs)
    return out


@pytest.mark.parametrize("name", METHODS)
def test_set_guess_is_read_at_align_time(base, name):
    from mrg_slam_amd import synth

    targets, pairs, _, first = base[name]
    bm, got = _fresh(name, targets, pairs)
    _same(got, first)
    other = synth.perturb_pose(np.eye(4), np.random.default_rng(72))
    bm.set_guess(1, other)
    moved = list(pairs)
    moved[1] = (pairs[1][0], pairs[1][1], other)
    _, want = _fresh(name, targets, moved)
    got = bm.align(INF)
    _same(got, want)
    assert got[1]["T"].tobytes() != first[1]["T"].tobytes()  # the new guess was used ...
    for k in (0, 2, 3):
        assert got[k].tobytes() == first[k].tobytes(), k  # ... by its pair alone


@pytest.mark.parametrize("name", METHODS)
def test_pair_list_errors_leave_the_batch_usable(base, name):
    import torch

    from mrg_slam_amd import BatchMatcher, MrgfeError
    from mrg_slam_amd._lib import ERR_INVALID

    targets, pairs, _, first = base[name]
    bm = BatchMatcher(_params(name))
    _fill(bm, targets, pairs)
    n_t, n_p = len(targets), len(pairs)
    src, eye = pairs[0][1], np.eye(4)
    d_src = torch.from_numpy(src).cuda(0)
    torch.cuda.synchronize()
    bad = [
        (lambda: bm.add_pair(-1, src, eye), "add_pair: target index -1 out of range"),
        (lambda: bm.add_pair(n_t, src, eye), f"add_pair: target index {n_t} out of range"),
        (lambda: bm.add_pair_device(-1, d_src.data_ptr(), len(src), eye), "add_pair: target index -1 out of range"),
        (lambda: bm.set_guess(n_p, eye), f"set_guess: pair index {n_p} out of range"),
        (lambda: bm.add_pair_device(0, 0, 5, eye), "add_pair: NULL cloud"),
        (lambda: bm.add_target_device(0, 5), "add_target: NULL cloud"),
    ]
    for call, text in bad:
        with pytest.raises(MrgfeError) as e:
            call()
        assert e.value.status == ERR_INVALID and str(e.value) == f"libmrgfe error {ERR_INVALID}: {text}"
        assert _num_pairs(bm) == n_p
    _same(bm.align(INF), first)


@pytest.mark.parametrize("name", METHODS)
def test_host_and_device_adds_mix(base, name):
    import torch

    from mrg_slam_amd import BatchMatcher

    targets, pairs, _, first = base[name]
    d_targets = [torch.from_numpy(t).cuda(0) for t in targets]
    d_sources = [torch.from_numpy(s).cuda(0) for _, s, _ in pairs]
    torch.cuda.synchronize()
    bm = BatchMatcher(_params(name))
    # target 0 and the even pairs from host memory, target 1 and the odd pairs from the memory uploaded above
    tids = [bm.add_target(targets[0]), bm.add_target_device(d_targets[1].data_ptr(), len(targets[1]))]
    for k, (ti, src, guess) in enumerate(pairs):
        if k % 2 == 0:
            bm.add_pair(tids[ti], src, guess)
        else:
            bm.add_pair_device(tids[ti], d_sources[k].data_ptr(), len(src), guess)
    _same(bm.align(INF), first)
    dev = BatchMatcher(_params(name))
    tids = [dev.add_target_device(d.data_ptr(), len(t)) for d, t in zip(d_targets, targets)]
    for (ti, src, guess), d in zip(pairs, d_sources):
        dev.add_pair_device(tids[ti], d.data_ptr(), len(src), guess)
    _same(dev.align(INF), first)


@pytest.mark.parametrize("name", METHODS)
def test_clear_and_refill(base, name):
    targets, pairs, _, first = base[name]
    bm, got = _fresh(name, targets, pairs)
    _same(got, first)
    bm.clear()
    assert _num_pairs(bm) == 0
    _fill(bm, targets, pairs)
    _same(bm.align(INF), first)
    # a different, smaller list on the same matcher: one target (the former second one), two pairs
    smaller = [(0, pairs[1][1], pairs[3][2]), (0, pairs[1][1][:1000], pairs[1][2])]
    bm.clear()
    _fill(bm, targets[1:], smaller)
    assert _num_pairs(bm) == 2
    _, want = _fresh(name, targets[1:], smaller)
    _same(bm.align(INF), want)


@pytest.mark.parametrize("name", METHODS)
def test_engine_statistics_without_an_ndt_engine(base, name):
    _, _, bm, first = base[name]
    if name == "NDT_HIP":
        ms, launches, nbytes = bm.kernel_stats()
        assert ms > 0 and launches > 0 and nbytes > 0
        big_ms, busy = bm.largest_launch()
        assert big_ms > 0 and sum(busy) > 0
        pts, nbrs = bm.pair_counts()
        assert pts > 0 and nbrs > 0
        assert bm.rounds() > 0
        return
    for mode in (-1, 0, 1, 2):
        assert bm.kernel_stats(mode) == (0.0, 0, 0.0)
        assert bm.pair_counts(mode) == (0.0, 0.0)
    assert bm.largest_launch() == (0.0, [0, 0, 0])
    if name.startswith("ICP_HIP"):
        assert bm.rounds() == int(first["evaluations"].max()) > 1  # a pair's evaluations are the rounds it was busy in
    else:
        assert bm.rounds() == 0
