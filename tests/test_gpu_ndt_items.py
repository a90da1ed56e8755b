"""GPU: the NDT derivative kernels' multi-tile work items, the reduction's unrolled loops and the round plan's tiles-per-item rule, held to the oracle.

A derivative launch cuts a pair into items of `ppt` 256-point tiles (csrc/ndt_derivatives.hip ndt_derivatives_item / ndt_derivatives_f64_item), ndt_sum_records
adds a pair's item records in a fixed order, and ndt_plan_kernel (device-stepped) and NdtEngine::host_plan (host-stepped) each pick ppt per round and kernel
variant.  On 256 CUs ppt > 1 needs half a million busy source points, so every other test of the suite runs at ppt == 1.  Here the hooks of
include/mrgfe_debug.h force ppt for single evaluations (mrgfe_dbg_ndt_evaluate_ppt), shrink the rule's work-group target so that a seven-pair batch walks
through ppt 8 ... 1 (mrgfe_dbg_set_ndt_round_shape), and report the rounds' pair and item counts (mrgfe_dbg_*_ndt_rounds); the oracle adds the same float terms
in the kernels' order for any ppt (oracle/ndt.cpp gpu_order_ppt) and tests/ndt_items_cases.py replays a batch's rounds from the rule as it is written down.

Every kind is held BIT FOR BIT.  For the float path (kinds 0 and 1) that is the bar of tests/test_gpu_ndt.py::test_evaluation_is_bit_identical_to_the_oracle_in_gpu_order.
For the f64 Hessian pass (kind 2) that test allows 1e-14 of the largest entry, for "the two C libraries' exp"; it holds exactly because nothing in the pass is
left to a library: its terms are IEEE f64 multiplications, additions and explicit fma in one written order on both sides (ndt_derivatives.hip's per-point
factorisation, restated in oracle/ndt.cpp compute_hessian_gpu_order), and its exp is csrc/glibc_exp.h, which tests/test_gpu_primitives.py holds bit for bit
against its host build and tests/test_glibc_exp.py against the C library the oracle calls.  Measured on an MI355X: deviation 0 on every case of this file."""
import numpy as np
import pytest

import ndt_items_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture()
def knobs():
    """process-wide switches, put back whatever the test did"""
    from mrg_slam_amd._lib import lib

    fused = lib().mrgfe_dbg_set_fused_launch(-1)
    try:
        yield lib()
    finally:
        lib().mrgfe_dbg_set_ndt_round_shape(0, 0)
        lib().mrgfe_dbg_set_host_control(-1)
        lib().mrgfe_dbg_set_fused_launch(fused)


def _registrations(monkeypatch, leaf, search, cls=None, **kw):
    """[(lookup, registration)]: the dense voxel lookup and the hashed one (MRGFE_FORCE_HASH is read when the registration is made)"""
    from mrg_slam_amd import NdtHip

    out = []
    for force_hash in ("0", "1"):
        monkeypatch.setenv("MRGFE_FORCE_HASH", force_hash)
        g = (cls or NdtHip)(resolution=leaf, **({"search": search} if cls is None else {}), **kw)
        assert g.setInputTarget(K.target()) == 0
        out.append(("hash" if force_hash == "1" else "dense", g))
    return out


def _assert_equals_oracle(got, want, mode, tag):
    """every bit of what the kind computes: score and gradient (0, 1), Hessian (0, 2)"""
    (sg, gg, Hg), (so, go, Ho) = got, want
    if mode != 2:
        assert K.same_bits([sg], [so]) and K.same_bits(gg, go), (tag, sg, so, np.abs(gg - go).max())
    if mode != 1:
        assert K.same_bits(Hg, Ho), (tag, np.abs(Hg - Ho).max() / max(np.abs(Ho).max(), np.finfo(np.float64).tiny))


# ---- single evaluations at a forced ppt -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", K.LEAVES)
@pytest.mark.parametrize("search", K.SEARCHES)
@pytest.mark.parametrize("ppt", K.PPTS)
def test_evaluation_at_forced_ppt_equals_the_gpu_order_oracle(ppt, search, leaf, monkeypatch):
    """every source size around the item boundaries (ndt_items_cases.sizes), dense and hashed lookup, the three kinds.  Liveness: at two items plus one point
    and at three ragged items the ppt result differs from the ppt = 1 result of the same kernel in at least one f64 bit — and by no more than the
    summation-order bound tests/test_oracle_ndt.py::test_gpu_order_mode_only_reorders_the_sums holds the oracle to (1e-12, f64 pass 1e-11, of max(1, largest))."""
    T, p = K.pose()
    regs = _registrations(monkeypatch, leaf, search)
    reordered = multi = 0
    for n in K.sizes(ppt):
        want = K.oracle_sums(n, search, leaf, ppt)
        if n >= 255:
            assert abs(want[0][0]) > 1e-3  # the source meets occupied voxels: there is something to add up
        for lookup, g in regs:
            g.setInputSource(K.source(n))
            got = {mode: g.evaluate(T, p, mode, ppt=ppt) for mode in (0, 1, 2)}
            for mode in (0, 1, 2):
                _assert_equals_oracle(got[mode], want[mode], mode, (ppt, search, leaf, n, lookup, mode))
            if n > 256 * ppt:
                one = {mode: g.evaluate(T, p, mode, ppt=1) for mode in (0, 1, 2)}
                for mode in (0, 1, 2):
                    (s1, g1, H1), (sk, gk, Hk) = one[mode], got[mode]
                    assert abs(sk - s1) <= 1e-12 * max(1.0, abs(s1))
                    np.testing.assert_allclose(gk, g1, rtol=0, atol=1e-12 * max(1.0, np.abs(g1).max()))
                    np.testing.assert_allclose(Hk, H1, rtol=0, atol=(1e-12 if mode != 2 else 1e-11) * max(1.0, np.abs(H1).max()))
                multi += 1
                reordered += int(any(not (K.same_bits([one[m][0]], [got[m][0]]) and K.same_bits(one[m][1], got[m][1]) and K.same_bits(one[m][2], got[m][2])) for m in (0, 1, 2)))
    print(f"ppt {ppt} {search} leaf {leaf}: {reordered} of {multi} multi-item evaluations differ from ppt = 1 in some bit")
    assert reordered >= 1


@pytest.mark.parametrize("leaf", K.LEAVES)
@pytest.mark.parametrize("ppt", K.PPTS)
def test_pcl_ndt_evaluation_at_forced_ppt_matches_the_gpu_order_oracle(ppt, leaf, monkeypatch):
    """PCL_NDT_HIP's f64 items (ndt_derivatives_f64_item) against orc.PclNdt(gpu_order=ppt): the tolerances of
    tests/test_gpu_pclndt.py::test_single_evaluation_matches_oracle against its GPU-order oracle (score 1e-14 relative, gradient and Hessian 5e-11 of the largest entry)"""
    from mrg_slam_amd import PclNdtHip
    from oracle import oracle as orc

    T, p = K.pose()
    regs = _registrations(monkeypatch, leaf, None, cls=PclNdtHip)
    o = orc.PclNdt(resolution=leaf, gpu_order=ppt, num_threads=8)
    assert o.setInputTarget(K.target()) == 0
    reordered = 0
    for n in K.sizes(ppt):
        o.setInputSource(K.source(n))
        want = {mode: o.evaluate(T, p, mode) for mode in (0, 1, 2)}
        for lookup, g in regs:
            g.setInputSource(K.source(n))
            for mode in (0, 1, 2):
                gs, gg, gH = g.evaluate(T, p, mode, ppt=ppt)
                ts, tg, tH = want[mode]
                if mode != 2:
                    assert n < 255 or abs(gs) > 1e-3
                    assert gs == pytest.approx(ts, rel=1e-14), (n, lookup, mode)
                    np.testing.assert_allclose(gg, tg, rtol=0, atol=5e-11 * np.abs(tg).max())
                if mode != 1:
                    np.testing.assert_allclose(gH, tH, rtol=0, atol=5e-11 * np.abs(tH).max())
                    np.testing.assert_array_equal(gH, gH.T)
                if n > 256 * ppt and mode == 0:
                    s1, g1, H1 = g.evaluate(T, p, 0, ppt=1)
                    assert abs(gs - s1) <= 1e-12 * max(1.0, abs(s1))
                    np.testing.assert_allclose(gH, H1, rtol=0, atol=1e-12 * max(1.0, np.abs(H1).max()))
                    reordered += int(not (K.same_bits([gs], [s1]) and K.same_bits(gg, g1) and K.same_bits(gH, H1)))
    assert reordered >= 1


# ---- first principles at ppt > 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True], ids=["origin", "shifted"])
@pytest.mark.parametrize("search", ["DIRECT7", "KDTREE"])
@pytest.mark.parametrize("res", [0.5, 0.37])
def test_multi_tile_items_match_the_first_principles_model(res, search, shifted):
    """tests/ndt_analytic.py in longdouble (ndt_model_cases.check_derivatives, its tolerances unchanged) against a 1300-point source — six tiles — cut into items
    of 2, 3 and 8 tiles: an item that started at the wrong point or dropped its ragged last tile would lose or repeat a sixth of the sums"""
    import ndt_model_cases
    from mrg_slam_amd import NdtHip

    evaluate = [lambda reg, T, p, mode, ppt=ppt: reg.evaluate(T, p, mode, ppt=ppt) for ppt in (2, 3, 8)]
    ndt_model_cases.check_derivatives(NdtHip(resolution=res, search=search), res, search, shifted, n_src=1300, evaluate=evaluate)


# ---- the reduction's unrolled loops ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppt,records", [(ppt, k) for ppt, ks in K.REDUCE_RECORDS.items() for k in ks])
def test_reduction_loop_boundaries(ppt, records):
    """ndt_sum_records adds a pair's records in four slices, 32 loads at a time from 125 records on and eight at a time from 29 on: record counts on both
    sides of each start, and two that mix all three loops, DIRECT7, kinds 0 and 2, against the GPU-order oracle"""
    from mrg_slam_amd import NdtHip

    n = 256 * ppt * records - 100
    assert -(-K.tiles_of(n) // ppt) == records and n < 100000
    T, p = K.pose()
    g = NdtHip(search="DIRECT7")
    assert g.setInputTarget(K.target()) == 0
    g.setInputSource(K.source(n))
    want = K.oracle_sums(n, "DIRECT7", 1.0, ppt, modes=(0, 2))
    assert abs(want[0][0]) > 1.0
    for mode in (0, 2):
        _assert_equals_oracle(g.evaluate(T, p, mode, ppt=ppt), want[mode], mode, (ppt, records, mode))


# ---- whole alignments at a forced ppt ----------------------------------------------------------------------------------------------------
def _align_case(n):
    from mrg_slam_amd import synth

    return K.source(n), synth.perturb_pose(K.relative_pose(), np.random.default_rng(n))


_drive_cache = {}


def _driven(n, ppt):
    from oracle import oracle as orc
    from oracle.replay import drive

    if (n, ppt) not in _drive_cache:
        src, guess = _align_case(n)
        o = orc.Ndt(transformation_epsilon=K.BATCH_EPS, num_threads=8, gpu_order_ppt=ppt)
        o.setInputTarget(K.target())
        o.setInputSource(src)
        T, conv, it, ev, modes = drive(o, K.ndt_params(K.BATCH_EPS), guess, n)
        _drive_cache[(n, ppt)] = ({"T": T, "converged": conv, "iterations": it, "evaluations": ev}, modes)
    return _drive_cache[(n, ppt)]


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("ppt", [2, 3, 8])
def test_alignment_at_forced_ppt_follows_the_gpu_order_replay(ppt, fused, knobs, monkeypatch):
    """NdtHip.align with MRGFE_PPT (read when the source is handed over) against oracle.replay.drive over orc.Ndt(gpu_order_ppt): fused launch on, a single
    registration's round is ndt_derivatives_single_kernel with its ticketed in-kernel sum; off, the items and the separate reduction.  Accepted by the rule of
    tests/test_gpu_soak.py::test_soak_all_methods (ndt_items_cases.agreement); the rounds' item counts are ceil(tiles / ppt)."""
    from mrg_slam_amd import NdtHip

    knobs.mrgfe_dbg_set_fused_launch(fused)
    monkeypatch.setenv("MRGFE_PPT", str(ppt))
    branches = {"exact": 0, "near": 0}
    for n in (1300, 2049, 6000):
        src, guess = _align_case(n)
        g = NdtHip(transformation_epsilon=K.BATCH_EPS)
        assert g.setInputTarget(K.target()) == 0
        g.setInputSource(src)
        g.align(guess)
        got = {"T": g.getFinalTransformation(), "converged": g.hasConverged(), "iterations": g.getFinalNumIteration(), "evaluations": g.evals}
        want, modes = _driven(n, ppt)
        how = K.agreement(got, want, modes)
        assert how is not None, (n, ppt, fused, got, want)
        branches[how] += 1
        n_pairs, n_items = g.ndt_rounds()
        assert len(n_pairs) == len(modes) and want["iterations"] >= 1
        for r, mode in enumerate(modes):
            expect = [0, 0, 0]
            expect[mode] = -(-K.tiles_of(n) // ppt)
            assert list(n_items[r]) == expect and list(n_pairs[r]) == [int(m == mode) for m in range(3)], (n, r)
    print(f"ppt {ppt} fused {fused}: {branches}")


# ---- batches under the natural rule --------------------------------------------------------------------------------------------------------
def _batch(first=0, count=None):
    from mrg_slam_amd import BatchMatcher

    targets, pairs = K.batch_workload()
    bm = BatchMatcher(params=K.ndt_params(K.BATCH_EPS))
    for t in targets:
        bm.add_target(t)
    for ti, src, guess in pairs[first:first + (len(pairs) - first if count is None else count)]:
        bm.add_pair(ti, src, guess)
    return bm


def _hold_to_replay(records, replay, tag):
    """every record against the replay's by the alignment rule; the f64 fields bit for bit wherever the transform is.  Returns the branch counts."""
    branches = {"exact": 0, "near": 0}
    for i, rec in enumerate(records):
        got, want = K.record_of(rec), replay[i]
        how = K.agreement(got, want, want["modes"])
        assert how is not None, (tag, i, got, want)
        branches[how] += 1
        if how == "exact":
            assert K.f64_fields_equal(got, want), (tag, i, np.abs(got["H"] - want["H"]).max(), got["trans_probability"] - want["trans_probability"])
    return branches


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("shape", K.ROUND_SHAPES, ids=lambda s: f"wg{s[0]}-max{s[1]}")
def test_batch_follows_the_lockstep_replay(shape, fused, knobs):
    """seven pairs of 31 to 3000 points under a round shape that takes them through several ppt values (liveness: tests/test_ndt_items_cpu.py, and below),
    device- and host-stepped: records equal the lock-step replay's, per round the busy pairs and the items are the replay's sums of ceil(tiles / ppt) for
    BOTH plan implementations, and the two ways of stepping give the same records bit for bit"""
    replay, schedule = K.batch_replay(*shape)
    values, split = K.schedule_is_live(schedule)
    assert len(values) >= 3 and split >= 1
    want_pairs, want_items = K.schedule_arrays(schedule)
    knobs.mrgfe_dbg_set_fused_launch(fused)
    knobs.mrgfe_dbg_set_ndt_round_shape(*shape)
    out = {}
    for host in (0, 1):
        knobs.mrgfe_dbg_set_host_control(host)
        bm = _batch()
        out[host] = bm.align()
        n_pairs, n_items = bm.ndt_rounds()
        np.testing.assert_array_equal(n_pairs, want_pairs, err_msg=f"host control {host}")
        np.testing.assert_array_equal(n_items, want_items, err_msg=f"host control {host}")
        print(f"shape {shape} fused {fused} host control {host}: {_hold_to_replay(out[host], replay, (shape, fused, host))}, ppt values {values}")
    for field in ("T", "H", "trans_probability", "converged", "iterations", "evaluations"):
        assert K.same_bits(out[0][field], out[1][field]) if out[0][field].dtype == np.float64 else np.array_equal(out[0][field], out[1][field]), field
    # a replay held at one tile per item is NOT what ran
    flat, _ = K.batch_replay(*shape, forced_ppt=1)
    assert any(not K.f64_fields_equal(K.record_of(out[0][i]), flat[i]) for i in range(len(flat)))


# ---- the node split ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 3])
def test_node_members_sum_their_own_tiles(members, knobs):
    """mrgfe_node_align cuts the pair list into one block per member and every member is a batch of its own: its rounds count ITS tiles, so its ppt — and with
    it the last bits of H and trans_probability — are those of the lock-step replay of its own sub-list, not those of one batch over the whole list.
    Transforms, flags and iteration counts agree between node and batch by the alignment rule."""
    from mrg_slam_amd import NodeMatcher

    shape = K.ROUND_SHAPES[0]
    knobs.mrgfe_dbg_set_ndt_round_shape(*shape)
    knobs.mrgfe_dbg_set_host_control(0)
    targets, pairs = K.batch_workload()
    whole = _batch().align()
    node = NodeMatcher([0] * members, params=K.ndt_params(K.BATCH_EPS))
    try:
        for t in targets:
            node.add_target(t)
        for ti, src, guess in pairs:
            node.add_pair(ti, src, guess)
        recs = node.align()
        differ = 0
        for m in range(members):
            first, count = node.shard(m)
            replay, schedule = K.batch_replay(*shape, 0, first, count)
            print(f"{members} members, member {m}: pairs {first}..{first + count - 1}, {_hold_to_replay(recs[first:first + count], replay, (members, m))}")
            n_pairs, n_items = node.ndt_rounds(m)
            want_pairs, want_items = K.schedule_arrays(schedule)
            np.testing.assert_array_equal(n_pairs, want_pairs)
            np.testing.assert_array_equal(n_items, want_items)
    finally:
        node.close()
    whole_replay, _ = K.batch_replay(*shape)
    _hold_to_replay(whole, whole_replay, "one batch")
    for i in range(len(pairs)):
        a, b = K.record_of(recs[i]), K.record_of(whole[i])
        assert K.agreement(a, b, whole_replay[i]["modes"]) is not None, i
        differ += int(not K.same_bits(a["H"], b["H"]))
    print(f"{members} members: H differs from the one-batch record on {differ} of {len(pairs)} pairs")
    assert differ >= 1
