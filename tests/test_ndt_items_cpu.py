"""CPU twin of tests/test_gpu_ndt_items.py: the lock-step replay of tests/ndt_items_cases.py with the GPU-order oracle in both roles.  It shows, without a
GPU, that the replay with one tile per item is oracle.replay.drive pair by pair, and that the round shapes the GPU tests use really walk a small batch
through several tiles-per-item values — so that a GPU test that passes has compared multi-tile items and not the ppt == 1 path once more."""
import numpy as np
import pytest

import ndt_items_cases as K


def test_the_rule_rounds_down_and_clamps():
    """clamp(tiles // wg_target, 1, max_ppt) as the plan states it: 256 CUs * 4 = 1024"""
    assert [K.ppt_rule(t, 1024, 8) for t in (0, 1023, 1024, 2047, 2048, 8191, 8192, 100000)] == [1, 1, 1, 1, 2, 7, 8, 8]
    assert [K.ppt_rule(t, 2, 8) for t in (1, 3, 4, 15, 16, 52)] == [1, 1, 2, 7, 8, 8]
    assert [K.ppt_rule(t, 3, 5) for t in (5, 6, 14, 15, 52)] == [1, 2, 4, 5, 5]


def test_one_tile_per_item_replay_is_drive_pair_by_pair():
    """with a work-group target no batch reaches, every round runs at ppt 1 and a pair's trajectory is the single-pair replay's"""
    from oracle import oracle as orc
    from oracle.replay import drive

    targets, pairs = K.batch_workload()
    records, schedule = K.batch_replay(1 << 20, 8)
    assert all(set(r["ppt"]) <= {0, 1} for r in schedule)
    for i, (ti, src, guess) in enumerate(pairs):
        o = orc.Ndt(num_threads=4, gpu_order_ppt=1)
        o.setInputTarget(targets[ti])
        o.setInputSource(src)
        T, conv, it, ev, modes = drive(o, K.ndt_params(K.BATCH_EPS), guess, len(src))
        r = records[i]
        assert np.array_equal(r["T"], T) and (r["converged"], r["iterations"], r["evaluations"], r["modes"]) == (conv, it, ev, modes), i
    # and the pairs leave in different rounds: the busy list shrinks while others still run
    assert len({len(r["modes"]) for r in records}) >= 3


@pytest.mark.parametrize("shape", K.ROUND_SHAPES, ids=lambda s: f"wg{s[0]}-max{s[1]}")
def test_round_shapes_walk_the_batch_through_the_item_sizes(shape):
    """liveness of the GPU test's batches, on the replay's own schedule: at least three tiles-per-item values occur, some round runs two kernel variants
    at different values, the item counts are the sums of ceil(tiles / ppt), and a replay held at one tile per item does NOT reproduce the f64 fields"""
    _, pairs = K.batch_workload()
    records, schedule = K.batch_replay(*shape)
    values, split = K.schedule_is_live(schedule)
    print(f"shape {shape}: {len(schedule)} rounds, ppt values {values}, {split} rounds with two values")
    assert len(values) >= 3 and max(values) == shape[1] and split >= 1
    for r in schedule:
        assert sum(r["n_pairs"]) >= 1 and all((n == 0) == (p == 0) for n, p in zip(r["n_pairs"], r["ppt"]))
        assert all(n <= i for n, i in zip(r["n_pairs"], r["n_items"]))
    flat, _ = K.batch_replay(*shape, forced_ppt=1)
    differ = [i for i in range(len(pairs)) if not K.f64_fields_equal(records[i], flat[i])]
    print(f"  records whose H / trans_probability differ from the one-tile replay: {differ}")
    assert differ
    # summation order is all that differs: the trajectories end together
    for a, b in zip(records, flat):
        assert K.agreement(a, b, [2]) is not None
        np.testing.assert_allclose(a["H"], b["H"], rtol=0, atol=1e-9 * np.abs(b["H"]).max())


@pytest.mark.parametrize("search,res,shifted", [("DIRECT7", 0.5, False), ("KDTREE", 0.37, True)])
def test_the_oracle_matches_the_model_at_every_item_size(search, res, shifted):
    """the yardstick itself: the GPU-order oracle over a 1300-point source (six tiles) in items of 1, 2, 3 and 8 tiles against tests/ndt_analytic.py in
    longdouble (ndt_model_cases.check_derivatives with its n_src and evaluate parameters, tolerances unchanged)"""
    import ndt_model_cases
    from oracle import oracle as orc

    def at(ppt):
        def evaluate(o, T, p, mode):
            o.set_gpu_order_ppt(ppt)
            return o.evaluate(T, p, mode)
        return evaluate

    ndt_model_cases.check_derivatives(orc.Ndt(resolution=res, search=search, num_threads=2), res, search, shifted, n_src=1300, evaluate=[at(k) for k in (1, 2, 3, 8)])


def test_item_size_moves_only_the_last_bits_of_a_multi_item_sum():
    """what the GPU test's liveness clause stands on: for a source of more than one item the oracle's sums at ppt 2, 3, 8 and 64 differ from those at ppt 1 in
    some bit, and a source of one tile does not notice ppt at all"""
    for ppt in K.PPTS:
        n = 512 * ppt + 1
        a, b = K.oracle_sums(n, "DIRECT7", 1.0, 1), K.oracle_sums(n, "DIRECT7", 1.0, ppt)
        assert any(not (K.same_bits([a[m][0]], [b[m][0]]) and K.same_bits(a[m][1], b[m][1]) and K.same_bits(a[m][2], b[m][2])) for m in (0, 1, 2)), ppt
        for m in (0, 1, 2):
            assert abs(a[m][0] - b[m][0]) <= 1e-12 * max(1.0, abs(a[m][0]))
            np.testing.assert_allclose(b[m][2], a[m][2], rtol=0, atol=(1e-12 if m != 2 else 1e-11) * max(1.0, np.abs(a[m][2]).max()))
        a, b = K.oracle_sums(255, "DIRECT7", 1.0, 1), K.oracle_sums(255, "DIRECT7", 1.0, ppt)
        assert all(K.same_bits([a[m][0]], [b[m][0]]) and K.same_bits(a[m][1], b[m][1]) and K.same_bits(a[m][2], b[m][2]) for m in (0, 1, 2))
