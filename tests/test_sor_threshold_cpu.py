"""CPU: StatisticalOutlierRemoval's threshold as one host/device source (csrc/sor_threshold.h), host build — the reference's sequential f64 sums, the
mean / variance / threshold tail, and the certificate that lets the device add the same terms in a tree (mrgfe_dbg_sor_threshold, on_device = 0, no
context)."""
import numpy as np

from sor_cases import bits, edge_arrays, ordinary_arrays, other_orders, reference, refused_arrays, sequential, sor_threshold, terms


def _assert_reference(name, dist, valid, mul, got):
    s, sq, nv, thr = reference(dist, valid, mul)
    assert bits(got["sum"]) == bits(s), name
    assert bits(got["sq_sum"]) == bits(sq), name
    assert got["valid"] == nv, name
    assert bits(got["thr"]) == bits(thr), (name, got["thr"], thr)


def _assert_order_free(name, dist, rng):
    """every other order of addition gives the sequential bits, for the distances and for their squares"""
    for t in terms(dist):
        want = bits(sequential(t))
        for k, other in enumerate(other_orders(t, rng)):
            assert bits(other) == want, (name, k)


def test_sums_and_threshold_equal_the_reference_loop():
    for name, d, v, mul in ordinary_arrays():
        _assert_reference(name, d, v, mul, sor_threshold(d, v, mul))
    for name, d, v, mul, _ in refused_arrays():
        _assert_reference(name, d, v, mul, sor_threshold(d, v, mul))


def test_certified_sums_do_not_depend_on_the_order():
    rng = np.random.default_rng(3)
    cases = ordinary_arrays()
    certified = 0
    for name, d, v, mul in cases:
        got = sor_threshold(d, v, mul)
        if got["certified"] == 1.0:
            certified += 1
            _assert_order_free(name, d, rng)
    # the test must not pass by refusing everything: uniform [0.02, 3] floats have their lowest set bit at 2^-29 or above (squares: 2^-35), so the bounds
    # are 2^23 and 2^17 where the sums of 30 000 terms stay below 9e4 < 2^17 and about 9.1e4 < 2^17
    assert certified >= 0.9 * len(cases), (certified, len(cases))


def test_order_dependent_sums_are_refused():
    rng = np.random.default_rng(4)
    for name, d, v, mul, expect in refused_arrays():
        got = sor_threshold(d, v, mul)
        if expect is not None:
            assert got["certified"] == float(expect), (name, got)
        if got["certified"] == 1.0:  # whatever the flag says, a 1 implies equality
            _assert_order_free(name, d, rng)
    # q of the `sum` terms: 2^-100 is the lowest set bit
    name, d, v, mul, _ = [c for c in refused_arrays() if c[0].startswith("2^-100 and 8193")][0]
    assert sor_threshold(d, v, mul)["q"] == -100.0, name
    # a negative or a non-finite term is never certified
    for bad in (-0.5, np.inf, np.nan):
        d = np.array([0.5, bad, 0.25], np.float32)
        assert sor_threshold(d, np.ones(3, np.uint32), 1.0)["certified"] == 0.0, bad


def test_edge_values_give_what_the_host_formula_gives():
    for name, d, v, mul in edge_arrays():
        got = sor_threshold(d, v, mul)
        _assert_reference(name, d, v, mul, got)
        assert got["certified"] == 1.0, name  # (few ordinary terms, or none)
    by_name = {c[0]: sor_threshold(*c[1:]) for c in edge_arrays()}
    assert np.isnan(by_name["n = 0"]["thr"]) and np.isnan(by_name["all zeros, none valid"]["thr"])  # 0 / 0
    assert not np.isfinite(by_name["valid = 0"]["thr"])  # sum / 0
    assert by_name["all zeros"]["thr"] == 0.0
    assert not np.isfinite(by_name["valid = 1"]["thr"]) and not np.isfinite(by_name["one point"]["thr"])  # a division by valid - 1 = 0
    assert by_name["n = 0"]["q"] == 2147483647.0  # no non-zero term
