"""Shared by tests/test_sor_threshold_cpu.py and tests/test_gpu_prefilter_statistical.py: the arrays StatisticalOutlierRemoval's threshold is held on,
a numpy restatement of the reference's loop, and the binding of mrgfe_dbg_sor_threshold."""
import ctypes as C

import numpy as np

KEYS = ("sum", "sq_sum", "valid", "thr", "certified", "q")


def sor_threshold(dist, valid, mul, on_device=0, ctx=None):
    """mrgfe_dbg_sor_threshold -> dict of its six outputs."""
    from mrg_slam_amd import _lib

    dist = np.ascontiguousarray(dist, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.uint32)
    assert dist.shape == valid.shape and dist.ndim == 1
    out = (C.c_double * 6)()
    _lib.check(_lib.lib().mrgfe_dbg_sor_threshold(ctx._h if ctx is not None else None, dist.ctypes.data_as(C.POINTER(C.c_float)), valid.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 len(dist), float(mul), int(on_device), out))
    return dict(zip(KEYS, [float(v) for v in out]))


def bits(x):
    """The bit pattern of a double; every NaN is one pattern (two NaNs count as equal)."""
    x = np.float64(x)
    return "nan" if np.isnan(x) else int(x.view(np.uint64))


def terms(dist):
    """The f64 terms of the two sums: dist_i and float(dist_i * dist_i)."""
    d = np.ascontiguousarray(dist, dtype=np.float32)
    with np.errstate(all="ignore"):
        return d.astype(np.float64), (d * d).astype(np.float64)


def sequential(t):
    """The reference's order: np.cumsum over f64 adds one element after the other."""
    return np.float64(np.cumsum(t)[-1]) if len(t) else np.float64(0.0)


def reference(dist, valid, mul):
    """pcl::StatisticalOutlierRemoval's sums and threshold restated: sum, sq_sum, valid, thr."""
    t, t2 = terms(dist)
    s, sq = sequential(t), sequential(t2)
    nv = np.float64(int(np.asarray(valid, dtype=np.uint64).sum()))
    with np.errstate(all="ignore"):
        mean = s / nv
        variance = (sq - s * s / nv) / (nv - np.float64(1.0))
        thr = mean + np.float64(mul) * np.sqrt(variance)
    return s, sq, nv, thr


def other_orders(t, rng):
    """Sums of the same terms in other orders: numpy's pairwise tree, reversed, five random permutations."""
    if not len(t):
        return [np.float64(0.0)]
    return [np.float64(np.sum(t)), sequential(t[::-1])] + [sequential(t[rng.permutation(len(t))]) for _ in range(5)]


def ordinary_arrays(count=24, seed=20261020):
    """Random arrays of 1 .. 30 000 floats in [0.02, 3] with zeros and invalid entries mixed in: (name, dist, valid, mul)."""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4097, 30000] + [int(v) for v in rng.integers(1, 30001, count - 11)]
    out = []
    for k, n in enumerate(sizes):
        d = rng.uniform(0.02, 3.0, n).astype(np.float32)
        v = np.ones(n, dtype=np.uint32)
        if n > 4:
            bad = rng.choice(n, max(1, n // 40), replace=False)  # queries that did not find all their neighbours: distance 0, not counted
            d[bad] = 0.0
            v[bad] = 0
            v[rng.choice(n, max(1, n // 100), replace=False)] = 0  # and invalid entries that still carry a distance (the loop adds it all the same)
            d[rng.choice(n, max(1, n // 60), replace=False)] = 0.0
        out.append((f"ordinary {k}: n={n}", d, v, float(rng.choice([0.5, 1.0, 1.2, 2.0]))))
    return out


def refused_arrays(seed=7):
    """Arrays whose sums may depend on the order: (name, dist, valid, mul, expect) with expect = 0 / 1 the certificate's answer, None where it is not fixed."""
    rng = np.random.default_rng(seed)
    out = []
    d = rng.uniform(0.05, 2.0, 20001).astype(np.float32)
    d[11111] = np.float32(1.3e-12)  # lowest set bit near 2^-63: the sum would have to stay below 2^-11
    out.append(("one 1.3e-12 term among 20 000 ordinary ones", d, np.ones(len(d), np.uint32), 1.0, 0))
    # One term 2^-100 (its float square underflows to zero: no term of sq_sum) and m terms 2^-60 (squares 2^-120): q = -100, the bound on the sum is 2^-48
    # = 4096 * 2^-60; the squares' bound 2^-68 is far away.  m = 4095 lies below the bound (certified, and equal in every order), 4096 and 8191 lie at
    # or above it (refused although still exact: the bound is one bit tighter than needed), 8193 and 20000 cross 2^(q + 53) = 2^-47: the sum cannot hold every term.
    for m, expect in ((4095, 1), (4096, 0), (8191, 0), (8193, 0), (20000, 0)):
        d = np.full(m + 1, np.float32(2.0 ** -60), dtype=np.float32)
        d[m // 3] = np.float32(2.0 ** -100)
        out.append((f"2^-100 and {m} x 2^-60", d, np.ones(m + 1, np.uint32), 1.0, expect))
    return out


def edge_arrays():
    z = np.zeros(100, np.float32)
    one = np.array([0.7], np.float32)
    some = np.linspace(0.1, 2.0, 50).astype(np.float32)
    v1 = np.zeros(50, np.uint32)
    v1[17] = 1
    return [("n = 0", np.zeros(0, np.float32), np.zeros(0, np.uint32), 1.0), ("all zeros", z, np.ones(100, np.uint32), 1.0), ("valid = 0", some, np.zeros(50, np.uint32), 1.0),
            ("valid = 1", some, v1, 1.0), ("one point", one, np.ones(1, np.uint32), 2.0), ("all zeros, none valid", z, np.zeros(100, np.uint32), 0.5)]
