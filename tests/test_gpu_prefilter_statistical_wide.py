"""GPU: STATISTICAL with statistical_mean_k 64..255 on the device-driven prefilter chain, behind the context switch mrgfe_ctx_set_wide_statistical_chains
(csrc/nn_grid.hip nn_knn_mean_dd_wide_kernel<R>: the mean distances out of a list of R = ceil((mean_k + 1) / 64) entries per lane, no neighbour rows).  Off
by default: a fresh context keeps these chains on route 0 (tests/test_gpu_sor_wide.py).  Every output is compared bit for bit on a uint32 view and in order
with the CPU oracle's stage composition, with the same context's host-driven route (mrgfe_dbg_set_prefilter_device_driven(0)) and with the same context with
the switch off.  Route 1 needs the threshold certificate (csrc/sor_threshold.h): it is restated in numpy here and held on the CPU for every case of the
sweep (the one test of this file that needs no GPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_knn_wide import full_sort
from test_gpu_prefilter_statistical_chains import FIELDS, PERIOD, check_counts, non_finite_cloud, oracle_chain, pack, params, same, uniform_cloud

gpu = pytest.mark.gpu

DOCUMENTED_ANOMALIES = 1 | 2 | 4 | 8 | 16 | 32 | 256  # the words mrgfe_ctx_prefilter_stats names (include/mrgfe.h)
NO_TERM, BAD_TERM = 0x7FFFFFFF, -0x7FFFFFFF           # csrc/sor_threshold.h kNoTerm / kBadTerm


@functools.lru_cache(maxsize=None)
def quarter_scan():
    from mrg_slam_amd import synth

    c = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 4711)[::4])
    c.setflags(write=False)
    return c


def vox(**more):
    return params(downsample_method="VOXELGRID", **more)


@pytest.fixture(scope="module")
def ctx():
    """both switches are ON for this module's context; tests that need one off switch it back in a finally"""
    from mrg_slam_amd import Context

    c = Context()
    c.set_statistical_chains(True)
    c.set_wide_statistical_chains(True)
    return c


def three_ways(cloud, p, ctx):
    """prefilter on the device-driven route with the wide switch on, on the host-driven route, and with the wide switch off:
    (fast, its stats, its k-NN stats, slow, its stats, off, its stats)"""
    from mrg_slam_amd import prefilter
    from mrg_slam_amd._lib import lib

    try:
        assert lib().mrgfe_dbg_set_prefilter_device_driven(1) == 1
        fast = prefilter(cloud, p, ctx=ctx)
        fs, ks = ctx.prefilter_stats(), ctx.knn_stats()
        assert lib().mrgfe_dbg_set_prefilter_device_driven(0) == 0
        slow = prefilter(cloud, p, ctx=ctx)
        ss = ctx.prefilter_stats()
        assert lib().mrgfe_dbg_set_prefilter_device_driven(1) == 1
        ctx.set_wide_statistical_chains(False)
        off = prefilter(cloud, p, ctx=ctx)
        os_ = ctx.prefilter_stats()
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)
        ctx.set_wide_statistical_chains(True)
    return fast, fs, ks, slow, ss, off, os_


def exact_three_ways(cloud, p, ctx, what, route=1):
    """fast == slow == switch off == oracle; the fast one on `route` (1: anomaly 0, the oracle's stage counts, the k-NN launch at mean_k + 1)"""
    exp, counts, _, _ = oracle_chain(cloud, p)
    fast, fs, ks, slow, ss, off, os_ = three_ways(cloud, p, ctx)
    print(what, "counts", counts, "stats", fs, "knn", ks)
    same(fast, exp, what)
    same(slow, exp, what + " (host-driven)")
    same(off, exp, what + " (switch off)")
    assert fs["route"] == route and ss["route"] == 0, (what, fs, ss)
    if p["statistical_mean_k"] >= 64:
        assert os_["route"] == 0, (what, os_)
    if route == 1:
        assert fs["anomaly"] == 0 and ks["k"] == p["statistical_mean_k"] + 1, (what, fs, ks)
        check_counts(p, fs, counts, what)
    return exp, counts, fs


# ---- the threshold certificate, restated (csrc/sor_threshold.h) ---------------------------------------------------------------------------------------------
def low_bit_exponent(v):
    """q with 2^q the lowest set bit of each float32 of v; NO_TERM for zeros, BAD_TERM for negative or non-finite values"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    normal = e != 0
    m = np.where(normal, m | 0x800000, m)
    q = np.where(normal, e - 150, -149)
    low = m & -m
    q = q + np.where(m != 0, np.log2(np.maximum(low, 1).astype(np.float64)).astype(np.int64), 0)
    q = np.where((b & 0x7FFFFFFF) == 0, NO_TERM, q)
    return np.where(((b >> 31) != 0) & ((b & 0x7FFFFFFF) != 0) | (e == 0xFF), BAD_TERM, q)


def certified(total, q):
    if q == NO_TERM:
        return True
    if q == BAD_TERM or not total >= 0.0:
        return False
    return total < 2.0 ** (q + 52)


def mean_distances(sqd, k1):
    """what sor_mean_dist_kernel makes of rows of squared distances sorted ascending (-1 beyond the cloud): valid iff entry k1 - 1 exists,
    dist = float(sum_{j = 1 .. k1 - 1} double(sqrtf(sqd_j)) / double(k1 - 1)) added in ascending j, 0 where not valid"""
    valid = sqd[:, k1 - 1] >= 0
    s = np.sqrt(np.where(valid[:, None], sqd[:, 1:k1], 0).astype(np.float32)).astype(np.float64)
    dist = (np.cumsum(s, axis=1)[:, -1] / np.float64(k1 - 1)).astype(np.float32)  # (cumsum adds one after the other)
    return np.where(valid, dist, np.float32(0)), valid


def sums_of(dist):
    """the reference's two sequential f64 sums and the lowest-bit exponents of their terms"""
    sq = (dist * dist).astype(np.float32)
    total = float(np.cumsum(dist.astype(np.float64))[-1])
    sq_total = float(np.cumsum(sq.astype(np.float64))[-1])
    return total, sq_total, int(low_bit_exponent(dist).min()), int(low_bit_exponent(sq).min())


# ---- the register-boundary sweep -----------------------------------------------------------------------------------------------------------------------------
SWEEP_K = [64, 127, 128, 191, 192, 255]  # k1 = 65, 128, 129, 192, 193, 256: both ends of each R
SWEEP_CHAINS = [("VOXELGRID 0.1", vox()), ("NONE", params()), ("APPROX 0.1", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=0.1))]
SWEEP = [(f"{name}, distance filter {'on' if dist else 'off'}, k {k}", dict(p, enable_distance_filter=dist, statistical_mean_k=k, statistical_stddev=1.0))
         for name, p in SWEEP_CHAINS for dist in (True, False) for k in SWEEP_K]


@functools.lru_cache(maxsize=None)
def sweep_rows(chain, dist):
    """the oracle's 256 nearest of every point the outlier stage of a sweep chain reads (one search serves every mean_k of the chain)"""
    from oracle import oracle as orc

    p = dict(SWEEP_CHAINS[chain][1], enable_distance_filter=dist)
    stage_in = oracle_chain(quarter_scan(), p)[3]
    assert len(stage_in) > 2000
    return orc.knn(stage_in, stage_in, 256)[1]


def sweep_certifies(which):
    p = SWEEP[which][1]
    dist, valid = mean_distances(sweep_rows(which // (2 * len(SWEEP_K)), p["enable_distance_filter"]), p["statistical_mean_k"] + 1)
    assert valid.all()
    total, sq_total, q, q_sq = sums_of(dist)
    return certified(total, q) and certified(sq_total, q_sq), (total, q, sq_total, q_sq)


def test_every_sweep_case_certifies_its_threshold_on_the_cpu():
    """No GPU: the tree sums of the device are the sequential ones whatever the order iff the sum is below 2^(q + 52) for 2^q the lowest set bit of the
    terms — held here over the oracle's mean distances, so that route 1 (anomaly 0) may be demanded of every case below."""
    for which, (name, _) in enumerate(SWEEP):
        ok, figures = sweep_certifies(which)
        assert ok, (name, figures)


@gpu
@pytest.mark.parametrize("which", range(len(SWEEP)), ids=[n for n, _ in SWEEP])
def test_register_boundaries_are_served_with_the_same_bits(ctx, which):
    name, p = SWEEP[which]
    assert sweep_certifies(which)[0], name
    _, counts, _ = exact_three_ways(quarter_scan(), p, ctx, name)
    assert 0 < counts[2] < counts[1], (name, counts)


# ---- the switch ------------------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_switch_is_off_by_default_and_changes_the_route_only():
    from mrg_slam_amd import Context, prefilter

    c = Context()
    p = vox(statistical_mean_k=100)
    out = []
    for on, route in ((None, 0), (True, 1), (False, 0)):
        if on is not None:
            c.set_wide_statistical_chains(on)
        out.append(prefilter(quarter_scan(), p, ctx=c))
        st = c.prefilter_stats()
        assert st["route"] == route and st["anomaly"] == 0, (on, st)
    assert len(out[0]) > 1000
    same(out[0], out[1], "switch on")
    same(out[0], out[2], "switch off again")
    # behind NONE the wide switch alone is not enough: the chain needs mrgfe_ctx_set_statistical_chains for its grid, as with mean_k <= 63
    c.set_wide_statistical_chains(True)
    none = params(statistical_mean_k=100)
    got = prefilter(quarter_scan(), none, ctx=c)
    assert c.prefilter_stats()["route"] == 0
    c.set_statistical_chains(True)
    same(prefilter(quarter_scan(), none, ctx=c), got, "NONE")
    assert c.prefilter_stats()["route"] == 1 and c.prefilter_stats()["anomaly"] == 0
    c.close()


@gpu
def test_mean_k_63_is_what_it_was(ctx):
    from mrg_slam_amd import prefilter

    p = vox(statistical_mean_k=63)
    got = {}
    try:
        for on in (True, False):
            ctx.set_wide_statistical_chains(on)
            got[on] = prefilter(quarter_scan(), p, ctx=ctx)
            st, ks = ctx.prefilter_stats(), ctx.knn_stats()
            assert st["route"] == 1 and st["anomaly"] == 0 and ks["k"] == 64, (on, st, ks)
    finally:
        ctx.set_wide_statistical_chains(True)
    same(got[True], got[False], "mean_k 63")
    same(got[True], oracle_chain(quarter_scan(), p)[0], "mean_k 63 (oracle)")


@gpu
def test_the_switch_is_inherited_and_mean_k_256_is_still_refused(ctx):
    from mrg_slam_amd import Context, MrgfeError, _lib, prefilter

    def held(c):
        on, inherited = C.c_int(-7), C.c_int(-7)
        assert _lib.lib().mrgfe_dbg_wide_statistical_chains(c._h, C.byref(on), C.byref(inherited)) == 0
        return on.value, inherited.value

    fresh = Context()
    assert held(fresh) == (0, 0) and held(ctx) == (1, 1)
    fresh.close()
    calls = ctx.prefilter_stats()["calls"]
    with pytest.raises(MrgfeError, match=r"\[1, 255\]") as e:
        prefilter(quarter_scan(), vox(statistical_mean_k=256), ctx=ctx)
    assert e.value.status == _lib.ERR_INVALID and ctx.prefilter_stats()["calls"] == calls  # refused before anything runs


# ---- lists that do not fill, or fill exactly -----------------------------------------------------------------------------------------------------------------
@gpu
def test_too_few_neighbours_for_the_narrow_list(ctx):
    """50 points, mean_k = 63: the k-NN stage sees fewer points than mean_k + 1, so no query is valid"""
    cloud = np.ascontiguousarray(quarter_scan()[:50])
    assert np.isfinite(cloud).all()
    p = params(statistical_mean_k=63, enable_distance_filter=False)
    exp, counts, _, _ = oracle_chain(cloud, p)
    assert counts[:2] == [50, 50]
    fast, fs, _, slow, ss, off, _ = three_ways(cloud, p, ctx)
    assert fs["route"] == 1 or (fs["route"] == 2 and fs["anomaly"] and not fs["anomaly"] & ~DOCUMENTED_ANOMALIES), fs
    assert ss["route"] == 0
    same(fast, exp, "50 points")
    same(slow, exp, "50 points (host-driven)")
    same(off, exp, "50 points (switch off)")


def outcome(cloud, p, ctx):
    from mrg_slam_amd import prefilter

    prefilter(cloud, p, ctx=ctx)
    st = ctx.prefilter_stats()
    return st["route"], st["anomaly"]


@gpu
@pytest.mark.parametrize("mean_k", [64, 255])
@pytest.mark.parametrize("short", [0, 1], ids=["exactly k1 points", "k1 - 1 points"])
def test_lists_that_fill_exactly_or_not_at_all(ctx, mean_k, short):
    """downsample NONE, distance filter off: mean_k + 1 points make every query valid with its list full to the last entry, one fewer makes none valid.
    The route is the one the narrow kernel takes for the same shape at mean_k = 5."""
    p = params(enable_distance_filter=False)
    narrow = outcome(uniform_cloud(5 + 1 - short), dict(p, statistical_mean_k=5), ctx)
    cloud = uniform_cloud(mean_k + 1 - short)
    what = f"mean_k {mean_k}, {len(cloud)} points"
    _, counts, fs = exact_three_ways(cloud, dict(p, statistical_mean_k=mean_k), ctx, what, route=narrow[0])
    assert (fs["route"], fs["anomaly"]) == narrow and counts[1] == len(cloud), (what, fs, narrow)


@gpu
def test_identical_points_tie_by_index_across_the_registers(ctx):
    """300 copies of one point and 60 scattered ones, mean_k = 100: zero distances, and among equals the lower index is the nearer"""
    rng = np.random.default_rng(31)
    cloud = np.concatenate([np.tile(np.float32([1.25, -0.5, 0.75, 9.0]), (300, 1)), uniform_cloud(60, seed=11)])[rng.permutation(360)]
    p = params(enable_distance_filter=False)
    narrow = outcome(cloud, dict(p, statistical_mean_k=20), ctx)
    _, counts, fs = exact_three_ways(cloud, dict(p, statistical_mean_k=100), ctx, "copies", route=narrow[0])
    assert (fs["route"], fs["anomaly"]) == narrow and 0 < counts[2] < 360, (fs, narrow, counts)


# ---- far and non-finite points -------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_points_far_from_the_scan(ctx):
    cloud = quarter_scan().copy()
    cloud[:10, :3] += np.float32(20.0)
    exact_three_ways(cloud, vox(statistical_mean_k=100, enable_distance_filter=False), ctx, "ten points 20 m off")


@gpu
def test_non_finite_points_are_handed_back(ctx):
    from mrg_slam_amd import _lib

    p = params(statistical_mean_k=100, enable_distance_filter=False)
    cloud = non_finite_cloud()
    fast, fs, _, slow, ss, off, os_ = three_ways(cloud, p, ctx)
    assert fs["route"] == 2 and fs["anomaly"] == _lib.PF_ANOMALY_NON_FINITE and ss["route"] == 0 and os_["route"] == 0, (fs, ss, os_)
    same(fast, slow, "non-finite")
    same(fast, off, "non-finite (switch off)")
    same(fast, oracle_chain(cloud, p)[0], "non-finite (oracle)")


# ---- the other entry points -------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_other_entry_points_take_the_same_route(ctx):
    """scan_callback, scan_callback_to_device, prefilter_records / scan_callback_records (32-byte records) and prefilter_to_device at mean_k = 100 behind
    VOXELGRID: route 1, and the bytes of the same call on route 0"""
    import torch

    from mrg_slam_amd import prefilter_records, prefilter_to_device, scan_callback, scan_callback_records, scan_callback_to_device
    from mrg_slam_amd._lib import lib

    scan, p = quarter_scan(), vox(statistical_mean_k=100)
    n = len(scan)
    data = memoryview(scan).cast("B")
    buf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")

    def to_device(fn):
        m = fn()
        ctx.synchronize()
        return buf[:m].cpu().numpy().copy()

    calls = {
        "scan_callback": lambda: np.array(scan_callback(data, n, 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)),
        "scan_callback_to_device": lambda: to_device(lambda: scan_callback_to_device(data, n, 1, 16, FIELDS, buf.data_ptr(), n, 0, None, PERIOD, None, p, ctx=ctx)),
        "prefilter_to_device": lambda: to_device(lambda: prefilter_to_device(scan, buf.data_ptr(), n, p, ctx=ctx)),
        "prefilter_records": lambda: np.array(prefilter_records(scan, 32, None, 0, p, ctx=ctx)),
        "scan_callback_records": lambda: np.array(scan_callback_records(data, n, 1, 16, FIELDS, 32, None, 0, 0, None, PERIOD, None, p, ctx=ctx)),
    }
    exp = oracle_chain(scan, p)[0]
    for name, call in calls.items():
        got = {}
        try:
            for mode in (1, 0):
                assert lib().mrgfe_dbg_set_prefilter_device_driven(mode) == mode
                got[mode] = call()
                st = ctx.prefilter_stats()
                assert st["route"] == mode and st["anomaly"] == 0, (name, mode, st)
                if mode == 1 and name.endswith("records"):
                    eg = ctx.egress_stats()
                    assert eg["launches"] == 1 and eg["waits"] == 0 and eg["bytes"] == len(exp) * 32, (name, eg)  # written behind the chain, in front of its wait
        finally:
            lib().mrgfe_dbg_set_prefilter_device_driven(1)
        assert got[1].dtype == got[0].dtype and got[1].shape == got[0].shape and got[1].tobytes() == got[0].tobytes(), name
        want = pack(exp, 32) if name.endswith("records") else exp
        assert got[1].tobytes() == np.ascontiguousarray(want).tobytes(), name


# ---- the kernel against first principles ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sixteenth_scan_sorted():
    cloud = np.ascontiguousarray(quarter_scan()[::4])
    cloud.setflags(write=False)
    return cloud, full_sort(cloud, cloud)[1]


@gpu
@pytest.mark.parametrize("k1", [65, 129, 193])
def test_mean_distances_against_a_full_sort(ctx, k1):
    """Not the oracle: all squared distances in the library's float expression, fully sorted by (distance, index) in numpy (tests/test_gpu_knn_wide.py),
    the f64 sum of their float square roots in ascending order, sor::threshold's formula over the reference's sequential sums, and the points whose mean
    distance is not above the threshold — against what the chain NONE -> STATISTICAL returns (distance filter off: the stage reads the cloud itself)."""
    from mrg_slam_amd import prefilter

    cloud, sqd = sixteenth_scan_sorted()
    assert 1500 < len(cloud) < 1800
    dist, valid = mean_distances(sqd, k1)
    assert valid.all() and (dist > 0).all()
    total, sq_total, q, q_sq = sums_of(dist)
    assert certified(total, q) and certified(sq_total, q_sq)
    nv = np.float64(valid.sum())
    thr = total / nv + 1.0 * np.sqrt((sq_total - total * total / nv) / (nv - 1))
    keep = ~(dist.astype(np.float64) > thr)
    assert 0 < keep.sum() < len(cloud)
    got = prefilter(cloud, params(statistical_mean_k=k1 - 1, enable_distance_filter=False), ctx=ctx)
    st, ks = ctx.prefilter_stats(), ctx.knn_stats()
    assert st["route"] == 1 and st["anomaly"] == 0 and ks["k"] == k1, (st, ks)
    same(got, cloud[keep], f"k1 {k1}")
