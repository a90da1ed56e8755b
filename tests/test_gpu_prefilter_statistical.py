"""GPU: [distance filter] -> VOXELGRID -> STATISTICAL — the reference's code-default prefilter chain — served by the device-driven chain (csrc/filters.hip:
one host wait, the k-NN lists consumed in registers, PCL's threshold from certified tree sums).  Every output is compared bit for bit and in order with
the host-driven passes (the switch at 0) and with the CPU oracle's chain; mrgfe_ctx_prefilter_stats says which route served a call."""
import numpy as np
import pytest

from conftest import small_cloud
from sor_cases import bits, edge_arrays, ordinary_arrays, refused_arrays, sor_threshold

pytestmark = pytest.mark.gpu

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1
FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
BASE = {"downsample_method": "VOXELGRID", "outlier_removal_method": "STATISTICAL", "distance_near_thresh": 0.1, "distance_far_thresh": 35.0,
        "downsample_resolution": 0.1, "downsample_min_points_per_voxel": 1, "statistical_mean_k": 20, "statistical_stddev": 1.0, "enable_distance_filter": True}


def params(**more):
    p = dict(BASE)
    p.update(more)
    return p


def oracle_chain(cloud, p):
    """The oracle's stages; returns the output and what decides the expected route: finite survivors of the distance filter, voxels (0 also for PCL's
    'leaf size too small' pass-through, which makes none)."""
    from oracle import oracle as orc

    c = np.ascontiguousarray(cloud, dtype=np.float32)
    if p["enable_distance_filter"]:
        c = orc.distance_filter(c, p["distance_near_thresh"], p["distance_far_thresh"])
    n_finite = int(np.isfinite(c[:, :3]).all(1).sum())
    voxels = 0
    if len(c):
        all_voxels, status = orc.voxelgrid(c, p["downsample_resolution"], 1)
        voxels = 0 if status != 0 else len(all_voxels)
        c, _ = orc.voxelgrid(c, p["downsample_resolution"], p["downsample_min_points_per_voxel"])
    if len(c):
        c, _ = orc.statistical_outlier(c, p["statistical_mean_k"], p["statistical_stddev"])
    return c, n_finite, voxels


@pytest.fixture(scope="module")
def ctx():
    from mrg_slam_amd import Context

    return Context()


@pytest.fixture(scope="module")
def street_scan():
    from mrg_slam_amd import synth

    return synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 4711)


def both_routes(cloud, p, ctx):
    """prefilter with the switch at 1 and at 0: (fast, its stats, slow, its stats)"""
    from mrg_slam_amd import prefilter
    from mrg_slam_amd._lib import lib

    try:
        assert lib().mrgfe_dbg_set_prefilter_device_driven(1) == 1
        fast = prefilter(cloud, p, ctx=ctx)
        fs = ctx.prefilter_stats()
        assert lib().mrgfe_dbg_set_prefilter_device_driven(0) == 0
        slow = prefilter(cloud, p, ctx=ctx)
        ss = ctx.prefilter_stats()
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)
    return fast, fs, slow, ss


SCAN_CASES = [params(), params(statistical_mean_k=30, statistical_stddev=1.2), params(downsample_resolution=0.3, downsample_min_points_per_voxel=2),
              params(enable_distance_filter=False), params(enable_distance_filter=False, statistical_mean_k=30, statistical_stddev=1.2)]


@pytest.fixture(scope="module")
def scan_expected(street_scan):
    return [oracle_chain(street_scan, p)[0] for p in SCAN_CASES]


@pytest.mark.parametrize("which", range(len(SCAN_CASES)))
def test_street_scan_is_served_device_driven_with_the_same_bits(street_scan, scan_expected, ctx, which):
    """Route 1 with the switch at 1, route 0 with it at 0, both equal to the oracle chain — through mrgfe_prefilter, mrgfe_prefilter_device and (below) the
    scan callback.  On the parent commit there is no stats call, and the route would be 0."""
    import torch

    from mrg_slam_amd import prefilter_to_device

    p, exp = SCAN_CASES[which], scan_expected[which]
    assert len(street_scan) > 20000 and len(exp) > 1000
    before = ctx.prefilter_stats()
    fast, fs, slow, ss = both_routes(street_scan, p, ctx)
    assert fs["route"] == 1 and fs["anomaly"] == 0 and ss["route"] == 0, (fs, ss)
    np.testing.assert_array_equal(fast, slow)
    np.testing.assert_array_equal(fast, exp)
    assert fs["points_out"] == len(exp) == fs["counts"][4] and fs["counts"][3] >= len(exp) and fs["counts"][0] <= len(street_scan)
    assert fs["calls"] == before["calls"] + 1 and fs["served"] == before["served"] + 1 and ss["calls"] == fs["calls"] + 1 and ss["served"] == fs["served"]
    buf = torch.empty((len(street_scan), 4), dtype=torch.float32, device="cuda:0")
    m = prefilter_to_device(street_scan, buf.data_ptr(), len(street_scan), p, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 1
    np.testing.assert_array_equal(buf[:m].cpu().numpy(), exp)


@pytest.mark.parametrize("mean_k,stddev", [(20, 1.0), (30, 1.2)])
def test_scan_callback_with_deskewing_and_a_transform(street_scan, ctx, mean_k, stddev):
    from mrg_slam_amd import scan_callback, synth
    from mrg_slam_amd._lib import lib
    from oracle import oracle as orc

    T = synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)
    p = params(statistical_mean_k=mean_k, statistical_stddev=stddev)
    c = orc.deskew(street_scan, ANG_V, PERIOD)
    c = orc.transform_points(T, np.ascontiguousarray(c))  # (every point of the synthetic scan is finite)
    exp = oracle_chain(c, p)[0]
    data = memoryview(np.ascontiguousarray(street_scan)).cast("B")
    got = {}
    try:
        for mode in (1, 0):
            assert lib().mrgfe_dbg_set_prefilter_device_driven(mode) == mode
            got[mode] = scan_callback(data, len(street_scan), 1, 16, FIELDS, 0, ANG_V, PERIOD, T, p, ctx=ctx)
            assert ctx.prefilter_stats()["route"] == mode
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)
    assert len(exp) > 1000
    np.testing.assert_array_equal(got[1], got[0])
    np.testing.assert_array_equal(got[1], exp)


def size_cases():
    rng = np.random.default_rng(20261004)
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6145, 10000] + [int(v) for v in rng.integers(300, 30000, 14)]
    cases = []
    for trial, n in enumerate(sizes):
        cloud = small_cloud(n, 1000 + trial, extent=(rng.uniform(3, 40), rng.uniform(3, 40), rng.uniform(0.5, 6)))
        kind = trial % 5
        if kind == 1:    # only the last points survive the distance filter
            cloud[: max(0, n - 7), :3] *= np.float32(1e-4)
        elif kind == 2:  # only the first points do
            cloud[min(n, 5):, :3] = np.float32(900.0)
        elif kind == 3 and n > 10:
            cloud[rng.choice(n, max(1, n // 50), replace=False), rng.integers(0, 3)] = np.nan
        # (kind 2 keeps its far threshold below the 900 m points: thousands of identical points passed through by PCL's too-small-leaf rule cost the CPU
        # oracle's search seconds; the pass-through has its case among the hand-backs)
        p = params(distance_far_thresh=float(rng.choice([8.0, 35.0] if kind == 2 else [8.0, 35.0, 1e4])), downsample_resolution=float(rng.choice([0.05, 0.1, 0.3, 1.0])),
                   downsample_min_points_per_voxel=int(rng.choice([1, 1, 2])), statistical_mean_k=int(rng.choice([1, 5, 20, 30, 63])),
                   statistical_stddev=float(rng.choice([0.5, 1.0, 2.0])))
        cases.append((f"trial {trial}: n={n} kind={kind}", cloud, p))
    for k in (1, 5, 20, 63):  # clouds of k, k + 1 and k + 2 points, far enough apart to stay one per voxel: the k + 1 nearest exist from k + 1 points on
        for n in (k, k + 1, k + 2):
            cases.append((f"n={n} around k={k}", small_cloud(n, 77 + n, extent=(12.0, 9.0, 2.0)), params(statistical_mean_k=k, downsample_resolution=0.05)))
    leaf = 0.25  # (exact in binary: a true lattice, whole shells of neighbours at one distance)
    g = np.stack(np.meshgrid(np.arange(-14, 15), np.arange(-12, 13), np.arange(-3, 4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(leaf)
    lattice = np.concatenate([g, np.linspace(0, 1, len(g), dtype=np.float32)[:, None]], 1)[rng.permutation(len(g))]
    cases.append(("lattice", lattice, params(downsample_resolution=leaf, statistical_mean_k=20)))
    cases.append(("lattice, k = 30", lattice, params(downsample_resolution=leaf, statistical_mean_k=30, statistical_stddev=0.5)))
    return cases


def test_sizes_at_tile_boundaries_and_random_parameters(ctx):
    """The size and kind list of test_device_driven_prefilter_chain_at_tile_boundaries_and_random_parameters (tests/test_gpu_filters.py) with the statistical
    filter behind the voxel grid, sizes k, k + 1, k + 2 around the neighbour count, and a lattice cloud whose neighbour distances tie.  fast == slow ==
    oracle, and the route is what the ORACLE's stage counts say: 2 when no finite point survives the distance filter or the voxel grid makes no voxel
    (PCL's pass-through of a too small leaf included), else 1 — any other hand-back fails."""
    cases = size_cases()
    handed_back = 0
    for name, cloud, p in cases:
        name = f"{name} {p}"
        exp, n_finite, voxels = oracle_chain(cloud, p)
        fast, fs, slow, ss = both_routes(cloud, p, ctx)
        print(f"{name}: {len(cloud)} -> {len(exp)} route {fs['route']} anomaly {fs['anomaly']} counts {fs['counts']}")
        np.testing.assert_array_equal(fast, slow, err_msg=name)
        np.testing.assert_array_equal(fast, exp, err_msg=name)
        want = 2 if (n_finite == 0 or voxels == 0) else 1
        assert fs["route"] == want and ss["route"] == 0, (name, fs, n_finite, voxels)
        if want == 1:
            assert fs["counts"][1] == n_finite and fs["counts"][2] == voxels and fs["counts"][4] == len(exp), (name, fs)
        handed_back += want == 2
    assert handed_back < len(cases) // 3  # (the list is mostly ordinary clouds)


HAND_BACKS = ["nothing survives the distance filter", "all points non-finite", "all points non-finite, no distance filter", "leaf size too small",
              "k-NN grid beyond its table"]


def hand_back_case(name, street_scan):
    """(cloud, parameters, the anomaly bit the device-driven chain must name)"""
    from mrg_slam_amd import _lib

    nan = np.full((50, 4), np.nan, dtype=np.float32)
    if name == "nothing survives the distance filter":
        return street_scan[::4], params(distance_near_thresh=500.0, distance_far_thresh=600.0), _lib.PF_ANOMALY_EMPTY
    if name == "all points non-finite":
        return nan, params(), _lib.PF_ANOMALY_EMPTY
    if name == "all points non-finite, no distance filter":
        return nan, params(enable_distance_filter=False), _lib.PF_ANOMALY_EMPTY
    if name == "leaf size too small":
        # PCL's "leaf size too small" test is (dx * dy * dz) > INT32_MAX in int64.  0.01 m leaves over 6 km: 6e5^3 = 2.2e17 cells, the cloud is passed through.
        return small_cloud(1500, 3, extent=(3000.0, 3000.0, 3000.0)), params(downsample_resolution=0.01, distance_far_thresh=1e9), _lib.PF_ANOMALY_OVERFLOW
    # The k-NN grid's cell edge is max(8 leaves, 0.2 m) = 0.2 m here and its table holds 2^24 - 1 = 16 777 215 cells; the cloud spans 60 km: 3e5 cells per axis,
    # 2.7e16 in all.  (The cloud is the "leaf size too small" case of tests/test_gpu_filters.py, but 0.01 m leaves over 60 km are 6e6^3 = 2.2e20 leaves, which
    # does not fit int64 and wraps to a negative number in PCL's test, in the oracle's and in both routes': NO implementation passes this cloud through, every
    # point becomes a voxel of its own.  With 8^3 leaves per cell a cloud below PCL's 2^31 leaves cannot outgrow the table unless the leaf is below 0.025 m.)
    return small_cloud(3000, 3, extent=(30000.0, 30000.0, 30000.0)), params(downsample_resolution=0.01, distance_far_thresh=1e9), _lib.PF_ANOMALY_CELLS


@pytest.mark.parametrize("name", HAND_BACKS)
def test_hand_backs_name_their_anomaly_and_give_the_same_output(street_scan, ctx, name):
    """Route 2, the anomaly bit, and the host-driven route's and the oracle's output."""
    cloud, p, bit = hand_back_case(name, street_scan)
    exp = oracle_chain(cloud, p)[0]
    fast, fs, slow, ss = both_routes(cloud, p, ctx)
    assert fs["route"] == 2 and fs["anomaly"] & bit and ss["route"] == 0, (name, fs, ss)
    np.testing.assert_array_equal(fast, slow, err_msg=name)
    np.testing.assert_array_equal(fast, exp, err_msg=name)
    assert len(exp) > 1000 or "survives" in name or "non-finite" in name, name


def test_mean_k_beyond_a_wavefront_s_list_is_not_served(street_scan, ctx):
    """mean_k = 64: k + 1 does not fit a wavefront's list — route 0, and whatever the host-driven passes do with it, at either setting of the switch"""
    from mrg_slam_amd import MrgfeError, _lib, prefilter

    outcome = []
    for mode in (1, 0):
        try:
            _lib.lib().mrgfe_dbg_set_prefilter_device_driven(mode)
            try:
                outcome.append(("ok", prefilter(street_scan[::4], params(statistical_mean_k=64), ctx=ctx).tobytes()))
            except MrgfeError as e:
                outcome.append(("error", e.status))
            assert ctx.prefilter_stats()["route"] == 0
        finally:
            _lib.lib().mrgfe_dbg_set_prefilter_device_driven(1)
    assert outcome[0] == outcome[1]


def test_threshold_kernels_equal_the_host_loop(street_scan, ctx):
    """mrgfe_dbg_sor_threshold with on_device = 1 (the chain's reduction and finish kernels) against on_device = 0 in all six outputs: on the mean
    distances of the street scan's voxel centroids, recomputed from mrgfe_knn, and on the CPU test's random, refused and edge arrays — the refused ones
    are refused on the device too.
    The certificate's hand-back INSIDE the chain (anomaly bit 8) shares its wiring with the hand-backs of the test above: one anomaly word, one test
    behind the wait.  It cannot be provoked through the public chain without depending on the cell-edge rule: the voxel grid's cell limit bounds the
    ratio of the distances.  There is no switch for it."""
    from mrg_slam_amd import knn
    from oracle import oracle as orc

    def same(name, d, v, mul):
        host, dev = sor_threshold(d, v, mul, 0), sor_threshold(d, v, mul, 1, ctx)
        for key in host:
            assert bits(host[key]) == bits(dev[key]), (name, key, host, dev)
        return host

    c = orc.distance_filter(street_scan, 0.1, 35.0)
    c, _ = orc.voxelgrid(c, 0.1, 1)
    for k, mul in ((20, 1.0), (30, 1.2)):
        _, sqd = knn(c, c, k + 1, ctx=ctx)
        dist = (np.sqrt(sqd[:, 1:]).astype(np.float64).cumsum(1)[:, -1] / np.float64(k)).astype(np.float32)  # (sequential f64 sum of the float roots)
        valid = (sqd[:, k] >= 0).astype(np.uint32)
        dist[valid == 0] = 0.0
        got = same(f"street scan k={k}", dist, valid, mul)
        assert got["certified"] == 1.0 and got["valid"] == len(c) and -40 <= got["q"] <= -20, got
    for name, d, v, mul in ordinary_arrays() + edge_arrays():
        same(name, d, v, mul)
    for name, d, v, mul, expect in refused_arrays():
        got = same(name, d, v, mul)
        assert got["certified"] == float(expect), (name, got)


def test_registration_takes_the_scan_over_with_the_chain_s_box(ctx):
    """mrgfe_scan_callback_device with STATISTICAL, then setInputSourceFromPrefilter (the source's search grid on the box the chain reported) against
    setInputSourceDevice on the same buffer."""
    import torch

    from mrg_slam_amd import GicpHip, prefilter, scan_callback_to_device, synth

    scene = synth.street_scene()
    tgt_raw, src_raw, rel = synth.scan_pair(0, "VLP16", scene)
    p = params()
    tgt = prefilter(tgt_raw, p, ctx=ctx)
    guess = synth.warm_guess(rel, 0)
    buf = torch.empty((len(src_raw), 4), dtype=torch.float32, device="cuda:0")
    data = memoryview(np.ascontiguousarray(src_raw)).cast("B")
    res = {}
    for how in ("from_prefilter", "device"):
        reg = GicpHip(transformation_epsilon=0.01, ctx=ctx)
        reg.setInputTarget(tgt)
        m = scan_callback_to_device(data, len(src_raw), 1, 16, FIELDS, buf.data_ptr(), buf.shape[0], 0, None, PERIOD, None, p, ctx=ctx)
        assert ctx.prefilter_stats()["route"] == 1 and m > 1000
        if how == "from_prefilter":
            reg.setInputSourceFromPrefilter(buf.data_ptr(), m)
        else:
            ctx.synchronize()
            reg.setInputSourceDevice(buf.data_ptr(), m)
        reg.align(guess)
        res[how] = (reg.getFinalTransformation().copy(), reg.hasConverged(), reg.getFinalNumIteration())
    np.testing.assert_array_equal(res["from_prefilter"][0], res["device"][0])
    assert res["from_prefilter"][1:] == res["device"][1:] and res["device"][2] >= 1


def test_chains_that_are_still_not_served(street_scan, ctx):
    from mrg_slam_amd import prefilter

    for down in ("APPROX_VOXELGRID", "NONE"):
        out = prefilter(street_scan[::3], params(downsample_method=down), ctx=ctx)
        st = ctx.prefilter_stats()
        assert st["route"] == 0 and st["points_out"] == len(out) > 100, (down, st)
