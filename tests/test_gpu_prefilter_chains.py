"""GPU: the prefilter chains the device-driven form serves besides VOXELGRID + RADIUS / STATISTICAL (csrc/filters.hip: the chain as three stages, one wait):

    downsample        outlier
    VOXELGRID         NONE
    APPROX_VOXELGRID  NONE, RADIUS
    NONE              NONE (distance filter only), RADIUS

with and without the distance filter.  Every case runs with the switch at 1 and at 0 and is compared with the CPU oracle's stage composition bit for bit
on a uint32 view (NaN centroids occur) and in order; mrgfe_ctx_prefilter_stats says which route served a call."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1
FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
BASE = {"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "downsample_method": "NONE", "downsample_resolution": 0.1,
        "downsample_min_points_per_voxel": 1, "outlier_removal_method": "NONE", "radius_radius": 0.5, "radius_min_neighbors": 2, "statistical_mean_k": 20,
        "statistical_stddev": 1.0}


def params(**more):
    p = dict(BASE)
    p.update(more)
    return p


def chains(leaf_a, leaf_b):
    """the newly served chains, (name, parameters) — each is run with and without the distance filter"""
    return [("distance filter only", params()),
            ("VOXELGRID", params(downsample_method="VOXELGRID", downsample_resolution=leaf_a)),
            ("VOXELGRID min 2", params(downsample_method="VOXELGRID", downsample_resolution=leaf_b, downsample_min_points_per_voxel=2)),
            ("NONE + RADIUS", params(outlier_removal_method="RADIUS")),
            ("APPROX", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=leaf_a)),
            ("APPROX + RADIUS", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=leaf_a, outlier_removal_method="RADIUS")),
            ("APPROX coarse + RADIUS", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=leaf_b, outlier_removal_method="RADIUS"))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, a.shape, b.shape)


def oracle_chain(cloud, p):
    """The oracle's stages as the reference composes them (a stage is skipped once nothing is left).  Returns the output and the point counts
    [after the distance filter, after the downsample, after the outlier filter]."""
    from oracle import oracle as orc

    c = np.ascontiguousarray(cloud, dtype=np.float32)
    if p["enable_distance_filter"]:
        c = orc.distance_filter(c, p["distance_near_thresh"], p["distance_far_thresh"])
    counts = [len(c)]
    if len(c) and p["downsample_method"] == "VOXELGRID":
        c, _ = orc.voxelgrid(c, p["downsample_resolution"], p["downsample_min_points_per_voxel"])
    elif len(c) and p["downsample_method"] == "APPROX_VOXELGRID":
        c = orc.approx_voxelgrid(c, p["downsample_resolution"])
    counts.append(len(c))
    if len(c) and p["outlier_removal_method"] == "RADIUS":
        c, _ = orc.radius_outlier(c, p["radius_radius"], p["radius_min_neighbors"])
    elif len(c) and p["outlier_removal_method"] == "STATISTICAL":
        c, _ = orc.statistical_outlier(c, p["statistical_mean_k"], p["statistical_stddev"])
    counts.append(len(c))
    return c, counts


def check_counts(p, fs, counts, what):
    """the count slots of mrgfe_ctx_prefilter_stats on route 1"""
    c = fs["counts"]
    assert c[0] == counts[0] and c[3] == counts[1] and c[4] == counts[2] == fs["points_out"], (what, fs, counts)
    if p["downsample_method"] == "APPROX_VOXELGRID":
        assert c[2] == c[3], (what, fs)
    if p["downsample_method"] == "NONE":
        assert c[2] == c[3] == c[0], (what, fs)
    if p["outlier_removal_method"] == "NONE":
        assert c[4] == c[3], (what, fs)


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


def remembered(ctx):
    from mrg_slam_amd._lib import lib

    flag, n, box = C.c_int(-1), C.c_size_t(0), np.zeros(6, dtype=np.float32)
    assert lib().mrgfe_dbg_prefilter_output(ctx._h, C.byref(flag), C.byref(n), box.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return bool(flag.value), n.value, box


# ---- 1. the street scan ----------------------------------------------------------------------------------------------------------------------------------
SCAN_CASES = [(f"{name}, distance filter {'on' if dist else 'off'}", dict(p, enable_distance_filter=dist)) for name, p in chains(0.1, 0.3) for dist in (True, False)]


@pytest.fixture(scope="module")
def scan_expected(street_scan):
    return [oracle_chain(street_scan, p) for _, p in SCAN_CASES]


@pytest.mark.parametrize("which", range(len(SCAN_CASES)), ids=[n for n, _ in SCAN_CASES])
def test_street_scan_is_served_device_driven_with_the_same_bits(street_scan, scan_expected, ctx, which):
    """Route 1 and anomaly 0 with the switch at 1, route 0 with it at 0, fast == slow == oracle and the count slots — through mrgfe_prefilter,
    mrgfe_prefilter_device and the scan callback."""
    import torch

    from mrg_slam_amd import prefilter_to_device, scan_callback

    (name, p), (exp, counts) = SCAN_CASES[which], scan_expected[which]
    assert len(street_scan) == 25952 and np.isfinite(street_scan).all()
    # every case is a non-empty output, a strict subset of its input where an outlier filter ran
    assert len(exp) > 0 and (p["outlier_removal_method"] == "NONE" or counts[2] < counts[1]), (name, counts)
    fast, fs, slow, ss = both_routes(street_scan, p, ctx)
    print(name, "counts", counts, "stats", fs)
    assert fs["route"] == 1 and fs["anomaly"] == 0 and ss["route"] == 0, (name, fs, ss)
    same(fast, slow, name)
    same(fast, exp, name)
    check_counts(p, fs, counts, name)
    buf = torch.empty((len(street_scan), 4), dtype=torch.float32, device="cuda:0")
    m = prefilter_to_device(street_scan, buf.data_ptr(), len(street_scan), p, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 1
    same(buf[:m].cpu().numpy(), exp, name + " (device)")
    rem, n_rem, box = remembered(ctx)  # every point is finite: the box is remembered, and it encloses the output
    assert rem and n_rem == m and (exp[:, :3] >= box[:3]).all() and (exp[:, :3] <= box[3:]).all(), (name, box)
    if p["outlier_removal_method"] == "NONE":
        assert np.array_equal(box[:3], exp[:, :3].min(0)) and np.array_equal(box[3:], exp[:, :3].max(0)), (name, box)  # ... exactly
    data = memoryview(np.ascontiguousarray(street_scan)).cast("B")
    got = scan_callback(data, len(street_scan), 1, 16, FIELDS, 0, None, PERIOD, None, p, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 1
    same(got, exp, name + " (scan callback)")


@pytest.mark.parametrize("name", ["APPROX + RADIUS", "VOXELGRID"])
def test_scan_callback_with_deskewing_and_a_transform(street_scan, ctx, name):
    from mrg_slam_amd import scan_callback, synth
    from mrg_slam_amd._lib import lib
    from oracle import oracle as orc

    T = synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)
    p = dict(chains(0.1, 0.3))[name]
    c = orc.deskew(street_scan, ANG_V, PERIOD)
    c = orc.transform_points(T, np.ascontiguousarray(c))  # (every point of the synthetic scan is finite)
    exp, counts = oracle_chain(c, p)
    data = memoryview(np.ascontiguousarray(street_scan)).cast("B")
    got = {}
    try:
        for mode in (1, 0):
            assert lib().mrgfe_dbg_set_prefilter_device_driven(mode) == mode
            got[mode] = scan_callback(data, len(street_scan), 1, 16, FIELDS, 0, ANG_V, PERIOD, T, p, ctx=ctx)
            st = ctx.prefilter_stats()
            assert st["route"] == mode and st["anomaly"] == 0, st
            if mode == 1:
                check_counts(p, st, counts, name)
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)
    assert len(exp) > 1000
    same(got[1], got[0], name)
    same(got[1], exp, name)


# ---- 2. tile and history boundaries ----------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 511, 512, 513, 2047, 2048, 2049, 4097]  # kTile is 2048, the approximate grid's history has 512 entries


def uniform_cloud(n, seed=20261020):
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(-3.0, 3.0, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0.0, 255.0, n).astype(np.float32)
    return c


def expected_route(p, counts):
    """1 unless the distance filter left nothing in front of another stage (anomaly bit 1).  An empty RESULT is served — also the one of a voxel grid
    whose min-points rule drops every voxel."""
    later_stage = p["downsample_method"] != "NONE" or p["outlier_removal_method"] != "NONE"
    return 2 if (counts[0] == 0 and later_stage) else 1


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_history_boundaries(ctx, n):
    """leaf 0.25, radius 0.5 / min 2 over seeded uniform clouds in +-3 m, every newly served chain with and without the distance filter"""
    cloud = uniform_cloud(n)
    for name, p0 in chains(0.25, 0.25):
        for dist in (True, False):
            p = dict(p0, enable_distance_filter=dist)
            what = f"n={n} {name} distance filter {'on' if dist else 'off'}"
            exp, counts = oracle_chain(cloud, p)
            fast, fs, slow, ss = both_routes(cloud, p, ctx)
            same(fast, slow, what)
            same(fast, exp, what)
            assert fs["route"] == expected_route(p, counts) and ss["route"] == 0, (what, fs, counts)
            if fs["route"] == 1:
                assert fs["anomaly"] == 0, (what, fs)
                check_counts(p, fs, counts, what)
            else:
                assert fs["anomaly"] & 1, (what, fs)
            if name == "NONE + RADIUS":
                if n <= 3:  # nobody has two neighbours: an empty result, served
                    assert fs["route"] == 1 and len(exp) == 0 and fs["points_out"] == 0, (what, fs)
                if n >= 511:
                    assert 0 < counts[2] < counts[1], (what, counts)


# ---- 3. the approximate grid's order dependence -------------------------------------------------------------------------------------------------------------
APPROX = params(enable_distance_filter=False, downsample_method="APPROX_VOXELGRID", downsample_resolution=0.1)


def two_cell_points(n, block, seed=5):
    """n points that alternate in blocks of `block` between the cells (0, 0, 0) and (0, -36, 36) of a 0.1 m grid: (0 * 7171 - 36 * 3079 + 36 * 4231) & 511 = 0,
    so both cells live in history entry 0"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), dtype=np.float32)
    c[:, :3] = rng.uniform(0.02, 0.08, (n, 3))
    second = (np.arange(n) // block) % 2 == 1
    c[second, 1] += np.float32(-3.6)
    c[second, 2] += np.float32(3.6)
    c[:, 3] = np.arange(n)
    cells = np.floor(c[:, :3] * (np.float32(1.0) / np.float32(0.1))).astype(np.int64)
    assert (cells[~second] == [0, 0, 0]).all() and (cells[second] == [0, -36, 36]).all()
    return c


@pytest.mark.parametrize("name,cloud,centroids", [("alternating", two_cell_points(100, 1), 100), ("blocks of 10", two_cell_points(100, 10), 10),
                                                  ("3000 copies", np.tile(np.array([[0.05, 0.05, 0.05, 1.0]], dtype=np.float32), (3000, 1)), 1)],
                         ids=["alternating", "blocks", "copies"])
def test_two_cells_that_share_a_history_entry(ctx, name, cloud, centroids):
    exp, counts = oracle_chain(cloud, APPROX)
    assert len(exp) == centroids, (name, len(exp))
    fast, fs, slow, ss = both_routes(cloud, APPROX, ctx)
    assert fs["route"] == 1 and fs["anomaly"] == 0 and ss["route"] == 0, (name, fs, ss)
    same(fast, slow, name)
    same(fast, exp, name)
    check_counts(APPROX, fs, counts, name)


def test_a_shuffled_cloud_gives_another_output_and_both_routes_follow(ctx):
    cloud = uniform_cloud(4097)
    shuffled = cloud[np.random.default_rng(3).permutation(len(cloud))]
    outs = []
    for c in (cloud, shuffled):
        for p in (APPROX, dict(APPROX, outlier_removal_method="RADIUS")):
            exp, _ = oracle_chain(c, p)
            fast, fs, slow, ss = both_routes(c, p, ctx)
            assert fs["route"] == 1 and ss["route"] == 0, (fs, ss)
            same(fast, slow, "shuffle")
            same(fast, exp, "shuffle")
            outs.append(fast)
    assert outs[0].shape != outs[2].shape or not np.array_equal(bits(outs[0]), bits(outs[2]))


def non_finite_cloud():
    rng = np.random.default_rng(77)
    c = uniform_cloud(3000, seed=9)
    bad = rng.choice(len(c), 120, replace=False)
    for j, i in enumerate(bad):
        c[i, j % 3] = (np.nan, np.inf, -np.inf, np.float32(1e30), np.float32(-1e30))[j % 5]
    c[bad[:6]] = np.nan
    return c


def test_non_finite_points_are_served_without_an_outlier_filter_and_not_remembered(ctx):
    """distance filter off: the approximate grid does not drop non-finite points (its INT_MIN cell takes what is out of range)"""
    import torch

    from mrg_slam_amd import prefilter_to_device

    cloud = non_finite_cloud()
    exp, counts = oracle_chain(cloud, APPROX)
    assert not np.isfinite(exp[:, :3]).all() and len(exp) > 100
    fast, fs, slow, ss = both_routes(cloud, APPROX, ctx)
    assert fs["route"] == 1 and fs["anomaly"] == 0 and ss["route"] == 0, (fs, ss)
    same(fast, slow, "non-finite")
    same(fast, exp, "non-finite")
    check_counts(APPROX, fs, counts, "non-finite")
    buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
    m = prefilter_to_device(cloud, buf.data_ptr(), len(cloud), APPROX, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 1 and m == len(exp)
    assert not remembered(ctx)[0]  # a box of the finite points would not enclose the cloud
    finite = cloud[np.isfinite(cloud[:, :3]).all(1) & (np.abs(cloud[:, :3]) < 1e20).all(1)]
    m = prefilter_to_device(finite, buf.data_ptr(), len(cloud), APPROX, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 1 and remembered(ctx)[:2] == (True, m)


@pytest.mark.parametrize("down", ["APPROX_VOXELGRID", "NONE"])
def test_non_finite_points_in_front_of_the_radius_filter_hand_the_call_back(ctx, down):
    from mrg_slam_amd import _lib

    cloud = non_finite_cloud()
    p = dict(APPROX, downsample_method=down, outlier_removal_method="RADIUS")
    fast, fs, slow, ss = both_routes(cloud, p, ctx)
    assert fs["route"] == 2 and fs["anomaly"] & _lib.PF_ANOMALY_NON_FINITE and ss["route"] == 0, (fs, ss)
    same(fast, slow, down)
    assert 0 < len(fast) < len(cloud)


# ---- 4. radius ties ---------------------------------------------------------------------------------------------------------------------------------------
def test_neighbours_at_exactly_the_radius_count(ctx):
    """A 21 x 17 x 2 lattice of 0.25 m steps (exact in binary), radius 0.5: the neighbours two steps along an axis are at exactly the radius and count.
    min_neighbors 12, 17 and 20 keep 706, 570 and 562 of the 714 points on the CPU; a sphere one ulp smaller keeps 570, 570 and none."""
    g = np.stack(np.meshgrid(np.arange(-10, 11), np.arange(-8, 9), np.arange(0, 2), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.25)
    rng = np.random.default_rng(11)
    cloud = np.concatenate([g + np.float32(4.0), rng.uniform(0, 1, (len(g), 1)).astype(np.float32)], 1)[rng.permutation(len(g))]
    for need in (12, 17, 20):
        for dist in (True, False):
            p = params(outlier_removal_method="RADIUS", radius_min_neighbors=need, enable_distance_filter=dist)
            exp, counts = oracle_chain(cloud, p)
            fast, fs, slow, ss = both_routes(cloud, p, ctx)
            assert fs["route"] == 1 and fs["anomaly"] == 0 and ss["route"] == 0, (need, fs, ss)
            same(fast, slow, need)
            same(fast, exp, need)
            check_counts(p, fs, counts, need)
            assert 0 < counts[2] < counts[1], (need, counts)
    # with the sphere shrunk by one ulp the points at exactly the radius are gone, and the result differs: the ties decide
    p = params(outlier_removal_method="RADIUS", radius_min_neighbors=12)
    tight = oracle_chain(cloud, dict(p, radius_radius=float(np.nextafter(np.float64(0.5), 0.0))))[0]
    assert len(tight) != len(oracle_chain(cloud, p)[0])


# ---- 5. hand-over -----------------------------------------------------------------------------------------------------------------------------------------
def test_registration_takes_the_scan_over_with_the_chain_s_box(ctx):
    """mrgfe_scan_callback_device with VOXELGRID + NONE, then setInputSourceFromPrefilter (the source's search grid on the box the chain reported) against
    setInputSourceDevice on the same buffer."""
    import torch

    from mrg_slam_amd import GicpHip, prefilter, scan_callback_to_device, synth

    scene = synth.street_scene()
    tgt_raw, src_raw, rel = synth.scan_pair(0, "VLP16", scene)
    p = params(downsample_method="VOXELGRID")
    tgt = prefilter(tgt_raw, p, ctx=ctx)
    guess = synth.warm_guess(rel, 0)
    buf = torch.empty((len(src_raw), 4), dtype=torch.float32, device="cuda:0")
    data = memoryview(np.ascontiguousarray(src_raw)).cast("B")
    res = {}
    for how in ("from_prefilter", "device"):
        reg = GicpHip(transformation_epsilon=0.01, ctx=ctx)
        reg.setInputTarget(tgt)
        m = scan_callback_to_device(data, len(src_raw), 1, 16, FIELDS, buf.data_ptr(), buf.shape[0], 0, None, PERIOD, None, p, ctx=ctx)
        assert ctx.prefilter_stats()["route"] == 1 and m > 1000 and remembered(ctx)[:2] == (True, m)
        if how == "from_prefilter":
            reg.setInputSourceFromPrefilter(buf.data_ptr(), m)
        else:
            ctx.synchronize()
            reg.setInputSourceDevice(buf.data_ptr(), m)
        reg.align(guess)
        res[how] = (reg.getFinalTransformation().copy(), reg.hasConverged(), reg.getFinalNumIteration())
    np.testing.assert_array_equal(res["from_prefilter"][0], res["device"][0])
    assert res["from_prefilter"][1:] == res["device"][1:] and res["device"][2] >= 1


# ---- 6. still host-driven ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [params(downsample_method="APPROX_VOXELGRID", outlier_removal_method="STATISTICAL"), params(outlier_removal_method="STATISTICAL"),
                               params(downsample_method="VOXELGRID", outlier_removal_method="STATISTICAL", statistical_mean_k=64)],
                         ids=["APPROX + STATISTICAL", "NONE + STATISTICAL", "mean_k 64"])
def test_chains_that_stay_host_driven(street_scan, ctx, p):
    from mrg_slam_amd import MrgfeError, _lib, prefilter

    outcome = []
    for mode in (1, 0):
        try:
            _lib.lib().mrgfe_dbg_set_prefilter_device_driven(mode)
            try:
                outcome.append(("ok", prefilter(street_scan[::4], p, ctx=ctx).tobytes()))
            except MrgfeError as e:
                outcome.append(("error", e.status))
            assert ctx.prefilter_stats()["route"] == 0
        finally:
            _lib.lib().mrgfe_dbg_set_prefilter_device_driven(1)
    assert outcome[0] == outcome[1]
