"""GPU: [distance filter] -> NONE | APPROX_VOXELGRID -> STATISTICAL on the device-driven chain, behind the context switch mrgfe_ctx_set_statistical_chains
(csrc/filters.hip, csrc/nn_grid.hip: nn_build_device_sized — the k-NN grid's cell edge is chosen on the device from the cloud's density).  Off by default:
a fresh context keeps these chains on route 0.  Every output is compared bit for bit on a uint32 view and in order with the CPU oracle's stage composition,
with the host-driven route (mrgfe_dbg_set_prefilter_device_driven(0)) and with the same context with the switch off; mrgfe_ctx_sor_grid_stats says what
the device chose, and the result must not depend on it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1
FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
BASE = {"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "downsample_method": "NONE", "downsample_resolution": 0.1,
        "downsample_min_points_per_voxel": 1, "outlier_removal_method": "STATISTICAL", "radius_radius": 0.5, "radius_min_neighbors": 2, "statistical_mean_k": 20,
        "statistical_stddev": 1.0}
CELLS_CAP = (1 << 24) - 1        # the k-NN grid's table (csrc/filters.hip kSorCellsCap)
DEFAULT_RULE = (1.0, 128.0, 4)   # start edge, crowding target, most halvings (csrc/filters.hip MRGFE_SOR_GRID_*)
MAX_DOUBLINGS = 8                # of the start edge, until the box fits the table (csrc/nn_grid.hip kNnSizedMaxDoublings)


def params(**more):
    p = dict(BASE)
    p.update(more)
    return p


CHAINS = [("NONE", params()), ("APPROX 0.1", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=0.1)),
          ("APPROX 0.3", params(downsample_method="APPROX_VOXELGRID", downsample_resolution=0.3))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, a.shape, b.shape)


def pack(cloud, step):
    """the records of a packed cloud: 16: the points; 32: x, y, z, 1.0f, intensity, 0, 0, 0 (the pcl::PointXYZI in memory)"""
    c = bits(cloud)
    if step == 16:
        return c.copy().view(np.uint8).reshape(-1)
    r = np.zeros((len(c), 8), dtype=np.uint32)
    r[:, :3] = c[:, :3]
    r[:, 3] = np.float32(1.0).view(np.uint32)
    r[:, 4] = c[:, 3]
    return r.view(np.uint8).reshape(-1)


def oracle_chain(cloud, p):
    """The oracle's stages as the reference composes them (a stage is skipped once nothing is left).  Returns the output, the point counts [after the
    distance filter, after the downsample, after the outlier filter], the finite points among the first, and the cloud the outlier filter read."""
    from oracle import oracle as orc

    c = np.ascontiguousarray(cloud, dtype=np.float32)
    if p["enable_distance_filter"]:
        c = orc.distance_filter(c, p["distance_near_thresh"], p["distance_far_thresh"])
    counts = [len(c)]
    n_finite = int(np.isfinite(c[:, :3]).all(1).sum())
    if len(c) and p["downsample_method"] == "VOXELGRID":
        c, _ = orc.voxelgrid(c, p["downsample_resolution"], p["downsample_min_points_per_voxel"])
    elif len(c) and p["downsample_method"] == "APPROX_VOXELGRID":
        c = orc.approx_voxelgrid(c, p["downsample_resolution"])
    counts.append(len(c))
    stage_in = c
    if len(c) and p["outlier_removal_method"] == "STATISTICAL":
        c, _ = orc.statistical_outlier(c, p["statistical_mean_k"], p["statistical_stddev"])
    counts.append(len(c))
    return c, counts, n_finite, stage_in


def check_counts(p, fs, counts, what):
    """the count slots of mrgfe_ctx_prefilter_stats on route 1"""
    c = fs["counts"]
    assert c[0] == counts[0] and c[3] == counts[1] and c[4] == counts[2] == fs["points_out"], (what, fs, counts)
    assert c[2] == c[3], (what, fs)
    if p["downsample_method"] == "NONE":
        assert c[2] == c[0], (what, fs)


def cells_at(stage_in, edge):
    """cells of the grid over the outlier stage's input at `edge`, in the library's float arithmetic"""
    xyz = stage_in[:, :3]
    ext = (xyz.max(0) - xyz.min(0)).astype(np.float32)
    dims = np.floor(ext / np.float32(edge)).astype(np.float64) + 1.0
    return float(np.prod(dims))


def check_grid_stats(g, rule, stage_in, what, settled=True):
    """mrgfe_ctx_sor_grid_stats of a served call under `rule` = (start edge, target, most halvings).  `settled`: the search ended because its rule was
    satisfied — the crowding within the target, the halvings at their limit or the table at its — and not because the fixed number of counting passes
    was spent (a cloud of exact copies never thins out; the crowding reported is the one measured in front of the last decision)."""
    start, target, max_h = rule
    assert g["sized"], (what, g)
    h = g["halvings"]
    assert 0 <= h <= max_h and g["edge"] == float(np.float32(g["start_edge"]) * np.float32(2.0) ** np.float32(-h)), (what, g)
    d = np.log2(g["start_edge"] / float(np.float32(start)))
    assert d == int(d) and 0 <= d <= MAX_DOUBLINGS, (what, g, start)  # the rule's start edge, doubled until the box fits
    assert 1 <= g["cells"] <= CELLS_CAP and g["cells"] == cells_at(stage_in, g["edge"]), (what, g)
    if settled:
        assert (0 < g["crowding"] <= target) or h == max_h or cells_at(stage_in, g["edge"] * 0.5) > CELLS_CAP, (what, g, rule)


@pytest.fixture(scope="module")
def ctx():
    """the switch is ON for this module's context; tests that need it off switch it back in a finally"""
    from mrg_slam_amd import Context

    c = Context()
    c.set_statistical_chains(True)
    return c


@pytest.fixture(scope="module")
def street_scan():
    from mrg_slam_amd import synth

    return synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 4711)


@pytest.fixture(scope="module")
def quarter_scan(street_scan):
    return np.ascontiguousarray(street_scan[::4])


def set_rule(rule=None):
    from mrg_slam_amd._lib import lib

    start, target, max_h = rule if rule else (0.0, 0.0, 0)
    assert lib().mrgfe_dbg_set_sor_grid_rule(C.c_float(start), C.c_double(target), int(max_h)) == 0


def three_ways(cloud, p, ctx):
    """prefilter on the device-driven route with the switch on, on the host-driven route, and with the context's switch off:
    (fast, its stats, its grid stats, slow, its stats, off, its stats)"""
    from mrg_slam_amd import prefilter
    from mrg_slam_amd._lib import lib

    try:
        assert lib().mrgfe_dbg_set_prefilter_device_driven(1) == 1
        fast = prefilter(cloud, p, ctx=ctx)
        fs, gs = ctx.prefilter_stats(), ctx.sor_grid_stats()
        assert lib().mrgfe_dbg_set_prefilter_device_driven(0) == 0
        slow = prefilter(cloud, p, ctx=ctx)
        ss = ctx.prefilter_stats()
        assert lib().mrgfe_dbg_set_prefilter_device_driven(1) == 1
        ctx.set_statistical_chains(False)
        off = prefilter(cloud, p, ctx=ctx)
        os_ = ctx.prefilter_stats()
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)
        ctx.set_statistical_chains(True)
    return fast, fs, gs, slow, ss, off, os_


# ---- 1. the default is untouched ------------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_off_by_default_and_changes_the_route_only(quarter_scan):
    from mrg_slam_amd import Context, prefilter

    c = Context()
    for name, p in CHAINS[:2]:
        out = []
        for on, route in ((None, 0), (True, 1), (False, 0)):
            if on is not None:
                c.set_statistical_chains(on)
            out.append(prefilter(quarter_scan, p, ctx=c))
            st = c.prefilter_stats()
            assert st["route"] == route and st["anomaly"] == 0, (name, on, st)
            assert c.sor_grid_stats()["sized"] == (route == 1), (name, on, c.sor_grid_stats())
        assert len(out[0]) > 500
        same(out[0], out[1], name)
        same(out[0], out[2], name)
    vox = params(downsample_method="VOXELGRID")
    got = []
    for on in (False, True):
        c.set_statistical_chains(on)
        got.append(prefilter(quarter_scan, vox, ctx=c))
        g = c.sor_grid_stats()
        assert c.prefilter_stats()["route"] == 1 and not g["sized"] and g["edge"] == 0 and g["cells"] == 0, (on, g)  # (the host's eight-leaves rule, as before)
    same(got[0], got[1], "VOXELGRID")
    c.close()


# ---- 2. served with the same bits -------------------------------------------------------------------------------------------------------------------------
SCAN_CASES = [(f"{name}, distance filter {'on' if dist else 'off'}, k {k} x {s}", dict(p, enable_distance_filter=dist, statistical_mean_k=k, statistical_stddev=s))
              for name, p in CHAINS for dist in (True, False) for k, s in ((20, 1.0), (30, 1.2), (1, 0.5), (63, 2.0))]


@pytest.fixture(scope="module")
def scan_expected(quarter_scan):
    return {}


def expected_of(cache, which, cloud):
    if which not in cache:
        cache[which] = oracle_chain(cloud, SCAN_CASES[which][1])
    return cache[which]


@pytest.mark.parametrize("which", range(len(SCAN_CASES)), ids=[n for n, _ in SCAN_CASES])
def test_quarter_scan_is_served_with_the_same_bits(quarter_scan, scan_expected, ctx, which):
    """Route 1, anomaly 0 and the count slots; fast == slow == switch off == oracle; through mrgfe_prefilter, mrgfe_prefilter_device and
    mrgfe_scan_callback_records at point steps 16 and 32; what mrgfe_ctx_sor_grid_stats must say of the chosen grid."""
    import torch

    from mrg_slam_amd import prefilter_to_device, scan_callback_records

    name, p = SCAN_CASES[which]
    exp, counts, _, stage_in = expected_of(scan_expected, which, quarter_scan)
    assert len(quarter_scan) == 6488 and 0 < counts[2] < counts[1], (name, counts)
    fast, fs, gs, slow, ss, off, os_ = three_ways(quarter_scan, p, ctx)
    print(name, "counts", counts, "stats", fs, "grid", gs)
    assert fs["route"] == 1 and fs["anomaly"] == 0 and ss["route"] == 0 and os_["route"] == 0, (name, fs, ss, os_)
    same(fast, exp, name)
    same(slow, exp, name + " (host-driven)")
    same(off, exp, name + " (switch off)")
    check_counts(p, fs, counts, name)
    check_grid_stats(gs, DEFAULT_RULE, stage_in, name)
    buf = torch.empty((len(quarter_scan), 4), dtype=torch.float32, device="cuda:0")
    m = prefilter_to_device(quarter_scan, buf.data_ptr(), len(quarter_scan), p, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 1
    same(buf[:m].cpu().numpy(), exp, name + " (device)")
    data = memoryview(quarter_scan).cast("B")
    for step in (16, 32):
        rec = scan_callback_records(data, len(quarter_scan), 1, 16, FIELDS, step, None, 0, 0, None, PERIOD, None, p, ctx=ctx)
        st, eg = ctx.prefilter_stats(), ctx.egress_stats()
        assert st["route"] == 1 and eg["waits"] == 0 and not eg["direct"], (name, step, st, eg)  # (a statistical chain's records are staged)
        want = pack(exp, step)
        assert rec.shape == want.shape and np.array_equal(np.asarray(rec).view(np.uint32), want.view(np.uint32)), (name, step)


@pytest.mark.parametrize("which", range(3), ids=[n for n, _ in CHAINS])
def test_scan_callback_with_deskewing_and_a_transform(quarter_scan, ctx, which):
    from mrg_slam_amd import scan_callback, synth
    from mrg_slam_amd._lib import lib
    from oracle import oracle as orc

    name, p = CHAINS[which]
    T = synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32)
    c = orc.deskew(quarter_scan, ANG_V, PERIOD)
    c = orc.transform_points(T, np.ascontiguousarray(c))  # (every point of the synthetic scan is finite)
    exp, counts, _, stage_in = oracle_chain(c, p)
    data = memoryview(quarter_scan).cast("B")
    got = {}
    try:
        for mode in (1, 0):
            assert lib().mrgfe_dbg_set_prefilter_device_driven(mode) == mode
            got[mode] = scan_callback(data, len(quarter_scan), 1, 16, FIELDS, 0, ANG_V, PERIOD, T, p, ctx=ctx)
            st = ctx.prefilter_stats()
            assert st["route"] == mode and st["anomaly"] == 0, (name, st)
            if mode == 1:
                check_counts(p, st, counts, name)
                check_grid_stats(ctx.sor_grid_stats(), DEFAULT_RULE, stage_in, name)
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)
    assert len(exp) > 500
    same(got[1], got[0], name)
    same(got[1], exp, name)


# ---- 3. the result does not depend on the edge ---------------------------------------------------------------------------------------------------------
RULES = [(0.05, 1.5, 4), (0.3, 1.5, 4), (1.0, 1.5, 4), (8.0, 1.5, 4), (200.0, 1.5, 4), (200.0, 1e9, 4), (1.0, 1e9, 4), (0.3, 1.5, 0), (8.0, 1.5, 0), (200.0, 1.5, 0)]


@pytest.mark.parametrize("which", (0, 1), ids=[n for n, _ in CHAINS[:2]])
def test_the_result_does_not_depend_on_the_rule(quarter_scan, ctx, which):
    from mrg_slam_amd import prefilter

    name, p = CHAINS[which]
    exp, counts, _, stage_in = oracle_chain(quarter_scan, p)
    edges = []
    try:
        for rule in RULES:
            set_rule(rule)
            got = prefilter(quarter_scan, p, ctx=ctx)
            st, g = ctx.prefilter_stats(), ctx.sor_grid_stats()
            print(name, rule, g)
            assert st["route"] == 1 and st["anomaly"] == 0, (name, rule, st)
            same(got, exp, f"{name} {rule}")
            check_grid_stats(g, rule, stage_in, f"{name} {rule}", settled=False)
            if rule[1] >= 1e9 or rule[2] == 0:
                assert g["halvings"] == 0, (rule, g)
            if rule[0] == 200.0 and g["halvings"] == 0:
                assert g["cells"] == 1, (rule, g)
            edges.append(g["edge"])
    finally:
        set_rule(None)
    assert len(set(edges)) >= 3, edges
    got = prefilter(quarter_scan, p, ctx=ctx)  # the defaults again
    check_grid_stats(ctx.sor_grid_stats(), DEFAULT_RULE, stage_in, name)
    same(got, exp, name)


# ---- 4. the smallest shapes at which the kernels can go wrong ----------------------------------------------------------------------------------------------
K = 5


def uniform_cloud(n, seed=20261020, lo=-3.0, hi=3.0):
    rng = np.random.default_rng(seed + n)
    c = rng.uniform(lo, hi, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0.0, 255.0, n).astype(np.float32)
    return c


def shape_cases():
    rng = np.random.default_rng(99)
    cases = [(f"n={n}", uniform_cloud(n), {}) for n in (1, 2, K, K + 1, K + 2, 255, 256, 257, 2047, 2048, 2049, 4097)]
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.25) + np.float32(1.0)
    lattice = np.concatenate([g, np.linspace(0, 1, len(g), dtype=np.float32)[:, None]], 1)[rng.permutation(len(g))]
    cases.append(("12^3 lattice", lattice, {}))
    copies = uniform_cloud(300, seed=5)
    copies[rng.choice(300, 100, replace=False)] = np.array([1.25, -0.5, 0.75, 9.0], dtype=np.float32)
    cases.append(("100 copies of one point", copies, {}))
    one_cell = uniform_cloud(500, seed=6, lo=0.05, hi=0.45)
    one_cell[:, :3] += np.array([5.0, 5.0, 1.0], dtype=np.float32)
    cases.append(("one start cell", one_cell, {}))
    far = np.concatenate([uniform_cloud(200, seed=7), uniform_cloud(200, seed=8)])
    far[200:, 0] += np.float32(3000.0)
    cases.append(("two clusters 3 km apart", far, {"distance_far_thresh": 1e4}))
    mixed = uniform_cloud(1500, seed=9)
    bad = rng.choice(len(mixed), 90, replace=False)
    for j, i in enumerate(bad):
        mixed[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    mixed[bad[:5]] = np.nan
    cases.append(("NaN / inf rows, distance filter on", mixed, {}))
    cases.append(("nothing survives", uniform_cloud(300, seed=10), {"distance_near_thresh": 50.0, "distance_far_thresh": 60.0}))
    return cases


@pytest.mark.parametrize("down", ["NONE", "APPROX_VOXELGRID"])
def test_small_and_awkward_shapes(ctx, down):
    """mean_k = 5.  fast == slow == switch off == oracle, and the route is what the ORACLE's stage counts say: 2 only when nothing finite survives the
    distance filter, else 1 — any other hand-back fails."""
    cases = shape_cases()
    handed_back = 0
    for name, cloud, more in cases:
        p = params(downsample_method=down, downsample_resolution=0.1, statistical_mean_k=K, **more)
        what = f"{down} {name}"
        exp, counts, n_finite, stage_in = oracle_chain(cloud, p)
        fast, fs, gs, slow, ss, off, os_ = three_ways(cloud, p, ctx)
        print(f"{what}: {len(cloud)} -> {counts} route {fs['route']} anomaly {fs['anomaly']} grid {gs}")
        same(fast, exp, what)
        same(slow, exp, what + " (host-driven)")
        same(off, exp, what + " (switch off)")
        want = 2 if n_finite == 0 else 1
        assert fs["route"] == want and ss["route"] == 0 and os_["route"] == 0, (what, fs, counts)
        if want == 1:
            assert fs["anomaly"] == 0, (what, fs)
            check_counts(p, fs, counts, what)
            check_grid_stats(gs, DEFAULT_RULE, stage_in, what, settled=False)
            if counts[1] <= K:  # fewer points than neighbours + 1: no query is valid
                assert fs["counts"][3] == counts[1], (what, fs)
        else:
            assert fs["anomaly"] & 1 and not fs["anomaly"] & 256, (what, fs)
        handed_back += want == 2
    assert handed_back * 3 <= len(cases)


# ---- 5. hand-backs ------------------------------------------------------------------------------------------------------------------------------------------
def non_finite_cloud():
    rng = np.random.default_rng(77)
    c = uniform_cloud(3000, seed=9)
    bad = rng.choice(len(c), 120, replace=False)
    for j, i in enumerate(bad):
        c[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    c[bad[:6]] = np.nan
    return c


HAND_BACKS = ["nothing survives the distance filter", "non-finite rows, distance filter off", "grid beyond its table"]


@pytest.mark.parametrize("down", ["NONE", "APPROX_VOXELGRID"])
@pytest.mark.parametrize("name", HAND_BACKS)
def test_hand_backs_name_their_anomaly_and_give_the_same_output(quarter_scan, ctx, name, down):
    """Route 2, the anomaly bit, and the host-driven route's and the oracle's output."""
    from conftest import small_cloud

    from mrg_slam_amd import _lib

    rule = None
    if name == "nothing survives the distance filter":
        cloud, more, bit = quarter_scan, {"distance_near_thresh": 500.0, "distance_far_thresh": 600.0}, _lib.PF_ANOMALY_EMPTY
    elif name == "non-finite rows, distance filter off":
        cloud, more, bit = non_finite_cloud(), {"enable_distance_filter": False}, _lib.PF_ANOMALY_NON_FINITE
    else:
        # 3000 points in a cube of 30 km; start edge 0.05 m, no halving.  The start edge is doubled at most 8 times, to 12.8 m: 2344 cells per axis, 1.3e10
        # in all against a table of 2^24 - 1 — the box fits at no allowed edge.
        cloud, more, bit, rule = small_cloud(3000, 3, extent=(30000.0, 30000.0, 30000.0)), {"distance_far_thresh": 1e9}, _lib.PF_ANOMALY_CELLS, (0.05, 0.0, 0)
    p = params(downsample_method=down, downsample_resolution=0.1, **more)
    exp = oracle_chain(cloud, p)[0]
    try:
        set_rule(rule)
        fast, fs, gs, slow, ss, off, os_ = three_ways(cloud, p, ctx)
    finally:
        set_rule(None)
    print(name, down, fs, gs)
    assert fs["route"] == 2 and fs["anomaly"] & bit and ss["route"] == 0 and os_["route"] == 0, (name, fs, ss, os_)
    if bit != _lib.PF_ANOMALY_CELLS:
        assert not fs["anomaly"] & _lib.PF_ANOMALY_CELLS, (name, fs)  # (an empty or non-finite cloud is no grid beyond its table)
    same(fast, exp, name)
    same(slow, exp, name)
    same(off, exp, name)
    if bit == _lib.PF_ANOMALY_CELLS:
        assert gs["sized"] and gs["cells"] == 1 and gs["start_edge"] == float(np.float32(0.05) * np.float32(256.0)), gs


def test_mean_k_beyond_a_wavefront_s_list_stays_host_driven(quarter_scan, ctx):
    from mrg_slam_amd import MrgfeError, _lib, prefilter

    outcome = []
    for mode in (1, 0):
        try:
            _lib.lib().mrgfe_dbg_set_prefilter_device_driven(mode)
            try:
                outcome.append(("ok", prefilter(quarter_scan, params(statistical_mean_k=64), ctx=ctx).tobytes()))
            except MrgfeError as e:
                outcome.append(("error", e.status))
            assert ctx.prefilter_stats()["route"] == 0 and not ctx.sor_grid_stats()["sized"]
        finally:
            _lib.lib().mrgfe_dbg_set_prefilter_device_driven(1)
    assert outcome[0] == outcome[1]


# ---- 6. hand-over to the registration -----------------------------------------------------------------------------------------------------------------------
def remembered(ctx):
    from mrg_slam_amd._lib import lib

    flag, n, box = C.c_int(-1), C.c_size_t(0), np.zeros(6, dtype=np.float32)
    assert lib().mrgfe_dbg_prefilter_output(ctx._h, C.byref(flag), C.byref(n), box.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return bool(flag.value), n.value, box


def test_registration_takes_the_scan_over_with_the_chain_s_box(ctx):
    """mrgfe_scan_callback_device with APPROX_VOXELGRID + STATISTICAL on the switched context, then setInputSourceFromPrefilter (the source's search grid on
    the box the chain reported) against setInputSourceDevice on the same buffer."""
    import torch

    from mrg_slam_amd import GicpHip, prefilter, scan_callback_to_device, synth

    scene = synth.street_scene()
    tgt_raw, src_raw, rel = synth.scan_pair(0, "VLP16", scene)
    p = params(downsample_method="APPROX_VOXELGRID", downsample_resolution=0.25)
    tgt = prefilter(tgt_raw, p, ctx=ctx)
    guess = synth.warm_guess(rel, 0)
    buf = torch.empty((len(src_raw), 4), dtype=torch.float32, device="cuda:0")
    data = memoryview(np.ascontiguousarray(src_raw)).cast("B")
    res = {}
    for how in ("from_prefilter", "device"):
        reg = GicpHip(transformation_epsilon=0.01, ctx=ctx)
        reg.setInputTarget(tgt)
        m = scan_callback_to_device(data, len(src_raw), 1, 16, FIELDS, buf.data_ptr(), buf.shape[0], 0, None, PERIOD, None, p, ctx=ctx)
        assert ctx.prefilter_stats()["route"] == 1 and ctx.sor_grid_stats()["sized"] and m > 1000 and remembered(ctx)[:2] == (True, m)
        if how == "from_prefilter":
            reg.setInputSourceFromPrefilter(buf.data_ptr(), m)
        else:
            ctx.synchronize()
            reg.setInputSourceDevice(buf.data_ptr(), m)
        reg.align(guess)
        res[how] = (reg.getFinalTransformation().copy(), reg.hasConverged(), reg.getFinalNumIteration())
    np.testing.assert_array_equal(res["from_prefilter"][0], res["device"][0])
    assert res["from_prefilter"][1:] == res["device"][1:] and res["device"][2] >= 1
