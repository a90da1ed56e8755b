"""GPU: the grid searches and the prefilters held to brute force off the origin.

Everything here is compared with the numpy model of tests/grid_cases.py — a full sort of all squared distances, dictionaries for the voxel grids —
and not with the oracle, whose searches are a uniform grid like the kernels' (tests/test_grid_placements_cpu.py holds the oracle to the same model).
The placements move the binning slack, the float cell of a query, the 2^24-cell cap and the float voxel keys away from the values every other test of
csrc/nn_grid.hip, nn_device.h, cellsort.hip and csrc/filters.hip leaves them at.  Every comparison is bit for bit; the fitness score alone is
compared at 1e-12 relative (a double sum whose order is the kernel's own), the tolerance tests/test_gpu_filters.py holds it to."""
import numpy as np
import pytest

import grid_cases as G
from conftest import small_cloud

pytestmark = pytest.mark.gpu


class _Models:
    """The model's answers, computed once per (placement, case) and shared by the tests of this module."""

    def __init__(self):
        self._memo = {}

    def get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def knn(self, name, k):
        return self.get(("knn", name, k), lambda: G.knn(*G.placement(name), k))


@pytest.fixture(scope="module")
def model():
    return _Models()


def _lib():
    from mrg_slam_amd._lib import lib

    return lib()


def _pose():
    from mrg_slam_amd import synth

    return synth.make_pose([0.05, -0.02, 0.01], synth.rot_xyz(0.001, 0.002, -0.003))


@pytest.mark.parametrize("name", G.SEARCH)
def test_nearest_neighbour(model, name):
    """reg.nearestKSearch1 (the occupancy-pyramid 1-NN search, one grid level): index and squared distance of the full scan, ties to the lowest index;
    a non-finite query has no neighbour."""
    from mrg_slam_amd import NdtHip

    cloud, q = G.placement(name)
    reg = NdtHip()
    reg.setInputTarget(cloud)  # (cross: the NDT voxels overflow and the registration says so; its search grid does not depend on them)
    idx, sqd = reg.nearestKSearch1(q)
    exp_i, exp_d = model.get(("nn1", name), lambda: G.nn1(cloud, q))
    fin = G.finite_rows(q)
    np.testing.assert_array_equal(idx, exp_i)
    np.testing.assert_array_equal(sqd[fin], exp_d[fin])
    assert (idx[~fin] == -1).all()


@pytest.mark.parametrize("sweep", [1, 0])
@pytest.mark.parametrize("name", G.FULL)
def test_fitness_and_matching_status(model, name, sweep):
    """calc_fitness_score under the identity and a small rigid pose, with the seed + sweep pass on and off, and the matching status of a fresh
    registration (identity final transformation): the mean of the brute-force distances; the inlier count is strict."""
    from mrg_slam_amd import NdtHip, calc_fitness_score

    cloud, q = G.placement(name)
    before = _lib().mrgfe_dbg_set_fit_sweep(-1)
    try:
        assert _lib().mrgfe_dbg_set_fit_sweep(sweep) == sweep
        for tag, T in (("identity", np.eye(4)), ("pose", _pose())):
            for max_range in G.MAX_RANGES:
                exp = model.get(("fitness", name, tag, max_range), lambda: G.fitness(cloud, q, T, max_range))
                got = calc_fitness_score(cloud, q, T, max_range)
                print(f"{name} sweep {sweep} {tag} max_range {max_range}: {got!r} model {exp!r}")
                assert got == pytest.approx(exp, rel=1e-12), (tag, max_range)
        reg = NdtHip()
        reg.setInputTarget(cloud)
        reg.setInputSource(q)
        for dist in (0.5, 0.05):
            err, inliers, fraction = model.get(("status", name, dist), lambda: G.matching_status(cloud, q, dist))
            st = reg.matchingStatus(dist)
            print(f"{name} sweep {sweep} dist {dist}: error {st.matching_error!r} / {err!r}, inliers {st.num_inliers} / {inliers}")
            assert st.matching_error == pytest.approx(err, rel=1e-12)
            assert (st.n_points, st.num_inliers) == (len(q), inliers)
            assert np.float32(st.inlier_fraction).tobytes() == np.float32(fraction).tobytes()
    finally:
        _lib().mrgfe_dbg_set_fit_sweep(before)


@pytest.mark.parametrize("k", [5, 20, 64, 65, 256])
@pytest.mark.parametrize("name", G.SEARCH)
def test_knn(model, name, k):
    """filters.knn, k <= 64 on the narrow kernel and 65, 256 on the wide one: the full sort by (distance, index), -1 where nothing is left."""
    from mrg_slam_amd import knn

    cloud, q = G.placement(name)
    idx, sqd = knn(cloud, q, k)
    exp_i, exp_d = model.knn(name, k)
    np.testing.assert_array_equal(idx, exp_i)
    np.testing.assert_array_equal(sqd, exp_d)


SET_SHIFT = np.array([12.5, -7.25, 3.0, 0.0], dtype=np.float32)


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("name", G.SEARCH)
def test_grid_set(model, name, k, rounds):
    """Grids over [the placement, a small cloud at the origin, an empty cloud, the placement at another offset] built together (NnGridSet), the third
    build from the cell-edge hints of the first two; the placement's queries against each.  k = 1 is the 1-NN search, k = 20 the k-NN climb."""
    from mrg_slam_amd.filters import grid_set_query

    cloud, q = G.placement(name)
    members = [cloud, small_cloud(500), np.zeros((0, 4), np.float32), cloud + SET_SHIFT]
    idx, sqd = grid_set_query(members, q, k, rounds)
    fin = G.finite_rows(q)
    for m, t in enumerate(members):
        exp_i, exp_d = model.get(("set", name, m, k), lambda: G.knn(t, q, k))
        np.testing.assert_array_equal(idx[m], exp_i, err_msg=f"member {m}")
        if k == 1:  # (the 1-NN search leaves the distance of a query without a neighbour undefined)
            found = exp_i[:, 0] >= 0
            np.testing.assert_array_equal(sqd[m][found], exp_d[found], err_msg=f"member {m}")
        else:
            np.testing.assert_array_equal(sqd[m], exp_d, err_msg=f"member {m}")
    assert (idx[:, ~fin] == -1).all() and (idx[2] == -1).all()


@pytest.mark.parametrize("radius,min_nb", G.RADIUS_PARAMS)
@pytest.mark.parametrize("name", G.SEARCH)
def test_radius_outlier(model, name, radius, min_nb):
    from mrg_slam_amd import RadiusOutlierRemoval

    cloud, _ = G.placement(name)
    ro = RadiusOutlierRemoval()
    ro.setRadiusSearch(radius)
    ro.setMinNeighborsInRadius(min_nb)
    ro.setInputCloud(cloud)
    exp, _ = model.get(("radius", name, radius, min_nb), lambda: G.radius_outlier(cloud, radius, min_nb))
    np.testing.assert_array_equal(ro.filter(), exp)


@pytest.mark.parametrize("mean_k,mul", G.STATISTICAL_PARAMS)
@pytest.mark.parametrize("name", G.SEARCH)
def test_statistical_outlier(model, name, mean_k, mul):
    """mean_k 10 and 30 on the narrow k-NN kernel, 100 on the wide one.  (tests/test_grid_placements_cpu.py asserts that no mean distance lies on
    the threshold, so the order of the kernel's sums cannot decide a point.)"""
    from mrg_slam_amd import StatisticalOutlierRemoval

    cloud, _ = G.placement(name)
    so = StatisticalOutlierRemoval()
    so.setMeanK(mean_k)
    so.setStddevMulThresh(mul)
    so.setInputCloud(cloud)
    exp = model.get(("statistical", name, mean_k, mul), lambda: G.statistical_outlier(cloud, mean_k, mul)[0])
    np.testing.assert_array_equal(so.filter(), exp)


@pytest.mark.parametrize("leaf", G.LEAVES)
@pytest.mark.parametrize("name", G.VOXEL)
def test_voxelgrid(model, name, leaf):
    """pcl::VoxelGrid: the model's dictionary and the oracle's stable order, voxel for voxel.  Only the cross overflows PCL's int32 index test (its
    2e5 m arms at any of these leaves) and is passed through."""
    from mrg_slam_amd import VoxelGrid
    from oracle import oracle as orc

    cloud, _ = G.placement(name)
    for min_pts in G.MIN_POINTS:
        vg = VoxelGrid()
        vg.setLeafSize(leaf, leaf, leaf)
        vg.setMinimumPointsNumberPerVoxel(min_pts)
        vg.setInputCloud(cloud)
        out = vg.filter()
        exp, overflow = model.get(("voxelgrid", name, leaf, min_pts), lambda: G.voxelgrid(cloud, leaf, min_pts))
        assert overflow == (name == "cross")
        assert vg.overflow == overflow, (leaf, min_pts)
        np.testing.assert_array_equal(out, exp, err_msg=f"min_points {min_pts}")
        o_exp, o_status = orc.voxelgrid(cloud, leaf, min_pts, orc.ORDER_STABLE)
        assert o_status == int(overflow)
        np.testing.assert_array_equal(out, o_exp, err_msg=f"min_points {min_pts} (oracle)")


@pytest.mark.parametrize("leaf", G.LEAVES)
@pytest.mark.parametrize("name", G.VOXEL)
def test_approx_voxelgrid(model, name, leaf):
    from mrg_slam_amd import ApproximateVoxelGrid

    cloud, _ = G.placement(name)
    f = ApproximateVoxelGrid()
    f.setLeafSize(leaf, leaf, leaf)
    f.setInputCloud(cloud)
    got = f.filter()
    exp = model.get(("approx", name, leaf), lambda: G.approx_voxelgrid(cloud, leaf))
    assert got.shape == exp.shape
    np.testing.assert_array_equal(got, exp)  # (NaN centroids of the cells the non-finite rows fall into compare equal)


@pytest.mark.parametrize("outlier,mean_k", G.CHAIN_OUTLIER)
@pytest.mark.parametrize("downsample", G.CHAIN_DOWNSAMPLE)
@pytest.mark.parametrize("name", G.FULL)
def test_fused_prefilter_chain(model, name, downsample, outlier, mean_k):
    """mrgfe_prefilter, device-driven and host-driven: both equal the model's three calls composed.  Which route served a case is not asserted (on the
    cross the device-driven grid is expected to hand the case back); only the output is."""
    from mrg_slam_amd import prefilter

    cloud, _ = G.placement(name)
    p = {"distance_near_thresh": G.CHAIN_NEAR, "distance_far_thresh": G.CHAIN_FAR, "downsample_method": downsample, "downsample_resolution": G.CHAIN_LEAF,
         "downsample_min_points_per_voxel": 1, "outlier_removal_method": outlier, "radius_radius": 0.5, "radius_min_neighbors": 2,
         "statistical_mean_k": mean_k, "statistical_stddev": G.CHAIN_STDDEV}
    exp = model.get(("chain", name, downsample, outlier, mean_k),
                    lambda: G.outlier_removal(G.chain_downsampled(name, downsample), outlier, mean_k=mean_k, stddev_mul=G.CHAIN_STDDEV))
    try:
        assert _lib().mrgfe_dbg_set_prefilter_device_driven(1) == 1
        fast = prefilter(cloud, p)
        assert _lib().mrgfe_dbg_set_prefilter_device_driven(0) == 0
        slow = prefilter(cloud, p)
    finally:
        _lib().mrgfe_dbg_set_prefilter_device_driven(1)
    np.testing.assert_array_equal(fast, exp, err_msg="device-driven")
    np.testing.assert_array_equal(slow, exp, err_msg="host-driven")
