"""CPU: the oracle's grid searches and prefilters held to the brute-force model of tests/grid_cases.py, bit for bit, on the placements that move
the grid layer off its comfortable inputs — coordinates kilometres from the origin, lattices whose points lie on cell faces, a dense blob with a
few points 2e5 m away (the 2^24-cell cap), a cloud inside one cell.  The oracle's searches are themselves a uniform grid with ring termination
(oracle/nn.h), so "kernel equals oracle" (tests/test_gpu_*.py) says nothing about a defect both grids share: here the oracle meets numpy, in
tests/test_gpu_grid_placements.py the kernels do."""
import numpy as np
import pytest

import grid_cases as G
from oracle import oracle as orc


@pytest.mark.parametrize("name", G.ORACLE_SEARCH)
def test_knn_and_nearest(name):
    cloud, q = G.placement(name)
    fin = G.finite_rows(q)
    for k in G.KNN_K:
        idx, sqd = orc.knn(cloud, q, k)
        exp_i, exp_d = G.knn(cloud, q, k)
        np.testing.assert_array_equal(idx, exp_i, err_msg=f"k={k}")
        np.testing.assert_array_equal(sqd, exp_d, err_msg=f"k={k}")
    bi, bd = orc.nn1_brute(cloud, q)
    exp_i, exp_d = G.nn1(cloud, q)
    np.testing.assert_array_equal(bi, exp_i)
    np.testing.assert_array_equal(bd[fin], exp_d[fin])
    assert (bi[~fin] == -1).all() and fin.sum() == len(q) - 2


@pytest.mark.parametrize("radius,min_nb", G.RADIUS_PARAMS)
@pytest.mark.parametrize("name", G.ORACLE_SEARCH)
def test_radius_outlier(name, radius, min_nb):
    cloud, _ = G.placement(name)
    out, keep = orc.radius_outlier(cloud, radius, min_nb)
    exp, exp_keep = G.radius_outlier(cloud, radius, min_nb)
    np.testing.assert_array_equal(keep, exp_keep)
    np.testing.assert_array_equal(out, exp)


@pytest.mark.parametrize("mean_k,mul", G.STATISTICAL_PARAMS)
@pytest.mark.parametrize("name", G.SEARCH)
def test_statistical_outlier(name, mean_k, mul):
    """The precondition of every StatisticalOutlierRemoval case (needle included: the GPU test uses it): no mean distance within 1e-9 relative of
    the threshold, so the order of the sums cannot decide a point; then the oracle against the model."""
    cloud, _ = G.placement(name)
    margin = G.statistical_margin(cloud, mean_k, mul)
    print(f"{name} mean_k {mean_k} stddev_mul {mul}: nearest mean distance to the threshold, relative {margin:.3g}")
    assert margin > G.STATISTICAL_MARGIN, "a mean distance lies on the threshold: change the placement's seed"
    if name not in G.ORACLE_SEARCH:
        return
    out, keep = orc.statistical_outlier(cloud, mean_k, mul)
    exp, exp_keep, _, _ = G.statistical_outlier(cloud, mean_k, mul)
    np.testing.assert_array_equal(keep, exp_keep)
    np.testing.assert_array_equal(out, exp)


@pytest.mark.parametrize("name", G.VOXEL)
def test_voxel_grids(name):
    cloud, _ = G.placement(name)
    for leaf in G.LEAVES:
        for min_pts in G.MIN_POINTS:
            out, status = orc.voxelgrid(cloud, leaf, min_pts, orc.ORDER_STABLE)
            exp, overflow = G.voxelgrid(cloud, leaf, min_pts)
            assert status == int(overflow) and overflow == (name == "cross"), (leaf, min_pts)
            np.testing.assert_array_equal(out, exp, err_msg=f"leaf {leaf} min_points {min_pts}")
        np.testing.assert_array_equal(orc.approx_voxelgrid(cloud, leaf), G.approx_voxelgrid(cloud, leaf), err_msg=f"approximate, leaf {leaf}")


@pytest.mark.parametrize("name", G.FULL)
def test_fitness_score(name):
    from mrg_slam_amd import synth

    cloud, q = G.placement(name)
    rel = synth.make_pose([0.05, -0.02, 0.01], synth.rot_xyz(0.001, 0.002, -0.003))
    for T in (np.eye(4), rel):
        for max_range in (float("inf"), 0.01):
            assert orc.calc_fitness_score(cloud, q, T, max_range) == pytest.approx(G.fitness(cloud, q, T, max_range), rel=1e-12)
    np.testing.assert_array_equal(orc.transform_points(rel, q)[G.finite_rows(q)], G.transform(rel, q)[G.finite_rows(q)])


@pytest.mark.parametrize("method", G.CHAIN_DOWNSAMPLE)
@pytest.mark.parametrize("name", G.FULL)
def test_prefilter_chain(name, method):
    """The three stages composed, as the GPU test runs them fused: the oracle's calls against the model's, and the statistical precondition on the
    clouds the outlier stage actually sees (the downsampled ones)."""
    cloud, _ = G.placement(name)
    c = orc.distance_filter(cloud, G.CHAIN_NEAR, G.CHAIN_FAR)
    if method == "VOXELGRID":
        c, _ = orc.voxelgrid(c, G.CHAIN_LEAF, 1)
    elif method == "APPROX_VOXELGRID":
        c = orc.approx_voxelgrid(c, G.CHAIN_LEAF)
    m = G.chain_downsampled(name, method)
    np.testing.assert_array_equal(c, m)
    for outlier, mean_k in G.CHAIN_OUTLIER:
        if outlier == "RADIUS":
            got, _ = orc.radius_outlier(c, 0.5, 2)
        elif outlier == "STATISTICAL":
            margin = G.statistical_margin(m, mean_k, G.CHAIN_STDDEV)
            print(f"{name} {method} mean_k {mean_k}: {len(m)} points, nearest mean distance to the threshold, relative {margin:.3g}")
            assert margin > G.STATISTICAL_MARGIN, "a mean distance lies on the threshold: change the placement's seed"
            got, _ = orc.statistical_outlier(c, mean_k, G.CHAIN_STDDEV)
        else:
            got = c
        np.testing.assert_array_equal(got, G.outlier_removal(m, outlier, mean_k=mean_k, stddev_mul=G.CHAIN_STDDEV), err_msg=f"{outlier} {mean_k}")


def test_placements_keep_the_voxel_keys_sensitive():
    """Points whose voxel changes between the float product floor(x * inverse_leaf) and double arithmetic: what a kernel that divides, or contracts
    the product into an FMA, would get wrong.  Recorded for every placement; the two the voxel tests lean on must keep at least 1000 of 3000."""
    counts = {}
    for name in G.VOXEL:
        cloud, _ = G.placement(name)
        counts[name] = {leaf: G.voxel_changes(cloud, leaf) for leaf in G.LEAVES}
        print(name, counts[name])
        assert counts[name][0.5] == 0  # a power of two: the product is exact
    assert counts["offset_utm"][0.37] >= 1000
    assert counts["lattice_leaf_0.1"][0.1] >= 1000


def test_placements_are_what_they_say():
    for name in G.SEARCH + G.LATTICE_LEAVES:
        cloud, q = G.placement(name)
        again = G._PLACEMENTS[name]()
        np.testing.assert_array_equal(cloud, again[0])
        np.testing.assert_array_equal(q, again[1])
        extra = {"cross": (6, 9), "needle": (1, 2)}.get(name, (0, 0))
        assert len(cloud) == G.N_TARGET + extra[0] and len(q) == G.N_QUERY + extra[1]
        assert (~G.finite_rows(cloud)).sum() == G.N_BAD_ROWS and (~G.finite_rows(q)).sum() == 2
        assert not cloud.flags.writeable and not q.flags.writeable
    cloud, _ = G.placement("lattice_0.5")
    assert len(np.unique(cloud[G.finite_rows(cloud), :3], axis=0)) <= 2000  # a third of the points are duplicates
    cloud, _ = G.placement("offset_utm")
    assert np.spacing(cloud[0, 1]) == 0.5 and np.spacing(cloud[0, 0]) == np.float32(0.03125)
