"""CPU: the oracle's NDT target build (oracle/ndt.cpp VoxelGridCovariance, under pclomp's and PCL 1.12's validity rule) against the independent
numpy model tests/ndt_leaves_model.py, on constructed scenes — one voxel per kind (regular, thin plane, exact axis-aligned plane, exact oblique
line, duplicates) and size (5, 6, 7, 30, 200 points) — at leaf sizes 1.0, 0.5, 0.37 (not a float), 2.0 and cloud origins (0, 0, 0),
(-37.3, 12.9, -2.2), (2500, -1800, 40).

TOLERANCES.  Keys, counts and grid bounds are exact.  Means and inverse covariances are held to the reference's OWN error, measured on the reference
alone (ndt_leaves_model.tolerances, computed per case when the test runs): the single-pass formula (sum xx^T - 2 sum x mean^T) / n + mean mean^T in
plain numpy float64 with the sums in point order, through the same eigh / floor / inverse, against the centred two-pass longdouble model; worst
relative deviation (max |difference| / max |entry| per leaf) over the scene, times 8 (the eigen-solver's and the 3 x 3 inverse's operation order
differ), floored at 1e-12.  The single pass loses eps |mean|^2 / lambda_max, so the figure grows with the distance from the origin and shrinks with
the leaf size.  Measured (regular and thin leaves | accepted rank-deficient leaves; the oracle's own deviation from the model beside it):

    leaf   origin (0,0,0)            (-37.3, 12.9, -2.2)         (2500, -1800, 40)
    1.0    2.8e-12 | 3.2e-12         5.6e-11 | 1.9e-11           3.5e-7 | 1.6e-7
    0.5    4.0e-12 | 4.2e-12         3.2e-10 | 1.6e-10           1.7e-6 | 9.8e-7
    0.37   2.5e-12 | 3.5e-12         4.4e-10 | 3.2e-10           2.2e-6 | 1.9e-6
    2.0    3.4e-12 | 2.2e-12         9.0e-12 | 5.2e-12           8.6e-8 | 5.5e-8

the oracle's regular / thin leaves deviate from the model by the same figures to two digits (it IS that single pass), so the margin is the factor 8.
Means: the reference's sequential float64 sum over n equals the longdouble mean rounded to float64 in every case (measured 0): the floor, 1e-12.

The f32 packing of the inverse covariance (NdtLeafRec::icov) is exposed by neither library (both hand out the f64 values): it is held through the
float-path derivatives of tests/test_oracle_ndt.py / tests/test_gpu_ndt.py with leaves from this model.

CLASS OUTCOMES UNDER THE PCL RULE (test_class_outcomes_under_the_pcl_rule): a rank-deficient leaf MUST be accepted and a `point` leaf rejected.
PCL 1.12's literal rule (eigenvalues down to -1e-12 pass, lambda_max > 0) does not give that: its bound is ABSOLUTE while the rounding noise of the
single-pass covariance is eps |mean|^2.  Measured on the oracle with the literal rule (accepted of 20 rank-deficient leaves | accepted of 4 `point`
leaves, per origin):
    leaf 1.0: 20 1 | 18 0 | 13 0     0.5: 20 1 | 20 0 | 10 0     0.37: 20 1 | 19 0 | 9 0     2.0: 20 0 | 20 0 | 13 0
— away from the origin it drops the planar voxels it was written to keep, and at the origin it keeps a voxel of identical points (covariance pure
noise, inverse 1e17).  Oracle and kernels shared that; both now take the noise level 4 eps max_r(sum x_r^2) into the rule on the PCL path
(oracle/quirks.h kPclVgcEigenNoiseMult, csrc/ndt_types.h; 1.5 eps max_r(sum x_r^2) bounds the noise of n sequentially added terms in a 3 x 3
spectral norm): the smaller eigenvalues may go down to -max(1e-12, noise), the largest must exceed the noise.  Over eight seeds of every scene
the single-pass noise reaches 0.033 of that bound on rank-deficient leaves and 0.018 on `point` leaves.  pclomp's rule is untouched.
"""
import numpy as np
import pytest

import ndt_leaves_model as M
from ndt_leaves_checks import ORIGIN_IDS, ORIGINS, RESOLUTIONS, case, check_leaves_against_model, check_pcl_rule_outcomes, check_scene_is_live
from oracle import oracle as orc


@pytest.mark.parametrize("origin", ORIGINS, ids=ORIGIN_IDS)
@pytest.mark.parametrize("res", RESOLUTIONS)
@pytest.mark.parametrize("which", ["Ndt", "PclNdt"])
def test_oracle_leaves_match_the_model(which, res, origin):
    cloud, model, tol = case(res, origin)
    check_scene_is_live(model)
    o = getattr(orc, which)(resolution=res)
    assert o.setInputTarget(cloud) == 0
    if which == "Ndt":
        keys, npts, mean, _, icov = o.leaves()
        acc = check_leaves_against_model(model, tol, keys, npts, mean, icov, grid=o.grid())
        rd = model.cls == "rank_deficient"
        assert 0 < acc[rd].sum() < rd.sum()  # rounding decides: both outcomes occur, the case is live
    else:
        keys, npts, ins, mean, icov, cent = o.leaves()
        check_leaves_against_model(model, tol, keys, npts, mean, icov, pcl_rule=True)
        np.testing.assert_array_equal(ins != 0, model.n >= M.MIN_POINTS)  # the radius search holds every leaf that reached 6 points
        np.testing.assert_array_equal(cent[:, :3], model.centroid)        # ... by its FLOAT centroid


@pytest.mark.parametrize("origin", ORIGINS, ids=ORIGIN_IDS)
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_class_outcomes_under_the_pcl_rule(res, origin):
    """see the module docstring: every exactly planar or collinear voxel lives, every voxel of identical points is dropped, at every origin"""
    cloud, model, _ = case(res, origin)
    o = orc.PclNdt(resolution=res)
    assert o.setInputTarget(cloud) == 0
    check_pcl_rule_outcomes(model, o.leaves()[1])


@pytest.mark.parametrize("res", [0.1, 0.37, 0.7])
def test_cell_index_follows_the_float_rule(res):
    """points on and next to cell faces, both signs: at least 20 of them lie in another cell by PCL's float rule than by exact arithmetic, and the
    library puts every one where the float rule says — keys, counts and the means (which pin the membership) equal the float-rule model's, and
    differ from what the exact cells would give"""
    cloud = M.face_cloud(res)
    fl, ex = M.cell_of(cloud[:, :3], res)
    differ = (fl != ex).any(1)
    print(f"leaf {res}: {differ.sum()} of {len(cloud)} points change cell under the float rule")
    assert differ.sum() >= 20
    assert (cloud[differ, :2] > 0).any() and (cloud[differ, :2] < 0).any()
    model = M.build(cloud, res)
    o = orc.Ndt(resolution=res)
    assert o.setInputTarget(cloud) == 0
    keys, npts, mean, _, _ = o.leaves()
    np.testing.assert_array_equal(keys, model.keys)
    np.testing.assert_array_equal(np.where(npts < 0, model.n, npts), model.n)
    for a, b in zip(o.grid(), model.grid):
        np.testing.assert_array_equal(a, b)
    assert M.rel_dev(mean, model.mean).max() <= 1e-12
    # every point that differs sits in the leaf of its float-rule cell: that leaf's count and mean are the model's, and the exact-rule key is another
    min_b, _, div_b = model.grid
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], dtype=np.int64)
    key_exact = (ex - min_b) @ mul
    assert (key_exact[differ] != model.point_key[differ]).all()
    exact_hist = dict(zip(*np.unique(key_exact, return_counts=True)))
    lib_hist = dict(zip(keys.tolist(), np.where(npts < 0, model.n, npts).tolist()))
    assert exact_hist != lib_hist
