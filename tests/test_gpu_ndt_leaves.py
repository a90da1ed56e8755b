"""GPU: the NDT target build of the HIP kernels (ndt_leaf_sums_kernel, ndt_leaf_finalize_kernel: single-pass covariance, dl_sym_eig3, eigenvalue floor
and V D V^-1 rebuild, rejection rule, lookup insertion) against the independent numpy model tests/ndt_leaves_model.py AND, bit for bit, against the
CPU oracle — on the constructed scenes of tests/test_ndt_leaves_cpu.py: regular, thin, exactly planar, exactly collinear and single-point voxels of
5 ... 200 points, leaf sizes 1.0, 0.5, 0.37, 2.0, origins (0, 0, 0), (-37.3, 12.9, -2.2), (2500, -1800, 40), the dense and the hashed lookup
(MRGFE_FORCE_HASH), the first build of an object and the rebuild of its later setInputTarget calls (NdtEngine::build_targets, one host wait).

Tolerances against the model: those of tests/test_ndt_leaves_cpu.py (its docstring has the figures: the single-pass formula in numpy float64 against
the centred longdouble model, times 8, floor 1e-12).  Against the oracle: none, every key, count, mean and inverse covariance bit for bit — with
nr_points == -1 on exactly the same leaves.  The rank-deficient voxels (at least 8 per scene, of which the oracle accepts some and rejects some at every
leaf size and origin: asserted) are what makes that new: whether such a leaf lives is the sign of an eigenvalue near 1e-16, so it needs every f64
operation of the sums, the covariance and the eigen-solver to round as the oracle's.

test_class_outcomes_under_the_pcl_rule_on_the_device is the device twin of the CPU test of that name (the rounding noise of the single-pass covariance
is part of the PCL path's rule: csrc/ndt_types.h kPclVgcEigenNoiseMult).

A rejected leaf must also be absent from scoring (test_rejected_leaves_are_absent_from_scoring): tolerances as in tests/ndt_model_cases.py."""
import numpy as np
import pytest

import ndt_leaves_model as M
from ndt_leaves_checks import ORIGIN_IDS, ORIGINS, RESOLUTIONS, case, check_leaves_against_model, check_pcl_rule_outcomes, check_scene_is_live

pytestmark = pytest.mark.gpu


def _oracle_leaves(which, res, cloud):
    from oracle import oracle as orc

    o = (orc.PclNdt if which == "PclNdtHip" else orc.Ndt)(resolution=res)
    assert o.setInputTarget(cloud) == 0
    lv = o.leaves()
    return (lv[0], lv[1], lv[3], lv[4]) if which == "PclNdtHip" else (lv[0], lv[1], lv[2], lv[4])


def _check(which, g, res, origin, seed=0):
    cloud, model, tol = case(res, origin, seed)
    check_scene_is_live(model)
    keys, npts, mean, icov = g.leaves()
    pcl = which == "PclNdtHip"
    check_leaves_against_model(model, tol, keys, npts, mean, icov, grid=g.grid(), pcl_rule=pcl)
    ok, on, om, oi = _oracle_leaves(which, res, cloud)
    np.testing.assert_array_equal(keys, ok)
    np.testing.assert_array_equal(npts, on)  # nr_points == -1 on exactly the same leaves
    np.testing.assert_array_equal(mean, om)
    np.testing.assert_array_equal(icov, oi)
    if not pcl:
        rd = model.cls == "rank_deficient"
        acc = on[rd] >= M.MIN_POINTS
        assert rd.sum() >= 8 and 0 < acc.sum() < rd.sum()  # the oracle accepts some and rejects some: the bit equality above is live


@pytest.mark.parametrize("origin", ORIGINS, ids=ORIGIN_IDS)
@pytest.mark.parametrize("res", RESOLUTIONS)
@pytest.mark.parametrize("force_hash", ["0", "1"])
@pytest.mark.parametrize("which", ["NdtHip", "PclNdtHip"])
def test_kernel_leaves_match_the_model_and_the_oracle(which, force_hash, res, origin, monkeypatch):
    import mrg_slam_amd

    monkeypatch.setenv("MRGFE_FORCE_HASH", force_hash)
    g = getattr(mrg_slam_amd, which)(resolution=res)
    cloud = case(res, origin)[0]
    assert g.setInputTarget(cloud) == 0  # the first build of the object
    _check(which, g, res, origin)
    other = case(res, origin, 1)[0]
    assert g.setInputTarget(other) == 0  # a later build: the voxel parameters are made on the device, one host wait
    _check(which, g, res, origin, 1)
    assert g.setInputTarget(cloud) == 0
    _check(which, g, res, origin)


@pytest.mark.parametrize("origin", ORIGINS, ids=ORIGIN_IDS)
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_class_outcomes_under_the_pcl_rule_on_the_device(res, origin):
    """see tests/test_ndt_leaves_cpu.py: every exactly planar or collinear voxel lives, every voxel of identical points is dropped, at every origin"""
    from mrg_slam_amd import PclNdtHip

    cloud, model, _ = case(res, origin)
    g = PclNdtHip(resolution=res)
    assert g.setInputTarget(cloud) == 0
    check_pcl_rule_outcomes(model, g.leaves()[1])


@pytest.mark.parametrize("search", ["DIRECT1", "DIRECT7"])
@pytest.mark.parametrize("res,origin", [(0.5, ORIGINS[1]), (0.37, ORIGINS[0])], ids=["0.5-near", "0.37-origin"])
def test_rejected_leaves_are_absent_from_scoring(res, origin, search):
    """source points inside `point`, `few` and rejected rank-deficient voxels (the voxels' own points: right on the distribution a wrongly kept leaf
    would hold) score exactly zero, gradient and Hessian too, float path and f64 Hessian pass; mixed with points of accepted voxels the result is the
    first-principles model's over the MODEL's leaves with those leaves removed — score 2e-6, float-path gradient and Hessian 1e-4 of the largest
    entry, f64 Hessian 1e-11 + leaf bound * max ||C|| ||q||^2 as in tests/ndt_model_cases.py (the leaf bound is the larger of the scene's two)."""
    import ndt_analytic
    from mrg_slam_amd import NdtHip
    from oracle import oracle as orc

    cloud, model, tol = case(res, origin)
    g = NdtHip(resolution=res, search=search)
    assert g.setInputTarget(cloud) == 0
    keys, npts, _, _ = g.leaves()
    np.testing.assert_array_equal(keys, model.keys)
    acc = npts >= M.MIN_POINTS
    gone = np.isin(model.cls, ("point", "few")) | ((model.cls == "rank_deficient") & ~acc)
    assert ((model.cls == "rank_deficient") & ~acc).sum() >= 2 and not acc[gone].any()
    pick = lambda leaves, k: np.concatenate([cloud[model.members[i][:k]] for i in leaves])  # noqa: E731
    dead = pick(np.flatnonzero(gone), 5)
    live = pick(np.flatnonzero(acc), 12)
    assert len(dead) >= 40 and len(live) >= 100
    # only such voxels: nothing at all
    g.setInputSource(dead)
    for mode in (0, 2):
        s, grad, H = g.evaluate(np.eye(4), np.zeros(6), mode)
        assert s == 0.0 and (grad == 0).all() and (H == 0).all(), (mode, s)
    # mixed with points of accepted voxels: the model without those leaves
    src = np.concatenate([dead, live])[np.random.default_rng(3).permutation(len(dead) + len(live))]
    g.setInputSource(src)
    p = np.array([0.004 * res, -0.006 * res, 0.003 * res, 3e-4, -4e-4, 6e-4])  # angles above the reference's small-angle cut (1e-4): 2.4 cm at 40 m
    T = orc.pose_to_matrix(p)
    xt = orc.transform_points(T, src)[:, :3]
    kept = acc & ~gone
    st = {}
    sa, ga, Ha = ndt_analytic.evaluate(src[:, :3], p, search, float(np.float32(res)), model.grid, model.for_evaluate(kept), transformed=xt, upstream_d1_sign=True,
                                       stats=st, dtype=np.longdouble)
    assert abs(sa) > 1e-3 and st["pairs"] >= 100
    f64_tol = 1e-11 + max(tol["icov"], tol["icov_rank_deficient"]) * st["max_icov_q2"]
    s0, g0, H0 = g.evaluate(T, p, 0)
    _, _, H2 = g.evaluate(T, p, 2)
    print(f"res {res} {search}: pairs {st['pairs']} score {sa:.6g} rel {abs(s0 - sa) / abs(sa):.2e} grad {np.abs(g0 - ga).max() / np.abs(ga).max():.2e} "
          f"H {np.abs(H0 - Ha).max() / np.abs(Ha).max():.2e} H64 {np.abs(H2 - Ha).max() / np.abs(Ha).max():.2e} (tolerance {f64_tol:.2e})")
    assert abs(s0 - sa) <= 2e-6 * abs(sa)
    np.testing.assert_allclose(g0, ga, rtol=0, atol=1e-4 * np.abs(ga).max())
    np.testing.assert_allclose(H0, Ha, rtol=0, atol=1e-4 * np.abs(Ha).max())
    np.testing.assert_allclose(H2, Ha, rtol=0, atol=f64_tol * np.abs(Ha).max())
