"""CPU: the oracle's optimisers (oracle/gicp.cpp, oracle/ndt.cpp, oracle/pcl_ndt.cpp) held to the first-principles models with the inputs,
preconditions and bars of tests/optimiser_cases.py, which tests/test_gpu_optimiser_steps.py applies to the HIP path; and the additions to
the models held against themselves.  The interior of NDT's More-Thuente line search and pcl::GICP's BFGS stay with the oracle comparison
(tests/optimiser_cases.py says why).

Largest oracle-against-model figures measured by this file (pytest -s prints them):
  trial cost, frozen terms   |de| / max(|e|, 1)  3.8e-14 up to 800 terms (bar 1e-12);  many blocks 4.7e-4 of their bar 1e-12 n / 800
  records (H, b, e)          0.005, 0.33 and 0.04 of their bar (b: the 33,025-point record)
  LM descent                 the frozen-term cost of the float read-out never rose at all (bar: the e bar)
  NDT pose arithmetic        0.52 ulp_f32 on the rotation block, 0 on the translation (bar 4);  step lengths inside [eps / 2, step_size]
and the four MEASURED quantities, whose bars — here and on the GPU — are ten times these:
  step equation  |(H + lambda I) d + b| / |b| per step   small 4.16e-8, 2.05e-6;  large 7.47e-7, 3.73e-5;
                                                         far 2.53e-6, 2.90e-4, 8.15e-3, (0.676, 0.143: not asserted), 7.11e-3
  damping floor  -lambda / max diag H                    small 1.54e-10, large 9.85e-9, far 2.86e-10
  ICP chain      max|dT| for maximum_iterations 1 .. 6   4.77e-7, 2.38e-7, 2.38e-7, 4.77e-7, 2.38e-7, 4.77e-7
  NDT direction  |delta / |delta| - Newton direction|    2.73e-6
360 m out the fourth and fifth steps are of 1e-5 rad, where a rotation entry's last float bit moves a point by 2e-5 m: the residual of the step equation
is then about |b| whatever the step, so those two steps are held to prefix, descent and termination only.  The composed-on-the-wrong-side residual,
0.10 .. 0.49 |b| from the model alone, is held against the large-rotation scene's bar."""
import numpy as np
import pytest

import gicp_analytic as ga
import gicp_cases as gc
import optimiser_cases as oc

ORACLE = gc.Backend("oracle")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    oc.report("oracle")


# ---- the models against themselves ----------------------------------------------------------------------------------------------------
def test_model_logarithm_inverts_the_exponential():
    rng = np.random.default_rng(0)
    for angle in (1e-6, 1e-2, 0.5, 2.5):
        xi = rng.normal(size=6)
        xi[:3] *= angle / np.linalg.norm(xi[:3])
        xi[3:] *= 100.0
        assert np.abs(ga.se3_log(ga.se3_exp(xi)) - xi).max() <= 1e-14 * np.abs(xi).max()
    # a float matrix: what rounding leaves off se(3) is dropped, the rest is the logarithm of the rounded pose
    T = gc.LARGE_POSE.astype(np.float32).astype(np.float64)
    assert np.abs(ga.se3_exp(ga.se3_log(T)) - T).max() <= 2e-7


def test_model_blocked_search_is_the_model_search():
    tgt, src, T = gc.pair_with_dropouts(1.0)
    q = ga.transform_float(T, src)
    for strict in (True, False):
        (a, da), (b, db) = oc.nearest_blocked(tgt, q, 2.0, strict, block=100), ga.nearest(tgt, q, 2.0, strict)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(da[np.isfinite(da)], db[np.isfinite(db)])
    assert oc.unambiguous(tgt, src, T, 2.0)
    gc.assert_unambiguous(tgt, src, T, 2.0)


@pytest.mark.parametrize("variant,res", [("fast", 1.0), ("vgicp", 0.37)])
def test_model_frozen_terms_are_the_model_terms(variant, res):
    """frozen_terms with the correspondences and M at one pose is ga.gicp_terms / ga.vgicp_terms"""
    tgt, src, T = gc.pair_with_dropouts(res)
    Ct, Cs = ga.covariances_fast(tgt)[0], ga.covariances_fast(src)[0]
    Ct, Cs = np.nan_to_num(Ct), np.nan_to_num(Cs)
    mine, _ = oc.frozen_terms(variant, tgt, src, Ct, Cs, T, T, res)
    theirs, _ = ga.vgicp_terms(tgt, src, Ct, Cs, T, res) if variant == "vgicp" else ga.gicp_terms(tgt, src, Ct, Cs, T)
    assert len(mine) == len(theirs) > 100
    for a, b in zip(mine.linearize(T, "left")[:3], theirs.linearize(T, "left")[:3]):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)


def test_model_icp_chain_starts_with_the_single_step():
    tgt, src, guess = oc.icp_inputs("changing")
    poses = ga.icp_chain(tgt, src, guess, 2, 2.0, True)
    np.testing.assert_array_equal(poses[0], guess.astype(np.float32))
    np.testing.assert_array_equal(poses[1], ga.icp_step(tgt, src, guess, 2.0, True)[0].astype(np.float32))
    np.testing.assert_array_equal(poses[2], ga.icp_step(tgt, src, poses[1], 2.0, True)[0].astype(np.float32))


def test_model_euler_angles_invert_the_pose_matrix():
    p = np.array([0.3, -0.2, 0.05, 0.4, -0.7, 1.1])
    np.testing.assert_allclose(oc.euler_xyz(oc.pose_to_matrix(p)), p, rtol=0, atol=1e-15)
    from oracle import oracle as orc

    assert np.abs(orc.pose_to_matrix(p).astype(np.float64) - oc.pose_to_matrix(p)).max() <= 1.2e-7  # the oracle's float matrix of the same pose


@pytest.mark.parametrize("n", oc.MANY_BLOCK_SIZES)
def test_many_block_seeds_are_unambiguous(n):
    assert oc.many_block_seed(n, oc.MANY_BLOCK_SEEDS[n]) == oc.MANY_BLOCK_SEEDS[n]


@pytest.mark.parametrize("variant", ["fast", "small", "vgicp"])
def test_model_tells_the_composition_sides_apart(variant):
    oc.check_wrong_side_is_told_apart(variant)


# ---- the oracle against the models ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,res", oc.VARIANTS)
@pytest.mark.parametrize("pose", ["small", "large", "far"])
def test_oracle_trial_costs(variant, res, pose):
    for n in gc.SOURCE_SIZES:
        tgt, src, T = oc.pose_case(pose, n)
        oc.check_trial_costs(ORACLE, variant, tgt, src, T, f"{pose} n={n} res={res}", res=res)


@pytest.mark.parametrize("variant,res", oc.VARIANTS)
def test_oracle_trial_costs_with_dropouts(variant, res):
    tgt, src, T = gc.pair_with_dropouts(res)
    oc.check_trial_costs(ORACLE, variant, tgt, src, T, f"dropouts res={res}", res=res)


@pytest.mark.parametrize("variant", ["fast", "vgicp"])
@pytest.mark.parametrize("n", oc.MANY_BLOCK_SIZES)
def test_oracle_many_block_records(variant, n):
    oc.check_many_blocks(ORACLE, variant, n)


@pytest.mark.parametrize("variant", ["fast", "small", "vgicp"])
@pytest.mark.parametrize("name", ["small", "large", "far"])
@pytest.mark.parametrize("n", [257, 700])
def test_oracle_lm_trajectory(variant, name, n):
    oc.check_trajectory(ORACLE, variant, name, n)


@pytest.mark.parametrize("which", ["near", "changing"])
@pytest.mark.parametrize("reciprocal", [False, True])
def test_oracle_icp_chain(which, reciprocal):
    oc.check_icp_chain(ORACLE, which, reciprocal)


@pytest.mark.parametrize("kind,search,res", oc.NDT_CONFIGS)
def test_oracle_ndt_newton_steps(kind, search, res):
    oc.check_ndt_steps(ORACLE, kind, search, res)
