"""CPU: tests/gicp_analytic.py (the GICP family from its cost function, numpy float64) held against itself — finite differences of its own
cost, the adjoint relation of its two Jacobians — and the oracle (oracle/gicp.cpp, oracle/pcl_gicp.cpp) held against it, with the inputs and
bars of tests/gicp_cases.py that tests/test_gpu_gicp_analytic.py applies to the HIP kernels.

Largest oracle-against-model discrepancies measured by this file (pytest -s prints them):
  H  |dH| / max|H| 2.9e-15      b  |db| / max|b| 1.5e-13      e  |de| / |e| 3.7e-14                                  (bar 1e-12)
  C  |dC| (w1 - w0) / w2   fast 1.5e-15, pcl 1.4e-15; degenerate neighbourhoods' eigenvalues 1.1e-15 off (1e-3, 1, 1)   (bars 1e-13, 1e-12)
  pcl::GICP functor  |df| / |f| 6.52e-6,  max|dg| / max|g| 6.51e-6      -> the bars, here and on the GPU: ten times these
  ICP step  max|dT| 5.79e-7                                              -> the bar: ten times this
b and e are within a factor of ten of their bar only 360 m from the origin (everywhere else 2e-14 at most): there r = m_B - T a has
ulp(360 m) = 5.7e-14 m of f64 rounding on a 5 cm residual, 1e-12 relative per term and 1e-13 after n terms, whichever order T a is
multiplied out in — the conditioning of the input, not an error of either side.  pcl's f and g: the functor takes d from a float matrix
and float points, 20 m * 2^-23 = 2e-6 m on a residual of a few cm, the same way for every point."""
import numpy as np
import pytest

import gicp_analytic as ga
import gicp_cases as gc

ORACLE = gc.Backend("oracle")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    gc.report("oracle")


# ---- the model against itself -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_terms():
    """Correspondences at a pose with a rotation of 1.2 rad, 0.1 m / 0.02 rad off the one the clouds meet at, model covariances throughout"""
    tgt, src = gc.pair(300, gc.LARGE_POSE, seed=11, n_target=400)
    T = ga.se3_exp([0.02, -0.01, 0.015, 0.1, -0.05, 0.08]) @ gc.LARGE_POSE
    Ct, _ = ga.covariances_fast(tgt)
    Cs, _ = ga.covariances_fast(src)
    terms, _ = ga.gicp_terms(tgt, src, Ct, Cs, T)
    assert len(terms) > 250
    return terms, T


@pytest.mark.parametrize("side", ["left", "right"])
def test_model_gradient_and_hessian_are_the_derivatives_of_its_cost(model_terms, side):
    """Central differences (h = 1e-4) of the frozen-M cost under exp(h xi) T / T exp(h xi) equal 2 b, and the differenced residuals
    reproduce H.  r' and r'' are of size |T a| ~ 20 m, so e''' ~ 6 |H| and the truncation h^2 e''' / 6 ~ 1e-8 max|H|; rounding
    e 2^-53 / h is smaller still: bar 1e-6 max|H| (1e-6 relative on H), a hundred times that — and b is required to be large enough
    (>= 1e-4 max|H|) for a wrong sign or a swapped block in it to show."""
    terms, T = model_terms
    H, b, e, n = terms.linearize(T, side)
    assert np.abs(b).max() >= 1e-4 * np.abs(H).max()
    h = 1e-4
    g, Jfd = np.zeros(6), np.zeros((n, 3, 6))
    for i in range(6):
        xi = np.zeros(6)
        xi[i] = h
        Tp, Tm = (ga.se3_exp(xi) @ T, ga.se3_exp(-xi) @ T) if side == "left" else (T @ ga.se3_exp(xi), T @ ga.se3_exp(-xi))
        g[i] = (terms.cost(Tp) - terms.cost(Tm)) / (2 * h)
        Jfd[:, :, i] = (terms.residuals(Tp) - terms.residuals(Tm)) / (2 * h)
    np.testing.assert_allclose(g, 2 * b, rtol=0, atol=1e-6 * np.abs(H).max())
    np.testing.assert_allclose(np.einsum("n,nai,nab,nbj->ij", terms.w, Jfd, terms.M, Jfd), H, rtol=0, atol=1e-6 * np.abs(H).max())


def test_model_left_and_right_forms_are_adjoint_related(model_terms):
    terms, T = model_terms
    Hl, bl, el, _ = terms.linearize(T, "left")
    Hr, br, er, _ = terms.linearize(T, "right")
    Ad = ga.adjoint(T)
    assert el == er
    np.testing.assert_allclose(Hr, Ad.T @ Hl @ Ad, rtol=0, atol=1e-12 * np.abs(Hl).max() * np.abs(Ad).sum(1).max() ** 2)
    np.testing.assert_allclose(br, Ad.T @ bl, rtol=0, atol=1e-12 * np.abs(bl).max() * np.abs(Ad).sum(1).max())
    np.testing.assert_allclose(ga.se3_exp(Ad @ [0.3, -0.2, 0.5, 1.0, 2.0, -1.0]) @ T, T @ ga.se3_exp([0.3, -0.2, 0.5, 1.0, 2.0, -1.0]), atol=1e-12)


def test_model_pcl_gradient_is_the_derivative_of_its_cost():
    """Central differences of the model's pcl::GICP cost (h = 1e-5; |d^3 f| ~ |a|^2 max M ~ 1e5 -> truncation ~ 1e-6, bar 1e-4 max|g|)"""
    tgt, src = gc.pair(300, gc.LARGE_POSE, seed=11, n_target=400)
    Ct, _ = ga.covariances_pcl(tgt)
    Cs, _ = ga.covariances_pcl(src)
    x = np.array([3.05, -1.9, 0.45, 0.8, -0.7, 0.9])
    f, g, n = ga.pcl_cost(tgt, src, Ct, Cs, gc.LARGE_POSE, x)
    assert n > 250
    for i in range(6):
        d = np.zeros(6)
        d[i] = 1e-5
        num = (ga.pcl_cost(tgt, src, Ct, Cs, gc.LARGE_POSE, x + d)[0] - ga.pcl_cost(tgt, src, Ct, Cs, gc.LARGE_POSE, x - d)[0]) / 2e-5
        assert abs(num - g[i]) <= 1e-4 * np.abs(g).max()


def test_model_icp_step_recovers_an_exact_rigid_copy():
    """Kabsch on exact correspondences lands on the motion: the step from a guess 5 mm / 1 mrad off (every nearest point is then the right one)"""
    tgt, src = gc.pair(300, gc.LARGE_POSE, seed=11, n_target=400, noise=0.0)
    guess = ga.se3_exp([0.001, -0.0005, 0.0008, 0.005, -0.003, 0.002]) @ gc.LARGE_POSE
    T, m = ga.icp_step(tgt, src, guess)
    assert m == 300
    np.testing.assert_allclose(T, gc.LARGE_POSE, atol=2e-5)  # float source coordinates and float query points: 20 m * 2^-23


# ---- the oracle against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,res", [("fast", 1.0), ("small", 1.0), ("vgicp", 1.0), ("vgicp", 0.37)])
@pytest.mark.parametrize("pose", ["small", "large", "far"])
def test_oracle_linearize(variant, res, pose):
    T = gc.LARGE_POSE if pose == "large" else gc.SMALL_POSE
    for n in (257, 700):
        tgt, src = gc.pair(n, T, offset=gc.FAR if pose == "far" else None)
        (H, b, e, m), _ = gc.check_linearize(ORACLE, variant, tgt, src, gc.nudged(T, gc.FAR if pose == "far" else (0, 0, 0)), f"{pose} n={n} res={res}", res=res)
        assert m > (0.5 if variant != "vgicp" else 0.1) * n


@pytest.mark.parametrize("variant,res", [("fast", 1.0), ("small", 1.0), ("vgicp", 1.0), ("vgicp", 0.37)])
def test_oracle_missing_correspondences(variant, res):
    tgt, src, T = gc.pair_with_dropouts(res)
    (H, b, e, m), _ = gc.check_linearize(ORACLE, variant, tgt, src, T, f"dropouts res={res}", res=res)
    assert 0 < m <= len(src) - len(src) // 3 - 4


def test_oracle_threshold_is_strict():
    gc.check_threshold(ORACLE)


@pytest.mark.parametrize("res", [1.0, 0.37])
def test_oracle_vgicp_weights(res):
    gc.check_voxel_weights(ORACLE, res)


@pytest.mark.parametrize("form", ["fast", "pcl"])
@pytest.mark.parametrize("k", [20, 10])
@pytest.mark.parametrize("n", [20, 21, 257])
def test_oracle_covariances(form, k, n):
    gc.check_covariances(ORACLE, form, gc.generic_cloud(n), k, f"n={n} k={k}")


@pytest.mark.parametrize("form", ["fast", "pcl"])
def test_oracle_planes(form):
    gc.check_planes(ORACLE, form)


@pytest.mark.parametrize("form", ["fast", "pcl"])
def test_oracle_degenerate_neighbourhoods(form):
    gc.check_degenerates(ORACLE, form)


def test_oracle_pcl_evaluate():
    gc.check_pcl(ORACLE)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_oracle_icp_step(reciprocal):
    gc.check_icp(ORACLE, reciprocal)
