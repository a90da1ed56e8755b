"""GPU: the HIP kernels of the GICP family (csrc/gicp.hip) against tests/gicp_analytic.py — the family written from its cost function in numpy
float64, independent of oracle/ — with the inputs, preconditions and bars of tests/gicp_cases.py, which tests/test_gicp_analytic_cpu.py applies
to the oracle.  The existing parity tests hold kernel and oracle against each other; a mistake the two share passes those and fails here.

Shapes: targets of 600 - 800 points, sources of 1, 255, 256, 257, 513 and 700 (one workgroup takes 256 points; gicp_block_reduce and
gicp_reduce_record join the partial records).  Bars: H, b, e 1e-12 max|.| (+ 1e-9 on b); covariances 1e-13 w2 / (w1 - w0).
pcl::GICP's f and g and the ICP step pass through float matrices: the oracle differs from the model by 6.52e-6 (f), 6.51e-6 (g) relative and
5.79e-7 (ICP, max|dT|) on the CPU, the bars here are ten times that: 6.52e-5, 6.51e-5, 5.79e-6."""
import numpy as np
import pytest

import gicp_analytic as ga
import gicp_cases as gc

pytestmark = pytest.mark.gpu

HIP = gc.Backend("hip")
VARIANTS = [("fast", 1.0), ("small", 1.0), ("vgicp", 1.0)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    gc.report("HIP kernels")


@pytest.mark.parametrize("variant,res", VARIANTS)
@pytest.mark.parametrize("n", gc.SOURCE_SIZES)
def test_linearize(variant, res, n):
    """(a) H, b, e and the correspondence count of one linearisation, every source size"""
    tgt, src = gc.pair(n, gc.SMALL_POSE)
    gc.check_linearize(HIP, variant, tgt, src, gc.nudged(gc.SMALL_POSE), f"n={n}", res=res)


@pytest.mark.parametrize("variant,res", VARIANTS + [("vgicp", 0.37)])
@pytest.mark.parametrize("n", [257, 700])
def test_linearize_at_a_large_rotation(variant, res, n):
    """(b) 1.2 rad about a skew axis, the source taken back through the pose: R for R^T, a left for a right Jacobian change H at O(1)"""
    tgt, src = gc.pair(n, gc.LARGE_POSE)
    (H, b, e, m), _ = gc.check_linearize(HIP, variant, tgt, src, gc.nudged(gc.LARGE_POSE), f"large rotation n={n} res={res}", res=res)
    assert m > 0.1 * n


@pytest.mark.parametrize("variant,res", VARIANTS + [("vgicp", 0.37)])
@pytest.mark.parametrize("n", [257, 700])
def test_linearize_far_from_the_origin(variant, res, n):
    """(c) both clouds 360 m out: a float in T a or in the residual moves e at 1e-5 relative.  (f64 itself is felt here: ulp(360 m) over a
    residual of 5 cm is 1e-12 per term, 1e-13 after n terms — the oracle is 1.5e-13 off the model on b, the largest figure of the CPU file.)"""
    tgt, src = gc.pair(n, gc.SMALL_POSE, offset=gc.FAR)
    (H, b, e, m), _ = gc.check_linearize(HIP, variant, tgt, src, gc.nudged(gc.SMALL_POSE, gc.FAR), f"far n={n} res={res}", res=res)
    assert m > 0.1 * n


@pytest.mark.parametrize("variant,res", VARIANTS + [("vgicp", 0.37)])
def test_missing_correspondences_add_nothing(variant, res):
    """(d) a third of the source beyond the distance limit / outside the voxel grid, NaN and Inf in both clouds: the model's count, and sums
    over the rest alone"""
    tgt, src, T = gc.pair_with_dropouts(res)
    (H, b, e, m), _ = gc.check_linearize(HIP, variant, tgt, src, T, f"dropouts res={res}", res=res)
    assert 0 < m <= len(src) - len(src) // 3 - 4


def test_max_correspondence_distance_is_strict():
    """(e)"""
    gc.check_threshold(HIP)


@pytest.mark.parametrize("res", [1.0, 0.37])
def test_vgicp_weights(res):
    """(f) voxels of 1, 2, 9 and 100 points, source points 1e-3 m on either side of a voxel face"""
    gc.check_voxel_weights(HIP, res)


@pytest.mark.parametrize("form", ["fast", "pcl"])
@pytest.mark.parametrize("k", [20, 10])
@pytest.mark.parametrize("n", [20, 21, 257])
def test_covariances(form, k, n):
    """(g) gicp_cov_kernel and pclgicp_cov_kernel on generic clouds; at n = 20 = k every neighbourhood is the whole cloud"""
    gc.check_covariances(HIP, form, gc.generic_cloud(n), k, f"n={n} k={k}")


@pytest.mark.parametrize("form", ["fast", "pcl"])
def test_planar_neighbourhoods(form):
    """(h) z = 0 -> diag(1, 1, 1e-3); a tilted plane -> I - (1 - 1e-3) n n^T; the tilted plane 360 m out"""
    gc.check_planes(HIP, form)


@pytest.mark.parametrize("form", ["fast", "pcl"])
def test_degenerate_neighbourhoods(form):
    """(i) a line, copies of one point, an octahedral blob: symmetric, eigenvalues (1e-3, 1, 1), no NaN; d^T C d = 1 along the line"""
    gc.check_degenerates(HIP, form)


def test_pcl_gicp_cost_and_gradient():
    """(j) bars 6.52e-5 (f), 6.51e-5 (g): ten times the oracle's 6.52e-6, 6.51e-6 against the model"""
    gc.check_pcl(HIP)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_single_step(reciprocal):
    """(k) bar 5.79e-6 on max|dT|: ten times the oracle's 5.79e-7 against the model"""
    gc.check_icp(HIP, reciprocal)


@pytest.mark.parametrize("variant", ["fast", "small", "vgicp"])
def test_batch_first_step_at_a_large_rotation(variant):
    """(l) pairs of 255, 256 and 257 source points, guesses set to the large-rotation pose, one iteration.  The damping of the first
    Levenberg-Marquardt trial is not among the product's parameters, so the step itself is not rebuilt here: the batch record is the
    single registration's bit for bit, and its Hessian is the model's at the (float) guess."""
    import mrg_slam_amd as M
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params, result_matrix

    cls, method = {"fast": (M.GicpHip, _lib.GICP_HIP), "small": (M.SmallGicpHip, _lib.SMALL_GICP_HIP), "vgicp": (M.VgicpHip, _lib.VGICP_HIP)}[variant]
    prm = default_params(method)
    prm.maximum_iterations, prm.transformation_epsilon = 1, 0.01
    guess = gc.nudged(gc.LARGE_POSE)
    Tf = guess.astype(np.float32).astype(np.float64)
    bm = M.BatchMatcher(prm)
    pairs = [gc.pair(n, gc.LARGE_POSE) for n in (255, 256, 257)]
    t = bm.add_target(pairs[0][0])
    for k, (_, src) in enumerate(pairs):
        bm.add_pair(t, src, np.eye(4))
        bm.set_guess(k, guess)
    res = bm.align(fitness_max_range=float("inf"))
    for k, (tgt, src) in enumerate(pairs):
        reg = gc.load(cls(maximum_iterations=1), tgt, src)
        reg.align(guess)
        np.testing.assert_array_equal(result_matrix(res[k]), reg.getFinalTransformation())
        assert not np.array_equal(result_matrix(res[k]), guess.astype(np.float32))  # a step was taken
        Ct, Cs = reg.covariances("target"), reg.covariances("source")
        terms, _ = (ga.vgicp_terms(tgt, src, Ct, Cs, Tf, prm.resolution) if variant == "vgicp" else ga.gicp_terms(tgt, src, Ct, Cs, Tf, prm.max_correspondence_distance))
        Hm = terms.linearize(Tf, "right" if variant == "small" else "left")[0]
        H = np.array(res[k]["H"]).reshape(6, 6)
        d = np.abs(H - Hm).max() / np.abs(Hm).max()
        gc.note("H  |dH| / max|H|", d)
        assert d <= 1e-12, f"{variant} pair {k}: record Hessian off the model's by {d:.3g} max|H|"
