"""CPU: pin the NDT oracle by analytic truth (no reference goldens exist - SURVEY.md §8c):
finite differences of its own score, recovery of a known SE(3), target-grid invariants."""
import numpy as np
import pytest

from conftest import small_cloud
from mrg_slam_amd import synth
from oracle import oracle as orc


def _pose_T(p):
    return orc.pose_to_matrix(np.asarray(p, dtype=np.float64))


def _make(n=3000, seed=0, **kw):
    tgt = small_cloud(n, seed)
    rel = synth.make_pose([0.25, -0.1, 0.03], synth.rot_xyz(0.01, -0.008, 0.03))
    src = orc.transform_points(np.linalg.inv(rel), tgt)  # source = target seen from the moved sensor
    src[:, :3] += np.random.default_rng(seed + 1).normal(0, 0.01, (len(src), 3)).astype(np.float32)
    ndt = orc.Ndt(**kw)
    assert ndt.setInputTarget(tgt) == 0
    ndt.setInputSource(src)
    return ndt, tgt, src, rel


def test_target_grid_matches_numpy_bruteforce():
    ndt, tgt, _, _ = _make()
    keys, npts, mean, cov, icov = ndt.leaves()
    min_b, max_b, div_b = ndt.grid()
    ijk = np.floor(tgt[:, :3] * np.float32(1.0)).astype(np.int64)
    np.testing.assert_array_equal(min_b, ijk.min(0))
    np.testing.assert_array_equal(max_b, ijk.max(0))
    lin = (ijk - min_b) @ np.array([1, div_b[0], div_b[0] * div_b[1]])
    uk, cnt = np.unique(lin, return_counts=True)
    np.testing.assert_array_equal(keys, uk)
    assert (np.diff(keys) > 0).all()
    counts = np.where(npts < 0, cnt, npts)
    np.testing.assert_array_equal(counts, cnt)
    for li in np.flatnonzero(npts >= 6)[:200]:
        pts = tgt[lin == keys[li], :3].astype(np.float64)
        np.testing.assert_allclose(mean[li], pts.mean(0), rtol=0, atol=1e-12)
        n = len(pts)
        c = np.cov(pts.T, bias=True) * (n - 1.0) / n  # PCL's (n-1)/n after the 1/n single-pass form
        w, V = np.linalg.eigh(c)
        w = np.maximum(w, 0.01 * w[2])
        c_reg = V @ np.diag(w) @ V.T
        np.testing.assert_allclose(cov[li], c_reg, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(icov[li] @ cov[li], np.eye(3), atol=1e-8)


@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1", "DIRECT26", "KDTREE"])
def test_gradient_and_hessian_match_finite_differences(search):
    ndt, _, src, rel = _make(n=6000, search=search)
    p0 = np.array([0.2, -0.05, 0.0, 0.012, -0.006, 0.025])
    # The score is only piecewise smooth (a point that hops to another voxel changes its set of Gaussians), so
    # keep the source points that stay well inside their voxel for every finite-difference probe.
    xt = orc.transform_points(_pose_T(p0), src)[:, :3]
    frac = xt - np.floor(xt)
    src = src[((frac > 0.1) & (frac < 0.9)).all(1)]
    assert len(src) > 1500
    ndt.setInputSource(src)
    s0, g0, H0 = ndt.evaluate(_pose_T(p0), p0, 0)
    assert s0 > 0 and np.isfinite(H0).all()
    # score+gradient-only mode returns the same score/gradient, zero Hessian
    s1, g1, H1 = ndt.evaluate(_pose_T(p0), p0, 1)
    assert s1 == s0 and (g1 == g0).all() and (H1 == 0).all()
    # hessian-only double path agrees with the float path to float precision
    _, _, H2 = ndt.evaluate(_pose_T(p0), p0, 2)
    np.testing.assert_allclose(H2, H0, rtol=0, atol=2e-4 * np.abs(H0).max())
    # float-path Hessian is symmetric only up to float rounding (reference computes all 36 entries)
    np.testing.assert_allclose(H0, H0.T, rtol=0, atol=1e-5 * np.abs(H0).max())
    g_fd = np.zeros(6)
    H_fd = np.zeros((6, 6))
    for k in range(6):
        h = 5e-4 if k < 3 else 4e-5
        pp, pm = p0.copy(), p0.copy()
        pp[k] += h
        pm[k] -= h
        sp, gp, _ = ndt.evaluate(_pose_T(pp), pp, 1)
        sm, gm, _ = ndt.evaluate(_pose_T(pm), pm, 1)
        g_fd[k] = (sp - sm) / (2 * h)
        H_fd[:, k] = (gp - gm) / (2 * h)
    # KDTREE membership flips when a voxel centroid crosses the search radius, not at voxel faces: loose check only
    tol_g, tol_h = (0.25, 0.25) if search == "KDTREE" else (2e-3, 5e-3)
    assert np.linalg.norm(g_fd - g0) < tol_g * np.linalg.norm(g0)
    assert np.linalg.norm(H_fd - H0) < tol_h * np.linalg.norm(H0)


def test_align_recovers_known_transform():
    ndt, tgt, src, rel = _make(n=6000, transformation_epsilon=0.001, maximum_iterations=64, num_threads=4)
    ndt.align(np.eye(4))
    T = ndt.getFinalTransformation().astype(np.float64)
    assert ndt.hasConverged()
    assert np.linalg.norm(T[:3, 3] - rel[:3, 3]) < 0.02
    assert synth.rotation_angle(T, rel) < 2e-3
    assert ndt.getFitnessScore() < 0.01
    aligned = ndt.align(np.eye(4), want_aligned=True)
    np.testing.assert_array_equal(aligned, orc.transform_points(ndt.getFinalTransformation(), src))


def test_align_is_thread_count_invariant():
    res = []
    for nt in (1, 3, 8):
        ndt, *_ = _make(num_threads=nt)
        ndt.align(np.eye(4))
        res.append((ndt.getFinalTransformation(), ndt.getHessian(), ndt.getFinalNumIteration(), ndt.evals))
    for r in res[1:]:
        np.testing.assert_array_equal(r[0], res[0][0])
        np.testing.assert_array_equal(r[1], res[0][1])
        assert r[2:] == res[0][2:]


def test_mrg_slam_parameterisation_clips_steps():
    # eps = 0.1, step_size = 0.1 (config/mrg_slam.yaml:102): every step has length in [0.05, 0.1]
    ndt, _, _, rel = _make(transformation_epsilon=0.1)
    guess = synth.make_pose([0.9, 0.3, 0.0], np.eye(3)) @ rel
    ndt.align(guess)
    assert ndt.hasConverged() and 1 <= ndt.getFinalNumIteration() <= 66
    T = ndt.getFinalTransformation()
    assert np.linalg.norm(T[:3, 3] - guess[:3, 3]) <= 0.1 * ndt.getFinalNumIteration() + 1e-6


def test_empty_and_degenerate_inputs():
    ndt = orc.Ndt()
    assert ndt.setInputTarget(np.zeros((0, 4), np.float32)) == -2
    ndt.setInputSource(small_cloud(100))
    ndt.align(np.eye(4))
    assert not ndt.hasConverged()
    np.testing.assert_array_equal(ndt.getFinalTransformation(), np.eye(4, dtype=np.float32))
    # target with no voxel reaching 6 points: zero score, zero step -> "converged" with the guess (ndt_omp quirk)
    sparse = small_cloud(40, extent=(200, 200, 50))
    ndt2 = orc.Ndt()
    assert ndt2.setInputTarget(sparse) == 0
    ndt2.setInputSource(sparse)
    g = synth.make_pose([0.3, 0, 0], np.eye(3))
    ndt2.align(g)
    assert ndt2.hasConverged() and ndt2.getFinalNumIteration() == 0
    np.testing.assert_array_equal(ndt2.getFinalTransformation(), g.astype(np.float32))
    # leaf size too small for the extent: index overflow is an error
    far = small_cloud(100)
    far[0, 0] = 1e6
    ndt3 = orc.Ndt(resolution=0.01)
    assert ndt3.setInputTarget(far) == -1


@pytest.mark.parametrize("eps", [0.1, 0.01])
def test_fused_and_unfused_float_sequences_agree(eps):
    """The reference's float rounding sequence is build dependent (x86: SSE only, CMakeLists.txt:15; aarch64: FMA,
    :19). The oracle's default sequence fuses the NDT three-term products; the unfused one must give the same
    alignment far inside the 1e-4 bar on a well-conditioned pair."""
    res = []
    for fused in (True, False):
        ndt, _, _, rel = _make(n=6000, transformation_epsilon=eps, num_threads=4, fused=fused)
        ndt.align(synth.warm_guess(rel, 2))
        res.append((ndt.getFinalTransformation().astype(np.float64), ndt.hasConverged(), ndt.getFinalNumIteration(), ndt.evals))
    (Ta, ca, ia, ea), (Tb, cb, ib, eb) = res
    assert (ca, ia, ea) == (cb, ib, eb)
    assert np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]) < 1e-5 and synth.rotation_angle(Ta, Tb) < 1e-5


@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1", "DIRECT26", "KDTREE"])
def test_gpu_order_mode_only_reorders_the_sums(search):
    """oracle.Ndt(gpu_order_ppt=k) adds the same per-pair terms in the HIP kernels' order (diagnostic mode): score, gradient and
    Hessian equal the reference-order values to summation-order rounding, for every tile count per item."""
    from conftest import small_cloud
    from mrg_slam_amd import synth

    tgt = small_cloud(5000, 21)
    rel = synth.make_pose([0.2, -0.1, 0.05], synth.rot_xyz(0.01, -0.02, 0.03))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:3700])
    T = synth.perturb_pose(rel, np.random.default_rng(2))
    p = np.array([T[0, 3], T[1, 3], T[2, 3], 0.011, -0.019, 0.031])
    ref = orc.Ndt(search=search, num_threads=2)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    for ppt in (1, 3, 8):
        g = orc.Ndt(search=search, num_threads=1, gpu_order_ppt=ppt)
        g.setInputTarget(tgt)
        g.setInputSource(src)
        for mode in (0, 1, 2):
            s0, g0, H0 = ref.evaluate(T, p, mode)
            s1, g1, H1 = g.evaluate(T, p, mode)
            assert abs(s1 - s0) <= 1e-12 * max(1.0, abs(s0))
            np.testing.assert_allclose(g1, g0, rtol=0, atol=1e-12 * max(1.0, np.abs(g0).max()))
            np.testing.assert_allclose(H1, H0, rtol=0, atol=(1e-12 if mode != 2 else 1e-11) * max(1.0, np.abs(H0).max()))


@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1", "DIRECT26"])
def test_derivatives_match_the_first_principles_model(search):
    """tests/ndt_analytic.py: score, gradient and Hessian of the Gaussian NDT model from rotation-matrix derivative products in
    float64 — independent of pclomp's expanded angle tables and float layouts.  The oracle's float path (modes 0 / 1) must agree at
    the float32 level, its f64 computeHessian (mode 2) at the f64 level."""
    import ndt_analytic
    from conftest import small_cloud
    from mrg_slam_amd import synth

    tgt = small_cloud(3000, 31)
    rel = synth.make_pose([0.3, -0.2, 0.05], synth.rot_xyz(0.02, -0.03, 0.06))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:700])
    o = orc.Ndt(search=search, num_threads=2)
    o.setInputTarget(tgt)
    o.setInputSource(src)
    keys, npts, mean, cov, icov = o.leaves()
    rng = np.random.default_rng(5)
    for trial in range(3):
        p = np.concatenate([rel[:3, 3] + rng.normal(0, 0.1, 3), np.array([0.02, -0.03, 0.06]) + rng.normal(0, 0.02, 3)])
        T = orc.pose_to_matrix(p)
        s0, g0, H0 = o.evaluate(T, p, 0)
        _, _, H2 = o.evaluate(T, p, 2)
        xt = orc.transform_points(T, src)[:, :3]  # the reference's float-transformed cloud
        sa, ga, Ha = ndt_analytic.evaluate(src[:, :3], p, search, 1.0, o.grid(), (keys, npts, mean, icov), transformed=xt, upstream_d1_sign=True)
        assert abs(s0 - sa) <= 2e-6 * abs(sa)
        np.testing.assert_allclose(g0, ga, rtol=0, atol=1e-4 * np.abs(ga).max())
        np.testing.assert_allclose(H0, Ha, rtol=0, atol=1e-4 * np.abs(Ha).max())   # float path: f32 rounding, amplified by thin voxels
        np.testing.assert_allclose(H2, Ha, rtol=0, atol=1e-11 * np.abs(Ha).max())  # f64 computeHessian: the same model to rounding
        # the one place where upstream leaves first principles: the sign of sin(ry) in the (ry, ry) second derivative
        _, _, Htrue = ndt_analytic.evaluate(src[:, :3], p, search, 1.0, o.grid(), (keys, npts, mean, icov), transformed=xt)
        diff = H2 - Htrue
        assert abs(diff[4, 4]) > 1e-9 * np.abs(Htrue).max()
        diff[4, 4] = 0
        assert np.abs(diff).max() <= 1e-11 * np.abs(Htrue).max()


@pytest.mark.parametrize("shifted", [False, True], ids=["origin", "shifted"])
@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1", "DIRECT26", "KDTREE"])
@pytest.mark.parametrize("res", [1.0, 0.5, 0.37, 2.0])
def test_derivatives_match_the_first_principles_model_off_the_unit_grid(res, search, shifted):
    """the same model and tolerances at leaf sizes where inv_leaf, outlier_ratio / res^3, the neighbour offsets and floor(x / leaf) are not what they
    are at 1.0, for every neighbourhood (KDTREE by a brute-force radius search over float centroids), on a cloud at the origin and one shifted by
    (-37.3, 12.9, -2.2); the model is given the FLOAT resolution (tests/ndt_model_cases.py)"""
    import ndt_model_cases

    ndt_model_cases.check_derivatives(orc.Ndt(resolution=res, search=search, num_threads=2), res, search, shifted)


@pytest.mark.parametrize("shifted", [False, True], ids=["origin", "shifted"])
@pytest.mark.parametrize("search,res", [("DIRECT7", 0.5), ("DIRECT7", 0.37), ("KDTREE", 0.5), ("KDTREE", 0.37)])
def test_derivatives_match_the_model_end_to_end_from_raw_points(search, res, shifted):
    """the leaves come from tests/ndt_leaves_model.py (raw target points -> cells, means, floored inverse covariances), not from the oracle: points ->
    score / gradient / Hessian is independent end to end.  f64-Hessian tolerance: ndt_model_cases.check_derivatives."""
    import ndt_model_cases

    ndt_model_cases.check_derivatives(orc.Ndt(resolution=res, search=search, num_threads=2), res, search, shifted, model_leaves=True)


@pytest.mark.parametrize("search", ["DIRECT1", "DIRECT7"])
@pytest.mark.parametrize("res", [0.37, 0.7])
def test_neighbourhood_lookup_follows_the_float_rule_on_cell_faces(res, search):
    import ndt_model_cases

    ndt_model_cases.check_face_lookup(orc.Ndt(resolution=res, search=search, num_threads=2), res, search)


def test_thread_sums_mode_agrees_with_point_order_sums(street_pair_vlp16):
    """The accumulation bench.py TIMES as cpu_baseline (ndt_omp's: one accumulator per OpenMP thread, added in thread order) against the
    checker's (per-point records added in point order): the same sums to rounding, the same alignment."""
    from mrg_slam_amd import synth

    tgt, src, rel = street_pair_vlp16
    guess = synth.warm_guess(rel, 3)
    p = np.concatenate([guess[:3, 3], orc.euler_xyz(guess)])
    ref = orc.Ndt(num_threads=2)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    for nt in (1, 3, 4):
        o = orc.Ndt(num_threads=nt, thread_sums=True)
        o.setInputTarget(tgt)
        o.setInputSource(src)
        for mode in (0, 1):
            s0, g0, h0 = ref.evaluate(guess, p, mode)
            s1, g1, h1 = o.evaluate(guess, p, mode)
            assert s1 == pytest.approx(s0, rel=1e-12)
            np.testing.assert_allclose(g1, g0, rtol=0, atol=1e-11 * np.abs(g0).max())
            np.testing.assert_allclose(h1, h0, rtol=0, atol=1e-11 * max(np.abs(h0).max(), 1e-300))
        ref.align(guess)
        o.align(guess)
        np.testing.assert_allclose(o.getFinalTransformation(), ref.getFinalTransformation(), atol=1e-6)
        assert o.getFinalNumIteration() == ref.getFinalNumIteration()
