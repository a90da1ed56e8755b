"""CPU: the oracle's restatement of pcl::NormalDistributionsTransform (oracle/pcl_ndt.cpp; PCL 1.12 — what registration_method "NDT" and every
unknown name run in the reference, registrations.cpp:115-129) against independent checks: the first-principles Gaussian model
(tests/ndt_analytic.py) over a brute-force radius search, finite differences, pclomp's float formulation with the KDTREE neighbourhood, PCL's
iteration rule, and the product's optimiser (csrc/ndt_ctl.h, formulation 1) stepped on the CPU with this oracle as its evaluator."""
import numpy as np
import pytest

from conftest import small_cloud
from oracle import oracle as orc


def _pair(n=3000, m=700, seed=31):
    from mrg_slam_amd import synth

    tgt = small_cloud(n, seed)
    rel = synth.make_pose([0.3, -0.2, 0.05], synth.rot_xyz(0.02, -0.03, 0.06))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:m])
    return tgt, src, rel


def _radius_lists(xt, cent, in_search, r):
    """brute force over ALL leaves: float squared distance (FLANN L2_Simple order) < float(r * r), sorted by (distance, leaf)"""
    out = []
    r2 = np.float32(np.float64(np.float32(r)) * np.float64(np.float32(r)))  # resolution_ is a float; radius * radius in double, cast to float
    c = cent[:, :3].astype(np.float32)
    for q in xt.astype(np.float32):
        d = c - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        hit = np.nonzero((d2 < r2) & (in_search != 0))[0]
        out.append([int(h) for h in hit[np.lexsort((hit, d2[hit]))]])
    return out


@pytest.mark.parametrize("res", [1.0, 1.5, 0.7])
def test_derivatives_match_the_first_principles_model(res):
    import ndt_analytic

    tgt, src, rel = _pair(n=12000)
    o = orc.PclNdt(resolution=res)
    assert o.setInputTarget(tgt) == 0
    o.setInputSource(src)
    keys, npts, ins, mean, icov, cent = o.leaves()
    assert ins.sum() > 20
    rng = np.random.default_rng(5)
    for trial in range(3):
        p = np.concatenate([rel[:3, 3] + rng.normal(0, 0.1, 3), np.array([0.02, -0.03, 0.06]) + rng.normal(0, 0.02, 3)])
        T = orc.pose_to_matrix(p)
        xt = orc.transform_points(T, src)[:, :3]
        nb = _radius_lists(xt, cent, ins, res)
        assert sum(len(l) for l in nb) > 0.8 * len(src) and max(len(l) for l in nb) >= 3
        sa, ga, Ha = ndt_analytic.evaluate(src[:, :3], p, None, float(np.float32(res)), None or ([0, 0, 0], [0, 0, 0], [1, 1, 1]), (keys, np.where(ins != 0, 6, 0), mean, icov), transformed=xt,
                                           upstream_d1_sign=True, nb_lists=nb)
        s0, g0, H0 = o.evaluate(T, p, 0)
        s1, g1, _ = o.evaluate(T, p, 1)
        _, _, H2 = o.evaluate(T, p, 2)
        # all f64: the model to rounding
        assert abs(s0 - sa) <= 1e-12 * abs(sa) and s1 == s0
        np.testing.assert_allclose(g0, ga, rtol=0, atol=1e-11 * np.abs(ga).max())
        assert (g1 == g0).all()
        np.testing.assert_allclose(H0, Ha, rtol=0, atol=1e-11 * np.abs(Ha).max())
        np.testing.assert_allclose(H2, H0, rtol=0, atol=1e-13 * np.abs(H0).max())


def test_gradient_and_hessian_match_finite_differences():
    tgt, src, rel = _pair(seed=8)
    o = orc.PclNdt()
    o.setInputTarget(tgt)
    o.setInputSource(src)
    p0 = np.concatenate([rel[:3, 3], [0.02, -0.03, 0.06]]) + 0.01
    # the float transform quantises the pose: differentiate the model over the oracle's own f64 score at float matrices is too coarse, so use steps
    # large against float rounding and compare loosely; the first-principles test above is the tight one
    h = 2e-3
    _, g, H = o.evaluate(orc.pose_to_matrix(p0), p0, 0)
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        sp, gp, _ = o.evaluate(orc.pose_to_matrix(p0 + e), p0 + e, 1)
        sm, gm, _ = o.evaluate(orc.pose_to_matrix(p0 - e), p0 - e, 1)
        assert abs((sp - sm) / (2 * h) - g[i]) <= 2e-2 * max(1.0, np.abs(g).max())
        if i != 4:  # row ry carries upstream's +sin(ry) (quirks.h kNdtHAngD1ZSign): not a derivative of the gradient
            np.testing.assert_allclose((gp - gm) / (2 * h), H[i], rtol=0, atol=8e-2 * np.abs(H).max())  # (points change voxels inside the step)


def test_agrees_with_pclomp_float_formulation_at_float_level():
    """same model, same neighbourhood (pclomp KDTREE = the radius search): the two classes' derivatives differ by float rounding only"""
    tgt, src, rel = _pair(seed=12)
    a = orc.PclNdt(resolution=1.0)
    b = orc.Ndt(resolution=1.0, search="KDTREE", num_threads=2)
    for o in (a, b):
        o.setInputTarget(tgt)
        o.setInputSource(src)
    p = np.concatenate([rel[:3, 3] + 0.05, [0.02, -0.03, 0.06]])
    T = orc.pose_to_matrix(p)
    sa, ga, Ha = a.evaluate(T, p, 0)
    sb, gb, Hb = b.evaluate(T, p, 0)
    assert abs(sa - sb) <= 1e-5 * abs(sa)
    np.testing.assert_allclose(ga, gb, rtol=0, atol=2e-4 * np.abs(ga).max())
    np.testing.assert_allclose(Ha, Hb, rtol=0, atol=2e-4 * np.abs(Ha).max())
    _, _, H2 = b.evaluate(T, p, 2)  # pclomp's f64 computeHessian: the same arithmetic as PCL's
    np.testing.assert_allclose(Ha, H2, rtol=0, atol=1e-12 * np.abs(Ha).max())


@pytest.mark.parametrize("ppt", [1, 3, 8])
def test_gpu_order_mode_only_reassociates(ppt):
    """the per-point factorisation the HIP kernel uses (exact algebra) in the kernel's summation tree: the same sums to f64 rounding"""
    tgt, src, rel = _pair(n=4000, m=1500, seed=3)
    a, b = orc.PclNdt(), orc.PclNdt(gpu_order=ppt, num_threads=2)
    for o in (a, b):
        o.setInputTarget(tgt)
        o.setInputSource(src)
    p = np.concatenate([rel[:3, 3] - 0.04, [0.02, -0.03, 0.06]])
    T = orc.pose_to_matrix(p)
    for mode in (0, 1, 2):
        s0, g0, H0 = a.evaluate(T, p, mode)
        s1, g1, H1 = b.evaluate(T, p, mode)
        assert abs(s0 - s1) <= 1e-12 * max(1.0, abs(s0))
        np.testing.assert_allclose(g1, g0, rtol=0, atol=1e-12 * max(1.0, np.abs(g0).max()))
        np.testing.assert_allclose(H1, H0, rtol=0, atol=1e-12 * max(1.0, np.abs(H0).max()))
    # and whole alignments end in the same place
    from mrg_slam_amd import synth

    for o in (a, b):
        o.__init__(transformation_epsilon=1e-5, maximum_iterations=30, gpu_order=o is b and ppt or 0)
        o.setInputTarget(tgt)
        o.setInputSource(src)
        o.align(synth.make_pose(rel[:3, 3] + 0.2, rel[:3, :3]))
    Ta, Tb = a.getFinalTransformation(), b.getFinalTransformation()
    assert a.getFinalNumIteration() == b.getFinalNumIteration() and a.evals == b.evals
    assert np.abs(Ta.astype(np.float64) - Tb).max() <= 1e-6


def test_iteration_rule_of_pcl_1_12():
    """nr_iterations_ >= max_iterations_ or |t_step|^2 <= transformation_epsilon_: with step_size 0.1 any epsilon >= 0.01 stops after ONE Newton
    iteration (mrg_slam's YAML has 0.1); a tight epsilon iterates on; max_iterations caps with >= (not >)"""
    from mrg_slam_amd import synth

    tgt, src, rel = _pair(n=4000, m=2000, seed=5)
    guess = synth.make_pose(rel[:3, 3] + np.array([0.4, -0.3, 0.0]), rel[:3, :3])
    runs = {}
    for eps, iters in ((0.1, 64), (0.01, 64), (1e-6, 64), (1e-12, 3)):
        o = orc.PclNdt(transformation_epsilon=eps, maximum_iterations=iters)
        o.setInputTarget(tgt)
        o.setInputSource(src)
        o.align(guess)
        runs[(eps, iters)] = (o.hasConverged(), o.getFinalNumIteration(), np.linalg.norm(o.getFinalTransformation()[:3, 3] - rel[:3, 3]))
    assert runs[(0.1, 64)][:2] == (True, 1) and runs[(0.01, 64)][:2] == (True, 1)
    assert runs[(1e-6, 64)][0] and 3 < runs[(1e-6, 64)][1] < 64 and runs[(1e-6, 64)][2] < 0.05 < runs[(0.1, 64)][2]
    assert runs[(1e-12, 3)][:2] == (True, 3)


def test_rejected_leaves_stay_in_the_radius_search():
    """VoxelGridCovariance pushes a leaf's centroid into the kd-tree BEFORE the eigenvalue check can reject the leaf, and radiusSearch has no
    nr_points test: such a leaf still answers, with the zero inverse covariance of the Leaf constructor — score only, no gradient"""
    rng = np.random.default_rng(2)
    tgt = small_cloud(2500, 4)
    # eight identical points: the covariance is exactly zero, lambda_2 <= 0 rejects the leaf
    dup = np.tile(np.array([[30.25, 30.25, 10.25, 0.5]], np.float32), (8, 1))
    tgt = np.concatenate([tgt, dup])
    o = orc.PclNdt()
    assert o.setInputTarget(tgt) == 0
    keys, npts, ins, mean, icov, cent = o.leaves()
    rej = np.nonzero((npts == -1) & (ins == 1))[0]
    assert len(rej) >= 1
    leaf = rej[np.argmin(np.abs(mean[rej] - dup[0, :3]).sum(1))]
    assert (icov[leaf] == 0).all()
    src = np.array([[30.3, 30.2, 10.3, 0.0]], np.float32)
    o.setInputSource(src)
    s, g, H = o.evaluate(np.eye(4), np.zeros(6), 0)
    import ndt_analytic

    d1, d2 = ndt_analytic.gauss_constants(1.0)
    assert abs(s - (-d1)) < 1e-15 and (g == 0).all() and (H == 0).all()  # exp(0) = 1: the pair scores -d1 and pulls nowhere
    # pclomp's KDTREE search inherits the same code
    b = orc.Ndt(search="KDTREE")
    b.setInputTarget(tgt)
    b.setInputSource(src)
    sb, gb, _ = b.evaluate(np.eye(4), np.zeros(6), 0)
    assert abs(sb - (-d1)) < 1e-6 and (gb == 0).all()
    # ... and its DIRECT searches test nr_points
    c = orc.Ndt(search="DIRECT7")
    c.setInputTarget(tgt)
    c.setInputSource(src)
    assert c.evaluate(np.eye(4), np.zeros(6), 0)[0] == 0.0


@pytest.mark.parametrize("seed,eps,res", [(1, 0.1, 1.0), (2, 1e-4, 1.0), (3, 1e-6, 2.0), (4, 1e-5, 0.5), (5, 1e-3, 1.5), (6, 1e-7, 1.0)])
def test_product_state_machine_follows_the_oracle(seed, eps, res):
    """mrg_slam_amd/csrc/ndt_ctl.h with formulation 1 (PCL's iteration test and zero-step rule), stepped on the CPU through mrgfe_dbg_ctl_* with the
    oracle answering its requests: the same evaluations, iterations, flag and final transformation as the oracle's own computeTransformation"""
    from mrg_slam_amd import synth
    from mrg_slam_amd._lib import PCL_NDT_HIP
    from mrg_slam_amd.registration import default_params
    from oracle.replay import drive

    rng = np.random.default_rng(seed)
    tgt = small_cloud(4000, seed)
    rel = synth.make_pose(rng.normal(0, 0.3, 3), synth.rot_xyz(*rng.normal(0, 0.03, 3)))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:3000])
    guess = synth.perturb_pose(rel if seed % 3 else np.eye(4), rng)
    o = orc.PclNdt(resolution=res, transformation_epsilon=eps, maximum_iterations=40)
    assert o.setInputTarget(tgt) == 0
    o.setInputSource(src)
    o.align(guess)
    p = default_params(PCL_NDT_HIP)
    p.resolution, p.transformation_epsilon, p.maximum_iterations = res, eps, 40
    d = orc.PclNdt(resolution=res, transformation_epsilon=eps, maximum_iterations=40)
    d.setInputTarget(tgt)
    d.setInputSource(src)
    T, conv, it, ev, modes = drive(d, p, guess, len(src))
    To = o.getFinalTransformation()
    assert conv == o.hasConverged() and it == o.getFinalNumIteration() and ev == o.evals
    assert (T == To).all()  # same f64 evaluations, same optimiser arithmetic: the same floats
    assert modes[0] == 0 and set(modes) <= {0, 1, 2}


def test_zero_step_rule():
    """PCL >= 1.11.1: a vanishing Newton step ends the alignment CONVERGED, a NaN one unconverged"""
    import ctypes as C

    from mrg_slam_amd._lib import PCL_NDT_HIP, check, lib
    from mrg_slam_amd.registration import default_params

    _fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    p = default_params(PCL_NDT_HIP)
    g = np.eye(4, dtype=np.float32)
    for H, grad, want in ((np.eye(6), np.zeros(6), 1), (np.full((6, 6), np.nan), np.ones(6), 0)):
        h = C.c_void_p()
        check(lib().mrgfe_dbg_ctl_create(C.byref(p), g.ctypes.data_as(_fp), 100, C.byref(h)))
        check(lib().mrgfe_dbg_ctl_result(h, 1.0, grad.ctypes.data_as(_dp), H.ctypes.data_as(_dp), 0.0))
        assert lib().mrgfe_dbg_ctl_request(h, None, None, None) == 0
        T, conv = np.empty((4, 4), dtype=np.float32), C.c_int(-1)
        check(lib().mrgfe_dbg_ctl_final(h, T.ctypes.data_as(_fp), C.byref(conv), None, None))
        assert conv.value == want
        lib().mrgfe_dbg_ctl_destroy(h)
