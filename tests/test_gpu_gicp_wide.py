"""GPU: the GICP family with correspondence_randomness beyond 64 (covariances from the wide k-NN kernel): covariances against the first-principles
numpy model (tests/gicp_cases.py, its own bar and precondition) and against the CPU oracle, one alignment per method at k = 80 under the
assertions of tests/test_gpu_gicp.py / tests/test_gpu_pclgicp.py, a SMALL_GICP_HIP batch with a keyed pair against single registrations, and the
refusal of k = 257."""
import numpy as np
import pytest

import gicp_cases as gc
from conftest import small_cloud

pytestmark = pytest.mark.gpu

HIP = gc.Backend("hip")
K = 80


def _pair(n=3000, seed=0):
    """the pair of tests/test_gpu_gicp.py"""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    tgt = small_cloud(n, seed)
    rel = synth.make_pose([0.2, -0.1, 0.03], synth.rot_xyz(0.01, -0.008, 0.03))
    src = orc.transform_points(np.linalg.inv(rel), small_cloud(n, seed + 50))
    return tgt, src, rel


def _pcl_pair(n=5000, seed=5, nsrc=4200):
    """the pair of tests/test_gpu_pclgicp.py"""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    tgt = small_cloud(n, seed)
    rel = synth.make_pose([0.22, -0.13, 0.04], synth.rot_xyz(0.015, -0.01, 0.035))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:nsrc])
    return tgt, src, rel


def _rot_angle(Ra, Rb):
    from mrg_slam_amd import synth

    return synth.rotation_angle(Ra, Rb)


@pytest.mark.parametrize("k", [65, 128])
@pytest.mark.parametrize("form", ["fast", "pcl"])
@pytest.mark.parametrize("n,seed", [(400, 7), (257, 7)])
def test_covariances_against_the_model(form, k, n, seed):
    """small_cloud(400, 7) / (257, 7): the numpy model alone gives relative eigen-gaps >= 0.042 (k = 65) and >= 0.14 (k = 128) on them, well above
    check_covariances' precondition of 1e-3"""
    gc.check_covariances(HIP, form, small_cloud(n, seed), k, f"n={n} k={k}")


@pytest.mark.parametrize("variant", ["fast", "small"])
def test_covariances_of_a_registration_match_the_oracle(variant):
    from mrg_slam_amd import GicpHip, SmallGicpHip
    from oracle import oracle as orc

    tgt, src, _ = _pair(2500, 7)
    g = (GicpHip if variant == "fast" else SmallGicpHip)(correspondence_randomness=K, transformation_epsilon=0.01)
    o = (orc.FastGicp if variant == "fast" else orc.SmallGicp)(correspondence_randomness=K, transformation_epsilon=0.01, num_threads=1)
    for r in (g, o):
        r.setInputTarget(tgt)
        r.setInputSource(src)
    for which in ("source", "target"):
        np.testing.assert_allclose(g.covariances(which), o.covariances(which), rtol=0, atol=1e-12)


def test_gicp_align_matches_oracle():
    from mrg_slam_amd import GicpHip
    from oracle import oracle as orc

    tgt, src, rel = _pair()
    g = GicpHip(correspondence_randomness=K, transformation_epsilon=0.01)
    o = orc.FastGicp(correspondence_randomness=K, transformation_epsilon=0.01, num_threads=4)
    for r in (g, o):
        r.setInputTarget(tgt)
        r.setInputSource(src)
    aligned = g.align(np.eye(4), want_aligned=True)
    o.align(np.eye(4))
    Tg, To = g.getFinalTransformation(), o.getFinalTransformation()
    assert g.hasConverged() == o.hasConverged()
    assert g.getFinalNumIteration() == o.getFinalNumIteration()
    assert np.linalg.norm(Tg[:3, 3].astype(np.float64) - To[:3, 3]) <= 1e-4
    assert _rot_angle(Tg[:3, :3], To[:3, :3]) <= 1e-4
    np.testing.assert_allclose(g.getHessian(), o.getFinalHessian(), rtol=0, atol=1e-6 * np.abs(o.getFinalHessian()).max())
    np.testing.assert_array_equal(aligned, orc.transform_points(Tg, src))
    assert g.getFitnessScore() == pytest.approx(o.getFitnessScore(), rel=1e-3)
    assert np.linalg.norm(Tg[:3, 3] - rel[:3, 3]) < 0.1


def test_small_gicp_align_matches_oracle():
    from mrg_slam_amd import SmallGicpHip
    from oracle import oracle as orc

    tgt, src, rel = _pair()
    g = SmallGicpHip(correspondence_randomness=K, transformation_epsilon=0.01)
    o = orc.SmallGicp(correspondence_randomness=K, transformation_epsilon=0.01, num_threads=1)
    for r in (g, o):
        r.setInputTarget(tgt)
        r.setInputSource(src)
    aligned = g.align(np.eye(4), want_aligned=True)
    o.align(np.eye(4))
    Tg, To = g.getFinalTransformation(), o.getFinalTransformation()
    assert g.hasConverged() == o.hasConverged()
    assert g.getFinalNumIteration() == o.getFinalNumIteration()
    assert np.linalg.norm(Tg[:3, 3].astype(np.float64) - To[:3, 3]) <= 1e-4
    assert _rot_angle(Tg[:3, :3], To[:3, :3]) <= 1e-4
    np.testing.assert_allclose(g.getHessian(), o.getFinalHessian(), rtol=0, atol=1e-6 * np.abs(o.getFinalHessian()).max())
    np.testing.assert_array_equal(aligned, orc.transform_points(Tg, src))
    assert np.linalg.norm(Tg[:3, 3] - rel[:3, 3]) < 0.1


def test_vgicp_align_matches_oracle():
    from mrg_slam_amd import VgicpHip
    from oracle import oracle as orc

    tgt, src, rel = _pair()
    g = VgicpHip(resolution=1.0, correspondence_randomness=K, transformation_epsilon=0.01)
    o = orc.FastVgicp(resolution=1.0, correspondence_randomness=K, transformation_epsilon=0.01, num_threads=1)
    for r in (g, o):
        r.setInputTarget(tgt)
        r.setInputSource(src)
    aligned = g.align(np.eye(4), want_aligned=True)
    o.align(np.eye(4))
    Tg, To = g.getFinalTransformation(), o.getFinalTransformation()
    assert g.hasConverged() == o.hasConverged()
    assert g.getFinalNumIteration() == o.getFinalNumIteration()
    assert np.linalg.norm(Tg[:3, 3].astype(np.float64) - To[:3, 3]) <= 1e-4
    assert _rot_angle(Tg[:3, :3], To[:3, :3]) <= 1e-4
    np.testing.assert_allclose(g.getHessian(), o.getFinalHessian(), rtol=0, atol=1e-6 * np.abs(o.getFinalHessian()).max())
    np.testing.assert_array_equal(aligned, orc.transform_points(Tg, src))


def test_pcl_gicp_align_matches_oracle():
    from mrg_slam_amd import PclGicpHip, select_registration_method
    from oracle import oracle as orc

    tgt, src, rel = _pcl_pair()
    g = select_registration_method({"registration_method": "GICP", "reg_transformation_epsilon": 0.01, "reg_correspondence_randomness": K, "reg_use_reciprocal_correspondences": True})
    assert type(g) is PclGicpHip
    o = orc.PclGicp(correspondence_randomness=K, transformation_epsilon=0.01, omp=False, num_threads=4, sum_threads=1)
    for r in (g, o):
        r.setInputTarget(tgt)
        r.setInputSource(src)
    aligned = g.align(np.eye(4), want_aligned=True)
    o.align(np.eye(4))
    Tg, To = g.getFinalTransformation(), o.getFinalTransformation()
    assert g.hasConverged() == o.hasConverged() and g.getFinalNumIteration() == o.getFinalNumIteration()
    np.testing.assert_array_equal(Tg, To)  # both formulations add their cost terms in the reference's order: the same BFGS trajectory, bit for bit
    assert np.linalg.norm(Tg[:3, 3].astype(np.float64) - rel[:3, 3]) < 5e-3  # and it is the motion
    np.testing.assert_array_equal(aligned, orc.transform_points(Tg, src))
    assert g.getFitnessScore() == pytest.approx(o.getFitnessScore(), rel=1e-3, abs=1e-9)


def test_small_gicp_batch_equals_single_registrations():
    """two pairs, the second through the keyframe store (its covariances are kept under the key with the k they were computed with); aligned twice, the
    second time from the store"""
    from mrg_slam_amd import BatchMatcher, SmallGicpHip, synth
    from mrg_slam_amd._lib import SMALL_GICP_HIP
    from mrg_slam_amd.registration import default_params, result_matrix
    from oracle import oracle as orc

    tgt = small_cloud(4000, 210)
    rng = np.random.default_rng(10)
    prm = default_params(SMALL_GICP_HIP)
    prm.transformation_epsilon = 0.01
    prm.correspondence_randomness = K
    bm = BatchMatcher(prm)
    t = bm.add_target(tgt)
    pairs = []
    for k in range(2):
        rel = synth.make_pose(rng.normal(0, 0.15, 3), synth.rot_xyz(*rng.normal(0, 0.015, 3)))
        src = orc.transform_points(np.linalg.inv(rel), tgt[: 2500 + 300 * k])
        guess = synth.perturb_pose(np.eye(4), rng)
        pairs.append((src, guess))
        bm.add_pair(t, src, guess, key=0 if k == 0 else 700 + k)
    res = bm.align(fitness_max_range=float("inf"))
    again = bm.align(fitness_max_range=float("inf"))
    for k, (src, guess) in enumerate(pairs):
        reg = SmallGicpHip(correspondence_randomness=K, transformation_epsilon=0.01)
        reg.setInputTarget(tgt)
        reg.setInputSource(src)
        reg.align(guess)
        np.testing.assert_array_equal(result_matrix(res[k]), reg.getFinalTransformation())
        np.testing.assert_array_equal(result_matrix(again[k]), reg.getFinalTransformation())
        assert res[k]["converged"] == int(reg.hasConverged()) and res[k]["iterations"] == reg.getFinalNumIteration()
        assert res[k]["fitness"] == pytest.approx(reg.getFitnessScore(), rel=1e-12)


@pytest.mark.parametrize("k", [257, 3])
def test_correspondence_randomness_outside_the_lists_is_refused(k):
    from mrg_slam_amd import BatchMatcher, GicpHip, MrgfeError, _lib
    from mrg_slam_amd.registration import default_params

    with pytest.raises(MrgfeError, match=r"\[4, 256\]") as e:
        GicpHip(correspondence_randomness=k)
    assert e.value.status == _lib.ERR_INVALID
    prm = default_params(_lib.SMALL_GICP_HIP)
    prm.correspondence_randomness = k
    with pytest.raises(MrgfeError, match=r"\[4, 256\]") as e:
        BatchMatcher(prm)
    assert e.value.status == _lib.ERR_INVALID


def test_the_widest_list_is_accepted():
    from mrg_slam_amd import GicpHip

    c = small_cloud(300, 3)
    g = GicpHip(correspondence_randomness=256)
    g.setInputTarget(c)
    g.setInputSource(c)
    cov = g.covariances("target")
    assert np.isfinite(cov).all()
    np.testing.assert_array_equal(cov, g.covariances("source"))
