"""Inputs shared by tests/test_gpu_icp_batch.py and tests/test_icp_controller_cpu.py: candidates cut out of structured random targets, moved by a
small rigid motion, with 3 cm of noise on the coordinates and a perturbed identity as the guess.  With transformation_epsilon = 1e-6 pcl's ICP
needs between four and seven iterations on them, so the pairs of one batch leave its busy list in different rounds."""
import numpy as np

from oracle.replay import small_cloud

EPS = 1e-6
SIZES = [2500, 31, 2817, 1000, 3000, 2049, 777]  # one block of 32 queries, ragged last blocks, block counts that differ between the pairs


def make_pairs(targets, sizes, seed=11, noise_seed=12):
    """[(target index, source, guess)]: pair k against targets[k % len(targets)]"""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    rng, nrng = np.random.default_rng(seed), np.random.default_rng(noise_seed)
    pairs = []
    for k, n in enumerate(sizes):
        ti = k % len(targets)
        rel = synth.make_pose(rng.normal(0, 0.15, 3), synth.rot_xyz(*rng.normal(0, 0.015, 3)))
        src = orc.transform_points(np.linalg.inv(rel), targets[ti][:n])
        src[:, :3] += nrng.normal(0, 0.03, (n, 3)).astype(np.float32)
        pairs.append((ti, src, synth.perturb_pose(np.eye(4), rng)))
    return pairs


def batch_workload():
    targets = [small_cloud(4000, 300), small_cloud(3000, 301)]
    return targets, make_pairs(targets, SIZES)


def icp_params(reciprocal=False, eps=EPS, maximum_iterations=64):
    from mrg_slam_amd._lib import ICP_HIP
    from mrg_slam_amd.registration import default_params

    p = default_params(ICP_HIP)
    p.transformation_epsilon, p.maximum_iterations = eps, maximum_iterations
    p.use_reciprocal_correspondences = int(reciprocal)
    return p


def pose_errors(Ta, Tb):
    """(translation distance in metres, rotation angle in radians) between two 4 x 4 poses"""
    from mrg_slam_amd import synth

    Ta, Tb = np.asarray(Ta, dtype=np.float64), np.asarray(Tb, dtype=np.float64)
    return float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])), float(synth.rotation_angle(Ta[:3, :3], Tb[:3, :3]))
