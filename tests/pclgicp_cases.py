"""Inputs shared by tests/test_gpu_pclgicp_batch.py: the candidates of tests/icp_cases.py (cut out of structured random targets of 4000 / 3000 points,
moved by a small rigid motion, 3 cm of noise, a perturbed identity as the guess) with transformation_epsilon = 0.01.  The source sizes hold one tile
of fewer than 256 points, odd n (the terms' n_pad), a tile boundary + 1 and ragged last blocks.

Checked on the CPU with orc.PclGicp (the oracle, not the code under test; ``PYTHONPATH=. python tests/pclgicp_cases.py`` prints it): all seven pairs converge,
in 2, 3 or 4 outer iterations, after 108 .. 292 functor evaluations that differ between the pairs — for serial pcl::GICP and for pclomp's sums of
8 threads alike — so the pairs of one batch leave its busy list in different rounds.  Check the same before adding a size."""
import numpy as np

from icp_cases import SIZES, make_pairs, pose_errors  # noqa: F401
from oracle.replay import small_cloud

EPS = 0.01


def batch_workload():
    targets = [small_cloud(4000, 300), small_cloud(3000, 301)]
    return targets, make_pairs(targets, SIZES)


def pcl_params(omp=False, num_threads=0, eps=EPS, maximum_iterations=64, max_optimizer_iterations=20):
    from mrg_slam_amd._lib import PCL_GICP_HIP, PCL_GICP_OMP_HIP
    from mrg_slam_amd.registration import default_params

    p = default_params(PCL_GICP_OMP_HIP if omp else PCL_GICP_HIP)
    p.transformation_epsilon, p.maximum_iterations, p.max_optimizer_iterations = eps, maximum_iterations, max_optimizer_iterations
    p.num_threads = num_threads
    return p


def oracle_for(params):
    """the CPU oracle with the sums the HIP method reproduces for these parameters"""
    from mrg_slam_amd._lib import PCL_GICP_OMP_HIP
    from oracle import oracle as orc

    omp = params.method == PCL_GICP_OMP_HIP
    threads = (params.num_threads if params.num_threads > 0 else 8) if omp else 1
    return orc.PclGicp(params.correspondence_randomness, params.max_correspondence_distance, params.transformation_epsilon, params.rotation_epsilon,
                       params.maximum_iterations, params.max_optimizer_iterations, omp=omp, num_threads=4, sum_threads=threads)


def oracle_results(params, targets, pairs):
    """[(T, converged, iterations, evaluations)] of the oracle, pair by pair"""
    out = []
    for ti, src, guess in pairs:
        o = oracle_for(params)
        o.setInputTarget(targets[ti])
        o.setInputSource(src)
        o.align(guess)
        out.append((o.getFinalTransformation(), o.hasConverged(), o.getFinalNumIteration(), o.evals))
    return out


if __name__ == "__main__":
    tg, pr = batch_workload()
    for omp in (False, True):
        res = oracle_results(pcl_params(omp), tg, pr)
        print("GICP_OMP (8 threads)" if omp else "GICP", [(c, it, ev) for _, c, it, ev in res])
