#!/usr/bin/env python3
"""LoopDetector::matching with registration_method "GICP" / "GICP_OMP" (PCL_GICP_HIP / PCL_GICP_OMP_HIP): K candidates of prefiltered loop-closure
size (the ~33k-point clouds of profiles/gicp_corr_modes.py prefiltered) against one new keyframe, wall time per matching() —
  sequential: one PclGicpHip registration, setInputTarget once, then per candidate setInputSource + align + getFitnessScore (the reference's loop,
              loop_detector.cpp:126-145, and the only route before batches took the two methods),
  batch:      one BatchMatcher on a context with set_bfgs_batches on: clear, add_target, K x add_pair, align(fitness range).
Both hand over host clouds; every repetition includes the target's covariances and grid.  python3 profiles/pclgicp_batch_profile.py [K ...]
Prints one JSON line per (method, K): median wall milliseconds of both routes, their ratio, the batch's rounds, the largest and the summed evaluation
count of the pairs, and whether the records were equal bit for bit."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FITNESS_RANGE = 4.5  # fitness_score_max_range of the loop detector
REPS = 5


def main():
    from mrg_slam_amd import BatchMatcher, Context, PclGicpHip, _lib, prefilter, synth
    from mrg_slam_amd.registration import default_params, result_matrix

    ks = [int(a) for a in sys.argv[1:]] or [1, 4, 8, 30]
    ctx = Context(0)
    ctx.set_bfgs_batches(True)
    scene = synth.street_scene()
    n_scans = 7
    poses = synth.arc_trajectory(n_scans)
    scans = [prefilter(synth.synth_lidar(scene, poses[k], "VLP64", synth.BASE_SEED + k), ctx=ctx) for k in range(n_scans)]
    target = scans[0]

    def candidate(k):  # a keyframe 1 .. 6 m away with a loop-closure-sized error on the guess (0.5 m / 2 deg)
        s = 1 + k % (n_scans - 1)
        rel = np.linalg.inv(poses[0]) @ poses[s]
        return scans[s], synth.perturb_pose(rel, np.random.default_rng(4242 + k), sigma_t=(0.5, 0.5, 0.1), sigma_r_deg=(0.5, 0.5, 2.0))

    for omp in (False, True):
        method = _lib.PCL_GICP_OMP_HIP if omp else _lib.PCL_GICP_HIP
        p = default_params(method)
        p.transformation_epsilon, p.maximum_iterations = 0.01, 64
        for K in ks:
            cands = [candidate(k) for k in range(K)]
            reg = PclGicpHip(transformation_epsilon=0.01, omp=omp, ctx=ctx)
            bm = BatchMatcher(p, ctx=ctx)
            t_seq, t_bat, singles, rec = [], [], None, None
            for rep in range(REPS + 1):
                ctx.synchronize()
                t0 = time.perf_counter()
                reg.setInputTarget(target)
                singles = []
                for src, guess in cands:
                    reg.setInputSource(src)
                    reg.align(guess)
                    singles.append((reg.getFinalTransformation(), reg.hasConverged(), reg.getFinalNumIteration(), reg.evals, reg.getFitnessScore(FITNESS_RANGE)))
                t_seq.append(time.perf_counter() - t0)
                ctx.synchronize()
                t0 = time.perf_counter()
                bm.clear()
                t = bm.add_target(target)
                for src, guess in cands:
                    bm.add_pair(t, src, guess)
                rec = bm.align(FITNESS_RANGE)
                t_bat.append(time.perf_counter() - t0)
            equal = all(np.array_equal(result_matrix(rec[k]), singles[k][0]) and (bool(rec[k]["converged"]), int(rec[k]["iterations"]), int(rec[k]["evaluations"])) == singles[k][1:4]
                        for k in range(K))
            seq_ms, bat_ms = 1e3 * float(np.median(t_seq[1:])), 1e3 * float(np.median(t_bat[1:]))
            evs = [int(r["evaluations"]) for r in rec]
            print(json.dumps({"method": "PCL_GICP_OMP_HIP" if omp else "PCL_GICP_HIP", "K": K, "points": [len(target)] + sorted({len(c[0]) for c in cands}),
                              "sequential_ms": round(seq_ms, 3), "batch_ms": round(bat_ms, 3), "sequential_over_batch": round(seq_ms / bat_ms, 3), "rounds": bm.rounds(),
                              "max_evaluations": max(evs), "sum_evaluations": sum(evs), "iterations": [int(r["iterations"]) for r in rec],
                              "converged": int(sum(int(r["converged"]) for r in rec)), "records_equal": bool(equal)}), flush=True)


if __name__ == "__main__":
    main()
