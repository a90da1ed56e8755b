"""ICP_HIP over a loop-closure-sized candidate list: 32 candidates against one keyframe, the shape of bench.py's `batch_32_candidates` (raw VLP-64
scans of the synthetic street behind the distance filter, ~130k points each; keyframe = scan 0, candidates = scans 1..4 in turn, warm guesses with
seeds 7000 + b, clouds resident in HBM, no fitness score).  ONE workload per invocation, in a fresh process:

  python profiles/icp_batch_profile.py --route batch|sequential [--reciprocal] [--eps 0.1] [--reps 6] [--out FILE.jsonl]

    batch        clear + add_device + align of one BatchMatcher(ICP_HIP): the lock-step rounds, one host wait per round
    sequential   one IcpHip object, setInputTarget once, then setInputSource + align candidate after candidate, the way LoopDetector::matching
                 (loop_detector.cpp:104-145) drives the registration: three stream waits per iteration and candidate

A call is timed from a device synchronise to a device synchronise; the first call (grid builds into cold buffers, allocations) is dropped, the figure is the
median of the rest.  Prints one JSON line: ms per call, ms per alignment, rounds (batch: lock-step rounds of the call; sequential: correspondence rounds
added up over the candidates), and a checksum of the final transformations, which the two routes of one mode must share.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def workload():
    """(host clouds, guesses [32, 4, 4], candidate scan per pair): generated before the process touches the GPU"""
    from mrg_slam_amd import synth

    scene = synth.street_scene(seed=1234, x_range=(-120.0, 420.0))
    poses = synth.weave_trajectory(5)
    scans = synth.synth_lidar_many(scene, poses, "VLP64", [synth.BASE_SEED + k for k in range(5)], cache_tag="street_r0_n5")
    cand = [1 + b % 4 for b in range(32)]
    guesses = np.stack([synth.warm_guess(synth.rel_pose(poses[0], poses[k]), 7000 + b) for b, k in enumerate(cand)])
    return scans, guesses, cand


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("batch", "sequential"), required=True)
    ap.add_argument("--reciprocal", action="store_true")
    ap.add_argument("--eps", type=float, default=0.1, help="reg_transformation_epsilon (bench.py's default)")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    raw, guesses, cand = workload()
    import torch

    from mrg_slam_amd import BatchMatcher, Context, IcpHip, distance_filter
    from mrg_slam_amd._lib import ICP_HIP
    from mrg_slam_amd.registration import default_params, result_matrix

    ctx = Context(0)
    host = [distance_filter(s, 0.1, 35.0, ctx=ctx) for s in raw]
    dev = [torch.from_numpy(s).to(torch.device("cuda", 0)) for s in host]
    torch.cuda.synchronize()
    times, finals, rounds = [], None, 0
    if a.route == "batch":
        p = default_params(ICP_HIP)
        p.transformation_epsilon = a.eps
        p.use_reciprocal_correspondences = int(a.reciprocal)
        bm = BatchMatcher(p, ctx)
        args = ([dev[0].data_ptr()], [len(host[0])], np.zeros(32, dtype=np.int32), [dev[k].data_ptr() for k in cand], [len(host[k]) for k in cand], guesses)
        for _ in range(a.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            bm.clear()
            bm.add_device(*args)
            rec = bm.align(-1.0)
            ctx.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        finals = np.stack([result_matrix(r) for r in rec])
        rounds, iterations, converged = bm.rounds(), [int(x) for x in rec["iterations"]], int(rec["converged"].sum())
    else:
        reg = IcpHip(transformation_epsilon=a.eps, use_reciprocal_correspondences=a.reciprocal, ctx=ctx)
        for _ in range(a.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            reg.setInputTargetDevice(dev[0].data_ptr(), len(host[0]))
            finals, iterations, converged, rounds = [], [], 0, 0
            for b, k in enumerate(cand):
                reg.setInputSourceDevice(dev[k].data_ptr(), len(host[k]))
                reg.align(guesses[b])
                finals.append(reg.getFinalTransformation())
                iterations.append(reg.getFinalNumIteration())
                converged += int(reg.hasConverged())
                rounds += reg.evals
            ctx.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        finals = np.stack(finals)
    ms = float(np.median(times[1:])) if len(times) > 1 else float(times[0])
    row = {"route": a.route, "reciprocal": bool(a.reciprocal), "eps": a.eps, "pairs": 32, "points_per_cloud": int(np.mean([len(host[k]) for k in cand])),
           "ms_per_call": ms, "ms_per_alignment": ms / 32.0, "ms_first_call": float(times[0]), "ms_calls": [round(t, 3) for t in times], "rounds": int(rounds),
           "iterations": iterations, "converged": converged, "finals_sha16": hashlib.sha256(np.ascontiguousarray(finals, dtype=np.float32).tobytes()).hexdigest()[:16]}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
