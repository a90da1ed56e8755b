"""Bounded best-candidate selection (BatchMatcher.align_best) against the full fitness path (BatchMatcher.align) on BASELINE config[3]: 256
loop-closure pairs from bench.make_loop_workload, getFitnessScore(inf), groups = new keyframes.  Full and bounded steps alternate in one process
after a warm-up, each timed to a device synchronisation; the fitness share of a step comes from mrgfe_batch_fitness_stats (full) and
mrgfe_batch_select_stats (bounded).  Then bench.run_detect_leg's shape (8 new keyframes against 4 laps of the ring) with fitness_selection set
both ways.  Prints one JSON object.

    python profiles/select_best_profile.py [--steps 10] [--warmup 2] [--no-detect]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-detect", action="store_true")
    args = ap.parse_args()

    import torch

    import bench
    from mrg_slam_amd import BatchMatcher, distance_filter, loop_detector
    from mrg_slam_amd._lib import NDT_HIP, SEARCH
    from mrg_slam_amd.registration import default_context, default_params

    raw, pairs = bench.make_loop_workload()
    scans = [distance_filter(s, 0.1, 35.0) for s in raw]
    dev = [torch.from_numpy(s).cuda() for s in scans]
    news = sorted({p[0] for p in pairs})
    group = np.array([news.index(p[0]) for p in pairs], dtype=np.int32)
    bm = BatchMatcher(transformation_epsilon=0.1, maximum_iterations=64)
    ctx = default_context()

    def queue():
        bm.clear()
        bm.add_device([dev[a].data_ptr() for a in news], [len(scans[a]) for a in news], np.array([news.index(p[0]) for p in pairs], dtype=np.int32),
                      [dev[p[1]].data_ptr() for p in pairs], [len(scans[p[1]]) for p in pairs], np.stack([p[2] for p in pairs]))

    times = {"full": [], "bounded": []}
    fit_ms = {"full": [], "bounded": []}
    counts = None
    ref = None
    for k in range(args.warmup + args.steps):
        for mode in ("full", "bounded"):
            queue()
            ctx.synchronize()
            t0 = time.perf_counter()
            if mode == "full":
                rec = bm.align(float("inf"))
            else:
                rec, state, best, score = bm.align_best(float("inf"), group)
            ctx.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            if mode == "full":
                fs = bm.fitness_stats()
                f_ms = fs["ms_block"] + fs["ms_sweep"] + fs["ms_far"]
                ref = rec
            else:
                ss = bm.select_stats()
                f_ms = ss["ms_bound"] + ss["ms_contend"]
                counts = {key: int(ss[key]) for key in ("exact", "pruned", "above_cap", "skipped", "to_sweep", "to_far")}
                ex = state == 0
                assert (rec["fitness"][ex] == ref["fitness"][ex]).all()
            if k >= args.warmup:
                times[mode].append(dt)
                fit_ms[mode].append(f_ms)
    out = {
        "what": "config[3]: 256 pairs, 64 new keyframes as groups, fitness_max_range inf, one GPU; median over steps, full and bounded alternating",
        "steps": args.steps,
        "full_step_ms": float(np.median(times["full"])),
        "bounded_step_ms": float(np.median(times["bounded"])),
        "full_fitness_ms": float(np.median(fit_ms["full"])),
        "full_fitness_note": "device ms of the block + seed/sweep + walk passes (HIP events; the early pass beside the rounds included)",
        "bounded_fitness_ms": float(np.median(fit_ms["bounded"])),
        "bounded_fitness_note": "host ms of the bound stage + the contender stage (both waits included)",
        "bounded_counts": counts,
    }
    if not args.no_detect:
        prm = default_params(NDT_HIP)
        prm.transformation_epsilon, prm.maximum_iterations, prm.resolution, prm.nn_search_method = 0.1, 64, 1.0, SEARCH["DIRECT7"]
        legs = {}
        for mode in ("full", "bounded"):
            loop_detector.DEFAULTS["fitness_selection"] = mode  # run_detect_leg builds its LoopDetector from the defaults
            try:
                legs[mode] = bench.run_detect_leg(ctx, prm, raw)
            finally:
                loop_detector.DEFAULTS["fitness_selection"] = "full"
        out["detect_leg"] = {mode: {g: {k: v for k, v in legs[mode][g].items() if k in ("detect_batched_ms", "superset_pairs", "loops", "same_loops")}
                                    for g in ("no_gating", "default_gates")} for mode in legs}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
