"""LoopDetector::detect as one call over a NODE (mrgfe_loop_create_node) against the same call over one batch, profiler off.

  python profiles/loop_detect_node_profile.py [--out FILE.json] [--reps 20] [--warmup 3] [--methods NDT_HIP]

The workload is the config3 detect() call of profiles/loop_detect_profile.py (8 new keyframes x ~30 candidates, every keyframe in a MapCloudStore on
device 0).  One repetition is one detect() from a reset LoopManager, ended by a device synchronise.  Routes:
  batch        (a) HipLoopDetector over a BatchMatcher: the route of the parent commit, the baseline
  devices_N    (b) over a NodeMatcher of N = 1, 2, 4, 8 members on DISTINCT devices 0 .. N - 1, as far as the machine has them: member 0 reads the store in
               place, the others keep replicas of the keyframes their blocks name
  shared_N     (c) over N members that share device 0 (all read the store in place)
  shared_N_copy    (c) with mrgfe_dbg_node_set_store_copy(1): every member reads replicas — the replica route on one card
Per route: the FIRST call (replicas cold, code objects and workspaces too — the batch route's first call is the yardstick for that part), the bytes
resident in the node after it (replicas; for the GICP family the covariance caches as well), then `--warmup` unrecorded calls and the median, 95th
percentile and minimum of `--reps` calls.  The routes run one after the other, not interleaved: a node holds a thread and a context per member.  The loops
of every route are compared with the batch route's before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--methods", default="NDT_HIP")
    args = ap.parse_args()
    import torch
    from loop_detect_profile import config3_workload, params

    from mrg_slam_amd import BatchMatcher, Context, HipLoopDetector, MapCloudStore, NodeMatcher

    ctx = Context(0)
    everything, calls = config3_workload(ctx)
    known, new = calls[0]
    store = MapCloudStore(ctx)
    for kf in everything:
        store.add(kf.store_key(), kf.cloud)
    n_dev = torch.cuda.device_count()
    out = {"reps": args.reps, "warmup": args.warmup, "devices": n_dev, "unit": "ms per detect()", "points_per_cloud": int(np.mean([len(k.cloud) for k in everything])), "results": {}}

    def one(det):
        det.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        found = det.detect(known, new)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), [(lp.key1.id, lp.key2.id, lp.relative_pose.tobytes(), lp.score) for lp in found]

    for method in args.methods.split(","):
        routes = [("batch", None, 0)]
        routes += [(f"devices_{n}", list(range(n)), 0) for n in (1, 2, 4, 8) if n <= n_dev]
        routes += [(f"shared_{n}", [0] * n, 0) for n in (2, 4, 8)]
        routes += [(f"shared_{n}_copy", [0] * n, 1) for n in (1, 2, 4)]
        want = None
        for name, devices, copy in routes:
            if devices is None:
                matcher = BatchMatcher(params(method), ctx)
            else:
                matcher = NodeMatcher(devices, params(method))
                matcher.set_store_copy(copy)
            det = HipLoopDetector(None, matcher, store)
            first_ms, loops = one(det)
            if want is None:
                want = loops
            assert loops == want, name
            resident = matcher.store_bytes()
            for _ in range(args.warmup):
                one(det)
            ms = np.array([one(det)[0] for _ in range(args.reps)])
            st = det.stats()
            rec = {"first_call_ms": first_ms, "resident_bytes_after_first_call": int(resident), "median": float(np.median(ms)), "p95": float(np.percentile(ms, 95)),
                   "min": float(ms.min()), "n": int(ms.size), "superset_pairs": st["superset_pairs"], "consistency_pairs": st["consistency_pairs"], "loops": len(loops)}
            if devices is not None:
                rec["last_align_store_stats"] = matcher.store_stats()
            out["results"][f"{method}/{name}"] = rec
            print(f"[loop_detect_node_profile] {method}/{name}: first {first_ms:.1f} ms, median {rec['median']:.2f} ms, p95 {rec['p95']:.2f} ms, resident {resident} B", file=sys.stderr, flush=True)
            det.close()
            del det, matcher
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
