"""LoopDetector::detect as one call (mrgfe_loop_detect) against the routes it replaces, profiler off, on one MI355X.

  python profiles/loop_detect_profile.py [--out FILE.json] [--reps 15] [--methods NDT_HIP,SMALL_GICP_HIP] [--workloads config3,ring]

Three routes over the SAME kind of batch and the same map store, timed in one process, alternating repetition by repetition:
  one_call           HipLoopDetector.detect: supersets, stage 1, mrgfe_batch_clear_pairs, stage 2 on the built targets, replay — inside libmrgfe.so
  mirror             LoopDetector.detect_batched(matcher=BatchMatcher, store=): the composed route of the parent commit — the same two batches queued from
                     Python with mrgfe_batch_clear between them (stage 2 builds its targets again), gates replayed in Python
  one_call_no_reuse  the one call with mrgfe_dbg_loop_set_stage_reuse(0): stage 2 clears the batch and builds its targets again; against one_call this
                     isolates the stage-2 target builds from everything else the one call saves

Two workloads:
  config3  a detect() call of 8 new keyframes x ~30 candidates (bench.py's run_detect_leg: 4 laps of the 64-keyframe ring are the graph, 8 consecutive
           keyframes of the next lap arrive in one call).  A repetition is one call from a reset LoopManager; the figure is ms per detect().
  ring     the ring session of tests/loop_session.py (64 keyframes, 6 per call, the loops become graph edges).  A repetition is the whole session from
           a reset LoopManager; the figure is ms per detect() call that had candidates = session time over those calls.
Every repetition ends in a device synchronise.  One warm-up repetition of every route comes first (code objects, the GICP covariance cache of the batch's
keyframe store, buffer growth).  Reported per route: median, minimum, 10th and 90th percentile over the repetitions; per pair of routes the median of the
per-repetition differences (the routes of one repetition run back to back) with its 10th and 90th percentile — a difference whose interval holds 0 is
within the run-to-run spread.  The Loop lists of the three routes are compared before anything is timed (the mirror from numpy's guesses: keys only)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUTES = ("one_call", "mirror", "one_call_no_reuse")


def params(method):
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params

    prm = default_params(getattr(_lib, method))
    prm.transformation_epsilon, prm.maximum_iterations = 0.01, 64
    return prm


def config3_workload(ctx):
    """bench.py's run_detect_leg: (known keyframes, [the one call's new keyframes])"""
    from mrg_slam_amd import distance_filter, synth
    from mrg_slam_amd.loop_detector import Edge, KeyFrame

    n_ring, radius, laps, n_new = 64, 40.0, 4, 8
    scene = synth.loop_scene(radius=radius)
    poses = synth.loop_trajectory(n_ring, radius)
    raw = synth.synth_lidar_many(scene, poses, "VLP64", [synth.BASE_SEED + 5000 + k for k in range(n_ring)], workers=16, cache_tag=f"loop_k{n_ring}_r{int(radius)}")
    clouds = [distance_filter(s, 0.1, 35.0, ctx=ctx) for s in raw]
    circ = 2.0 * np.pi * radius
    rng = np.random.default_rng(4243)
    kfs = []
    for lap in range(laps + 1):
        for k in range(n_ring):
            est = synth.perturb_pose(poses[k], rng, sigma_t=(0.3, 0.3, 0.05), sigma_r_deg=(0.3, 0.3, 1.0))
            kf = KeyFrame(id=len(kfs) + 1, cloud=clouds[k], estimate=est, accum_distance=lap * circ + circ * k / n_ring, slam_uuid="a", first_keyframe=(len(kfs) == 0))
            if kfs:
                prev = kfs[-1]
                rel = np.linalg.inv(kf.estimate) @ prev.estimate
                kf.prev_edge = Edge(kf, prev, rel)
                prev.next_edge = Edge(kf, prev, rel)
                kf.connected.add(prev.id)
                prev.connected.add(kf.id)
            kfs.append(kf)
    first_new = laps * n_ring + 10
    known, new = kfs[:first_new], kfs[first_new: first_new + n_new]  # (every neighbour of a known keyframe is known or new)
    new[-1].next_edge = None
    return known + new, [(known, new)]


def ring_workload(ctx):
    from loop_session import make_ring_session
    from mrg_slam_amd import prefilter

    kfs, order = make_ring_session(64, "VLP64", prefilter=lambda c: prefilter(c, {"downsample_resolution": 0.2}, ctx=ctx))
    return kfs, (kfs, order)


class Session:
    """one route over one workload: run() = one repetition, returns (seconds, calls with candidates, loops)"""

    def __init__(self, route, method, ctx, store, everything, calls):
        from mrg_slam_amd import BatchMatcher, HipLoopDetector
        from mrg_slam_amd.loop_detector import LoopDetector, LoopManager

        self.route, self.ctx, self.everything, self.calls = route, ctx, everything, calls
        self.connected = [set(k.connected) for k in everything]
        self.bm = BatchMatcher(params(method), ctx)
        if route == "mirror":
            self.det = LoopDetector(matcher=self.bm, store=store)
            self._reset = lambda: setattr(self.det, "loop_manager", LoopManager())
            self._detect = self.det.detect_batched
        else:
            self.det = HipLoopDetector(None, self.bm, store)
            self.det.set_stage_reuse(route == "one_call")
            self._reset = self.det.reset
            self._detect = self.det.detect

    def _call_list(self):
        if isinstance(self.calls, list):
            yield from self.calls
            return
        kfs, order = self.calls  # the ring session: six keyframes per call
        known = []
        for g0 in range(0, len(order), 6):
            new = [kfs[i] for i in order[g0:g0 + 6]]
            yield known, new
            known += new

    def run(self):
        for k, c in zip(self.everything, self.connected):
            k.connected = set(c)
        self._reset()
        loops, busy, builds = [], 0, 0
        self.ctx.synchronize()
        t0 = time.perf_counter()
        for known, new in self._call_list():
            self.det.last_batched = None
            found = self._detect(known, new)
            for lp in found:
                lp.key1.connected.add(lp.key2.id)
                lp.key2.connected.add(lp.key1.id)
            loops += found
            if self.det.last_batched is not None:
                busy += 1
                builds += getattr(self.det, "last_target_builds", 0)
        self.ctx.synchronize()
        return time.perf_counter() - t0, busy, loops, builds


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--methods", default="NDT_HIP,SMALL_GICP_HIP")
    ap.add_argument("--workloads", default="config3,ring")
    args = ap.parse_args()
    from mrg_slam_amd import Context, MapCloudStore

    ctx = Context(0)
    out = {"reps": args.reps, "unit": "ms per detect() call that had candidates", "results": {}}
    for wl in args.workloads.split(","):
        everything, calls = (config3_workload if wl == "config3" else ring_workload)(ctx)
        store = MapCloudStore(ctx)
        for kf in everything:
            store.add(kf.store_key(), kf.cloud)
        for method in args.methods.split(","):
            sessions = {r: Session(r, method, ctx, store, everything, calls) for r in ROUTES}
            # warm-up, and the three routes give the same loops
            first = {r: s.run() for r, s in sessions.items()}
            keys = {r: [(lp.key1.id, lp.key2.id) for lp in f[2]] for r, f in first.items()}
            poses = {r: [lp.relative_pose.tobytes() for lp in f[2]] for r, f in first.items()}
            assert keys["one_call"] == keys["mirror"] == keys["one_call_no_reuse"], keys
            assert poses["one_call"] == poses["one_call_no_reuse"]
            busy = first["one_call"][1]
            ms = {r: [] for r in ROUTES}
            for rep in range(args.reps):
                for r in (ROUTES if rep % 2 == 0 else ROUTES[::-1]):
                    dt, b, _, _ = sessions[r].run()
                    assert b == busy
                    ms[r].append(1e3 * dt / busy)
            rec = {r: spread(ms[r]) for r in ROUTES}
            diff = lambda a, b: spread(np.asarray(ms[a]) - np.asarray(ms[b]))  # noqa: E731
            rec["mirror_minus_one_call"] = diff("mirror", "one_call")
            rec["no_reuse_minus_one_call"] = diff("one_call_no_reuse", "one_call")  # the stage-2 target builds
            st = sessions["one_call"].det.stats()
            rec["calls_with_candidates"] = busy
            rec["loops"] = len(keys["one_call"])
            rec["target_builds_per_repetition"] = {"one_call": first["one_call"][3], "one_call_no_reuse": first["one_call_no_reuse"][3]}
            rec["last_call"] = st
            rec["points_per_cloud"] = int(np.mean([len(k.cloud) for k in everything]))
            out["results"][f"{wl}/{method}"] = rec
            print(f"[loop_detect_profile] {wl}/{method}: " + ", ".join(f"{r} {rec[r]['median']:.2f} ms" for r in ROUTES), file=sys.stderr, flush=True)
            del sessions
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
