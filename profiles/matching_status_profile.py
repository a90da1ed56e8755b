"""The scan-matching status as one call against the three calls it replaces, on one VLP-64 pair of the synthetic street (raw scans, ~130k points
each), for NDT_OMP and FAST_GICP.

  python profiles/matching_status_profile.py time [--out FILE.json] [--windows 15] [--calls 5]
      End-to-end times, profiler off.  Routes, timed in the same process on the same pair, alternating window by window:
        old           mrgfe_reg_align with the aligned cloud downloaded -> mrgfe_reg_fitness -> mrgfe_reg_nn1_target of the aligned cloud -> the host count
        new           mrgfe_reg_align without the download -> mrgfe_reg_matching_status
        align_only    mrgfe_reg_align without the download: what both routes share
        fitness_only  mrgfe_reg_fitness alone, after an align
        status_only   mrgfe_reg_matching_status alone, after an align: expected to cost about one fitness_only
      A window is `calls` calls behind a warm-up of every route and ends in a device synchronise; the figure of a window is its time per call.
      Reported per route: median, 10th and 90th percentile of the windows.  The two routes' numbers are compared before anything is timed.

  python profiles/matching_status_profile.py once --route old|new --method NDT_OMP|FAST_GICP
      One status of one route behind one align, for `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ...`: the launch and copy
      counts (subtract those of `--route align_only`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

METHODS = ("NDT_OMP", "FAST_GICP")
ROUTES = ("old", "new", "align_only", "fitness_only", "status_only")
DIST = 0.5  # scan_matching_odometry_component.cpp:405


class Pair:
    def __init__(self, method: str):
        from mrg_slam_amd import Context, select_registration_method, synth

        self.ctx = Context(0)
        tgt, src, rel = synth.scan_pair(0, "VLP64", synth.street_scene())
        self.n = len(src)
        self.guess = np.eye(4, dtype=np.float32)
        self.reg = select_registration_method({"registration_method": method}, ctx=self.ctx)
        self.reg.setInputTarget(tgt)
        self.reg.setInputSource(src)

    def old(self):
        aligned = self.reg.align(self.guess, want_aligned=True)
        err = self.reg.getFitnessScore()
        _, sqd = self.reg.nearestKSearch1(aligned)
        inliers = int(np.count_nonzero(sqd.astype(np.float64) < DIST * DIST))
        return err, inliers, np.float32(inliers) / np.float32(len(aligned))

    def new(self):
        self.reg.align(self.guess)
        s = self.reg.matchingStatus(DIST)
        return s.matching_error, s.num_inliers, s.inlier_fraction

    def run(self, route: str):
        if route == "old":
            return self.old()
        if route == "new":
            return self.new()
        if route == "align_only":
            return self.reg.align(self.guess)
        if route == "fitness_only":
            return self.reg.getFitnessScore()
        return self.reg.matchingStatus(DIST)


def time_routes(args):
    rows = []
    for method in METHODS:
        p = Pair(method)
        for route in ROUTES:
            for _ in range(3):
                p.run(route)
        a, b = p.old(), p.new()
        assert a == b, f"{method}: the routes differ: old {a}, new {b}"
        per = {route: [] for route in ROUTES}
        for _ in range(args.windows):
            for route in ROUTES:  # alternating: a drift of the machine lands on every route alike
                p.ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    p.run(route)
                p.ctx.synchronize()
                per[route].append(1e3 * (time.perf_counter() - t0) / args.calls)
        for route in ROUTES:
            v = np.array(per[route])
            rows.append({"method": method, "route": route, "points": p.n, "matching_error": a[0], "inliers": a[1], "windows": args.windows, "calls_per_window": args.calls,
                         "ms_median": float(np.median(v)), "ms_p10": float(np.percentile(v, 10)), "ms_p90": float(np.percentile(v, 90))})
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def once(args):
    p = Pair(args.method)
    out = p.run(args.route)
    p.ctx.synchronize()
    print(json.dumps({"method": args.method, "route": args.route, "points": p.n, "result": None if out is None or args.route == "align_only" else [float(x) for x in np.atleast_1d(out)]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--out", default="")
    t.add_argument("--windows", type=int, default=15)
    t.add_argument("--calls", type=int, default=5)
    o = sub.add_parser("once")
    o.add_argument("--route", choices=("old", "new", "align_only"), required=True)
    o.add_argument("--method", choices=METHODS, default="NDT_OMP")
    a = ap.parse_args()
    (time_routes if a.cmd == "time" else once)(a)
