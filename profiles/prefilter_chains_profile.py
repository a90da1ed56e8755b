"""The prefilter chains the device-driven form serves since the chain became three stages, per call: library against library.

  python profiles/prefilter_chains_profile.py time [--calls 200] [--warmup 20] [--out FILE.json]
      mrgfe_prefilter_device on the ~130k-point VLP-64 scan and the ~26k-point VLP-16 scan of the street for every newly served chain (distance filter on;
      NONE + RADIUS and APPROX_VOXELGRID also with it off): median and p95 of `calls` calls behind `warmup` calls, the route mrgfe_ctx_prefilter_stats
      reports, the point count and a checksum of the output, which must not depend on the library.  One JSON line per combination.
      The library is the one MRGFE_LIB names (MRGFE_LIB_ALLOW_MISSING=1 for one older than the binding table).

  python profiles/prefilter_chains_profile.py ab LIB [LIB ...] [--rounds 2]
      `time` in a fresh child process per library file, the libraries alternating `rounds` times: the baseline is the parent commit's library built to a
      second path (there every one of these chains runs the host-driven passes).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = {"enable_distance_filter": True, "downsample_method": "NONE", "downsample_resolution": 0.1, "outlier_removal_method": "NONE", "radius_radius": 0.5,
        "radius_min_neighbors": 2}
CHAINS = [("distance filter only", {}),
          ("VOXELGRID 0.1", {"downsample_method": "VOXELGRID"}),
          ("VOXELGRID 0.3 / min 2", {"downsample_method": "VOXELGRID", "downsample_resolution": 0.3, "downsample_min_points_per_voxel": 2}),
          ("NONE + RADIUS", {"outlier_removal_method": "RADIUS"}),
          ("NONE + RADIUS, no distance filter", {"outlier_removal_method": "RADIUS", "enable_distance_filter": False}),
          ("APPROX 0.1", {"downsample_method": "APPROX_VOXELGRID"}),
          ("APPROX 0.1, no distance filter", {"downsample_method": "APPROX_VOXELGRID", "enable_distance_filter": False}),
          ("APPROX 0.1 + RADIUS", {"downsample_method": "APPROX_VOXELGRID", "outlier_removal_method": "RADIUS"}),
          ("APPROX 0.3 + RADIUS", {"downsample_method": "APPROX_VOXELGRID", "downsample_resolution": 0.3, "outlier_removal_method": "RADIUS"})]


def time_chains(args):
    import torch

    from mrg_slam_amd import Context, prefilter_to_device, synth

    ctx = Context(0)
    rows = []
    for sensor in ("VLP64", "VLP16"):
        cloud = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), sensor, synth.BASE_SEED if sensor == "VLP64" else 4711))
        buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
        for name, more in CHAINS:
            p = dict(BASE, **more)
            for _ in range(args.warmup):
                m = prefilter_to_device(cloud, buf.data_ptr(), len(cloud), p, ctx=ctx)
            ms = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                m = prefilter_to_device(cloud, buf.data_ptr(), len(cloud), p, ctx=ctx)
                ms.append((time.perf_counter() - t0) * 1e3)
            route = ctx.prefilter_stats()["route"] if hasattr(ctx, "prefilter_stats") else None
            ctx.synchronize()
            row = {"sensor": sensor, "n": len(cloud), "chain": name, "median_ms": round(float(np.median(ms)), 4), "p95_ms": round(float(np.percentile(ms, 95)), 4),
                   "route": route, "points_out": int(m), "sha": hashlib.sha256(buf[:m].cpu().numpy().tobytes()).hexdigest()[:12]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def ab(args):
    for r in range(args.rounds):
        for lib in args.libs:
            env = dict(os.environ, MRGFE_LIB=os.path.abspath(lib), MRGFE_LIB_ALLOW_MISSING="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "time", "--calls", str(args.calls), "--warmup", str(args.warmup)], env=env, capture_output=True,
                                 text=True, timeout=600)
            if out.returncode != 0:
                print(out.stderr[-2000:], file=sys.stderr)
                sys.exit(out.returncode)
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    print(json.dumps(dict(json.loads(line), lib=lib, round=r)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--calls", type=int, default=200)
    t.add_argument("--warmup", type=int, default=20)
    t.add_argument("--out")
    a = sub.add_parser("ab")
    a.add_argument("libs", nargs="+")
    a.add_argument("--rounds", type=int, default=2)
    a.add_argument("--calls", type=int, default=200)
    a.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    time_chains(args) if args.cmd == "time" else ab(args)
