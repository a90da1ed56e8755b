"""The first-keyframe ground fill on the Ouster configuration's shape (config/mrg_slam_ouster.yaml:158-160: radius 7.5, RANSAC; map_cloud_resolution 0.05:
150 rings x 943 angles = 141450 generated points) behind a 33k-point keyframe: the street scene's VLP-64 scan behind the default prefilter, thinned evenly
to 33000 points.

  python profiles/ground_fill_profile.py time [--out FILE.json] [--calls 15] [--cloud FILE.npy]
      End-to-end milliseconds per mrgfe_map_store_fill_ground call, profiler off, both variants, with and without the download of the filled cloud: each
      call fills the same stored keyframe into a fresh key of a fresh store (the call runs once per session; nothing is warm but the context's buffers,
      which the first, untimed call of each variant grows).  Median, minimum and maximum of `calls`.  The RANSAC share is the RANSAC variant's median
      minus the simple variant's: the two differ in nothing else.  The output of every variant is compared with the host entry point's before timing.

  python profiles/ground_fill_profile.py once --variant ransac|simple --cloud FILE.npy
      One fill and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`: the kernel's own time and the launch counts.  The cloud is read
      from FILE.npy (a `time` run with the same --cloud writes it), so that the traced process launches nothing else.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADIUS, RESOLUTION, POINTS = 7.5, 0.05, 33000


def keyframe_cloud(path: str):
    from mrg_slam_amd import prefilter, synth

    if path and os.path.exists(path):
        return np.ascontiguousarray(np.load(path), dtype=np.float32)
    c = np.ascontiguousarray(prefilter(synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED)))
    if len(c) > POINTS:
        c = np.ascontiguousarray(c[np.linspace(0, len(c) - 1, POINTS).astype(np.int64)])
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.save(path, c)
    return c


def run_time(args):
    from mrg_slam_amd import MapCloudStore, default_context, fill_ground_plane

    cloud = keyframe_cloud(args.cloud)
    ctx = default_context()
    est = np.eye(4)
    out = {"points": int(len(cloud)), "radius": RADIUS, "map_resolution": RESOLUTION, "calls": args.calls, "variants": {}}
    for variant in ("simple", "ransac"):
        simple = variant == "simple"
        ref, info = fill_ground_plane(cloud, RADIUS, RESOLUTION, simple=simple, estimate=est)
        for want_cloud in (True, False):
            ms = []
            for call in range(args.calls + 1):
                store = MapCloudStore()
                store.add(1, cloud)
                ctx.synchronize()
                t0 = time.perf_counter()
                got, info2 = store.fill_ground(1, 2, RADIUS, RESOLUTION, simple=simple, estimate=est, want_cloud=want_cloud)
                t1 = time.perf_counter()
                if call:  # (the first call grows the context's buffers)
                    ms.append((t1 - t0) * 1e3)
                elif want_cloud:
                    assert got.tobytes() == ref.tobytes() and info2["n_added"] == info["n_added"]
                del store
            # (the wrapper's own numpy allocation of the output buffer is inside the clock when the cloud is wanted)
            out["variants"][f"{variant}{'' if want_cloud else '_no_download'}"] = {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
                                                                                   "n_rings": info["n_rings"], "n_angles": info["n_angles"], "n_added": info["n_added"],
                                                                                   "ransac_iterations": info["ransac_iterations"], "has_model": info["has_model"]}
    v = out["variants"]
    out["ransac_share_ms"] = v["ransac_no_download"]["median_ms"] - v["simple_no_download"]["median_ms"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def run_once(args):
    from mrg_slam_amd import MapCloudStore

    cloud = keyframe_cloud(args.cloud)
    store = MapCloudStore()
    store.add(1, cloud)
    _, info = store.fill_ground(1, 2, RADIUS, RESOLUTION, simple=args.variant == "simple", estimate=np.eye(4), want_cloud=False)
    print(json.dumps({"variant": args.variant, "points": int(len(cloud)), "n_added": info["n_added"], "ransac_iterations": info["ransac_iterations"]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "once"))
    ap.add_argument("--out", default="")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--cloud", default="")
    ap.add_argument("--variant", choices=("ransac", "simple"), default="ransac")
    a = ap.parse_args()
    (run_time if a.mode == "time" else run_once)(a)
