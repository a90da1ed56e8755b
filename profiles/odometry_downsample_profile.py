"""mrgfe_odom_frame with downsample_method VOXELGRID 0.1, per frame: library against library.

  python profiles/odometry_downsample_profile.py time [--pairs 200] [--warmup 10] [--out FILE.json]
      SMALL_GICP_HIP and NDT_HIP over pair 0 of the street (VLP-64, ~130k points, and VLP-16, ~26k): `pairs` times mrgfe_odom_reset, the first frame (the
      downsampled cloud becomes the target) and the second frame (downsample, source, align from a warm prediction), each call timed on the host: medians
      and p95, the downsample route mrgfe_odom_stats reports (where the library has it), the points handed on and a checksum of the last result record.
      The library is the one MRGFE_LIB names (MRGFE_LIB_ALLOW_MISSING=1 for one older than the binding table).

  python profiles/odometry_downsample_profile.py ab LIB [LIB ...] [--rounds 2]
      `time` in a fresh child process per library file, the libraries alternating `rounds` times; the baseline is the parent commit's library.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_frames(args):
    import mrg_slam_amd as M
    from mrg_slam_amd import Context, HipOdometry, _lib, synth

    L = _lib.lib()
    ctx = Context(0)
    rows = []
    for sensor in ("VLP64", "VLP16"):
        tgt, src, rel = synth.scan_pair(0, sensor, synth.street_scene())
        clouds = [np.ascontiguousarray(tgt), np.ascontiguousarray(src)]
        delta = np.ascontiguousarray(synth.warm_guess(rel, 0).astype(np.float32).T)
        for method in ("SmallGicpHip", "NdtHip"):
            reg = getattr(M, method)(transformation_epsilon=0.01, ctx=ctx)
            odo = HipOdometry(reg, {"downsample_method": "VOXELGRID", "downsample_resolution": 0.1, "keyframe_delta_translation": 100.0})
            lay = _lib.KeyframeParams()
            out = _lib.OdomResult()
            ms = [[], []]
            for it in range(args.warmup + args.pairs):
                odo.reset()
                for k in (0, 1):
                    c = clouds[k]
                    L.mrgfe_keyframe_default_params(C.byref(lay))
                    lay.width = len(c)
                    t0 = time.perf_counter()
                    _lib.check(L.mrgfe_odom_frame(odo._h, C.byref(lay), c.ctypes.data_as(C.c_void_p), c.nbytes, 100.0 + 0.1 * k,
                                                  delta.ctypes.data_as(C.POINTER(C.c_float)) if k else None, 0, None, C.byref(out)))
                    if it >= args.warmup:
                        ms[k].append((time.perf_counter() - t0) * 1e3)
            try:
                route = odo.stats()["route"]
            except AttributeError:
                route = None
            row = {"sensor": sensor, "n": len(clouds[1]), "method": method, "first_frame_median_ms": round(float(np.median(ms[0])), 4),
                   "first_frame_p95_ms": round(float(np.percentile(ms[0], 95)), 4), "aligned_frame_median_ms": round(float(np.median(ms[1])), 4),
                   "aligned_frame_p95_ms": round(float(np.percentile(ms[1], 95)), 4), "route": route, "n_source": int(out.n_source), "outcome": int(out.outcome),
                   "iterations": int(out.iterations), "sha": hashlib.sha256(bytes(out)).hexdigest()[:12]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            odo.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def ab(args):
    for r in range(args.rounds):
        for lib in args.libs:
            env = dict(os.environ, MRGFE_LIB=os.path.abspath(lib), MRGFE_LIB_ALLOW_MISSING="1")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "time", "--pairs", str(args.pairs), "--warmup", str(args.warmup)], env=env, capture_output=True,
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
    t.add_argument("--pairs", type=int, default=200)
    t.add_argument("--warmup", type=int, default=10)
    t.add_argument("--out")
    a = sub.add_parser("ab")
    a.add_argument("libs", nargs="+")
    a.add_argument("--rounds", type=int, default=2)
    a.add_argument("--pairs", type=int, default=200)
    a.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    time_frames(args) if args.cmd == "time" else ab(args)
