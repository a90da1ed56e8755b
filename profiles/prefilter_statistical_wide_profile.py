"""[distance filter] -> VOXELGRID(0.1) | NONE -> STATISTICAL with statistical_mean_k 64 .. 255 through mrgfe_scan_callback_device, per raw scan: the
device-driven chain behind mrgfe_ctx_set_wide_statistical_chains (nn_knn_mean_dd_wide_kernel<R>: no neighbour rows, one wait) against the host-driven passes
of a library without the switch (route 0: [n][mean_k + 1] rows written and read back).

  python profiles/prefilter_statistical_wide_profile.py time [--switch 1] [--calls 40] [--warmup 10] [--ks 64,100,255,20,63]
      every configuration (2 sensors x 2 chains x the mean_k list) in THIS process, one JSON line each: median and p25 / p75 of `calls` calls behind `warmup`
      calls (host clock around a call that ends in the chain's wait), the route, the point count and a checksum of the output, and the k-NN launch's
      HIP-event time (mrgfe_ctx_knn_stats).  The library is the one MRGFE_LIB names; --switch is ignored by a library that has no switch.

  python profiles/prefilter_statistical_wide_profile.py ab PARENT_LIB THIS_LIB [--rounds 3] [--calls 40]
      `time` in a fresh child process per library and round, the two libraries alternating; then the table of profiles/prefilter_statistical_wide_summary.md
      on stdout (per configuration the median over the rounds, and the spread of the rounds' medians).  mean_k 20 and 63 are the regression check of the
      narrow path: both libraries serve them on route 1 with the same kernel.

  python profiles/prefilter_statistical_wide_profile.py sweep [--calls 30]
      NONE -> STATISTICAL at mean_k 64 / 100 / 255 under other rules of the device-sized grid (start edge, crowding target, most halvings), one process.
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

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
CHAINS = {"VOXELGRID": {"downsample_method": "VOXELGRID", "downsample_resolution": 0.1, "downsample_min_points_per_voxel": 1}, "NONE": {"downsample_method": "NONE"}}
SENSORS = ("VLP16", "VLP64")


def chain_params(chain, k):
    return dict({"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "outlier_removal_method": "STATISTICAL",
                 "statistical_mean_k": k, "statistical_stddev": 1.0}, **CHAINS[chain])


def scan_of(sensor):
    from mrg_slam_amd import synth

    return np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), sensor, synth.BASE_SEED if sensor == "VLP64" else 4711))


def set_rule(rule):
    import ctypes as C

    from mrg_slam_amd._lib import lib

    s, t, h = rule if rule else (0.0, 0.0, 0)
    lib().mrgfe_dbg_set_sor_grid_rule(C.c_float(s), C.c_double(t), int(h))


def timed(ctx, cloud, buf, p, calls, warmup):
    from mrg_slam_amd import scan_callback_to_device

    data = memoryview(cloud).cast("B")
    m = 0
    for _ in range(warmup):
        m = scan_callback_to_device(data, len(cloud), 1, 16, FIELDS, buf.data_ptr(), len(cloud), 0, None, 0.1, None, p, ctx=ctx)
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        m = scan_callback_to_device(data, len(cloud), 1, 16, FIELDS, buf.data_ptr(), len(cloud), 0, None, 0.1, None, p, ctx=ctx)
        ms.append((time.perf_counter() - t0) * 1e3)
    st = ctx.prefilter_stats()
    row = {"median_ms": round(float(np.median(ms)), 4), "p25_ms": round(float(np.percentile(ms, 25)), 4), "p75_ms": round(float(np.percentile(ms, 75)), 4),
           "route": st["route"], "anomaly": st["anomaly"], "points_out": int(m), "knn_ms": round(ctx.knn_stats()["ms"], 4), "knn_k": int(ctx.knn_stats()["k"])}
    ctx.synchronize()
    row["sha"] = hashlib.sha256(buf[:m].cpu().numpy().tobytes()).hexdigest()[:12]
    return row


def switched_context(on):
    from mrg_slam_amd import Context
    from mrg_slam_amd._lib import lib

    ctx = Context(0)
    ctx.set_statistical_chains(True)
    if on and hasattr(lib(), "mrgfe_ctx_set_wide_statistical_chains"):
        ctx.set_wide_statistical_chains(True)
        return ctx, 1
    return ctx, 0


def time_all(args):
    import torch

    ctx, sw = switched_context(args.switch)
    for sensor in SENSORS:
        cloud = scan_of(sensor)
        buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
        for chain in CHAINS:
            for k in args.ks:
                row = timed(ctx, cloud, buf, chain_params(chain, k), args.calls, args.warmup)
                print(json.dumps(dict({"sensor": sensor, "n": len(cloud), "chain": chain, "k": k, "switch": sw}, **row)), flush=True)


def ab(args):
    me = os.path.abspath(__file__)
    rows = []
    for r in range(args.rounds):
        for which, lib in enumerate(args.libs):
            env = dict(os.environ, MRGFE_LIB=os.path.abspath(lib), MRGFE_LIB_ALLOW_MISSING="1")
            cmd = [sys.executable, me, "time", "--calls", str(args.calls), "--warmup", str(args.warmup), "--ks", ",".join(str(k) for k in args.ks)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                print(out.stderr[-2000:], file=sys.stderr)
                sys.exit(out.returncode)
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), lib=("parent", "this")[which], round=r))
                    print(json.dumps(rows[-1]), flush=True)
    print()
    print("| scan | chain | mean_k | parent: route, ms per call (spread), k-NN launch ms | this build: route, ms per call (spread), k-NN launch ms | call, this / parent | same output |")
    print("|---|---|---|---|---|---|---|")
    for sensor in SENSORS:
        for chain in CHAINS:
            for k in args.ks:
                cell, med, sha = [], [], []
                for lib in ("parent", "this"):
                    sel = [x for x in rows if (x["sensor"], x["chain"], x["k"], x["lib"]) == (sensor, chain, k, lib)]
                    calls, knn = [x["median_ms"] for x in sel], [x["knn_ms"] for x in sel]
                    med.append(float(np.median(calls)))
                    sha.append({x["sha"] for x in sel})
                    cell.append(f"{sorted({x['route'] for x in sel})}, {med[-1]:.3f} ({max(calls) - min(calls):.3f}), {float(np.median(knn)):.3f}")
                print(f"| {sensor} {sel[0]['n']} | {chain} | {k} | {cell[0]} | {cell[1]} | {med[1] / med[0]:.2f} | {'yes' if sha[0] == sha[1] and len(sha[0]) == 1 else 'NO'} |")


RULES = [None, (1.0, 256.0, 4), (1.0, 512.0, 4), (1.0, 1024.0, 4), (2.0, 512.0, 4), (1.0, 64.0, 4), (1.0, 1e9, 0), (2.0, 1e9, 0), (0.5, 1e9, 0)]


def sweep(args):
    import torch

    ctx, _ = switched_context(1)
    for sensor in SENSORS:
        cloud = scan_of(sensor)
        buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
        for k in (64, 100, 255):
            for rule in RULES:
                set_rule(rule)
                row = timed(ctx, cloud, buf, chain_params("NONE", k), args.calls, 5)
                print(json.dumps(dict({"sensor": sensor, "chain": "NONE", "k": k, "rule": rule, "grid": ctx.sor_grid_stats()}, **row)), flush=True)
    set_rule(None)


if __name__ == "__main__":
    ks = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--switch", type=int, default=1)
    a = sub.add_parser("ab")
    a.add_argument("libs", nargs=2)
    a.add_argument("--rounds", type=int, default=3)
    for p in (t, a):
        p.add_argument("--calls", type=int, default=40)
        p.add_argument("--warmup", type=int, default=10)
        p.add_argument("--ks", type=ks, default=[64, 100, 255, 20, 63])
    s = sub.add_parser("sweep")
    s.add_argument("--calls", type=int, default=30)
    args = ap.parse_args()
    {"time": time_all, "ab": ab, "sweep": sweep}[args.cmd](args)
