"""[distance filter] -> NONE | APPROX_VOXELGRID(0.1) -> STATISTICAL through mrgfe_scan_callback_device, per raw scan: the device-driven chain behind
mrgfe_ctx_set_statistical_chains (the k-NN grid's edge chosen on the device, nn_build_device_sized) against the host-driven passes of a library without it.

  python profiles/prefilter_statistical_chains_profile.py time --sensor VLP64 --chain NONE --k 20 [--switch 1] [--rule START,TARGET,HALVINGS]
                                                               [--calls 200] [--warmup 30]
      ONE configuration in this process: median and p25 / p75 of `calls` calls behind `warmup` calls (host clock around a call that ends in the chain's
      wait), the route, the point count and a checksum of the output, the grid the device chose (mrgfe_ctx_sor_grid_stats) and the k-NN launch's
      HIP-event time (mrgfe_ctx_knn_stats).  The library is the one MRGFE_LIB names; --switch is ignored by a library that has no switch.

  python profiles/prefilter_statistical_chains_profile.py ab LIB [LIB ...] [--rounds 1] [--calls 200]
      `time` in a fresh child process per library and configuration (2 sensors x 2 chains x mean_k 20 / 30), the libraries alternating: the baseline is
      the parent commit's library built to a second path (there these chains run the host-driven passes, route 0).

  python profiles/prefilter_statistical_chains_profile.py sweep [--calls 60]
      the rules (start edge, crowding target, most halvings) of one library side by side in one process, per sensor and chain: for choosing defaults.

  python profiles/prefilter_statistical_chains_profile.py handbacks [--scans 100] [--scans64 40]
      `scans` VLP-16 and `scans64` VLP-64 scans of different seeds and poses through both chains: calls per route and per anomaly bit.
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
CHAINS = {"NONE": {"downsample_method": "NONE"}, "APPROX": {"downsample_method": "APPROX_VOXELGRID", "downsample_resolution": 0.1}}
STDDEV = {20: 1.0, 30: 1.2}


def chain_params(chain, k):
    return dict({"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "outlier_removal_method": "STATISTICAL",
                 "statistical_mean_k": k, "statistical_stddev": STDDEV.get(k, 1.0)}, **CHAINS[chain])


def scan_of(sensor, seed=None, shift=0.0):
    from mrg_slam_amd import synth

    pose = np.eye(4)
    pose[0, 3] = shift
    if seed is None:
        seed = synth.BASE_SEED if sensor == "VLP64" else 4711
    return np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), pose, sensor, seed))


def set_rule(rule):
    import ctypes as C

    from mrg_slam_amd._lib import lib

    if hasattr(lib(), "mrgfe_dbg_set_sor_grid_rule"):
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
           "route": st["route"], "anomaly": st["anomaly"], "points_out": int(m)}
    if hasattr(ctx, "sor_grid_stats"):
        try:
            row["grid"] = ctx.sor_grid_stats()
        except AttributeError:  # (an older library under MRGFE_LIB)
            pass
    row["knn_ms"] = round(ctx.knn_stats()["ms"], 4)
    ctx.synchronize()
    row["sha"] = hashlib.sha256(buf[:m].cpu().numpy().tobytes()).hexdigest()[:12]
    return row


def switch_on(ctx, on):
    from mrg_slam_amd._lib import lib

    if on and hasattr(lib(), "mrgfe_ctx_set_statistical_chains"):
        ctx.set_statistical_chains(True)
        return 1
    return 0


def time_one(args):
    import torch

    from mrg_slam_amd import Context

    ctx = Context(0)
    sw = switch_on(ctx, args.switch)
    rule = tuple(float(v) for v in args.rule.split(",")) if args.rule else None
    set_rule(rule)
    cloud = scan_of(args.sensor)
    buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
    row = timed(ctx, cloud, buf, chain_params(args.chain, args.k), args.calls, args.warmup)
    print(json.dumps(dict({"sensor": args.sensor, "n": len(cloud), "chain": args.chain, "k": args.k, "switch": sw, "rule": rule}, **row)), flush=True)


def ab(args):
    me = os.path.abspath(__file__)
    for r in range(args.rounds):
        for sensor in ("VLP16", "VLP64"):
            for chain in CHAINS:
                for k in (20, 30):
                    for lib in args.libs:
                        env = dict(os.environ, MRGFE_LIB=os.path.abspath(lib), MRGFE_LIB_ALLOW_MISSING="1")
                        cmd = [sys.executable, me, "time", "--sensor", sensor, "--chain", chain, "--k", str(k), "--calls", str(args.calls), "--warmup", str(args.warmup)]
                        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                        if out.returncode != 0:
                            print(out.stderr[-2000:], file=sys.stderr)
                            sys.exit(out.returncode)
                        for line in out.stdout.splitlines():
                            if line.startswith("{"):
                                print(json.dumps(dict(json.loads(line), lib=os.path.basename(lib), round=r)), flush=True)


RULES = [None, (0.5, 32.0, 4), (1.0, 32.0, 4), (2.0, 32.0, 4), (1.0, 16.0, 4), (1.0, 64.0, 4), (1.0, 128.0, 4), (2.0, 64.0, 4), (1.0, 1e9, 0), (0.5, 1e9, 0), (2.0, 1e9, 0), (0.25, 1e9, 0)]


def sweep(args):
    import torch

    from mrg_slam_amd import Context

    ctx = Context(0)
    switch_on(ctx, 1)
    for sensor in ("VLP16", "VLP64"):
        cloud = scan_of(sensor)
        buf = torch.empty((len(cloud), 4), dtype=torch.float32, device="cuda:0")
        for chain in CHAINS:
            for k in (20, 30):
                for rule in RULES:
                    set_rule(rule)
                    row = timed(ctx, cloud, buf, chain_params(chain, k), args.calls, 10)
                    print(json.dumps(dict({"sensor": sensor, "chain": chain, "k": k, "rule": rule}, **row)), flush=True)
    set_rule(None)


def handbacks(args):
    import torch

    from mrg_slam_amd import Context, scan_callback_to_device

    ctx = Context(0)
    switch_on(ctx, 1)
    for sensor in ("VLP16", "VLP64"):
        tally = {}
        edges = {}
        buf = None
        scans = args.scans if sensor == "VLP16" else args.scans64
        for s in range(scans):
            cloud = scan_of(sensor, 1000 + s, shift=0.37 * s)
            if buf is None or buf.shape[0] < len(cloud):
                buf = torch.empty((len(cloud) + 4096, 4), dtype=torch.float32, device="cuda:0")
            data = memoryview(cloud).cast("B")
            for chain in CHAINS:
                scan_callback_to_device(data, len(cloud), 1, 16, FIELDS, buf.data_ptr(), buf.shape[0], 0, None, 0.1, None, chain_params(chain, 20 + 10 * (s % 2)), ctx=ctx)
                st, g = ctx.prefilter_stats(), ctx.sor_grid_stats()
                key = (chain, st["route"], st["anomaly"])
                tally[key] = tally.get(key, 0) + 1
                ek = (chain, g["edge"], g["halvings"])
                edges[ek] = edges.get(ek, 0) + 1
        for (chain, route, anomaly), cnt in sorted(tally.items()):
            print(json.dumps({"sensor": sensor, "chain": chain, "route": route, "anomaly": anomaly, "scans": cnt, "of": scans}), flush=True)
        for (chain, edge, h), cnt in sorted(edges.items()):
            print(json.dumps({"sensor": sensor, "chain": chain, "edge": edge, "halvings": h, "scans": cnt}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--sensor", default="VLP64", choices=["VLP16", "VLP64"])
    t.add_argument("--chain", default="NONE", choices=list(CHAINS))
    t.add_argument("--k", type=int, default=20)
    t.add_argument("--switch", type=int, default=1)
    t.add_argument("--rule", default="")
    t.add_argument("--calls", type=int, default=200)
    t.add_argument("--warmup", type=int, default=30)
    a = sub.add_parser("ab")
    a.add_argument("libs", nargs="+")
    a.add_argument("--rounds", type=int, default=1)
    a.add_argument("--calls", type=int, default=200)
    a.add_argument("--warmup", type=int, default=30)
    s = sub.add_parser("sweep")
    s.add_argument("--calls", type=int, default=60)
    h = sub.add_parser("handbacks")
    h.add_argument("--scans", type=int, default=100)
    h.add_argument("--scans64", type=int, default=40)
    args = ap.parse_args()
    {"time": time_one, "ab": ab, "sweep": sweep, "handbacks": handbacks}[args.cmd](args)
