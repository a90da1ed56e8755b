"""The per-scan egress: what it costs to get the filtered scan as the 32-byte records of the message, per call, library against library.

  python profiles/scan_egress_profile.py time [--calls 200] [--warmup 20]
      On the ~130k-point VLP-64 scan and the ~26k-point VLP-16 scan of the street, for VOXELGRID 0.1 + RADIUS, VOXELGRID 0.1 + STATISTICAL and NONE + NONE
      (distance filter on), point_step 32, the C ABI called through ctypes with every buffer made once:
        a  mrgfe_scan_callback, then the compiled host loop that writes the records (profiles/scan_egress_host_loop.cpp, -O2)
        b  mrgfe_scan_callback_device, one device-to-host copy of the kept points, the same loop
        c  mrgfe_scan_callback_records into a page-locked buffer (direct)
        d  mrgfe_scan_callback_records into a pageable buffer (staged)
        e  c with d_out_xyzi
      (c - e only where the library has the call).  Median and p95 of `calls` calls behind `warmup`, the route, the egress statistics and a checksum of the
      records, which must be the same in every row of a workload.  One JSON line per row.  The library is the one MRGFE_LIB names.

  python profiles/scan_egress_profile.py ab LIB [LIB ...] [--rounds 3] [--summary FILE.md]
      `time` in a fresh child process per library file, the libraries alternating `rounds` times (the baseline: the parent commit's library built to a second
      path), then the summary: per workload the medians of every row per library and round, and the spread of row a over its own repeated runs.
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

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
BASE = {"enable_distance_filter": True, "downsample_method": "NONE", "downsample_resolution": 0.1, "outlier_removal_method": "NONE", "radius_radius": 0.5,
        "radius_min_neighbors": 2}
CHAINS = [("VOXELGRID 0.1 + RADIUS", {"downsample_method": "VOXELGRID", "outlier_removal_method": "RADIUS"}),
          ("VOXELGRID 0.1 + STATISTICAL", {"downsample_method": "VOXELGRID", "outlier_removal_method": "STATISTICAL"}),
          ("NONE + NONE", {})]
ROWS = {"a": "scan_callback + host loop", "b": "scan_callback_device + D2H + host loop", "c": "records, page-locked (direct)", "d": "records, pageable (staged)",
        "e": "records, page-locked, with d_out_xyzi"}


def host_loop():
    """the compiled per-point loop (built next to its source when missing or older)"""
    src, so = os.path.join(HERE, "scan_egress_host_loop.cpp"), os.path.join(HERE, "scan_egress_host_loop.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    fn = C.CDLL(so).records_from_packed
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_size_t, C.c_void_p]
    return fn


def time_rows(args):
    import torch

    from mrg_slam_amd import Context, synth
    from mrg_slam_amd._lib import check, lib
    from mrg_slam_amd.filters import _scan_params

    L, loop, ctx = lib(), host_loop(), Context(0)
    has_records = hasattr(L, "mrgfe_scan_callback_records") and getattr(L.mrgfe_scan_callback_records, "argtypes", None)
    u8p, fp, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_void_p
    for sensor in ("VLP64", "VLP16"):
        cloud = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), sensor, synth.BASE_SEED if sensor == "VLP64" else 4711))
        n = len(cloud)
        data = cloud.view(np.uint8).reshape(-1)
        packed = np.empty((n, 4), dtype=np.float32)               # a, b: the packed points on the host
        records = np.empty(n * 32, dtype=np.uint8)                # a, b, d: pageable
        pinned = np.empty(n * 32, dtype=np.uint8)                 # c, e: page-locked
        check(L.mrgfe_pin_host_buffer(ctx._h, pinned.ctypes.data_as(vp), pinned.nbytes))
        dbuf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        hbuf = torch.from_numpy(packed)
        m = C.c_size_t(0)
        try:
            for name, more in CHAINS:
                q = _scan_params(n, 1, 16, FIELDS, 0, None, 0.1, None, dict(BASE, **more), ctx)
                dp = data.ctypes.data_as(u8p)

                def row_a():
                    check(L.mrgfe_scan_callback(ctx._h, C.byref(q), dp, packed.ctypes.data_as(fp), C.byref(m)))
                    loop(packed.ctypes.data, m.value, records.ctypes.data)
                    return records

                def row_b():
                    check(L.mrgfe_scan_callback_device(ctx._h, C.byref(q), dp, vp(dbuf.data_ptr()), C.byref(m)))
                    hbuf[: m.value].copy_(dbuf[: m.value])
                    loop(packed.ctypes.data, m.value, records.ctypes.data)
                    return records

                def row_new(dst, dev):
                    def run():
                        check(L.mrgfe_scan_callback_records(ctx._h, C.byref(q), dp, 32, dst.ctypes.data_as(vp), dst.nbytes, vp(dbuf.data_ptr()) if dev else None, C.byref(m)))
                        return dst
                    return run

                rows = [("a", row_a), ("b", row_b)]
                if has_records:
                    rows += [("c", row_new(pinned, False)), ("d", row_new(records, False)), ("e", row_new(pinned, True))]
                for key, run in rows:
                    for _ in range(args.warmup):
                        run()
                    ms = []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        out = run()
                        ms.append((time.perf_counter() - t0) * 1e3)
                    row = {"sensor": sensor, "n": n, "chain": name, "row": key, "what": ROWS[key], "median_ms": round(float(np.median(ms)), 4),
                           "p95_ms": round(float(np.percentile(ms, 95)), 4), "route": ctx.prefilter_stats()["route"], "points_out": int(m.value),
                           "sha": hashlib.sha256(out[: m.value * 32].tobytes()).hexdigest()[:12]}
                    if key in "cde":
                        row["egress"] = ctx.egress_stats()
                    print(json.dumps(row), flush=True)
        finally:
            ctx.synchronize()
            L.mrgfe_unpin_host_buffer(ctx._h, pinned.ctypes.data_as(vp))


def summary(rows, libs, path):
    """per workload: every row's median per library and round; the spread of row a (max - min of its medians over all runs of the command)"""
    lines = ["# Scan egress: the filtered scan as 32-byte records, per call", "",
             "`profiles/scan_egress_profile.py ab` on one MI355X: the libraries alternate in one command, a fresh process per run; medians of the calls of a row in ms.",
             "Rows: " + "; ".join(f"({k}) {v}" for k, v in ROWS.items()) + ".",
             "Columns: library file and round (`libmrgfe_parent.so`: the parent commit's library, which has rows (a) and (b) only).  The host loop of (a) and (b) is "
             "`profiles/scan_egress_host_loop.cpp`, -O2, without the copy `pcl::toROSMsg` adds.", ""]
    work = sorted({(r["sensor"], r["chain"]) for r in rows}, key=lambda w: (w[0] != "VLP64", w[1]))
    for sensor, chain in work:
        sel = [r for r in rows if (r["sensor"], r["chain"]) == (sensor, chain)]
        shas = {r["sha"] for r in sel}
        a_runs = [r["median_ms"] for r in sel if r["row"] == "a"]
        lines += [f"## {sensor} ({sel[0]['n']} points), {chain}: {sel[0]['points_out']} points out, route {sel[0]['route']}", "",
                  f"records identical in every row and run: {'yes' if len(shas) == 1 else 'NO ' + str(sorted(shas))}; "
                  f"row (a) over its {len(a_runs)} runs: {min(a_runs):.4f} - {max(a_runs):.4f} ms (spread {max(a_runs) - min(a_runs):.4f} ms)", "",
                  "| row | " + " | ".join(f"{os.path.basename(lib)} r{r}" for r in sorted({x["round"] for x in sel}) for lib in libs) + " |",
                  "|---|" + "---|" * (len(libs) * len({x["round"] for x in sel}))]
        for key in ROWS:
            cells = []
            for r in sorted({x["round"] for x in sel}):
                for lib in libs:
                    hit = [x for x in sel if x["row"] == key and x["round"] == r and x["lib"] == lib]
                    cells.append(f"{hit[0]['median_ms']:.4f}" if hit else "-")
            lines.append(f"| ({key}) | " + " | ".join(cells) + " |")
        eg = [x for x in sel if x["row"] in "cde" and "egress" in x]
        if eg:
            last = {x["row"]: x["egress"] for x in eg}
            lines += ["", "egress statistics of the last call: " + "; ".join(f"({k}) direct {int(v['direct'])}, launches {v['launches']}, extra waits {v['waits']}, "
                                                                             f"host-copied {v['copied']} of {v['bytes']} bytes" for k, v in sorted(last.items()))]
        lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines))


def ab(args):
    rows = []
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
                    rows.append(dict(json.loads(line), lib=lib, round=r))
                    print(json.dumps(rows[-1]), flush=True)
    if args.summary:
        summary(rows, args.libs, args.summary)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--calls", type=int, default=200)
    t.add_argument("--warmup", type=int, default=20)
    a = sub.add_parser("ab")
    a.add_argument("libs", nargs="+")
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--calls", type=int, default=200)
    a.add_argument("--warmup", type=int, default=20)
    a.add_argument("--summary")
    args = ap.parse_args()
    time_rows(args) if args.cmd == "time" else ab(args)
