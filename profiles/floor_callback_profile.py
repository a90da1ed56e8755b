"""Floor detection on the message's bytes and the keyframe callback on a cloud in HBM, each against the route it stands for, on the street scene's
VLP-64 scan: the prefiltered scan the components really receive (about 33k points) and the raw scan (about 132k points).

  python profiles/floor_callback_profile.py time [--label NAME] [--calls 40] [--out FILE.json]
      One process, one library file (mrg_slam_amd/libmrgfe.so, or MRGFE_LIB with MRGFE_LIB_ALLOW_MISSING=1 for an older one: routes whose entry
      point that file lacks are left out).  Milliseconds per call, profiler off; every route of a table is called in turn, `calls` times round, behind
      five warm-up rounds, with the context synchronised before each timing (every call returns behind its own last wait).  Median, 10th and 90th
      percentile per route.  Floor detection (default parameters, both clouds asked for), layouts packed 16 B, pcl::PointXYZI 32 B, Velodyne 22 B:
        callback        mrgfe_floor_callback
        composed        mrgfe_ingest_pointcloud2 into a device buffer -> mrgfe_floor_detect_device
        detect_device   mrgfe_floor_detect_device alone on that buffer (the refactored body, old against new)
      Keyframe callback (0 and 2 centres, kept cloud asked for with centres, as the component does):
        bytes           mrgfe_keyframe_callback on the packed bytes
        device          mrgfe_keyframe_callback_device on the same cloud in a device buffer
      The outputs of the routes of a table are compared before anything is timed.

  python profiles/floor_callback_profile.py ab --parent FILE.so [--calls 40] [--out FILE.json]
      The comparison the change is held to: child processes of `time`, parent / new / parent / new — the composed route is taken on the PARENT's
      library file, the two parent runs give the run-to-run spread — and the table of profiles/floor_callback_summary.md.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V22 = np.dtype({"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"], "offsets": [0, 4, 8, 12, 16, 18], "itemsize": 22})
LAYOUTS = {"packed16": (16, 12), "pcl32": (32, 16), "velodyne22": (22, 12)}  # point_step, intensity offset (x, y, z at 0, 4, 8)


def payload(cloud, layout):
    from mrg_slam_amd.io import pcl_xyzi_records

    if layout == "packed16":
        return np.array(cloud.view(np.uint8).reshape(-1), copy=True)
    if layout == "pcl32":
        return np.array(pcl_xyzi_records(cloud).reshape(-1), copy=True)
    rec = np.zeros(len(cloud), dtype=V22)
    for k, f in enumerate(("x", "y", "z", "intensity")):
        rec[f] = cloud[:, k]
    rec["ring"] = np.arange(len(cloud)) % 64
    return np.array(rec.view(np.uint8).reshape(-1), copy=True)


def timed(ctx, routes, calls):
    """{name: per-call milliseconds} of the callables in `routes`, called in turn."""
    per = {name: [] for name in routes}
    for it in range(5 + calls):
        for name, fn in routes.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= 5:
                per[name].append(dt)
    return per


def time_all(args):
    import torch

    from mrg_slam_amd import Context, MapCloudStore, _lib, prefilter, synth

    L, check = _lib.lib(), _lib.check
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    ctx = Context(0)
    ctx.set_byte_layouts(True)
    raw = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED))
    shapes = {"prefiltered": np.ascontiguousarray(prefilter(raw, ctx=ctx)), "raw": raw}
    rows = []

    def report(table, shape, case, per, n):
        for name, v in per.items():
            v = np.array(v)
            rows.append({"label": args.label, "table": table, "shape": shape, "points": n, "case": case, "route": name, "calls": len(v), "ms_median": float(np.median(v)),
                         "ms_p10": float(np.percentile(v, 10)), "ms_p90": float(np.percentile(v, 90))})
            print(json.dumps(rows[-1]), flush=True)

    q = _lib.FloorParams()
    L.mrgfe_floor_default_params(C.byref(q))
    for shape, cloud in shapes.items():
        n = len(cloud)
        dbuf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        filt, inl = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32)
        for layout, (step, off_i) in LAYOUTS.items():
            data = payload(cloud, layout)
            lay = _lib.KeyframeParams(n, 1, step, 0, 0, 4, 8, off_i)
            res = {k: _lib.FloorResult() for k in ("callback", "composed", "detect_device")}
            outs = {}

            def detect_device(r=res["detect_device"]):
                check(L.mrgfe_floor_detect_device(ctx._h, C.byref(q), C.c_void_p(dbuf.data_ptr()), n, C.byref(r), filt.ctypes.data_as(fp), inl.ctypes.data_as(fp)))

            def composed(r=res["composed"]):
                check(L.mrgfe_ingest_pointcloud2(ctx._h, data.ctypes.data_as(u8), n, 1, step, 0, 0, 4, 8, off_i, None, C.c_void_p(dbuf.data_ptr())))
                check(L.mrgfe_floor_detect_device(ctx._h, C.byref(q), C.c_void_p(dbuf.data_ptr()), n, C.byref(r), filt.ctypes.data_as(fp), inl.ctypes.data_as(fp)))

            def callback(r=res["callback"]):
                check(L.mrgfe_floor_callback(ctx._h, C.byref(q), C.byref(lay), data.ctypes.data_as(C.c_void_p), data.nbytes, C.byref(r), filt.ctypes.data_as(fp), inl.ctypes.data_as(fp)))

            routes = {"composed": composed, "detect_device": detect_device}
            if hasattr(L, "mrgfe_floor_callback"):
                routes["callback"] = callback
            for name, fn in routes.items():  # the routes agree before they are timed
                fn()
                r = res[name]
                outs[name] = (bytes(r), filt[: r.n_filtered].tobytes(), inl[: r.n_inliers].tobytes() if r.found else b"")
            assert all(o == outs["composed"] for o in outs.values()), (shape, layout)
            report("floor", shape, f"{layout}, {_lib.FLOOR_REASONS[res['composed'].reason]}", timed(ctx, routes, args.calls), n)

    for shape, cloud in shapes.items():
        n = len(cloud)
        dbuf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        check(L.mrgfe_ingest_pointcloud2(ctx._h, cloud.ctypes.data_as(u8), n, 1, 16, 0, 0, 4, 8, 12, None, C.c_void_p(dbuf.data_ptr())))
        lay = _lib.KeyframeParams(n, 1, 16, 0, 0, 4, 8, 12)
        kept = np.empty((n, 4), np.float32)
        for k in (0, 2):
            centres = np.array([[4.0, 1.0, -1.0], [-6.0, -3.0, 0.0]], np.float32)[:k]
            cp, kp = (centres.ctypes.data_as(fp), kept.ctypes.data_as(fp)) if k else (None, None)
            stores = {"bytes": MapCloudStore(ctx), "device": MapCloudStore(ctx)}  # (a store per route: every call stores a new keyframe)
            keys = {"bytes": 0, "device": 0}
            nk, nr = C.c_size_t(0), C.c_size_t(0)

            def by_bytes():
                keys["bytes"] += 1
                check(L.mrgfe_keyframe_callback(stores["bytes"]._h, keys["bytes"], C.byref(lay), cloud.ctypes.data_as(C.c_void_p), cloud.nbytes, cp, k, 9.0, kp, C.byref(nk), None, C.byref(nr)))

            def by_device():
                keys["device"] += 1
                check(L.mrgfe_keyframe_callback_device(stores["device"]._h, keys["device"], C.c_void_p(dbuf.data_ptr()), n, cp, k, 9.0, kp, C.byref(nk), None, C.byref(nr)))

            routes = {"bytes": by_bytes}
            if hasattr(L, "mrgfe_keyframe_callback_device"):
                routes["device"] = by_device
            outs = {}
            for name, fn in routes.items():
                fn()
                outs[name] = (nk.value, nr.value, stores[name].generate([1], [np.eye(4)], None, 0.0).tobytes())
                assert nk.value + nr.value == n and (k == 0 or 0 < nr.value < n), (shape, k, name, nk.value, nr.value)
            assert all(o == outs["bytes"] for o in outs.values()), (shape, k)
            report("keyframe", shape, f"{k} centres", timed(ctx, routes, args.calls), n)
            del stores
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def ab(args):
    runs = []
    for label, libfile in (("parent_1", args.parent), ("new_1", ""), ("parent_2", args.parent), ("new_2", "")):
        env = dict(os.environ)
        env.pop("MRGFE_LIB", None)
        if libfile:
            env.update(MRGFE_LIB=os.path.abspath(libfile), MRGFE_LIB_ALLOW_MISSING="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "time", "--label", label, "--calls", str(args.calls)], env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], flush=True)
            raise SystemExit(f"{label}: exit status {p.returncode}")
        runs += [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
        print(f"{label}: done", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(runs, f, indent=1)
    med = {(r["label"], r["table"], r["shape"], r["case"], r["route"]): r for r in runs}

    def m(label, *key):
        r = med.get((label,) + key)
        return "–" if r is None else f"{r['ms_median']:.3f} ({r['ms_p10']:.3f} – {r['ms_p90']:.3f})"

    print("\n| floor detection | points | layout | parent: composed | parent again | new: callback | new again | parent: detect_device | parent again | new: detect_device | new again |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for (label, table, shape, case, route), r in med.items():
        if (label, table, route) == ("parent_1", "floor", "composed"):
            k = ("floor", shape, case)
            print(f"| {shape} | {r['points']} | {case} | {m('parent_1', *k, 'composed')} | {m('parent_2', *k, 'composed')} | {m('new_1', *k, 'callback')} | {m('new_2', *k, 'callback')} | "
                  f"{m('parent_1', *k, 'detect_device')} | {m('parent_2', *k, 'detect_device')} | {m('new_1', *k, 'detect_device')} | {m('new_2', *k, 'detect_device')} |")
    print("\n| keyframe callback | points | centres | parent: bytes | parent again | new: bytes | new again | new: device | new again |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (label, table, shape, case, route), r in med.items():
        if (label, table, route) == ("parent_1", "keyframe", "bytes"):
            k = ("keyframe", shape, case)
            print(f"| {shape} | {r['points']} | {case} | {m('parent_1', *k, 'bytes')} | {m('parent_2', *k, 'bytes')} | {m('new_1', *k, 'bytes')} | {m('new_2', *k, 'bytes')} | "
                  f"{m('new_1', *k, 'device')} | {m('new_2', *k, 'device')} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--label", default="new")
    t.add_argument("--calls", type=int, default=40)
    t.add_argument("--out", default="")
    b = sub.add_parser("ab")
    b.add_argument("--parent", required=True)
    b.add_argument("--calls", type=int, default=40)
    b.add_argument("--out", default="")
    a = ap.parse_args()
    (time_all if a.cmd == "time" else ab)(a)
