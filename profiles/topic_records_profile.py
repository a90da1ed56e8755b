"""The three cloud messages written on the device against the composed routes they stand for, on one MI355X (needs a GPU; no fall-back).

Workload: one synthetic VLP-64 scan of the street scene (~131k points), packed 16-byte layout, subscribers on.  Per stage the wall time of one call
(host clock around a call that ends in its own device wait), C ABI through ctypes, every buffer made once; per round ONE call of each of three rows,
alternating: the composed route, the new call, the composed route again.  The two composed columns measure the spread of the same code in the same run.

  coloured points   composed: mrgfe_scan_callback_records (page-locked), a second host unpack of the message, the compiled colour loop
                    new:      mrgfe_scan_callback_outputs, both destinations page-locked
  aligned points    composed: mrgfe_odom_frame with aligned_xyzi, the compiled 32-byte loop       (NDT_HIP, VOXELGRID 0.5 downsample, the same scan again)
                    new:      mrgfe_odom_frame_records, page-locked, on a twin handle
  keyframe clouds   composed: mrgfe_keyframe_callback with kept and removed, two such loops       (3 centres, radius 3 m)
                    new:      mrgfe_keyframe_callback_records, both destinations page-locked

The host loops: profiles/topic_records_host_loops.cpp and profiles/scan_egress_host_loop.cpp, -O2, without the copy pcl::toROSMsg adds.
The bar: the new call's median is no higher than the composed route's (the mean of its two medians) by more than their difference.  The outputs of both
routes are compared byte for byte before anything is timed.

  python profiles/topic_records_profile.py --calls 60 --warmup 8 --out profiles/topic_records_summary.md"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
CHAIN = {"enable_distance_filter": True, "downsample_method": "VOXELGRID", "downsample_resolution": 0.1, "outlier_removal_method": "RADIUS", "radius_radius": 0.5,
         "radius_min_neighbors": 2}


def shared_object(name):
    """a compiled host loop (built next to its source when missing or older)"""
    src, so = os.path.join(HERE, name + ".cpp"), os.path.join(HERE, name + ".so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    return C.CDLL(so)


def alternate(rows, calls, warmup):
    """rows: [(name, callable)]; one call of each per round -> {name: [ms]}"""
    for _ in range(warmup):
        for _, run in rows:
            run()
    ms = {name: [] for name, _ in rows}
    for _ in range(calls):
        for name, run in rows:
            t0 = time.perf_counter()
            run()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def report(stage, n, ms, extra):
    a1, a2, new = (float(np.median(ms[k])) for k in ("composed", "composed again", "new"))
    spread = abs(a1 - a2)
    row = {"stage": stage, "n": n, "composed_ms": round(a1, 4), "composed_again_ms": round(a2, 4), "new_ms": round(new, 4), "spread_ms": round(spread, 4),
           "new_p95_ms": round(float(np.percentile(ms["new"], 95)), 4), "composed_p95_ms": round(float(np.percentile(ms["composed"], 95)), 4),
           "holds": bool(new <= 0.5 * (a1 + a2) + spread)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def measure(args):
    import torch  # noqa: F401  (one HIP runtime for the process)

    from mrg_slam_amd import Context, NdtHip, HipOdometry, MapCloudStore, synth, _lib
    from mrg_slam_amd._lib import check, lib
    from mrg_slam_amd.filters import _scan_params

    L = lib()
    loops, loop32 = shared_object("topic_records_host_loops"), shared_object("scan_egress_host_loop").records_from_packed
    loop32.restype, loop32.argtypes = None, [C.c_void_p, C.c_size_t, C.c_void_p]
    loops.unpack_xyzi.restype, loops.unpack_xyzi.argtypes = None, [C.c_void_p] + [C.c_size_t] * 6 + [C.c_void_p]
    loops.colour_loop.restype, loops.colour_loop.argtypes = None, [C.c_void_p, C.c_size_t, C.c_void_p]
    u8p, fp, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_void_p
    cloud = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED))
    n = len(cloud)
    data = cloud.view(np.uint8).reshape(-1)
    ctx = Context(0)
    pinned = [np.empty(n * 32, dtype=np.uint8) for _ in range(4)]
    for b in pinned:
        check(L.mrgfe_pin_host_buffer(ctx._h, b.ctypes.data_as(vp), b.nbytes))
    host = [np.empty(n * 32, dtype=np.uint8) for _ in range(3)]
    packed = [np.empty((n, 4), dtype=np.float32) for _ in range(2)]
    out = []
    try:
        # ---- coloured points ----
        q = _scan_params(n, 1, 16, FIELDS, 0, np.array([0.1, 0.0, 0.2], dtype=np.float32), 0.1, None, CHAIN, ctx)
        m, mc = C.c_size_t(0), C.c_size_t(0)
        o = _lib.ScanOutputs()
        o.point_step, o.records, o.capacity_bytes, o.colored_records, o.colored_capacity_bytes = 32, pinned[0].ctypes.data, pinned[0].nbytes, pinned[1].ctypes.data, pinned[1].nbytes

        def colored_composed():
            check(L.mrgfe_scan_callback_records(ctx._h, C.byref(q), data.ctypes.data_as(u8p), 32, pinned[2].ctypes.data_as(vp), pinned[2].nbytes, None, C.byref(m)))
            loops.unpack_xyzi(data.ctypes.data, n, 16, 0, 4, 8, 12, host[0].ctypes.data)
            loops.colour_loop(host[0].ctypes.data, n, host[1].ctypes.data)

        def colored_new():
            check(L.mrgfe_scan_callback_outputs(ctx._h, C.byref(q), data.ctypes.data_as(u8p), C.byref(o), C.byref(m), C.byref(mc)))

        colored_composed()
        m_composed = m.value
        colored_new()
        assert mc.value == n and m.value == m_composed and np.array_equal(host[1], pinned[1]) and np.array_equal(pinned[0][: 32 * m.value], pinned[2][: 32 * m.value])
        ms = alternate([("composed", colored_composed), ("new", colored_new), ("composed again", colored_composed)], args.calls, args.warmup)
        colored_new()  # (the statistics below are those of the new call)
        out.append(report("coloured points", n, ms, {"route": ctx.prefilter_stats()["route"], "second_egress": ctx.second_egress_stats()}))

        # ---- aligned points ----
        params = {"downsample_method": "VOXELGRID", "downsample_resolution": 0.5, "keyframe_delta_translation": 1e9, "keyframe_delta_angle": 1e9, "keyframe_delta_time": 1e9}
        twins = [HipOdometry(NdtHip(transformation_epsilon=0.01, ctx=ctx), params) for _ in range(2)]
        lay = _lib.KeyframeParams()
        L.mrgfe_keyframe_default_params(C.byref(lay))
        lay.width = n
        res, na, stamp = _lib.OdomResult(), C.c_size_t(0), [100.0, 100.0]

        def aligned_composed():
            stamp[0] += 0.1
            check(L.mrgfe_odom_frame(twins[0]._h, C.byref(lay), data.ctypes.data_as(vp), data.nbytes, stamp[0], None, 0, packed[0].ctypes.data_as(fp), C.byref(res)))
            if res.outcome == _lib.ODOM_ACCEPTED:
                loop32(packed[0].ctypes.data, n, host[0].ctypes.data)

        def aligned_new():
            stamp[1] += 0.1
            check(L.mrgfe_odom_frame_records(twins[1]._h, C.byref(lay), data.ctypes.data_as(vp), data.nbytes, stamp[1], None, 0, 32, pinned[0].ctypes.data_as(vp), pinned[0].nbytes,
                                             C.byref(na), C.byref(res)))

        for _ in range(2):  # the first frame, then an accepted one
            aligned_composed()
            aligned_new()
        assert res.outcome == _lib.ODOM_ACCEPTED and na.value == n and np.array_equal(host[0], pinned[0])
        ms = alternate([("composed", aligned_composed), ("new", aligned_new), ("composed again", aligned_composed)], args.calls, args.warmup)
        aligned_new()
        out.append(report("aligned points", n, ms, {"egress": ctx.egress_stats()}))

        # ---- keyframe clouds ----
        store = MapCloudStore(ctx)
        centres = np.array([[6.0, 1.0, 0.0], [-8.0, -2.0, 0.5], [0.0, 9.0, 0.0]], dtype=np.float32)
        key, nk, nr, r2 = [0], C.c_size_t(0), C.c_size_t(0), float(np.float32(9.0))

        def keyframe_composed():
            key[0] += 1
            check(L.mrgfe_keyframe_callback(store._h, key[0], C.byref(lay), data.ctypes.data_as(vp), data.nbytes, centres.ctypes.data_as(fp), 3, r2, packed[0].ctypes.data_as(fp),
                                            C.byref(nk), packed[1].ctypes.data_as(fp), C.byref(nr)))
            loop32(packed[0].ctypes.data, nk.value, host[0].ctypes.data)
            loop32(packed[1].ctypes.data, nr.value, host[2].ctypes.data)

        def keyframe_new():
            key[0] += 1
            check(L.mrgfe_keyframe_callback_records(store._h, key[0], C.byref(lay), data.ctypes.data_as(vp), data.nbytes, centres.ctypes.data_as(fp), 3, r2, 32,
                                                    pinned[0].ctypes.data_as(vp), pinned[0].nbytes, C.byref(nk), pinned[3].ctypes.data_as(vp), pinned[3].nbytes, C.byref(nr)))

        keyframe_composed()
        keyframe_new()
        assert 0 < nr.value < n and np.array_equal(host[0][: 32 * nk.value], pinned[0][: 32 * nk.value]) and np.array_equal(host[2][: 32 * nr.value], pinned[3][: 32 * nr.value])
        ms = alternate([("composed", keyframe_composed), ("new", keyframe_new), ("composed again", keyframe_composed)], args.calls, args.warmup)
        keyframe_new()
        out.append(report("keyframe clouds", n, ms, {"kept": nk.value, "removed": nr.value, "egress": ctx.egress_stats(), "second_egress": ctx.second_egress_stats()}))
    finally:
        ctx.synchronize()
        for b in pinned:
            L.mrgfe_unpin_host_buffer(ctx._h, b.ctypes.data_as(vp))
    return out


def summary(rows, args):
    lines = ["# Topic records: the coloured, aligned and keyframe cloud messages written on the device", "",
             f"One MI355X, one synthetic VLP-64 scan of {rows[0]['n']} points, subscribers on; median wall time of one call in ms over {args.calls} calls per row after "
             f"{args.warmup} warm-up rounds, the three rows alternating call by call (`profiles/topic_records_profile.py`, which describes the composed routes).  "
             "`spread`: the difference of the composed route's two medians in the same run.  `holds`: new <= mean of the two composed medians + spread.", "",
             "| stage | composed | composed again | spread | new call | new p95 | composed p95 | holds |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['stage']} | {r['composed_ms']:.3f} | {r['composed_again_ms']:.3f} | {r['spread_ms']:.3f} | {r['new_ms']:.3f} | {r['new_p95_ms']:.3f} | "
                     f"{r['composed_p95_ms']:.3f} | {'yes' if r['holds'] else 'NO: the new call loses'} |")
    lines += ["", "Both routes' outputs were equal byte for byte before the timing.  The composed routes leave out the copy `pcl::toROSMsg` makes of the host-built cloud.",
              "", "Raw rows:", "", "```json"] + [json.dumps(r) for r in rows] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "topic_records_summary.md"))
    a = ap.parse_args()
    summary(measure(a), a)
