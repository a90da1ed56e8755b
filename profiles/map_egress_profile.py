"""The map as one call (``mrgfe_map_store_publish``) against the calls and host passes it replaces, and stored keyframes read back
(``mrgfe_map_store_read``) against the host copies a caller would otherwise keep.  One MI355X, profiler off.

  python profiles/map_egress_profile.py [--parent-lib PARENT.so] [--reps 15] [--sizes 50,200,800] [--out-dir profiles] [--render EARLIER.json]

Map stores of 50, 200 and 800 prefiltered keyframes, built as tests/extra_measurements.py builds its 200 (five prefiltered VLP-64 scans of the street scene,
poses 1 m apart).  Routes, alternating repetition by repetition behind two warm-up rounds (which one goes first alternates too), host clock around each:

  publish, composed   generate(copy=False) -> io.pcl_xyzi_records of the view on the host (the numpy pack stands in for the C++ loop of an adapter:
                      pcl::toROSMsg over every map point).  With --parent-lib the generate goes to THAT library file (the parent commit's build), loaded
                      beside this tree's, through the same ctypes calls MapCloudStore.generate makes.
  publish, one call   MapCloudStore.publish(point_step=32, copy=False)
  save, composed      generate(copy=False) -> the two numpy `+=` offset passes (apps/mrg_slam_component.cpp:1104-1116) -> io.write_pcd_binary to a tmpfs path
  save, one call      MapCloudStore.publish(point_step=16, offsets=(utm, enu), copy=False) -> header + the records to the same tmpfs path (MapPublisher.save_map's
                      file step); its call alone is reported too
  read                MapCloudStore.read of 64 keyframes, 32- and 16-byte records, against io.pcl_xyzi_records / a copy of the host clouds

The driver starts every GPU step as a process of its own under a time limit and stops at the first one that fails; it touches no GPU itself.  It writes
map_egress_summary.md and map_egress_summary.json into --out-dir."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UTM, ENU = (364000.25, 5621000.5, 31.125), (-12.5, 7.75, 0.3)
RESOLUTION = 0.1  # config/mrg_slam.yaml:235


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}


def paired(a, b):
    return stats(np.asarray(a) - np.asarray(b))


class ParentStore:
    """mrgfe_map_store of another library file, fed and read the way MapCloudStore does it (a kept, page-locked download buffer; a view comes back)."""

    def __init__(self, L):
        self.L, self.ctx, self.h = L, C.c_void_p(), C.c_void_p()
        assert L.mrgfe_ctx_create(0, C.byref(self.ctx)) == 0 and L.mrgfe_map_store_create(self.ctx, C.byref(self.h)) == 0
        self.out, self.points = None, 0

    def add(self, key, cloud):
        assert self.L.mrgfe_map_store_add(self.h, key, cloud.ctypes.data_as(C.POINTER(C.c_float)), len(cloud), 16) == 0
        self.points += len(cloud)

    def generate(self, keys, poses, first_keyframe=None, resolution=0.1, min_points_per_voxel=1, distance_far_thresh=10000.0, skip_first_cloud=False, copy=False):
        if self.out is None:
            self.out = np.zeros((self.points + self.points // 4, 4), dtype=np.float32)
            self.L.mrgfe_pin_host_buffer(self.ctx, self.out.ctypes.data_as(C.c_void_p), self.out.nbytes)
        ks = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
        P = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64).T.reshape(16) for p in poses]))
        first = np.zeros(len(keys), dtype=np.uint8)
        m = C.c_size_t(0)
        assert self.L.mrgfe_map_store_generate(self.h, len(keys), ks.ctypes.data_as(C.POINTER(C.c_uint64)), P.ctypes.data_as(C.POINTER(C.c_double)),
                                               first.ctypes.data_as(C.POINTER(C.c_uint8)), float(resolution), int(min_points_per_voxel), float(distance_far_thresh),
                                               int(skip_first_cloud), self.out.ctypes.data_as(C.POINTER(C.c_float)), self.points, C.byref(m)) == 0
        return self.out[: m.value]


def load_other(path):
    from mrg_slam_amd import _lib

    _lib.lib()  # (the package's library first: it brings the HIP runtime the way the package wants it)
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
    return L


def step_prepare(a):
    """Five prefiltered keyframe clouds into the work folder."""
    from mrg_slam_amd import Context, prefilter, synth

    scene, poses = synth.street_scene(), synth.arc_trajectory(5, step=0.3, yaw_rate_deg=0.5)
    raw = synth.synth_lidar_many(scene, poses, "VLP64", [synth.BASE_SEED + k for k in range(5)], workers=5)
    ctx = Context(0)
    clouds = [np.ascontiguousarray(prefilter(r, ctx=ctx)) for r in raw]
    np.savez(os.path.join(a.work, "clouds.npz"), *clouds)
    return {"points_per_keyframe": [len(c) for c in clouds]}


def load_clouds(a):
    z = np.load(os.path.join(a.work, "clouds.npz"))
    return [np.ascontiguousarray(z[k]) for k in z.files]


def step_map(a):
    from mrg_slam_amd import Context, MapCloudStore, synth
    from mrg_slam_amd.io import pcd_binary_header, pcl_xyzi_records, write_pcd_binary

    K, clouds = a.keyframes, load_clouds(a)
    poses = [synth.make_pose([1.0 * k, 0.3 * k, 0.0], synth.rot_z(0.01 * k)) for k in range(K)]
    keys = list(range(1, K + 1))
    store = MapCloudStore(Context(0))
    composed = ParentStore(load_other(a.parent_lib)) if a.parent_lib else MapCloudStore(Context(0))
    for k in keys:
        store.add(k, clouds[(k - 1) % 5])
        composed.add(k, clouds[(k - 1) % 5])
    o1, o2 = np.asarray(UTM, np.float64).astype(np.float32), np.asarray(ENU, np.float64).astype(np.float32)
    path_a, path_b = os.path.join(a.tmpfs, "map_a.pcd"), os.path.join(a.tmpfs, "map_b.pcd")
    kept = {"a_offsets_ms": [], "a_write_ms": [], "b_call_ms": []}

    def publish_composed():
        x = composed.generate(keys, poses, None, RESOLUTION, copy=False)
        kept["a32"] = pcl_xyzi_records(x)

    def publish_one_call():
        kept["b32"] = store.publish(keys, poses, None, resolution=RESOLUTION, point_step=32, copy=False)

    def save_composed():
        x = composed.generate(keys, poses, None, RESOLUTION, copy=False)
        t = time.perf_counter()
        x[:, :3] += o1
        x[:, :3] += o2
        kept["a_offsets_ms"].append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        write_pcd_binary(path_a, x)
        kept["a_write_ms"].append(1e3 * (time.perf_counter() - t))

    def save_one_call():
        t = time.perf_counter()
        msg = store.publish(keys, poses, None, resolution=RESOLUTION, point_step=16, offsets=(UTM, ENU), copy=False)
        kept["b_call_ms"].append(1e3 * (time.perf_counter() - t))
        with open(path_b, "wb") as f:
            f.write(pcd_binary_header(msg["width"]))
            f.write(memoryview(msg["data"]))

    out = {"keyframes": K, "points_in": int(sum(len(clouds[(k - 1) % 5]) for k in keys)), "composed_lib": os.path.basename(a.parent_lib) or "this tree", "reps": a.reps}
    for name, fa, fb in (("publish", publish_composed, publish_one_call), ("save", save_composed, save_one_call)):
        ta, tb = [], []
        for j in range(2 + a.reps):
            for which in ((0, 1) if j % 2 == 0 else (1, 0)):
                t = time.perf_counter()
                (fa, fb)[which]()
                (ta, tb)[which].append(1e3 * (time.perf_counter() - t))
        ta, tb = ta[2:], tb[2:]
        out[name] = {"composed_ms": stats(ta), "one_call_ms": stats(tb), "composed_minus_one_call_ms": paired(ta, tb)}
        if name == "publish":
            assert np.array_equal(kept["a32"].reshape(-1), kept["b32"]["data"]), "the routes' records differ"
            out["points_out"], out["record_bytes"] = int(kept["b32"]["width"]), int(kept["b32"]["row_step"])
            out["publish"]["egress_stats"] = store.egress_stats()
        else:
            assert open(path_a, "rb").read() == open(path_b, "rb").read(), "the routes' files differ"
            out["save"].update(composed_offset_passes_ms=stats(kept["a_offsets_ms"][2:]), composed_write_ms=stats(kept["a_write_ms"][2:]), one_call_publish_alone_ms=stats(kept["b_call_ms"][2:]))
    # where the composed publish spends its time: the generate alone
    tg = []
    for _ in range(max(5, a.reps // 3)):
        t = time.perf_counter()
        composed.generate(keys, poses, None, RESOLUTION, copy=False)
        tg.append(1e3 * (time.perf_counter() - t))
    out["publish"]["composed_generate_alone_ms"] = stats(tg)
    for p in (path_a, path_b):
        os.remove(p)
    return out


def step_read(a):
    from mrg_slam_amd import Context, MapCloudStore
    from mrg_slam_amd.io import pcl_xyzi_records

    clouds = load_clouds(a)
    store = MapCloudStore(Context(0))
    keys = list(range(1, 65))
    host = {k: clouds[(k - 1) % 5] for k in keys}  # the second copy of every keyframe the host keeps today
    for k in keys:
        store.add(k, host[k])
    out = {"keyframes": len(keys), "points": int(sum(len(c) for c in host.values())), "host_bytes_no_longer_needed": int(sum(c.nbytes for c in host.values())), "reps": a.reps}
    for step in (32, 16):
        ta, tb = [], []
        for j in range(2 + a.reps):
            for which in ((0, 1) if j % 2 == 0 else (1, 0)):
                t = time.perf_counter()
                if which == 0:
                    got_a = [pcl_xyzi_records(host[k]) if step == 32 else host[k].copy() for k in keys]
                else:
                    got_b = store.read(keys, step)
                (ta, tb)[which].append(1e3 * (time.perf_counter() - t))
        assert all(np.array_equal(x.view(np.uint8).reshape(-1), y.reshape(-1)) for x, y in zip(got_a, got_b))
        out[f"records_{step}"] = {"host_copies_ms": stats(ta[2:]), "read_ms": stats(tb[2:]), "host_minus_read_ms": paired(ta[2:], tb[2:]), "bytes": int(sum(y.nbytes for y in got_b)),
                                  "egress_stats": store.egress_stats()}
    return out


def row(name, s):
    return f"| {name} | {s['median']:.2f} | {s['p10']:.2f} | {s['p90']:.2f} |"


def write_summary(a, res):
    lines = ["# Map egress: one call against the composed route", "",
             f"One MI355X, profiler off; {res['prepare']['points_per_keyframe']} points in the five prefiltered keyframe clouds; resolution {RESOLUTION}; host clock, ms; "
             f"{a.reps} repetitions behind 2 warm-up rounds, the routes alternating.  The composed route's `generate` runs on `{res['maps'][0]['composed_lib']}`.  "
             "The numpy pack (`io.pcl_xyzi_records`) stands in for the C++ loop of an adapter (`pcl::toROSMsg` over every map point).", ""]
    for m in res["maps"]:
        lines += [f"## {m['keyframes']} keyframes: {m['points_in']} points in, {m['points_out']} out, {m['record_bytes']} bytes of 32-byte records", "",
                  "| route | median | p10 | p90 |", "|---|---|---|---|",
                  row("publish, composed: generate(view) + host pack", m["publish"]["composed_ms"]), row("… its generate alone", m["publish"]["composed_generate_alone_ms"]),
                  row("publish, one call (point_step 32)", m["publish"]["one_call_ms"]), row("publish: composed − one call, paired", m["publish"]["composed_minus_one_call_ms"]),
                  row("save, composed: generate(view) + two offset passes + write_pcd_binary (tmpfs)", m["save"]["composed_ms"]),
                  row("… its two offset passes", m["save"]["composed_offset_passes_ms"]), row("… its file write", m["save"]["composed_write_ms"]),
                  row("save, one call (point_step 16, two offsets) + header and records to tmpfs", m["save"]["one_call_ms"]),
                  row("… its publish alone", m["save"]["one_call_publish_alone_ms"]), row("save: composed − one call, paired", m["save"]["composed_minus_one_call_ms"]), "",
                  f"Last publish: {m['publish']['egress_stats']}.", ""]
        for name in ("publish", "save"):
            d = m[name]["composed_minus_one_call_ms"]["median"]
            lines.append(f"- {name}: the one call is {'faster' if d > 0 else 'NOT faster'} by {abs(d):.2f} ms (median of the paired differences).")
        lines.append("")
    r = res["read"]
    lines += [f"## read of {r['keyframes']} keyframes ({r['points']} points)", "", "| route | median | p10 | p90 |", "|---|---|---|---|"]
    for step in (32, 16):
        s = r[f"records_{step}"]
        lines += [row(f"{step}-byte records from the host copies ({'pcl_xyzi_records' if step == 32 else 'a copy'} per keyframe)", s["host_copies_ms"]),
                  row(f"{step}-byte records, `read` ({s['bytes']} bytes; {s['egress_stats']})", s["read_ms"]), row("host − read, paired", s["host_minus_read_ms"])]
    for step in (32, 16):
        s = r[f"records_{step}"]
        d, gbs = s["host_minus_read_ms"]["median"], s["bytes"] / s["read_ms"]["median"] / 1e6
        lines += ["", f"- {step}-byte records: `read` is {'faster' if d > 0 else 'NOT faster'} than the host copies by {abs(d):.2f} ms.  Its time is the download into a fresh, pageable "
                  f"array ({gbs:.1f} GB/s here), which records made from clouds the host already holds do not pay" + (" — only the host's pack costs more." if d > 0 else ".")]
    lines += ["", "What `read` buys is not time but the second copy of every keyframe cloud the host keeps today.",
              f"Host memory no longer needed for these {r['keyframes']} keyframes: {r['host_bytes_no_longer_needed']} bytes (16 per stored point; it grows with the session).", ""]
    with open(os.path.join(a.out_dir, "map_egress_summary.md"), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(a.out_dir, "map_egress_summary.json"), "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="the library file the composed route's generate calls (default: this tree's)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="50,200,800")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--tmpfs", default="/dev/shm")
    ap.add_argument("--render", default="", help="write the summary again from an earlier run's map_egress_summary.json; nothing is run")
    ap.add_argument("--step", default="", help="(internal) prepare | map | read: one GPU step, its result as JSON into --result")
    ap.add_argument("--keyframes", type=int, default=0)
    ap.add_argument("--work", default="")
    ap.add_argument("--result", default="")
    a = ap.parse_args()
    if a.step:
        res = {"prepare": step_prepare, "map": step_map, "read": step_read}[a.step](a)
        with open(a.result, "w") as f:
            json.dump(res, f)
        return 0
    os.makedirs(a.out_dir, exist_ok=True)
    if a.render:
        write_summary(a, json.load(open(a.render)))
        return 0
    with tempfile.TemporaryDirectory() as work:
        def run(step, limit, *extra):
            result = os.path.join(work, "result.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--work", work, "--result", result, "--reps", str(a.reps), "--tmpfs", a.tmpfs,
                   "--parent-lib", a.parent_lib, *extra]
            print("+", step, *extra, flush=True)
            rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
            if rc != 0:
                print(f"step {step} {' '.join(extra)} ended with status {rc}: stopping", flush=True)
                sys.exit(rc)  # nothing more is started on the GPU
            return json.load(open(result))

        res = {"prepare": run("prepare", 240), "maps": []}
        for K in [int(s) for s in a.sizes.split(",")]:
            res["maps"].append(run("map", 300, "--keyframes", str(K)))
        res["read"] = run("read", 120)
    write_summary(a, res)
    print(open(os.path.join(a.out_dir, "map_egress_summary.md")).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
