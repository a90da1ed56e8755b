"""The keyframe callback as one call against the calls it replaces, on one VLP-64 keyframe cloud (the street scene's scan behind the default prefilter).

  python profiles/keyframe_callback_profile.py time [--out FILE.json] [--windows 15] [--calls 20] [--cloud FILE.npy]
      End-to-end times, profiler off.  What one keyframe costs until it is in the map store AND queued once as a loop-closure target and once as
      a candidate, timed in the same process on the same cloud, alternating window by window:
        new   mrgfe_keyframe_callback -> mrgfe_batch_add_target_from_store -> mrgfe_batch_add_pair_from_store
        old   mrgfe_remove_points_near (with other robots) -> mrgfe_map_store_add -> mrgfe_batch_add_target -> first mrgfe_batch_add_pair_keyed
      for 0 and 2 other robots, the packed 16-byte layout and 32-byte pcl::PointXYZI records (the old route names them by MRGFE_LAYOUT_PCL_XYZI).
      A window is `calls` keyframes (a fresh key each) behind a warm-up of both routes and ends in a device synchronise; the figure of a window is
      its time per keyframe.  Reported per route: median, minimum, 10th and 90th percentile of the windows.  The kept and removed clouds of the two
      routes are compared before anything is timed.  The batches are cleared and their keyed stores emptied between windows, outside the clock.

  python profiles/keyframe_callback_profile.py once --route new|old [--robots 0|2] [--layout packed16|pcl32] --cloud FILE.npy
      One keyframe into the store by one route and nothing else (no batch), for `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ...`:
      the launch and copy counts of mrgfe_keyframe_callback against mrgfe_remove_points_near -> mrgfe_map_store_add.  The cloud is read from
      FILE.npy (a `time` run with the same --cloud writes it), so that the traced process launches nothing else.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADIUS_SQR = 4.0  # robot_remove_points_radius 2.0 (config/mrg_slam.yaml:134)
ROUTES = ("new", "old")


class Routes:
    def __init__(self, layout: str, robots: int, with_batch: bool = True, cloud_file: str = ""):
        from mrg_slam_amd import BatchMatcher, Context, MapCloudStore, _lib, prefilter, synth
        from mrg_slam_amd.io import pcl_xyzi_records

        self.lib, self._lib = _lib.lib(), _lib
        self.ctx = Context(0)
        if cloud_file and os.path.exists(cloud_file):  # (a traced process must launch nothing but the call it traces: the cloud comes from a file)
            self.cloud = np.ascontiguousarray(np.load(cloud_file), dtype=np.float32)
        else:
            self.cloud = np.ascontiguousarray(prefilter(synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED), ctx=self.ctx))
            if cloud_file:
                os.makedirs(os.path.dirname(os.path.abspath(cloud_file)), exist_ok=True)
                np.save(cloud_file, self.cloud)
        self.n = n = len(self.cloud)
        packed = layout == "packed16"
        self.payload = np.array(self.cloud.view(np.uint8).reshape(-1) if packed else pcl_xyzi_records(self.cloud).reshape(-1), copy=True)
        self.stride = 16 if packed else _lib.LAYOUT_PCL_XYZI  # what the old route's host-pointer calls are told about the same bytes
        self.p = _lib.KeyframeParams()
        self.lib.mrgfe_keyframe_default_params(C.byref(self.p))
        self.p.width, self.p.point_step, self.p.off_intensity = n, (16 if packed else 32), (12 if packed else 16)
        # two other robots in the sensor frame: one a few metres ahead (its sphere holds points of the scan), one out of range
        self.centres = np.ascontiguousarray(np.array([[6.0, 0.5, -1.0], [55.0, -20.0, 0.0]], dtype=np.float32)[:robots])
        self.kept, self.removed = np.empty((n, 4), dtype=np.float32), np.empty((n, 4), dtype=np.float32)
        self.nk, self.nr = C.c_size_t(0), C.c_size_t(0)
        self.stores = {r: MapCloudStore(self.ctx) for r in ROUTES}
        self.batches = {r: BatchMatcher(ctx=self.ctx) for r in ROUTES} if with_batch else None
        self.guess = np.ascontiguousarray(np.eye(4, dtype=np.float32))
        self.key = 0

    def new(self):
        fp = C.POINTER(C.c_float)
        L, check, s = self.lib, self._lib.check, self.stores["new"]
        self.key += 1
        k = len(self.centres)
        check(L.mrgfe_keyframe_callback(s._h, self.key, C.byref(self.p), self.payload.ctypes.data_as(C.c_void_p), self.payload.nbytes,
                                        self.centres.ctypes.data_as(fp) if k else None, k, RADIUS_SQR, self.kept.ctypes.data_as(fp) if k else None, C.byref(self.nk),
                                        self.removed.ctypes.data_as(fp) if k else None, C.byref(self.nr)))
        if self.batches:
            b = self.batches["new"]
            t = check(L.mrgfe_batch_add_target_from_store(b._h, s._h, self.key))
            check(L.mrgfe_batch_add_pair_from_store(b._h, t, s._h, self.key, self.guess.ctypes.data_as(fp)))

    def old(self):
        fp = C.POINTER(C.c_float)
        L, check, s, h = self.lib, self._lib.check, self.stores["old"], self.ctx._h
        self.key += 1
        k = len(self.centres)
        src, n, stride = self.payload.ctypes.data_as(fp), self.n, self.stride
        if k:  # (with no other robot the reference keeps the message's cloud: nothing to remove, :396)
            check(L.mrgfe_remove_points_near(h, src, n, stride, self.centres.ctypes.data_as(fp), k, RADIUS_SQR, self.kept.ctypes.data_as(fp), C.byref(self.nk),
                                             self.removed.ctypes.data_as(fp), C.byref(self.nr)))
            src, n, stride = self.kept.ctypes.data_as(fp), self.nk.value, 16
        else:
            self.nk.value, self.nr.value = n, 0
        check(L.mrgfe_map_store_add(s._h, self.key, src, n, stride))
        if self.batches:
            b = self.batches["old"]
            t = check(L.mrgfe_batch_add_target(b._h, src, n, stride))
            check(L.mrgfe_batch_add_pair_keyed(b._h, t, self.key, src, n, stride, self.guess.ctypes.data_as(fp)))

    def run(self, route: str):
        (self.new if route == "new" else self.old)()

    def outputs(self, route: str):
        """(kept, removed) of the last call, and the stored cloud."""
        self.ctx.synchronize()
        k = len(self.centres)
        kept = self.kept[: self.nk.value].copy() if k else self.cloud
        stored = self.stores[route].generate([self.key], [np.eye(4)], None, 0.0)
        return kept, self.removed[: self.nr.value].copy(), stored

    def between_windows(self):
        if self.batches:
            for b in self.batches.values():
                b.clear()
                b.forget()


def time_routes(args):
    rows = []
    for layout in ("packed16", "pcl32"):
        for robots in (0, 2):
            r = Routes(layout, robots, cloud_file=args.cloud)
            outs = {}
            for route in ROUTES:  # warm-up of every shape, and the outputs the routes must agree on
                for _ in range(5):
                    r.run(route)
                outs[route] = r.outputs(route)
            for a, b in zip(outs["new"], outs["old"]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the routes differ"
            assert np.array_equal(outs["new"][0].view(np.uint32), outs["new"][2].view(np.uint32)), "the stored cloud is not the kept cloud"
            r.between_windows()
            per = {route: [] for route in ROUTES}
            for _ in range(args.windows):
                for route in ROUTES:  # alternating: a drift of the machine lands on both routes alike
                    r.ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        r.run(route)
                    r.ctx.synchronize()
                    per[route].append(1e3 * (time.perf_counter() - t0) / args.calls)
                    r.between_windows()
            for route in ROUTES:
                v = np.array(per[route])
                rows.append({"layout": layout, "robots": robots, "route": route, "points_in": r.n, "points_kept": len(outs[route][0]), "points_removed": len(outs[route][1]),
                             "windows": args.windows, "calls_per_window": args.calls, "ms_median": float(np.median(v)), "ms_min": float(v.min()),
                             "ms_p10": float(np.percentile(v, 10)), "ms_p90": float(np.percentile(v, 90))})
                print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def once(args):
    assert os.path.exists(args.cloud), "once: give --cloud FILE written by an earlier `time` run (the prefilter would add its launches to the trace)"
    r = Routes(args.layout, args.robots, with_batch=False, cloud_file=args.cloud)
    r.ctx.synchronize()
    r.run(args.route)
    r.ctx.synchronize()
    print(json.dumps({"route": args.route, "robots": args.robots, "layout": args.layout, "points_in": r.n, "points_kept": r.nk.value, "points_removed": r.nr.value}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--out", default="")
    t.add_argument("--windows", type=int, default=15)
    t.add_argument("--calls", type=int, default=20)
    o = sub.add_parser("once")
    o.add_argument("--route", choices=ROUTES, required=True)
    o.add_argument("--robots", type=int, choices=(0, 2), default=2)
    o.add_argument("--layout", choices=("packed16", "pcl32"), default="packed16")
    for sp in (t, o):
        sp.add_argument("--cloud", default="", help="the keyframe cloud as an .npy file: loaded when it exists, else computed (GPU prefilter) and written there")
    a = ap.parse_args()
    (time_routes if a.cmd == "time" else once)(a)
