"""The scan callback as one call against the four calls it replaces, on one VLP-64 scan (default prefilter parameters, transform on).

  python profiles/scan_callback_profile.py time [--out FILE.json] [--windows 15] [--calls 20]
      End-to-end times, profiler off.  Routes, timed in the same process on the same scan, alternating window by window:
        new_host / new_device   mrgfe_scan_callback / mrgfe_scan_callback_device
        old_host / old_device   mrgfe_ingest_pointcloud2 -> mrgfe_deskew (if deskewing) -> mrgfe_transform_cloud -> mrgfe_prefilter / _device
      for deskewing on and off, a pageable and a page-locked payload, the packed 16-byte layout and 32-byte pcl::PointXYZI records.  A window is
      `calls` calls behind a warm-up of every route and ends in a device synchronise; the figure of a window is its time per call.  Reported per
      route: median, minimum, 10th and 90th percentile of the windows.  Outputs of the two routes are compared before anything is timed.

  python profiles/scan_callback_profile.py once --route new_host|new_device|old_host|old_device [--deskew 0|1] [--layout packed16|pcl32]
      One call of one route and nothing else, for `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ...`: the launch and copy counts.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
PERIOD = 0.1


class Routes:
    def __init__(self, layout: str, pinned: bool):
        import torch

        from mrg_slam_amd import Context, _lib, synth
        from mrg_slam_amd.io import pcl_xyzi_records

        self.torch, self.lib, self._lib = torch, _lib.lib(), _lib
        self.ctx = Context(0)
        cloud = synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED)
        self.n = n = len(cloud)
        raw = cloud.view(np.uint8).reshape(-1) if layout == "packed16" else pcl_xyzi_records(cloud).reshape(-1)
        self.step, self.off_i = (16, 12) if layout == "packed16" else (32, 16)
        if pinned:
            self._pin = torch.empty(len(raw), dtype=torch.uint8).pin_memory()
            self.payload = self._pin.numpy()
            self.payload[:] = raw
        else:
            self.payload = np.array(raw, copy=True)
        self.T = np.ascontiguousarray(synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32).T)  # column-major
        self.tmp = [np.empty((n, 4), dtype=np.float32) for _ in range(3)]
        self.out = np.empty((n, 4), dtype=np.float32)
        self.dbuf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        self.m = C.c_size_t(0)
        self.pf = _lib.PrefilterParams()
        self.lib.mrgfe_prefilter_default_params(C.byref(self.pf))

    def scan_params(self, deskew: bool):
        p = self._lib.ScanParams()
        self.lib.mrgfe_scan_default_params(C.byref(p))
        p.width, p.point_step, p.off_intensity = self.n, self.step, self.off_i
        p.deskew = int(deskew)
        p.ang_v[:] = [float(v) for v in ANG_V]
        p.scan_period = PERIOD
        p.transform = 1
        p.T[:] = [float(v) for v in self.T.reshape(16)]
        return p

    def new(self, deskew: bool, device: bool):
        fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        p = self.scan_params(deskew)
        if device:
            self._lib.check(self.lib.mrgfe_scan_callback_device(self.ctx._h, C.byref(p), self.payload.ctypes.data_as(u8), C.c_void_p(self.dbuf.data_ptr()), C.byref(self.m)))
        else:
            self._lib.check(self.lib.mrgfe_scan_callback(self.ctx._h, C.byref(p), self.payload.ctypes.data_as(u8), self.out.ctypes.data_as(fp), C.byref(self.m)))
        return self.m.value

    def old(self, deskew: bool, device: bool):
        fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L, h, n, check = self.lib, self.ctx._h, self.n, self._lib.check
        a, b, c = (t.ctypes.data_as(fp) for t in self.tmp)
        check(L.mrgfe_ingest_pointcloud2(h, self.payload.ctypes.data_as(u8), n, 1, self.step, 0, 0, 4, 8, self.off_i, a, None))
        cur = a
        if deskew:
            check(L.mrgfe_deskew(h, cur, n, 16, ANG_V.ctypes.data_as(fp), PERIOD, b))
            cur = b
        check(L.mrgfe_transform_cloud(h, cur, n, 16, self.T.ctypes.data_as(fp), c))
        if device:
            check(L.mrgfe_prefilter_device(h, C.byref(self.pf), c, n, 16, C.c_void_p(self.dbuf.data_ptr()), C.byref(self.m)))
        else:
            check(L.mrgfe_prefilter(h, C.byref(self.pf), c, n, 16, self.out.ctypes.data_as(fp), C.byref(self.m)))
        return self.m.value

    def run(self, route: str, deskew: bool):
        return (self.new if route.startswith("new") else self.old)(deskew, route.endswith("device"))

    def result(self, route: str, m: int) -> np.ndarray:
        self.ctx.synchronize()
        return self.dbuf[:m].cpu().numpy() if route.endswith("device") else self.out[:m].copy()


ROUTES = ("new_host", "old_host", "new_device", "old_device")


def time_routes(args):
    rows = []
    for layout in ("packed16", "pcl32"):
        for pinned in (False, True):
            r = Routes(layout, pinned)
            for deskew in (True, False):
                outs = {}
                for route in ROUTES:  # warm-up of every shape, and the outputs the routes must agree on
                    for _ in range(5):
                        m = r.run(route, deskew)
                    outs[route] = r.result(route, m)
                for route in ROUTES[1:]:
                    assert np.array_equal(outs[route], outs["new_host"]), f"{route} differs from new_host"
                per = {route: [] for route in ROUTES}
                for _ in range(args.windows):
                    for route in ROUTES:  # alternating: a drift of the machine lands on every route alike
                        r.ctx.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            r.run(route, deskew)
                        r.ctx.synchronize()
                        per[route].append(1e3 * (time.perf_counter() - t0) / args.calls)
                for route in ROUTES:
                    v = np.array(per[route])
                    rows.append({"layout": layout, "payload": "page-locked" if pinned else "pageable", "deskew": deskew, "route": route, "points_in": r.n,
                                 "points_out": len(outs[route]), "windows": args.windows, "calls_per_window": args.calls, "ms_median": float(np.median(v)),
                                 "ms_min": float(v.min()), "ms_p10": float(np.percentile(v, 10)), "ms_p90": float(np.percentile(v, 90))})
                    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def once(args):
    r = Routes(args.layout, False)
    m = r.run(args.route, bool(args.deskew))
    r.ctx.synchronize()
    print(json.dumps({"route": args.route, "deskew": bool(args.deskew), "layout": args.layout, "points_in": r.n, "points_out": m}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--out", default="")
    t.add_argument("--windows", type=int, default=15)
    t.add_argument("--calls", type=int, default=20)
    o = sub.add_parser("once")
    o.add_argument("--route", choices=ROUTES, required=True)
    o.add_argument("--deskew", type=int, default=1)
    o.add_argument("--layout", choices=("packed16", "pcl32"), default="packed16")
    a = ap.parse_args()
    (time_routes if a.cmd == "time" else once)(a)
