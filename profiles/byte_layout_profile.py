"""What the byte-aligned record reader costs: the VLP-64 scan of profiles/scan_callback_profile.py through mrgfe_scan_callback_device as Velodyne's
22-byte records (mrgfe_ctx_set_byte_layouts: the kernels' byte-aligned instantiations) and as the same records padded to 24 bytes (a strict layout: the
kernels as they were).  Deskewing and the transform on, default prefilter parameters.

  python profiles/byte_layout_profile.py time [--layouts v22,p24] [--out FILE.json] [--windows 15] [--calls 20]
      The whole call, profiler off: windows of `calls` calls behind a warm-up, each ending in a device synchronise, the layouts alternating window by
      window.  The outputs of the layouts are compared (identical) before anything is timed.  Median, minimum, 10th / 90th percentile per layout.

  python profiles/byte_layout_profile.py loop --layout v22|p24 [--calls 200]
      `calls` calls of one layout behind a warm-up and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`: the head kernel
      (scan_head_kernel<...>) in steady state.

MRGFE_LIB=<another libmrgfe.so> MRGFE_LIB_ALLOW_MISSING=1 runs an older library (p24 only: it has no byte layouts)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ANG_V = np.array([0.3, -0.2, 0.9], dtype=np.float32)
STEP = {"v22": 22, "p24": 24}


class Scan:
    def __init__(self, layouts):
        import torch

        from mrg_slam_amd import Context, _lib, synth

        self.lib, self._lib = _lib.lib(), _lib
        self.ctx = Context(0)
        if "v22" in layouts:
            self.ctx.set_byte_layouts(True)
        cloud = synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP64", synth.BASE_SEED)
        self.n = n = len(cloud)
        rng = np.random.default_rng(5)
        self.payload = {}
        for name in layouts:  # x@0 y@4 z@8 intensity@12, ring and time behind them (random), p24: two more bytes
            rec = rng.integers(0, 256, (n, STEP[name]), dtype=np.uint8)
            rec[:, :16] = cloud.view(np.uint8).reshape(n, 16)
            self.payload[name] = rec.reshape(-1)
        self.T = np.ascontiguousarray(synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32).T)  # column-major
        self.dbuf = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        self.m = C.c_size_t(0)

    def params(self, name):
        p = self._lib.ScanParams()
        self.lib.mrgfe_scan_default_params(C.byref(p))
        p.width, p.point_step = self.n, STEP[name]
        p.deskew = 1
        p.ang_v[:] = [float(v) for v in ANG_V]
        p.scan_period = 0.1
        p.transform = 1
        p.T[:] = [float(v) for v in self.T.reshape(16)]
        return p

    def run(self, name):
        p = self.params(name)
        self._lib.check(self.lib.mrgfe_scan_callback_device(self.ctx._h, C.byref(p), self.payload[name].ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(self.dbuf.data_ptr()),
                                                            C.byref(self.m)))
        return self.m.value

    def result(self, m):
        self.ctx.synchronize()
        return self.dbuf[:m].cpu().numpy()


def time_layouts(args):
    layouts = args.layouts.split(",")
    s = Scan(layouts)
    outs = {}
    for name in layouts:
        for _ in range(5):
            m = s.run(name)
        outs[name] = s.result(m)
    for name in layouts[1:]:
        assert np.array_equal(outs[name].view(np.uint32), outs[layouts[0]].view(np.uint32)), f"{name} differs from {layouts[0]}"
    per = {name: [] for name in layouts}
    for _ in range(args.windows):
        for name in layouts:
            s.ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                s.run(name)
            s.ctx.synchronize()
            per[name].append(1e3 * (time.perf_counter() - t0) / args.calls)
    rows = []
    for name in layouts:
        v = np.array(per[name])
        rows.append({"lib": os.environ.get("MRGFE_LIB", "this tree"), "layout": name, "points_in": s.n, "points_out": len(outs[name]), "windows": args.windows,
                     "calls_per_window": args.calls, "ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_p10": float(np.percentile(v, 10)),
                     "ms_p90": float(np.percentile(v, 90))})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def loop(args):
    s = Scan([args.layout])
    for _ in range(5 + args.calls):
        m = s.run(args.layout)
    s.ctx.synchronize()
    print(json.dumps({"layout": args.layout, "calls": 5 + args.calls, "points_in": s.n, "points_out": m}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--layouts", default="v22,p24")
    t.add_argument("--out", default="")
    t.add_argument("--windows", type=int, default=15)
    t.add_argument("--calls", type=int, default=20)
    o = sub.add_parser("loop")
    o.add_argument("--layout", choices=tuple(STEP), required=True)
    o.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    (time_layouts if a.cmd == "time" else loop)(a)
