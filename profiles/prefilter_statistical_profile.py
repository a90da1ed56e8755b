"""The reference's code-default prefilter chain, distance filter -> VOXELGRID 0.1 -> STATISTICAL, per call and per route.

  python profiles/prefilter_statistical_profile.py time [--calls 200] [--warmup 20] [--switches 1,0] [--out FILE.json]
      mrgfe_prefilter_device and mrgfe_scan_callback_device (transform on) on a ~130k-point VLP-64 scan and the ~26k-point VLP-16 scan, k = 20 and 30, with
      mrgfe_dbg_set_prefilter_device_driven at 1 and at 0: median and p95 of `calls` calls behind `warmup` calls, the route mrgfe_ctx_prefilter_stats
      reports (where the library has it), the last k-NN launch of mrgfe_ctx_knn_stats (HIP events: the device-driven chain's nn_knn_mean_dd_kernel, the
      host-driven passes' nn_knn_kernel) and a checksum of the output, which must not depend on the route.  One JSON line per combination.
      The library is the one MRGFE_LIB names (MRGFE_LIB_ALLOW_MISSING=1 for one older than the binding table).

  python profiles/prefilter_statistical_profile.py ab LIB [LIB ...] [--rounds 2]
      `time` in a fresh child process per library file, the libraries alternating `rounds` times: the baseline is the parent commit's library built to a
      second path, the switch-at-0 route of the new build only the cross-check that the baseline is the same code.

  python profiles/prefilter_statistical_profile.py once --mode 1|0 [--scan VLP64|VLP16] [--k 20] [--calls 3]
      `calls` calls of mrgfe_prefilter_device and nothing else, for `rocprofv3 --hip-trace --stats -- python ...`: the stream waits, allocations and
      launches per call are the difference of the counts of two such runs (2 and 12 calls) over the ten calls between them; the start-up (the first call's
      allocations, event creation) cancels.
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


class Bench:
    def __init__(self, sensor: str):
        import torch

        from mrg_slam_amd import Context, _lib, synth

        self.torch, self.lib, self._lib = torch, _lib.lib(), _lib
        self.ctx = Context(0)
        seed = synth.BASE_SEED if sensor == "VLP64" else 4711
        self.cloud = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), sensor, seed))
        self.n = len(self.cloud)
        self.T = np.ascontiguousarray(synth.make_pose([0.3, -0.1, 0.45], synth.rot_xyz(0.01, -0.02, 1.2)).astype(np.float32).T)  # column-major
        self.dbuf = torch.empty((self.n, 4), dtype=torch.float32, device="cuda:0")
        self.m = C.c_size_t(0)

    def params(self, k: int):
        pf = self._lib.PrefilterParams()
        self.lib.mrgfe_prefilter_default_params(C.byref(pf))
        pf.outlier_removal_method, pf.statistical_mean_k, pf.statistical_stddev, pf.downsample_resolution = 2, k, 1.0, 0.1
        sp = self._lib.ScanParams()
        self.lib.mrgfe_scan_default_params(C.byref(sp))
        sp.width, sp.point_step, sp.off_intensity, sp.transform = self.n, 16, 12, 1
        sp.T[:] = [float(v) for v in self.T.reshape(16)]
        sp.filters = pf
        return pf, sp

    def call(self, entry: str, pf, sp) -> int:
        if entry == "prefilter_device":
            self._lib.check(self.lib.mrgfe_prefilter_device(self.ctx._h, C.byref(pf), self.cloud.ctypes.data_as(C.POINTER(C.c_float)), self.n, 16,
                                                            C.c_void_p(self.dbuf.data_ptr()), C.byref(self.m)))
        else:
            self._lib.check(self.lib.mrgfe_scan_callback_device(self.ctx._h, C.byref(sp), self.cloud.view(np.uint8).reshape(-1).ctypes.data_as(C.POINTER(C.c_uint8)),
                                                                C.c_void_p(self.dbuf.data_ptr()), C.byref(self.m)))
        return self.m.value

    def route(self):
        if not hasattr(self.lib, "mrgfe_ctx_prefilter_stats"):
            return None
        return self.ctx.prefilter_stats()["route"]


def time_routes(args):
    rows = []
    for sensor in ("VLP64", "VLP16"):
        b = Bench(sensor)
        for k in (20, 30):
            pf, sp = b.params(k)
            for entry in ("prefilter_device", "scan_callback_device"):
                for mode in args.switches:
                    assert b.lib.mrgfe_dbg_set_prefilter_device_driven(mode) == mode
                    for _ in range(args.warmup):
                        m = b.call(entry, pf, sp)
                    b.ctx.synchronize()
                    ms = []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        m = b.call(entry, pf, sp)  # (the call returns behind its last wait: the result is in the device buffer)
                        ms.append(1e3 * (time.perf_counter() - t0))
                    knn = b.ctx.knn_stats()
                    out = b.dbuf[:m].cpu().numpy()
                    row = {"lib": os.path.basename(os.environ.get("MRGFE_LIB", "libmrgfe.so")), "sensor": sensor, "points_in": b.n, "k": k, "entry": entry, "switch": mode,
                           "route": b.route(), "points_out": int(m), "sha": hashlib.sha256(out.tobytes()).hexdigest()[:12], "calls": args.calls,
                           "ms_median": float(np.median(ms)) if ms else None, "ms_p95": float(np.percentile(ms, 95)) if ms else None,
                           "ms_min": float(np.min(ms)) if ms else None, "knn_ms": knn["ms"], "knn_queries": knn["queries"]}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        b.lib.mrgfe_dbg_set_prefilter_device_driven(1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def ab(args):
    for r in range(args.rounds):
        for lib in args.libs:
            env = dict(os.environ, MRGFE_LIB=os.path.abspath(lib), MRGFE_LIB_ALLOW_MISSING="1")
            print(f"# round {r} {lib}", flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), "time", "--calls", str(args.calls), "--warmup", str(args.warmup)], env=env, check=True, timeout=args.timeout)


def once(args):
    b = Bench(args.scan)
    pf, _ = b.params(args.k)
    assert b.lib.mrgfe_dbg_set_prefilter_device_driven(args.mode) == args.mode
    m = 0
    for _ in range(args.calls):
        m = b.call("prefilter_device", pf, None)
    b.ctx.synchronize()
    print(json.dumps({"switch": args.mode, "route": b.route(), "scan": args.scan, "k": args.k, "calls": args.calls, "points_in": b.n, "points_out": m}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--calls", type=int, default=200)
    t.add_argument("--warmup", type=int, default=20)
    t.add_argument("--out", default="")
    t.add_argument("--switches", type=lambda v: [int(x) for x in v.split(",")], default=[1, 0])
    a = sub.add_parser("ab")
    a.add_argument("libs", nargs="+")
    a.add_argument("--rounds", type=int, default=2)
    a.add_argument("--calls", type=int, default=200)
    a.add_argument("--warmup", type=int, default=20)
    a.add_argument("--timeout", type=float, default=240.0)
    o = sub.add_parser("once")
    o.add_argument("--mode", type=int, choices=(0, 1), required=True)
    o.add_argument("--scan", choices=("VLP64", "VLP16"), default="VLP64")
    o.add_argument("--k", type=int, default=20)
    o.add_argument("--calls", type=int, default=3)
    ns = ap.parse_args()
    {"time": time_routes, "ab": ab, "once": once}[ns.cmd](ns)
