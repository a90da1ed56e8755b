"""The odometry frame as one call against the calls it replaces, on full-size frames: 130k-point VLP-64 scans of the street scene behind the default
prefilter (the ~33k-point clouds the odometry really registers), 0.3 m apart, fed in ping-pong order so that consecutive frames are always one step apart.

  python profiles/odometry_callback_profile.py [--composed-lib OLD.so] [--frames 220] [--warmup 20] [--scans 12] [--out FILE.json]

Per frame, timed with the host clock around the frame's calls (every route ends in host waits of its own):
  composed   mrgfe_ingest_pointcloud2 (into one of two device buffers) -> mrgfe_reg_set_source_device -> mrgfe_reg_align -> mrgfe_reg_matching_status (when
             the status is wanted) -> mrgfe_reg_final_transformation -> mrgfe_reg_source_becomes_target (when the frame becomes the keyframe); first frame:
             mrgfe_reg_set_target_device.  Its guesses and decisions come from the library's controller stepped through mrgfe_dbg_odom_ctl_* (compiled
             arithmetic, as a C++ integrator's own would be), so that the two routes see the same guesses.  With --composed-lib these calls go to THAT
             library file (the parent commit's build), loaded beside this tree's.
  one_call   mrgfe_odom_frame on this tree's library.
The routes alternate frame by frame (which one goes first alternates too), on registrations of their own on one context each.  Before anything is timed
the routes' results are compared over the whole warm-up.  Reported per method (NDT_HIP, SMALL_GICP_HIP) and with / without the status: median, 10th and
90th percentile of the per-frame times, the keyframe switches and the outcomes seen."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FP = C.POINTER(C.c_float)


def load_other(path):
    """a second library file beside the package's: its entry points typed from the package's binding table (what it lacks is simply not bound)"""
    from mrg_slam_amd import _lib

    _lib.lib()  # (the package's library first: it brings the HIP runtime the way the package wants it)
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
    return L


class Composed:
    def __init__(self, L, method, want_status, cap):
        import torch

        from mrg_slam_amd import _lib

        self.L, self.T, self.want_status = L, _lib.lib(), want_status
        self.ctx = C.c_void_p()
        assert L.mrgfe_ctx_create(0, C.byref(self.ctx)) == 0
        p = _lib.RegParams()
        L.mrgfe_reg_default_params(method, C.byref(p))
        self.reg = C.c_void_p()
        assert L.mrgfe_reg_create(self.ctx, C.byref(p), C.byref(self.reg)) == 0
        op = _lib.OdomParams()
        self.T.mrgfe_odom_default_params(C.byref(op))
        self.ctl = C.c_void_p()
        assert self.T.mrgfe_dbg_odom_ctl_create(C.byref(op), C.byref(self.ctl)) == 0
        self.buf = [torch.empty((cap, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]  # the keyframe lives in the other one
        self.k = 0
        self.status, self.out = _lib.MatchingStatus(), _lib.OdomResult()
        self.guess, self.final, self.aligns = np.zeros(16, np.float32), np.zeros(16, np.float32), C.c_int(0)

    def frame(self, payload, n, stamp):
        L, T = self.L, self.T
        d = C.c_void_p(self.buf[self.k & 1].data_ptr())
        assert L.mrgfe_ingest_pointcloud2(self.ctx, payload.ctypes.data_as(C.POINTER(C.c_uint8)), n, 1, 16, 0, 0, 4, 8, 12, None, d) == 0
        T.mrgfe_dbg_odom_ctl_begin(self.ctl, stamp, None, C.byref(self.aligns), self.guess.ctypes.data_as(FP))
        if not self.aligns.value:
            assert L.mrgfe_reg_set_target_device(self.reg, d, n) == 0
            T.mrgfe_dbg_odom_ctl_end(self.ctl, 0, None, C.byref(self.out))
            self.k += 1
            return self.out
        assert L.mrgfe_reg_set_source_device(self.reg, d, n) == 0
        assert L.mrgfe_reg_align(self.reg, self.guess.ctypes.data_as(FP), None) == 0
        if self.want_status:
            assert L.mrgfe_reg_matching_status(self.reg, 0.5, None, C.byref(self.status)) == 0
        L.mrgfe_reg_final_transformation(self.reg, self.final.ctypes.data_as(FP))
        T.mrgfe_dbg_odom_ctl_end(self.ctl, L.mrgfe_reg_has_converged(self.reg), self.final.ctypes.data_as(FP), C.byref(self.out))
        if self.out.new_keyframe:
            assert L.mrgfe_reg_source_becomes_target(self.reg) == 0
            self.k += 1
        return self.out


class OneCall:
    def __init__(self, method, want_status):
        from mrg_slam_amd import _lib

        self.T, self.want_status = _lib.lib(), want_status
        self.ctx = C.c_void_p()
        assert self.T.mrgfe_ctx_create(0, C.byref(self.ctx)) == 0
        p = _lib.RegParams()
        self.T.mrgfe_reg_default_params(method, C.byref(p))
        self.reg = C.c_void_p()
        assert self.T.mrgfe_reg_create(self.ctx, C.byref(p), C.byref(self.reg)) == 0
        op = _lib.OdomParams()
        self.T.mrgfe_odom_default_params(C.byref(op))
        self.odom = C.c_void_p()
        assert self.T.mrgfe_odom_create(self.reg, C.byref(op), C.byref(self.odom)) == 0
        self.lay = _lib.KeyframeParams()
        self.T.mrgfe_keyframe_default_params(C.byref(self.lay))
        self.out = _lib.OdomResult()

    def frame(self, payload, n, stamp):
        self.lay.width = n
        assert self.T.mrgfe_odom_frame(self.odom, C.byref(self.lay), payload.ctypes.data_as(C.c_void_p), payload.nbytes, stamp, None, self.want_status, None, C.byref(self.out)) == 0
        return self.out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--composed-lib", default="", help="the library file the composed route calls (default: this tree's)")
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from mrg_slam_amd import Context, _lib, prefilter, synth

    scene, poses = synth.street_scene(), synth.arc_trajectory(a.scans, step=0.3, yaw_rate_deg=0.5)
    raw = synth.synth_lidar_many(scene, poses, "VLP64", [synth.BASE_SEED + k for k in range(a.scans)], workers=min(12, a.scans))
    pctx = Context(0)
    clouds = [np.ascontiguousarray(prefilter(r, ctx=pctx)) for r in raw]
    payloads = [np.array(c.view(np.uint8).reshape(-1), copy=True) for c in clouds]
    order = list(range(a.scans)) + list(range(a.scans - 2, 0, -1))  # ping-pong
    L_old = load_other(a.composed_lib) if a.composed_lib else _lib.lib()
    rows = []
    for method, name in ((_lib.NDT_HIP, "NDT_HIP"), (_lib.SMALL_GICP_HIP, "SMALL_GICP_HIP")):
        for want_status in (0, 1):
            routes = {"composed": Composed(L_old, method, want_status, max(len(c) for c in clouds) + 16), "one_call": OneCall(method, want_status)}
            per = {r: [] for r in routes}
            switches, outcomes = 0, [0, 0, 0, 0, 0]
            for j in range(a.warmup + a.frames):
                k = order[j % len(order)]
                outs = {}
                for r in (("composed", "one_call") if j % 2 == 0 else ("one_call", "composed")):
                    t0 = time.perf_counter()
                    o = routes[r].frame(payloads[k], len(clouds[k]), 10.0 + 0.1 * j)
                    dt = 1e3 * (time.perf_counter() - t0)
                    outs[r] = (o.outcome, o.new_keyframe, bytes(o.odom), bytes(o.trans))
                    if j >= a.warmup:
                        per[r].append(dt)
                if j < a.warmup or not a.composed_lib:
                    assert outs["composed"] == outs["one_call"], (name, j, "the routes differ")
                switches += int(j >= a.warmup and bool(outs["one_call"][1]))
                outcomes[outs["one_call"][0]] += int(j >= a.warmup)
            for r in routes:
                v = np.array(per[r])
                rows.append({"method": name, "want_status": want_status, "route": r, "composed_lib": os.path.basename(a.composed_lib) or "this tree", "points_raw": len(raw[0]),
                             "points_registered": len(clouds[0]), "frames": a.frames, "keyframe_switches": switches, "outcomes": dict(zip(_lib.ODOM_OUTCOMES, outcomes)), "ms_median": float(np.median(v)), "ms_p10": float(np.percentile(v, 10)),
                             "ms_p90": float(np.percentile(v, 90)), "ms_min": float(v.min())})
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
