"""The graph database's two loops as one call each against the per-item calls they replace, on VLP-64 keyframe clouds (synthetic scans of the
street scene along an arc, behind the default prefilter: about 33k points each).

  python profiles/graph_update_profile.py time [--out FILE.json] [--windows 12] [--clouds FILE.npz]
      End-to-end times, profiler off, both routes in the same process on the same store contents, alternating window by window.
        edges   new  mrgfe_map_store_edges, the whole list in one call
                old  mrgfe_map_store_information_matrix edge by edge
                for E = 1, 4, 13 edges (13: ten odometry edges keyframe k+1 -> k and three loop edges of the newest keyframe), with COLD grid caches
                (before every timed call, outside the clock, the single calls' cache is filled with eight other keyframes and the one call's set is
                rebuilt for another one: no key1 of the list has a grid, as in a tick whose keyframes are new) and WARM (the same list again).
        add     new  mrgfe_map_store_add_keyframes, M messages in one call
                old  mrgfe_keyframe_callback with 0 centres, message by message
                for M = 1, 10, 200 keyframe messages with pageable 16-byte and 32-byte (pcl::PointXYZI) records; a fresh store per window and route
                (created, and its first arena chunk allocated, outside the clock).
      The figure of a window is its time per CALL of the route (one list / one bulk of M messages).  Reported per route: median, minimum, 10th and
      90th percentile of the windows.  The two routes' results are compared (identical bits) before anything is timed.

  python profiles/graph_update_profile.py once --route edges_new|edges_old|add_new|add_old [--n 13] --clouds FILE.npz
      One call of one route and nothing else, for `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ...`.  The clouds come from
      FILE.npz (a `time` run with the same --clouds writes it).  The edge routes first put the keyframes into the store with mrgfe_map_store_add:
      one host-to-device copy per keyframe and no launch, to be subtracted from the trace's counts.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 11          # keyframes of the edge workload
N_FLUSH = 9     # small keyframes that only serve to push the others' grids out of the caches
ROUTES = ("new", "old")


def keyframe_clouds(ctx, path):
    from mrg_slam_amd import prefilter, synth

    if path and os.path.exists(path):
        z = np.load(path)
        return [np.ascontiguousarray(z[f"c{k}"], dtype=np.float32) for k in range(K)], z["poses"]
    scene, poses = synth.street_scene(), np.stack(synth.arc_trajectory(K))
    clouds = [np.ascontiguousarray(prefilter(synth.synth_lidar(scene, poses[k], "VLP64", synth.BASE_SEED + k), ctx=ctx)) for k in range(K)]
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.savez(path, poses=poses, **{f"c{k}": c for k, c in enumerate(clouds)})
    return clouds, poses


def edge_list(poses, E):
    """Keys are keyframe index + 1.  E odometry edges up to ten, then loop edges of the newest keyframe against the oldest ones."""
    from mrg_slam_amd import synth

    rng = np.random.default_rng(3)
    n_odo = min(E, 10) if E != 4 else 3
    pairs = [(k + 1, k) for k in range(n_odo)] + [(n_odo, j) for j in range(E - n_odo)]
    return [(a + 1, b + 1, synth.perturb_pose(np.linalg.inv(poses[a]) @ poses[b], rng, (0.05, 0.05, 0.02), (0.2, 0.2, 0.5))) for a, b in pairs]


class Edges:
    def __init__(self, ctx, clouds, poses, E):
        from mrg_slam_amd import MapCloudStore, _lib

        self.L, self._lib, self.ctx = _lib.lib(), _lib, ctx
        self.store = MapCloudStore(ctx)
        for k, c in enumerate(clouds):
            self.store.add(k + 1, c)
        rng = np.random.default_rng(9)
        for j in range(N_FLUSH):
            self.store.add(100 + j, rng.normal(0, 5, (500, 4)).astype(np.float32))
        self.p = _lib.InfParams()
        self.L.mrgfe_inf_default_params(C.byref(self.p))
        self.E = E
        self.rec = (_lib.GraphEdge * E)()
        for i, (k1, k2, rel) in enumerate(edge_list(poses, E)):
            self.rec[i].key1, self.rec[i].key2 = k1, k2
            self.rec[i].relpose[:] = np.asarray(rel, dtype=np.float64).T.reshape(16).tolist()
        self.flush_rec = (_lib.GraphEdge * 1)()
        self.flush_rec[0].key1, self.flush_rec[0].key2 = 100 + N_FLUSH - 1, 100
        self.flush_rec[0].relpose[:] = np.eye(4).reshape(16).tolist()
        self.inf, self.fit = np.zeros((E, 36)), np.zeros(E)
        self.eye = np.ascontiguousarray(np.eye(4).reshape(16))
        ctx.synchronize()

    def new(self):
        dp = C.POINTER(C.c_double)
        self._lib.check(self.L.mrgfe_map_store_edges(self.store._h, C.byref(self.p), self.E, self.rec, self.inf.ctypes.data_as(dp), self.fit.ctypes.data_as(dp)))

    def old(self):
        dp = C.POINTER(C.c_double)
        for i in range(self.E):
            r = self.rec[i]
            self._lib.check(self.L.mrgfe_map_store_information_matrix(self.store._h, C.byref(self.p), r.key1, r.key2, r.relpose, self.inf[i].ctypes.data_as(dp),
                                                                      C.cast(self.fit[i:].ctypes.data, dp)))

    def make_cold(self):
        """No key1 of the list has a grid afterwards: eight other keyframes fill the single calls' cache, another one replaces the one call's set."""
        dp = C.POINTER(C.c_double)
        out = C.c_double(0)
        for j in range(N_FLUSH - 1):
            self._lib.check(self.L.mrgfe_map_store_fitness(self.store._h, 100 + j, 100 + j + 1, self.eye.ctypes.data_as(dp), 1e300, C.byref(out)))
        m, f = np.zeros(36), np.zeros(1)
        self._lib.check(self.L.mrgfe_map_store_edges(self.store._h, C.byref(self.p), 1, self.flush_rec, m.ctypes.data_as(dp), f.ctypes.data_as(dp)))

    def run(self, route):
        (self.new if route == "new" else self.old)()


class Adds:
    def __init__(self, ctx, clouds, M, layout):
        from mrg_slam_amd import _lib
        from mrg_slam_amd.io import pcl_xyzi_records

        self.L, self._lib, self.ctx, self.M = _lib.lib(), _lib, ctx, M
        packed = layout == "packed16"
        self.payloads = [np.array(c.view(np.uint8).reshape(-1) if packed else pcl_xyzi_records(c).reshape(-1), copy=True) for c in clouds]  # pageable
        self.msgs = (_lib.KeyframeMsg * M)()
        for i in range(M):
            c, buf = clouds[i % len(clouds)], self.payloads[i % len(clouds)]
            p = _lib.KeyframeParams()
            self.L.mrgfe_keyframe_default_params(C.byref(p))
            p.width, p.point_step, p.off_intensity = len(c), (16 if packed else 32), (12 if packed else 16)
            self.msgs[i].layout, self.msgs[i].data, self.msgs[i].data_bytes = p, buf.ctypes.data, buf.nbytes
        self.points = sum(len(clouds[i % len(clouds)]) for i in range(M))
        self.key = 0
        self.stores = {}
        self.nk = C.c_size_t(0)

    def fresh_stores(self):
        from mrg_slam_amd import MapCloudStore

        self.stores = {}  # (the old ones go first: a window's clouds are freed before the next window's are allocated)
        for r in ROUTES:
            self.stores[r] = MapCloudStore(self.ctx)
            self.stores[r].add(1 << 40, np.zeros((1, 4), np.float32))  # the first arena chunk
        self.ctx.synchronize()

    def new(self):
        for i in range(self.M):
            self.key += 1
            self.msgs[i].key = self.key
        self._lib.check(self.L.mrgfe_map_store_add_keyframes(self.stores["new"]._h, self.M, self.msgs, None))

    def old(self):
        s = self.stores["old"]._h
        for i in range(self.M):
            self.key += 1
            m = self.msgs[i]
            self._lib.check(self.L.mrgfe_keyframe_callback(s, self.key, C.byref(m.layout), m.data, m.data_bytes, None, 0, 4.0, None, C.byref(self.nk), None, None))

    def run(self, route):
        (self.new if route == "new" else self.old)()


def stats(v, **kw):
    v = np.array(v)
    return dict(kw, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_p10=float(np.percentile(v, 10)), ms_p90=float(np.percentile(v, 90)))


def time_routes(args):
    from mrg_slam_amd import Context

    ctx = Context(0)
    clouds, poses = keyframe_clouds(ctx, args.clouds)
    rows = []
    for E in (1, 4, 13):
        e = Edges(ctx, clouds, poses, E)
        outs = {}
        for route in ROUTES:
            for _ in range(3):
                e.make_cold()
                e.run(route)
            outs[route] = (e.inf.copy(), e.fit.copy())
        assert np.array_equal(outs["new"][0].view(np.uint64), outs["old"][0].view(np.uint64)) and np.array_equal(outs["new"][1].view(np.uint64), outs["old"][1].view(np.uint64)), "the routes differ"
        for cache in ("cold", "warm"):
            per = {r: [] for r in ROUTES}
            for _ in range(args.windows):
                for route in ROUTES:  # alternating: a drift of the machine lands on both routes alike
                    spent = 0.0
                    for _ in range(args.edge_calls):
                        e.make_cold()
                        if cache == "warm":
                            e.run(route)
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        e.run(route)  # (both routes wait for their results themselves)
                        spent += time.perf_counter() - t0
                    per[route].append(1e3 * spent / args.edge_calls)
            for route in ROUTES:
                rows.append(stats(per[route], workload="edges", n=E, cache=cache, route=route, points_per_keyframe=int(np.mean([len(c) for c in clouds])), windows=args.windows,
                                  calls_per_window=args.edge_calls))
                print(json.dumps(rows[-1]), flush=True)
        del e
    for layout in ("packed16", "pcl32"):
        for M, calls in ((1, 20), (10, 6), (200, 1)):
            a = Adds(ctx, clouds, M, layout)
            a.fresh_stores()
            for route in ROUTES:
                a.run(route)
            k = a.key
            got = [a.stores[r].generate([kk], [np.eye(4)], None, 0.0, distance_far_thresh=0.0) for r, kk in (("new", k - M), ("old", k))]  # the last message of each
            assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)) and a.stores["new"].bytes() == a.stores["old"].bytes(), "the routes differ"
            per = {r: [] for r in ROUTES}
            for _ in range(args.windows):
                a.fresh_stores()
                for route in ROUTES:
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        a.run(route)
                    ctx.synchronize()
                    per[route].append(1e3 * (time.perf_counter() - t0) / calls)
            for route in ROUTES:
                rows.append(stats(per[route], workload="add", n=M, layout=layout, route=route, points=a.points, windows=args.windows, calls_per_window=calls))
                print(json.dumps(rows[-1]), flush=True)
            a.stores = {}
            del a
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def once(args):
    from mrg_slam_amd import Context

    assert os.path.exists(args.clouds), "once: give --clouds FILE.npz written by an earlier `time` run (the prefilter would add its launches to the trace)"
    ctx = Context(0)
    clouds, poses = keyframe_clouds(ctx, args.clouds)
    kind, route = args.route.split("_")
    if kind == "edges":
        w = Edges(ctx, clouds, poses, args.n)
    else:
        w = Adds(ctx, clouds, args.n, args.layout)
        w.fresh_stores()
    ctx.synchronize()
    w.run(route)
    ctx.synchronize()
    print(json.dumps({"route": args.route, "n": args.n, "setup_h2d_copies": (K + N_FLUSH) if kind == "edges" else 2}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--out", default="")
    t.add_argument("--windows", type=int, default=12)
    t.add_argument("--edge-calls", type=int, default=5)
    o = sub.add_parser("once")
    o.add_argument("--route", choices=("edges_new", "edges_old", "add_new", "add_old"), required=True)
    o.add_argument("--n", type=int, default=13)
    o.add_argument("--layout", choices=("packed16", "pcl32"), default="pcl32")
    for sp in (t, o):
        sp.add_argument("--clouds", default="", help="the keyframe clouds as an .npz file: loaded when it exists, else computed (GPU prefilter) and written there")
    a = ap.parse_args()
    (time_routes if a.cmd == "time" else once)(a)
