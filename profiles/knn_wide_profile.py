#!/usr/bin/env python3
"""k-NN kernels, narrow and wide (nn_knn_kernel / nn_knn_wide_kernel<R>, csrc/nn_grid.hip), on the self k-NN of the ~130k-point VLP-64 street scan
(distance filter only: the GICP covariance search of BASELINE config[2]).

  python3 profiles/knn_wide_profile.py [--other OTHER_LIB.so] [--rounds N] [--out FILE.md]

Kernel time is the library's own (HIP events around the launch, mrgfe_ctx_knn_stats); candidates per query come from a counted launch.  Every
measurement is a fresh child process: one warm-up call, then REPS calls, the median kept.  With --other (a libmrgfe.so of another commit) the
children alternate — other, this, other, this ... — over --rounds rounds, k = 20 and 64 in both and k = 65 / 128 / 256 in this build only: the
narrow kernel is the same code in both, so their difference has to lie within the spread of the other build's own rounds.  The CPU oracle's time for
the same call on the same machine is recorded for scale.  Writes the summary as markdown to --out (default profiles/knn_wide_summary.md)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 7
NARROW, WIDE = (20, 64), (65, 128, 256)


def scan_130k(ctx=None):
    from mrg_slam_amd import synth

    scene = synth.street_scene()
    raw = synth.synth_lidar(scene, synth.arc_trajectory(2)[0], "VLP64", synth.BASE_SEED)
    if ctx is None:
        from oracle import oracle as orc

        return orc.distance_filter(raw, 0.1, 35.0)
    from mrg_slam_amd import distance_filter

    return distance_filter(raw, 0.1, 35.0, ctx=ctx)


def child(ks):
    """one process, one library (MRGFE_LIB or the tree's): per k the median kernel ms of REPS calls after a warm-up, and the candidates per query"""
    from mrg_slam_amd import Context, knn
    from mrg_slam_amd._lib import lib

    ctx = Context(0)
    t = scan_130k(ctx)
    out = {"points": len(t)}
    for k in ks:
        knn(t, t, k, ctx=ctx)  # warm-up: allocations, code object load
        ms = []
        for _ in range(REPS):
            knn(t, t, k, ctx=ctx)
            ms.append(ctx.knn_stats()["ms"])
        lib().mrgfe_dbg_set_fit_stats(1)
        idx, _ = knn(t, t, k, ctx=ctx)
        st = ctx.knn_stats()
        lib().mrgfe_dbg_set_fit_stats(0)
        out[str(k)] = {"ms": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "candidates_per_query": st["candidates"] / max(st["queries"], 1.0),
                       "rows_complete": bool((idx[:, -1] >= 0).all())}
    print("RESULT " + json.dumps(out), flush=True)


def run_child(lib_path, ks):
    env = dict(os.environ)
    env.pop("MRGFE_LIB", None)
    if lib_path:
        env["MRGFE_LIB"] = os.path.abspath(lib_path)
        env["MRGFE_LIB_ALLOW_MISSING"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", ",".join(map(str, ks))], env=env, capture_output=True, text=True, timeout=240)
    if p.returncode != 0:
        sys.exit(f"child failed ({p.returncode}) with {lib_path or 'this build'}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")  # nothing more is started
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def oracle_times():
    from oracle import oracle as orc

    t = scan_130k()
    out = {}
    for k in WIDE:
        t0 = time.perf_counter()
        orc.knn(t, t, k)
        out[k] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--other", help="libmrgfe.so of another commit (the parent) to alternate with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_wide_summary.md"))
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child([int(k) for k in a.child.split(",")])
    this, other = [], []
    for r in range(a.rounds):
        if a.other:
            other.append(run_child(a.other, NARROW))
            print(f"round {r}: other {json.dumps(other[-1])}", flush=True)
        this.append(run_child(None, NARROW + WIDE))
        print(f"round {r}: this  {json.dumps(this[-1])}", flush=True)
    orc_s = {} if a.no_oracle else oracle_times()
    lines = ["# k-NN, narrow and wide: self k-NN of the 130k-point street scan", "",
             f"{this[0]['points']} points (VLP-64 street scan, distance filter only), one wavefront per query.  Kernel time from HIP events around the launch",
             f"(`mrgfe_ctx_knn_stats`); each figure is the median of {REPS} calls after a warm-up call in a fresh process, one process per round, the two",
             "builds alternating (other, this, other, this ...).  Produced by `profiles/knn_wide_profile.py`.", ""]
    if other:
        lines += ["## Narrow kernel (`nn_knn_kernel`), parent build against this one", "", "| k | parent ms per round | this ms per round | parent spread | median difference |", "|---|---|---|---|---|"]
        for k in NARROW:
            po, pt = [x[str(k)]["ms"] for x in other], [x[str(k)]["ms"] for x in this]
            lines.append(f"| {k} | {', '.join(f'{v:.4f}' for v in po)} | {', '.join(f'{v:.4f}' for v in pt)} | {max(po) - min(po):.4f} | {np.median(pt) - np.median(po):+.4f} |")
        lines.append("")
    lines += ["## This build, all k", "", "| k | kernel | ms per 130k queries (rounds) | candidates per query | CPU oracle, same call, same machine (s) |", "|---|---|---|---|---|"]
    for k in NARROW + WIDE:
        kern = "nn_knn_kernel" if k <= 64 else f"nn_knn_wide_kernel<{(k + 63) // 64}>"
        ms = [x[str(k)]["ms"] for x in this]
        assert all(x[str(k)]["rows_complete"] for x in this)
        lines.append(f"| {k} | `{kern}` | {', '.join(f'{v:.3f}' for v in ms)} | {this[0][str(k)]['candidates_per_query']:.1f} | {f'{orc_s[k]:.2f}' if k in orc_s else ''} |")
    lines += ["", "The CPU oracle column is the whole `orc.knn` call (its own search structure and search, host threads) — a scale, not a competitor.", ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
