"""What the bounded best-candidate selection costs and saves on a node: the config[3] pair list (bench.make_loop_workload(): 256 loop-closure pairs on
64 VLP-64 keyframes behind the distance filter, groups = new keyframes, max_range = inf) through NodeMatcher([0] * m) for m = 1, 2, 4, 8 members.

  python profiles/node_select_profile.py [--out-dir profiles] [--runs 3] [--members 1,2,4,8]

Per member count: `align` (every candidate scored exactly) and `align_best` (two stages, the selection over the whole list between them), one warm-up
and then --runs timed runs each; and BatchMatcher.align_best on one batch holding the whole list.  A run is the wall time from the clear that starts
queueing the list to the records (clear, the add calls, the align), clouds in pageable host memory, every cloud keyed: after the warm-up the node's
targets and candidates and the batch's candidates are resident, the batch's targets go up every run (a batch has no keyed targets).
Before anything is timed, what the selection decides — states, winners, scores, every record's fitness, the intervals — and the records' T, converged,
iterations, evaluations and pair_id are compared with the one batch's, byte for byte.  H and trans_probability are COUNTED, not asserted: at this size
(130k-point clouds) the last bits of the NDT alignment's own Hessian and probability sums follow the composition of its launches, with mrgfe_node_align as
with mrgfe_node_align_best (the tool counts both against the one batch); the selection reads neither.

The members of every node here share ONE card: what the figures show is the cost of the protocol (two posts and two waits per member, the selection on
the calling thread, smaller launches per member), NOT scaling over GPUs.  Writes node_select_times.json and node_select_summary.md into --out-dir."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INF = float("inf")
REG = dict(transformation_epsilon=0.1, maximum_iterations=64)


def workload():
    import bench
    from mrg_slam_amd import distance_filter

    raw, pairs = bench.make_loop_workload()
    scans = [np.ascontiguousarray(distance_filter(s, 0.1, 35.0)) for s in raw]
    news = sorted({p[0] for p in pairs})
    group = np.array([news.index(p[0]) for p in pairs], dtype=np.int32)
    return scans, pairs, news, group


def queue(m, scans, pairs, news, node):
    m.clear()
    tid = {a: (m.add_target(scans[a], key=1000 + a) if node else m.add_target(scans[a])) for a in news}
    for a, b, guess, _ in pairs:
        m.add_pair(tid[a], scans[b], guess, key=1 + b)


def timed(fn, runs):
    out = []
    for k in range(runs + 1):  # the first run warms up
        t0 = time.perf_counter()
        res = fn()
        if k:
            out.append(1e3 * (time.perf_counter() - t0))
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--members", default="1,2,4,8")
    args = ap.parse_args()
    from mrg_slam_amd import BatchMatcher, NodeMatcher

    scans, pairs, news, group = workload()
    members = [int(x) for x in args.members.split(",")]
    times = {"pairs": len(pairs), "groups": len(news), "points_per_cloud_mean": float(np.mean([len(s) for s in scans])), "runs": args.runs, "unit": "ms per call, queueing included",
             "note": "the members of a node share one card: the protocol's cost, not scaling", "node": {}}

    bm = BatchMatcher(**REG)

    def batch_best():
        queue(bm, scans, pairs, news, node=False)
        return bm.align_best(INF, group)

    t, ref = timed(batch_best, args.runs)
    ref_bounds = bm.fit_bounds()
    times["batch_align_best"] = {"ms": t, "select_stats": bm.select_stats()}
    queue(bm, scans, pairs, news, node=False)
    ref_full = bm.align(INF)
    for m in members:
        node = NodeMatcher([0] * m, **REG)

        def node_best():
            queue(node, scans, pairs, news, node=True)
            return node.align_best(INF, group)

        def node_full():
            queue(node, scans, pairs, news, node=True)
            return node.align(INF)

        t_best, got = timed(node_best, args.runs)
        stats, bounds = node.select_stats(), node.fit_bounds()
        for a, b in zip((got[0]["fitness"],) + got[1:] + bounds, (ref[0]["fitness"],) + ref[1:] + ref_bounds):
            assert a.tobytes() == b.tobytes(), f"{m} members: the selection differs from the one batch's"
        t_full, full = timed(node_full, args.runs)
        for f in ("T", "converged", "iterations", "evaluations", "pair_id"):
            assert got[0][f].tobytes() == ref[0][f].tobytes(), f"{m} members: {f} of align_best differs from the one batch's"

        def differing(a, b):
            return {f: k for f in a.dtype.names for k in [int(sum(a[f][i].tobytes() != b[f][i].tobytes() for i in range(len(a))))] if k}

        times["node"][str(m)] = {"align_best_ms": t_best, "align_ms": t_full, "select_stats": stats,
                                 "pairs_differing_from_one_batch": {"align": differing(full, ref_full), "align_best": differing(got[0], ref[0])}}
        print(f"{m} members: align {statistics.median(t_full):.2f} ms, align_best {statistics.median(t_best):.2f} ms; {stats}", flush=True)
        node.close()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "node_select_times.json"), "w") as f:
        json.dump(times, f, indent=1)
    med = statistics.median
    lines = ["# Bounded selection on a node: config[3], one MI355X", "",
             f"{len(pairs)} pairs in {len(news)} groups (new keyframes), max_range = inf, NDT_HIP; median of {args.runs} runs after a warm-up, milliseconds per call from",
             "the clear that starts queueing to the records (`profiles/node_select_profile.py`; every run in `node_select_times.json`).", "",
             "**All members of a node share the one card.** The figures show what the two-stage protocol costs (two posts and two waits per member, the selection",
             "on the calling thread, smaller launches per member), not how the node scales over GPUs.", "",
             "| members | `align` | `align_best` | `align_best` / `align` | pruned | exact | bound stage (largest member) | contender stage |", "|---|---|---|---|---|---|---|---|"]
    for m in members:
        r = times["node"][str(m)]
        s = r["select_stats"]
        lines.append(f"| {m} | {med(r['align_ms']):.2f} | {med(r['align_best_ms']):.2f} | {med(r['align_best_ms']) / med(r['align_ms']):.3f} | {int(s['pruned'])} | {int(s['exact'])} | "
                     f"{s['ms_bound']:.2f} | {s['ms_contend']:.2f} |")
    b = times["batch_align_best"]
    one = times["node"].get("1")
    lines += ["", f"One batch holding the whole list, `BatchMatcher.align_best`: {med(b['ms']):.2f} ms ({int(b['select_stats']['pruned'])} pruned)."
              + (f"  The one-member node against it: {med(one['align_best_ms']) / med(b['ms']):.3f} (the node keeps its targets resident by key, the batch uploads them every run)." if one else ""),
              "", "States, winners, scores, fitness values, intervals, T, converged, iterations, evaluations and pair_id were compared with the one batch's before timing,",
              "byte for byte, for every member count.  H and trans_probability are counted, not asserted: at this size the last bits of the NDT alignment's own sums",
              "follow the composition of its launches, in `align` as in `align_best`; the selection reads neither.  Pairs differing from the one batch",
              "(`align` / `align_best`): "
              + "; ".join(f"{m} members: {times['node'][str(m)]['pairs_differing_from_one_batch']['align'] or 'none'} / {times['node'][str(m)]['pairs_differing_from_one_batch']['align_best'] or 'none'}" for m in members) + "."]
    with open(os.path.join(args.out_dir, "node_select_summary.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
