#!/usr/bin/env python3
"""PCL_NDT_HIP (and NDT_HIP as a yardstick) in the reference's summation order, opened per context by mrgfe_ctx_set_ndt_reference_order:
    python3 profiles/pclndt_reforder_profile.py [soak scenes=1200] [soak seed=79] [out dir=profiles]
1. the PCL NDT soak (oracle/replay.py pclndt_soak) with the default context switched on — every scene must equal the reference-order oracle bit for bit; a
   scene that does not is written to <out dir>/pclndt_reforder_case_<n>.npz (clouds, guess, parameters) — and the same scenes on the default path, which
   names the scenes that leave the 1e-4 bar there;
2. one config[1]-sized pair (VLP-64 street scans, ~130k points, warm guess): milliseconds per evaluation (kinds 0 and 2) and per alignment, reference order
   against the default path of the same library, for PCL_NDT_HIP and NDT_HIP (DIRECT7).
Writes <out dir>/pclndt_reforder_summary.md (the measured part) and prints the same figures as one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def soak(cases, seed, out_dir):
    from mrg_slam_amd._lib import default_context
    from oracle.replay import pclndt_soak, soak_scene

    out = {}
    for name, on in (("reference_order", True), ("default", False)):
        default_context().set_ndt_reference_order(on)
        try:
            t0 = time.perf_counter()
            st = pclndt_soak(cases, seed)
            st["seconds"] = time.perf_counter() - t0
        finally:
            default_context().set_ndt_reference_order(False)
        out[name] = st
    if out["reference_order"]["exact"] != cases:  # find and keep the scenes: the same draws as pclndt_soak
        from mrg_slam_amd import PclNdtHip
        from oracle import oracle as orc

        default_context().set_ndt_reference_order(True)
        try:
            rng = np.random.default_rng(seed)
            kept = []
            for c in range(cases):
                tgt, src, guess, _ = soak_scene(rng)
                eps, res, iters = float(rng.choice([0.1, 0.01, 1e-3, 1e-5, 1e-7])), float(rng.choice([0.5, 1.0, 1.5, 2.0])), int(rng.choice([35, 64]))
                g, o = PclNdtHip(resolution=res, transformation_epsilon=eps, maximum_iterations=iters), orc.PclNdt(resolution=res, transformation_epsilon=eps, maximum_iterations=iters)
                for r in (g, o):
                    r.setInputTarget(tgt)
                    r.setInputSource(src)
                    r.align(guess)
                if not np.array_equal(g.getFinalTransformation(), o.getFinalTransformation()) and len(kept) < 4:
                    np.savez_compressed(os.path.join(out_dir, f"pclndt_reforder_case_{c}.npz"), tgt=tgt, src=src, guess=guess, res=res, eps=eps, iters=iters)
                    kept.append(c)
            out["reference_order"]["kept_cases"] = kept
        finally:
            default_context().set_ndt_reference_order(False)
    return out


def timings():
    from mrg_slam_amd import Context, NdtHip, PclNdtHip, distance_filter, synth
    from oracle import oracle as orc

    scene = synth.street_scene()
    tgt, src, rel = synth.scan_pair(0, "VLP64", scene)
    ft, fs = distance_filter(tgt), distance_filter(src)
    guess = synth.warm_guess(rel, 0)
    p = np.array([0.2, -0.05, 0.01, 0.012, -0.006, 0.025])
    T = orc.pose_to_matrix(p)
    out = {"points": int(len(fs))}
    for label, cls, kw in (("PCL_NDT_HIP", PclNdtHip, dict(transformation_epsilon=1e-5, maximum_iterations=30)),
                           ("NDT_HIP", NdtHip, dict(transformation_epsilon=0.001, maximum_iterations=64, search="DIRECT7"))):
        row = {}
        for name, on in (("default", False), ("reference_order", True)):
            ctx = Context(0)
            ctx.set_ndt_reference_order(on)
            r = cls(ctx=ctx, **kw)
            assert r.setInputTarget(ft) == 0
            r.setInputSource(fs)
            m = {}
            for mode in (0, 2):
                t = []
                for rep in range(6):
                    t0 = time.perf_counter()
                    r.evaluate(T, p, mode)
                    t.append(1e3 * (time.perf_counter() - t0))
                m[f"evaluate_kind{mode}_ms"] = float(np.median(t[1:]))
                m[f"pairs_per_point_kind{mode}"] = r.eval_neighbours / len(fs)
            t = []
            for rep in range(4):
                t0 = time.perf_counter()
                r.align(guess)
                t.append(1e3 * (time.perf_counter() - t0))
            m["align_ms"] = float(np.median(t[1:]))
            m["iterations"], m["evaluations"] = int(r.getFinalNumIteration()), int(r.evals)
            row[name] = m
            del r
            ctx.close()
        out[label] = row
    return out


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 1200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 79
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    res = {"timings": timings(), "soak": soak(cases, seed, out_dir)}
    s, tm = res["soak"], res["timings"]
    lines = ["# PCL_NDT_HIP in the reference's summation order (`mrgfe_ctx_set_ndt_reference_order`)", "",
             "Measured by `profiles/pclndt_reforder_profile.py` on one MI355X.", "",
             f"## Soak: {cases} random scenes (`oracle/replay.py pclndt_soak`, seed {seed}) against the reference-order oracle", "",
             "| path | bit-identical | over the 1e-4 bar | worst (m / rad) | flag or iteration mismatches | evaluation-count mismatches | iterations | seconds |", "|---|---|---|---|---|---|---|---|"]
    for name in ("reference_order", "default"):
        st = s[name]
        lines.append(f"| {name.replace('_', ' ')} | {st['exact']} / {st['cases']} | {st['over_bar']} | {st['worst']:.3g} | {st['flag_or_iteration_mismatch']} | {st['evaluation_count_mismatch']} | "
                     f"{st['iterations_total']} | {st['seconds']:.0f} |")
    lines += ["", "Scenes over the bar on the default path: " + ("; ".join(f"{c['case']} ({c['dt_m']:.3g} m, {c['dr_rad']:.3g} rad, {c['iterations_oracle']} iterations)" for c in s["default"]["over_bar_cases"]) or "none") + ".",
              "Scenes over the bar in reference order: " + ("; ".join(c["case"] for c in s["reference_order"]["over_bar_cases"]) or "none") + ".", "",
              f"## One full-size pair ({tm['points']} source points, host wall time, median)", "",
              "| method | path | evaluation, kind 0 (ms) | evaluation, kind 2 (ms) | alignment (ms) | iterations | evaluations | (point, voxel) pairs per point |", "|---|---|---|---|---|---|---|---|"]
    for label in ("PCL_NDT_HIP", "NDT_HIP"):
        for name in ("default", "reference_order"):
            m = tm[label][name]
            lines.append(f"| {label} | {name.replace('_', ' ')} | {m['evaluate_kind0_ms']:.2f} | {m['evaluate_kind2_ms']:.2f} | {m['align_ms']:.1f} | {m['iterations']} | {m['evaluations']} | {m['pairs_per_point_kind0']:.2f} |")
    with open(os.path.join(out_dir, "pclndt_reforder_summary.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
