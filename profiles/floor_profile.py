"""Per-scan cost of floor detection (mrgfe_floor_detect / mrgfe_floor_detect_device, csrc/floor.hip) on prefiltered VLP-16 and VLP-64 street scans:
median HIP-event time per stage (band, normals, RANSAC, inliers), host waits and RANSAC waves, wall time of the call; next to it the CPU time of the
test-side numpy restatement (tests/floor_reference.py) on the same scans, labelled as such — it is a restatement in Python, not PCL.

    python profiles/floor_profile.py [--scans 20] [--out record.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=20)
    ap.add_argument("--cpu-scans", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the medians as JSON to this file")
    a = ap.parse_args()

    import torch

    import floor_reference as fr
    from mrg_slam_amd import FloorDetection, prefilter, prefilter_to_device, synth

    scene = synth.street_scene()
    poses = synth.arc_trajectory(a.scans)
    report = {}
    for model in ("VLP16", "VLP64"):
        raws = [synth.synth_lidar(scene, poses[k], model, 8100 + k) for k in range(a.scans)]
        clouds = [prefilter(r) for r in raws]
        fd = FloorDetection()
        for c in clouds[:3]:  # warm-up: buffers grow, kernels load
            fd.detect(c)
        rows = {"wall_ms": [], "band_ms": [], "normals_ms": [], "ransac_ms": [], "inliers_ms": [], "host_waits": [], "ransac_waves": [], "iterations": [],
                "n_in": [], "n_clipped": [], "n_filtered": [], "n_inliers": []}
        for c in clouds:
            t0 = time.perf_counter()
            fd.detect(c)
            rows["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            st = fd.stage_times()
            for k in ("band_ms", "normals_ms", "ransac_ms", "inliers_ms", "host_waits", "ransac_waves"):
                rows[k].append(st[k])
            rows["iterations"].append(fd.last.iterations)
            rows["n_in"].append(len(c))
            rows["n_clipped"].append(fd.last.n_clipped)
            rows["n_filtered"].append(fd.last.n_filtered)
            rows["n_inliers"].append(fd.last.n_inliers)
        # device input: the prefilter chain's output left in HBM
        buf = torch.empty((max(len(r) for r in raws), 4), dtype=torch.float32, device="cuda")
        dev_wall = []
        for r in raws:
            n = prefilter_to_device(r, buf.data_ptr(), buf.shape[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fd.detect_device(buf.data_ptr(), n, want_clouds=False)
            dev_wall.append((time.perf_counter() - t0) * 1e3)
        cpu = []
        for c in clouds[: a.cpu_scans]:
            t0 = time.perf_counter()
            fr.detect(c, {})
            cpu.append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in rows.items()}
        med["device_input_wall_ms"] = statistics.median(dev_wall)
        med["numpy_restatement_cpu_ms (not PCL)"] = statistics.median(cpu)
        report[model] = med
        print(model, json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in med.items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
