"""GPU: floor detection (csrc/floor.hip, mrgfe_floor_detect*) against the test-side restatement of FloorDetectionComponent::detect
(tests/floor_reference.py): the height band bit for bit, the normal filter's flags up to boundary cases, RANSAC bit for bit (coefficients, inliers,
iterations, skipped samples), detect() end to end, the device-input entry point, and the component's callback over a scan sequence."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import floor_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def scans():
    from mrg_slam_amd import prefilter, synth

    scene = synth.street_scene()
    poses = synth.arc_trajectory(30)
    out = {"VLP16": [prefilter(synth.synth_lidar(scene, poses[k], "VLP16", 7100 + k)) for k in range(30)],
           "VLP64": [prefilter(synth.synth_lidar(scene, poses[k], "VLP64", 7200 + k)) for k in range(2)]}
    return out


def _plane_close(a, b, deg=0.5, dist=0.02):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ang = math.degrees(math.acos(min(1.0, abs(float(np.dot(a[:3], b[:3])) / (np.linalg.norm(a[:3]) * np.linalg.norm(b[:3]))))))
    return ang <= deg and abs(a[3] - b[3]) <= dist


def _band(cloud, p):
    R, _ = fr.tilt_rotations(p.get("tilt_deg", 0.0))
    t = fr.transform(R, cloud)
    return t[fr.band_flags(t, p.get("sensor_height", 2.0), p.get("height_clip_range", 1.0))]


def test_height_band_is_bit_identical(scans):
    from mrg_slam_amd import FloorDetection

    for model in ("VLP16", "VLP64"):
        for cloud in scans[model][:2]:
            fd = FloorDetection(use_normal_filtering=False)
            fd.detect(cloud)
            ref = fr.detect(cloud, {"use_normal_filtering": False})
            got = fd.last.filtered
            assert fd.last.n_clipped == ref["n_clipped"] == len(ref["filtered"]) > 1000
            assert got.shape == ref["filtered"].shape and got.tobytes() == ref["filtered"].tobytes(), model


def test_normal_flags_match_up_to_the_boundary(scans):
    from mrg_slam_amd.floor_detection import floor_normals

    total, bad = 0, 0
    for cloud in scans["VLP16"][:2] + scans["VLP64"][:1]:
        band = _band(cloud, {})
        nr, keep = floor_normals(band, 20.0)
        rn, rkeep, ra = fr.normals(band, 20.0)
        cos_t = math.cos(20.0 * math.pi / 180.0)
        near = np.abs(ra - cos_t) < 1e-4
        differ = keep != rkeep
        assert not (differ & ~near).any(), np.nonzero(differ & ~near)[0][:10]
        total += len(band)
        bad += int(differ.sum())
        ok = np.isfinite(rn).all(axis=1)
        assert (np.isfinite(nr).all(axis=1) == ok).all()
        # the normals themselves agree to float rounding (device atan2f / sinf / cosf are not glibc's)
        agree = np.abs(np.abs(np.sum(nr[ok].astype(np.float64) * rn[ok], axis=1)) - 1.0) < 1e-4
        assert agree.sum() >= 0.999 * ok.sum()
    assert bad <= max(1, total // 1000)


def _synthetic_clouds():
    rng = np.random.default_rng(20241016)
    clouds = []
    for n in (0, 1, 2, 3, 4):
        clouds.append(rng.uniform(-5, 5, (n, 4)).astype(f32))
    line = np.zeros((40, 4), f32)
    line[:, 0] = np.arange(40, dtype=f32) * f32(0.25)
    clouds.append(line)  # all collinear: every sample skipped
    for i in range(200):
        n = int(rng.choice([10, 50, 100, 300, 1000]))
        frac = rng.uniform(0.3, 0.95)
        m = int(n * frac)
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        if i % 3 == 0:
            nrm = np.array([0.0, math.sin(math.radians(15)), math.cos(math.radians(15))])  # a slope
        u = np.cross(nrm, [1.0, 0, 0] if abs(nrm[0]) < 0.9 else [0, 1.0, 0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        a, b = rng.uniform(-8, 8, (2, m))
        on = (a[:, None] * u + b[:, None] * v + nrm * rng.uniform(-3, 3) + rng.normal(scale=0.02, size=(m, 3)))
        off = rng.uniform(-8, 8, (n - m, 3))
        pts = np.concatenate([on, off])
        if i % 5 == 0:  # duplicates
            pts = np.concatenate([pts, pts[: max(1, n // 4)]])
        if i % 7 == 0:  # quantised coordinates: exact zeros in the differences
            pts = np.round(pts * 4) / 4
        pts = pts[rng.permutation(len(pts))]
        clouds.append(np.c_[pts, rng.uniform(0, 1, len(pts))].astype(f32))
    for n in (20000, 20000):
        m = int(n * 0.8)
        g = np.c_[rng.uniform(-20, 20, (m, 2)), -1.73 + rng.normal(scale=0.02, size=m)]
        off = rng.uniform(-20, 20, (n - m, 3))
        clouds.append(np.c_[np.concatenate([g, off]), np.zeros(n)].astype(f32))
    return clouds


def test_ransac_is_bit_identical_to_the_sequential_loop():
    from mrg_slam_amd.floor_detection import floor_ransac

    clouds = _synthetic_clouds()
    assert len(clouds) >= 200
    skipped_seen = 0
    for i, c in enumerate(clouds):
        g, r = floor_ransac(c, 0.1), fr.ransac(c, 0.1)
        assert g["has_model"] == r["has_model"], i
        assert (g["iterations"], g["skipped"]) == (r["iterations"], r["skipped"]), (i, len(c), g["iterations"], r["iterations"], g["skipped"], r["skipped"])
        skipped_seen += r["skipped"] > 0
        if r["has_model"]:
            assert g["coeffs"].tobytes() == r["coeffs"].tobytes(), (i, g["coeffs"], r["coeffs"])
            assert np.array_equal(g["inliers"], r["inliers"]), i
    assert skipped_seen >= 2


def test_detect_end_to_end(scans):
    from mrg_slam_amd import FloorDetection

    cloud = scans["VLP16"][0]
    fd = FloorDetection()
    got = fd.detect(cloud)
    band = _band(cloud, {})
    from mrg_slam_amd.floor_detection import floor_normals

    _, gkeep = floor_normals(band, 20.0)
    ref = fr.detect(cloud, {})
    assert got is not None and ref["found"] and fd.last.reason == "found"
    if np.array_equal(gkeep, ref["keep"]):
        assert got.tobytes() == ref["coeffs"].tobytes()
        assert (fd.last.iterations, fd.last.n_inliers, fd.last.n_filtered) == (ref["iterations"], len(ref["inliers"]), len(ref["filtered"]))
        assert fd.last.inliers.tobytes() == ref["inliers"].tobytes()
    else:
        assert _plane_close(got, ref["coeffs"])
    assert abs(float(got[3]) - 1.73) < 0.05 and float(got[2]) > 0.99
    # no floor in the band, a 15 degree slope, too few points: none, for the reference's reason
    sky = cloud[cloud[:, 2] > -0.5]
    rng = np.random.default_rng(9)
    a, b = rng.uniform(-10, 10, (2, 4000))
    slope = np.c_[a, b, -2.0 + b * math.tan(math.radians(15)), np.zeros(4000)].astype(f32)
    slope = slope[np.abs(slope[:, 2] + 2.0) < 0.9]
    for c, p in ((sky, {}), (slope, {}), (cloud, {"floor_pts_thresh": 10**6})):
        fd = FloorDetection(**p)
        assert fd.detect(c) is None
        ref = fr.detect(c, p)
        assert not ref["found"] and fd.last.reason == ref["reason"], (fd.last.reason, ref["reason"])
    assert FloorDetection(floor_pts_thresh=10**6).detect(cloud) is None
    # a tilted sensor: the scan seen through R_y(12 deg)^T, detected with tilt_deg = 12
    R, _ = fr.tilt_rotations(12.0)
    tilted = cloud.copy()
    tilted[:, :3] = (cloud[:, :3].astype(np.float64) @ R.astype(np.float64)).astype(f32)  # rows: R^T p
    fd = FloorDetection(tilt_deg=12.0)
    got = fd.detect(tilted)
    ref = fr.detect(tilted, {"tilt_deg": 12.0})
    assert got is not None and ref["found"]
    assert _plane_close(got, ref["coeffs"])
    expect = np.r_[R.T.astype(np.float64) @ np.array([0, 0, 1.0]), 1.73]
    assert _plane_close(got, expect, deg=1.0, dist=0.05)


def test_device_input_matches_host_input(scans):
    import torch

    from mrg_slam_amd import FloorDetection, prefilter_to_device, synth

    scene = synth.street_scene()
    raw = synth.synth_lidar(scene, np.eye(4), "VLP16", 7300)
    buf = torch.empty((len(raw), 4), dtype=torch.float32, device="cuda")
    n = prefilter_to_device(raw, buf.data_ptr(), len(raw))
    torch.cuda.synchronize()
    host_cloud = buf[:n].cpu().numpy()
    a, b = FloorDetection(), FloorDetection()
    ga = a.detect_device(buf.data_ptr(), n)
    gb = b.detect(host_cloud)
    assert a.last.found and ga.tobytes() == gb.tobytes()
    for f in ("reason", "n_clipped", "n_filtered", "n_inliers", "iterations", "skipped"):
        assert getattr(a.last, f) == getattr(b.last, f), f
    assert a.last.filtered.tobytes() == b.last.filtered.tobytes() and a.last.inliers.tobytes() == b.last.inliers.tobytes()
    st = a.stage_times()
    assert st["ransac_waves"] >= 1 and st["host_waits"] >= 3


def test_component_over_a_sequence(scans):
    from mrg_slam_amd import FloorDetectionComponent
    from mrg_slam_amd.floor_detection import floor_normals

    hip, ref = FloorDetectionComponent(), FloorDetectionComponent(ops=fr.ReferenceOps())
    exact, found = 0, 0
    for k, cloud in enumerate(scans["VLP16"]):
        a, b = hip.cloud_callback(cloud), ref.cloud_callback(cloud)
        assert len(a) == len(b) and len(a) in (0, 4), (k, a, b)  # FloorCoeffs: four coefficients, or none (empty)
        found += len(a) == 4
        _, gkeep = floor_normals(_band(cloud, {}), 20.0)
        _, rkeep, _ = fr.normals(_band(cloud, {}), 20.0)
        if np.array_equal(gkeep, rkeep):
            assert np.asarray(a, f32).tobytes() == np.asarray(b, f32).tobytes(), k
            exact += 1
        elif a:
            assert _plane_close(a, b), k
    assert hip.cloud_callback(np.zeros((0, 4), f32)) is None
    assert exact >= 20 and found >= 25
