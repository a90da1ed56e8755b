"""CPU: the test-side restatement of floor detection (tests/floor_reference.py) and the ABI defaults of mrgfe_floor_params."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import floor_reference as fr  # noqa: E402

f32 = np.float32


def test_mt19937_pin():
    mt = fr.MT19937(5489)
    for _ in range(9999):
        mt()
    assert mt() == 4123659995  # the 10000th output of the default-seeded mt19937 (C++11 [rand.predef])


def test_band_edges():
    h, r = 2.0, 1.0
    z = np.array([-(h - r), -(h + r), -2.0, np.nextafter(f32(-(h + r)), f32(-10)), np.nextafter(f32(-(h - r)), f32(-10))], dtype=f32)
    cloud = np.zeros((len(z), 4), dtype=f32)
    cloud[:, 2] = z
    keep = fr.band_flags(cloud, h, r)
    assert keep.tolist() == [False, True, True, False, True]


def test_normal_agrees_with_eigh():
    rng = np.random.default_rng(3)
    for _ in range(20):
        pts = rng.normal(size=(10, 3)).astype(f32) * np.array([2.0, 1.0, 0.05], dtype=f32)
        cloud = np.concatenate([pts, np.zeros((10, 1), f32)], axis=1)
        n = fr.point_normal(cloud, np.arange(10))
        w, v = np.linalg.eigh(np.cov(pts.astype(np.float64).T, bias=True))
        ref = v[:, 0]
        assert abs(abs(float(np.dot(n, ref))) - 1.0) < 1e-4, (n, ref)
    # fewer than three neighbours: NaN normal, and the filter drops it
    n = fr.point_normal(np.zeros((2, 4), f32), np.array([0, 1, -1]))
    assert np.isnan(n).all()
    keep, _ = fr.normal_keep(n[None, :], 20.0)
    assert not keep[0]


def test_reference_ransac_recovers_a_plane_with_clutter():
    rng = np.random.default_rng(11)
    m = 600
    ground = np.c_[rng.uniform(-10, 10, (m, 2)), np.full(m, -1.73)].astype(f32)
    clutter = rng.uniform(-10, 10, (200, 3)).astype(f32)
    clutter[:, 2] = np.abs(clutter[:, 2]) + 0.5
    cloud = np.concatenate([np.c_[ground, np.zeros(m)], np.c_[clutter, np.zeros(200)]]).astype(f32)
    r = fr.ransac(cloud, 0.1)
    assert r["has_model"] and r["skipped"] == 0 and 1 <= r["iterations"] < 50
    c = r["coeffs"] * np.sign(r["coeffs"][2])
    assert np.allclose(c, [0, 0, 1, 1.73], atol=1e-5), c
    assert set(r["inliers"].tolist()) == set(range(m))
    # fewer than three points: no model, iterations_ = INT_MAX - 1 (getSamples); collinear points: every sample skipped
    r2 = fr.ransac(cloud[:2])
    assert r2["iterations"] == 2**31 - 2 and not r2["has_model"]
    line = np.zeros((50, 4), f32)
    line[:, 0] = np.arange(50, dtype=f32)
    rl = fr.ransac(line)
    assert not rl["has_model"] and rl["iterations"] == 0 and rl["skipped"] == fr.MAX_SKIP


def test_reference_detect_reasons():
    rng = np.random.default_rng(5)
    m = 2000
    ground = np.c_[rng.uniform(-15, 15, (m, 2)), np.full(m, -1.73), np.zeros(m)].astype(f32)
    r = fr.detect(ground, {"use_normal_filtering": False})
    assert r["found"] and np.allclose(r["coeffs"], [0, 0, 1, 1.73], atol=1e-5)
    assert fr.detect(ground + np.array([0, 0, 10, 0], f32), {})["reason"] == "none_after_clip"
    assert fr.detect(ground, {"use_normal_filtering": False, "floor_pts_thresh": m + 1})["reason"] == "too_few_filtered"
    assert fr.detect(np.zeros((0, 4), f32))["reason"] == "empty_input"


def test_default_params_match_the_documented_defaults():
    os.environ.setdefault("MRGFE_NO_TORCH", "1")
    from mrg_slam_amd import _lib
    from mrg_slam_amd.floor_detection import DEFAULTS

    q = _lib.FloorParams()
    _lib.lib().mrgfe_floor_default_params(C.byref(q))
    got = {f: getattr(q, f) for f, _ in _lib.FloorParams._fields_}
    # apps/floor_detection_component.cpp:55-62 and config/mrg_slam.yaml:113-122
    assert got == {"tilt_deg": 0.0, "sensor_height": 2.0, "height_clip_range": 1.0, "floor_pts_thresh": 512, "floor_normal_thresh_deg": 10.0,
                   "use_normal_filtering": 1, "normal_filter_thresh_deg": 20.0}
    assert {k: (int(v) if isinstance(v, bool) else v) for k, v in DEFAULTS.items()} == got
    assert {k: (int(v) if isinstance(v, bool) else v) for k, v in fr.DEFAULTS.items()} == got
