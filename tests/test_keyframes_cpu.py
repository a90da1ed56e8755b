"""CPU: the host side of the keyframe callback — ``KeyframeUpdater`` (src/mrg_slam/keyframe_updater.cpp:13-37) and the centre arithmetic of
``MrgSlamComponent::cloud_callback`` (apps/mrg_slam_component.cpp:397-407) against a numpy / scipy model written from the reference's text, the
binding's mirror of ``mrgfe_keyframe_params``, and what the three new entry points do with NULL arguments (no GPU is touched)."""
import ctypes as C

import numpy as np

TRANS, ANGLE = 1.0, 0.5236  # config/mrg_slam.yaml:163-164


def model_angle(R):
    """|rotation vector| of R by scipy where it is installed, else by the trace formula: what AngleAxisd(R).angle() is, up to rounding."""
    try:
        from scipy.spatial.transform import Rotation

        return float(np.linalg.norm(Rotation.from_matrix(R).as_rotvec()))
    except ImportError:
        return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


class ModelUpdater:
    """keyframe_updater.cpp:13-37 line by line on numpy's general inverse and product."""

    def __init__(self, trans, angle):
        self.trans, self.angle, self.first, self.accum, self.prev = trans, angle, True, 0.0, np.eye(4)

    def update(self, pose):
        if self.first:
            self.first, self.prev = False, np.array(pose)
            return True
        delta = np.linalg.inv(self.prev) @ pose
        dx, da = float(np.linalg.norm(delta[:3, 3])), model_angle(delta[:3, :3])
        if dx < self.trans and da < self.angle:
            return False
        self.accum += dx
        self.prev = np.array(pose)
        return True


def pose(t, rz=0.0, rx=0.0, ry=0.0):
    from mrg_slam_amd import synth

    return synth.make_pose(np.asarray(t, dtype=np.float64), synth.rot_xyz(rx, ry, rz))


def fresh():
    from mrg_slam_amd.keyframes import KeyframeUpdater

    u = KeyframeUpdater(TRANS, ANGLE)
    assert u.update(np.eye(4)) is True  # the first frame is always a keyframe (:17-21) ...
    assert u.get_accum_distance() == 0.0  # ... and adds no distance
    return u


def test_first_frame_is_a_keyframe_wherever_it_is():
    from mrg_slam_amd.keyframes import KeyframeUpdater

    u = KeyframeUpdater(TRANS, ANGLE)
    assert u.update(pose([100.0, -3.0, 2.0], 1.0)) is True and u.get_accum_distance() == 0.0
    assert u.update(pose([100.0, -3.0, 2.0], 1.0)) is False  # the same pose again: dx = 0 and da = 0


def test_thresholds_are_strict_comparisons():
    """:29-30 is ``dx < trans && da < angle -> return false``: a pose just BELOW both thresholds starts no keyframe; a pose EXACTLY at a threshold
    fails the strict comparison, so — as in the reference, and in the model above — it starts one, like a pose just above it."""
    below_t, below_a = np.nextafter(TRANS, 0.0), ANGLE - 1e-9
    u = fresh()
    assert u.update(pose([below_t, 0, 0], below_a)) is False and u.get_accum_distance() == 0.0
    for t, a in ((TRANS, 0.0), (np.nextafter(TRANS, 2.0), 0.0)):  # translation: at the threshold (dx == 1.0 exactly), just above it
        u, m = fresh(), ModelUpdater(TRANS, ANGLE)
        m.update(np.eye(4))
        assert u.update(pose([t, 0, 0], a)) is m.update(pose([t, 0, 0], a)) is True
        assert u.get_accum_distance() == t
    # rotation about z by the threshold: atan2 / the quaternion round the angle, so hold it against the mirror's own angle at and around the threshold
    from mrg_slam_amd.keyframes import KeyframeUpdater, angle_axis_angle

    P = pose([0.25, 0, 0], ANGLE)
    da = angle_axis_angle(P[:3, :3])
    assert abs(da - ANGLE) < 1e-15 * 8
    for thresh, expect in ((np.nextafter(da, 4.0), False), (da, True), (np.nextafter(da, 0.0), True)):  # da < thresh, da == thresh, da > thresh
        u = KeyframeUpdater(TRANS, thresh)
        u.update(np.eye(4))
        assert u.update(P) is expect
        assert u.get_accum_distance() == (0.25 if expect else 0.0)  # the distance grows only on an update (:34)


def test_angle_axis_angle_against_the_model():
    from mrg_slam_amd import synth
    from mrg_slam_amd.keyframes import angle_axis_angle

    rng = np.random.default_rng(5)
    assert angle_axis_angle(np.eye(3)) == 0.0
    for _ in range(200):
        R = synth.rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
        assert abs(angle_axis_angle(R) - model_angle(R)) < 1e-9
    for a in (1e-12, 1e-7, 0.5, np.pi - 1e-7, np.pi):  # tiny angles (where 2 acos(w) would lose them) and the half turn
        assert abs(angle_axis_angle(synth.rot_z(a)) - a) < 1e-12


def test_random_walk_and_the_accumulated_distance():
    from mrg_slam_amd.keyframes import KeyframeUpdater

    rng = np.random.default_rng(11)
    u, m = KeyframeUpdater(TRANS, ANGLE), ModelUpdater(TRANS, ANGLE)
    T, decisions = pose([3.0, -2.0, 0.5], 0.3), []
    for step in range(200):
        T = T @ pose(rng.normal(0, 0.35, 3) * [1, 1, 0.1], rng.normal(0, 0.2), rng.normal(0, 0.02), rng.normal(0, 0.02))
        a, b = u.update(T), m.update(T)
        assert a is b, step
        decisions.append(a)
        assert abs(u.get_accum_distance() - m.accum) <= 1e-12 * max(1.0, m.accum)
    assert 20 < sum(decisions) < 180  # both outcomes occur many times
    assert u.get_accum_distance() > 20.0


def test_centres_are_cast_to_float_after_the_double_product():
    from mrg_slam_amd.keyframes import others_positions_sensor, robot_radius_sqr

    odom = pose([1234.567891234, -987.654321987, 12.3456789], 0.7, 0.01, -0.02)
    map2odom = pose([-1200.123456789, 950.987654321, -3.2], -0.4)
    others = np.array([[31.23456789, -40.98765432, 9.87654321], [33.3333333, -37.7777777, 9.1111111], [0.0, 0.0, 0.0]])
    got = others_positions_sensor(odom, map2odom, others)
    assert got.dtype == np.float32 and got.shape == (3, 3)
    M = np.linalg.inv(odom) @ map2odom
    want = np.stack([(M @ np.r_[p, 1.0])[:3] for p in others])
    np.testing.assert_array_equal(got, want.astype(np.float32))  # f64 product, one rounding
    early = (M.astype(np.float32) @ np.c_[others, np.ones(3)].astype(np.float32).T).T[:, :3]  # cast first: a different result at these magnitudes
    assert not np.array_equal(got, early)
    # float(r * r) with the product in double (:406-407), not float(r) * float(r)
    r = 1.3
    assert robot_radius_sqr(r) == float(np.float32(r * r)) != float(np.float32(r) * np.float32(r))
    assert robot_radius_sqr(2.0) == 4.0


def test_callback_control_flow_with_injected_ops():
    """KeyframeCallback over scripted point operations: no call when the pose starts no keyframe, centres in the sensor frame, the removed cloud only
    when it is asked for, the original message kept when there is no other robot."""
    from mrg_slam_amd.keyframes import KeyframeCallback, others_positions_sensor

    calls = []

    class Ops:
        def keyframe(self, key, msg, centres, radius, want_removed):
            calls.append((key, len(centres), radius, want_removed))
            return np.zeros((3, 4), np.float32), (np.ones((2, 4), np.float32) if want_removed else None)

    cb = KeyframeCallback({"keyframe_delta_trans": TRANS, "keyframe_delta_angle": ANGLE, "robot_remove_points_radius": 1.5}, ops=Ops())
    cloud = np.zeros((5, 4), np.float32)
    r = cb.cloud_callback(np.eye(4), cloud)
    assert r is not None and r.key == 1 and r.kept is None and r.removed is None and r.accum_distance == 0.0  # no other robot: the message's cloud
    assert cb.cloud_callback(pose([0.5, 0, 0]), cloud) is None and len(calls) == 1
    cb.others_odom_poses = {"b": [4.0, 1.0, 0.0], "c": [9.0, 9.0, 1.0]}
    cb.trans_odom2map = pose([0.5, 0.25, 0.0], 0.1)
    odom = pose([2.0, 0, 0], 0.2)
    r = cb.cloud_callback(odom, cloud, removed_points_wanted=True)
    assert r.key == 2 and r.accum_distance == 2.0 and len(r.kept) == 3 and len(r.removed) == 2
    np.testing.assert_array_equal(r.centres_sensor, others_positions_sensor(odom, np.linalg.inv(cb.trans_odom2map), [[4.0, 1.0, 0.0], [9.0, 9.0, 1.0]]))
    r = cb.cloud_callback(pose([5.0, 0, 0]), cloud, key=77)
    assert r.key == 77 and r.removed is None
    assert calls == [(1, 0, 1.5, False), (2, 2, 1.5, True), (77, 2, 1.5, False)]


def test_struct_size_and_defaults():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    assert L.mrgfe_keyframe_params_size() == C.sizeof(_lib.KeyframeParams) == 32
    p = _lib.KeyframeParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    L.mrgfe_keyframe_default_params(C.byref(p))
    assert (p.width, p.height, p.point_step, p.row_step, p.off_x, p.off_y, p.off_z, p.off_intensity) == (0, 1, 16, 0, 0, 4, 8, 12)
    L.mrgfe_keyframe_default_params(None)  # a NULL pointer is ignored


def test_null_arguments_are_refused():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    p = _lib.KeyframeParams()
    L.mrgfe_keyframe_default_params(C.byref(p))
    p.width = 4
    cloud = np.zeros((4, 4), np.float32)
    data, out = cloud.ctypes.data_as(C.c_void_p), cloud.ctypes.data_as(C.POINTER(C.c_float))
    nk, nr = C.c_size_t(7), C.c_size_t(7)
    g = np.eye(4, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert L.mrgfe_keyframe_callback(None, 1, C.byref(p), data, 64, None, 0, 4.0, out, C.byref(nk), out, C.byref(nr)) == _lib.ERR_INVALID
    assert _lib.last_error().startswith("mrgfe_keyframe_callback:")
    assert L.mrgfe_keyframe_callback(None, 1, None, None, 0, None, 0, 4.0, None, None, None, None) == _lib.ERR_INVALID
    assert L.mrgfe_batch_add_target_from_store(None, None, 1) == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_batch_add_target_from_store:")
    assert L.mrgfe_batch_add_pair_from_store(None, 0, None, 1, g) == _lib.ERR_INVALID and _lib.last_error().startswith("mrgfe_batch_add_pair_from_store:")
    assert L.mrgfe_batch_add_pair_from_store(None, 0, None, 1, None) == _lib.ERR_INVALID
