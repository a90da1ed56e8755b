"""CPU: the scan-matching status record (``mrgfe_matching_status``) and its host arithmetic, ``mrgfe_status_poses`` —
``isometry2pose`` of the final transformation and of ``final.inverse() * msf_delta``
(apps/scan_matching_odometry_component.cpp:419,426-427) — against a numpy restatement.  No GPU is needed: the poses take no context."""
import ctypes as C

import numpy as np

_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)


def _quat(R):
    """Eigen::Quaterniond(Matrix3d) as x y z w, in float64 (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl for a 3 x 3 matrix;
    ``odometry.quat_w`` is its w in float).  Returns the quaternion and the branch taken: -1 trace > 0, else the index of the largest diagonal element."""
    R = np.asarray(R, dtype=np.float64)
    q = np.zeros(4)
    t = (R[0, 0] + R[1, 1]) + R[2, 2]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
        return q, -1
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (R[k, j] - R[j, k]) * t
    q[j] = (R[j, i] + R[i, j]) * t
    q[k] = (R[k, i] + R[i, k]) * t
    return q, i


def _pose(T):
    T = np.asarray(T, dtype=np.float64)
    q, branch = _quat(T[:3, :3])
    return np.concatenate([T[:3, 3], q]), branch


def _error_f64(final32, delta32):
    """(R^T, -R^T t) * delta in float64 from the float inputs."""
    F, D = final32.astype(np.float64), delta32.astype(np.float64)
    E = np.eye(4)
    E[:3, :3] = F[:3, :3].T @ D[:3, :3]
    E[:3, 3] = F[:3, :3].T @ D[:3, 3] - F[:3, :3].T @ F[:3, 3]
    return _pose(E)[0]


def _call(final32, delta32=None, sentinel=None):
    from mrg_slam_amd import _lib

    Fc = np.ascontiguousarray(final32.T, dtype=np.float32)
    Dc = None if delta32 is None else np.ascontiguousarray(delta32.T, dtype=np.float32)
    rel = np.full(7, np.nan)
    err = np.full(7, np.nan if sentinel is None else sentinel)
    st = _lib.lib().mrgfe_status_poses(Fc.ctypes.data_as(_fp), None if Dc is None else Dc.ctypes.data_as(_fp), rel.ctypes.data_as(_dp), err.ctypes.data_as(_dp))
    assert st == 0
    return rel, err


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _rigid(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, dtype=np.float32)
    T[:3, 3] = np.asarray(t, dtype=np.float32)
    return T


def _random_rigid(rng, max_t=50.0):
    axis = rng.normal(size=3)
    return _rigid(_rot(axis, rng.uniform(-np.pi, np.pi)), rng.uniform(-max_t, max_t, 3))


def _check(final32, delta32):
    rel, err = _call(final32, delta32)
    want, branch = _pose(final32)
    assert rel.tobytes() == want.tobytes(), (rel, want)  # floats widened exactly, then f64 + - * / sqrt: the same roundings
    tol = 2e-6 * (1.0 + np.linalg.norm(final32[:3, 3].astype(np.float64)) + np.linalg.norm(delta32[:3, 3].astype(np.float64)))
    want_err = _error_f64(final32, delta32)
    assert np.all(np.abs(err - want_err) <= tol), (err, want_err, tol)
    return branch


def test_struct_size_and_layout():
    from mrg_slam_amd import _lib

    assert _lib.lib().mrgfe_matching_status_size() == 144 == C.sizeof(_lib.MatchingStatus)
    S = _lib.MatchingStatus
    assert (S.has_converged.offset, S.n_points.offset, S.num_inliers.offset, S.inlier_fraction.offset, S.matching_error.offset) == (0, 4, 8, 12, 16)
    assert (S.relative_pose.offset, S.prediction_error.offset, S.has_prediction.offset, S.reserved.offset) == (24, 80, 136, 140)


def test_identity():
    I = np.eye(4, dtype=np.float32)
    rel, err = _call(I, I)
    assert rel.tolist() == [0, 0, 0, 0, 0, 0, 1] and err.tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert _check(I, I) == -1


def test_random_rigid_transforms():
    rng = np.random.default_rng(20240607)
    for _ in range(200):
        _check(_random_rigid(rng), _random_rigid(rng))


def test_every_branch_of_the_quaternion_conversion():
    """trace > 0, and each diagonal element largest with trace <= 0 — among them rotations by exactly pi (R = diag(1, -1, -1) and its kin: trace -1)."""
    rng = np.random.default_rng(7)
    cases = [(_rot([0.2, -0.3, 0.9], 0.4), -1)]
    for i in range(3):
        axis = np.zeros(3)
        axis[i] = 1.0
        exact_pi = -np.eye(3)
        exact_pi[i, i] = 1.0
        cases.append((exact_pi, i))
        cases.append((_rot(axis + [0.05, -0.04, 0.03], 3.0), i))
        cases.append((_rot(axis + [-0.02, 0.05, 0.04], -2.9), i))
    seen = set()
    for R, want_branch in cases:
        T = _rigid(R, rng.uniform(-5, 5, 3))
        assert _pose(T)[1] == want_branch
        seen.add(_check(T, _random_rigid(rng, 5.0)))
        rel, _ = _call(T)
        assert abs(np.linalg.norm(rel[3:]) - 1.0) < 1e-6
    assert seen == {-1, 0, 1, 2}
    # the exact half turn about x: (x y z w) = (1 0 0 0)
    rel, _ = _call(_rigid(np.diag([1.0, -1.0, -1.0]), [1, 2, 3]))
    assert rel.tolist() == [1, 2, 3, 1, 0, 0, 0]


def test_null_delta_leaves_the_prediction_error_untouched():
    rng = np.random.default_rng(3)
    T = _random_rigid(rng)
    rel, err = _call(T, None, sentinel=12345.5)
    assert rel.tobytes() == _pose(T)[0].tobytes()
    assert err.tolist() == [12345.5] * 7
    # ... and it may then be NULL
    from mrg_slam_amd import _lib

    Fc = np.ascontiguousarray(T.T)
    assert _lib.lib().mrgfe_status_poses(Fc.ctypes.data_as(_fp), None, rel.ctypes.data_as(_dp), None) == 0


def test_python_status_poses_wrapper():
    from mrg_slam_amd.registration import status_poses

    rng = np.random.default_rng(11)
    T, D = _random_rigid(rng), _random_rigid(rng)
    rel, err = status_poses(T, D)
    a, b = _call(T, D)
    assert rel.tobytes() == a.tobytes() and err.tobytes() == b.tobytes()
    assert status_poses(T)[1] is None


def test_null_arguments_are_invalid_and_need_no_device():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    F = np.eye(4, dtype=np.float32)
    rel, err = np.zeros(7), np.zeros(7)
    assert L.mrgfe_status_poses(None, None, rel.ctypes.data_as(_dp), err.ctypes.data_as(_dp)) == _lib.ERR_INVALID
    assert L.mrgfe_status_poses(F.ctypes.data_as(_fp), None, None, err.ctypes.data_as(_dp)) == _lib.ERR_INVALID
    assert L.mrgfe_status_poses(F.ctypes.data_as(_fp), F.ctypes.data_as(_fp), rel.ctypes.data_as(_dp), None) == _lib.ERR_INVALID
    assert b"mrgfe_status_poses" in L.mrgfe_last_error()
    s = _lib.MatchingStatus()
    assert L.mrgfe_reg_matching_status(None, 0.5, None, C.byref(s)) == _lib.ERR_INVALID
    assert b"mrgfe_reg_matching_status" in L.mrgfe_last_error()
