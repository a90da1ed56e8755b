"""Host mirror of the keyframe path of ``MrgSlamComponent`` (``apps/mrg_slam_component.cpp:358-456`` of the reference, ``cloud_callback``) with
``KeyframeUpdater::update`` (src/mrg_slam/keyframe_updater.cpp:13-37) in front of it: decide whether the odometry pose starts a new keyframe,
bring the other robots' positions into the sensor frame, split off the points that hit them, and hand the kept cloud to the keyframe.

``ops`` supplies the point operations, as in ``prefiltering.py``: by default the HIP path in one call (``mrgfe_keyframe_callback``: the message
goes up once and the kept cloud stays in the shared :class:`MapCloudStore`, where map generation, the edge information matrices and loop closure
name it by key); a test injects the composed route or the CPU oracle, and the SAME control flow runs over all of them.

What the ROS side does around it (the message filter that pairs odometry and cloud, ``odom2isometry``, the publishers, ``add_odom_keyframe``)
stays with the caller: poses are 4 x 4 float64 matrices (``Eigen::Isometry3d``), the cloud is a PointCloud2 given as a dict (``data``, ``width``,
``height``, ``point_step``, ``fields``, optionally ``row_step``) or a packed [n, 4] float32 array."""
from __future__ import annotations

import dataclasses

import numpy as np

DEFAULTS = {  # config/mrg_slam.yaml:134,163-164 (the component's declare_parameter defaults are 2.0 / 2.0 / 2.0: apps/mrg_slam_component.cpp:255,287-288)
    "keyframe_delta_trans": 1.0,
    "keyframe_delta_angle": 0.5236,
    "robot_remove_points_radius": 2.0,
}


def angle_axis_angle(R) -> float:
    """``Eigen::AngleAxisd(R).angle()`` in double.  [UPSTREAM-RECALL] Eigen 3.3 Geometry/AngleAxis.h (it is not in the reference tree):
    ``AngleAxis::operator=(MatrixBase)`` goes through ``QuaternionType(mat)`` (the conversion ``loop_detector._quat_from_matrix`` restates), and
    ``operator=(QuaternionBase q)`` is ``n = q.vec().norm(); if (n < epsilon) n = q.vec().stableNorm(); angle = n != 0 ? 2 * atan2(n, |q.w()|) : 0``.
    The result lies in [0, pi]."""
    from .loop_detector import _quat_from_matrix

    q = _quat_from_matrix(R, np.float64)  # (w, x, y, z)
    v = q[1:]
    n = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    if n < np.finfo(np.float64).eps:
        m = float(np.max(np.abs(v)))  # stableNorm: scaled by the largest magnitude
        n = m * float(np.sqrt(np.sum((v / m) ** 2))) if m > 0.0 else 0.0
    return 2.0 * float(np.arctan2(n, abs(float(q[0])))) if n != 0.0 else 0.0


def isometry_inverse(T) -> np.ndarray:
    """``Eigen::Isometry3d::inverse()``: the rotation transposed, the translation -R^T t (Transform.h, mode Isometry), in double."""
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    Rt = T[:3, :3].T
    out[:3, :3] = Rt
    out[:3, 3] = -(Rt @ T[:3, 3])
    return out


class KeyframeUpdater:
    """keyframe_updater.cpp:7-44: the first pose always starts a keyframe; afterwards one starts unless the pose is closer than
    ``keyframe_delta_trans`` AND turned by less than ``keyframe_delta_angle`` from the previous keyframe's pose (both comparisons strict, :29-30).
    ``accum_distance`` grows by the translation only when a keyframe starts (:34)."""

    def __init__(self, keyframe_delta_trans: float = DEFAULTS["keyframe_delta_trans"], keyframe_delta_angle: float = DEFAULTS["keyframe_delta_angle"]):
        self.keyframe_delta_trans = float(keyframe_delta_trans)
        self.keyframe_delta_angle = float(keyframe_delta_angle)
        self.is_first = True
        self.accum_distance = 0.0
        self.prev_keypose = np.eye(4)

    def update(self, pose) -> bool:
        pose = np.array(pose, dtype=np.float64)
        if self.is_first:  # :17-21
            self.is_first = False
            self.prev_keypose = pose
            return True
        delta = isometry_inverse(self.prev_keypose) @ pose  # :24
        t = delta[:3, 3]
        dx = float(np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]))  # delta.translation().norm()
        da = angle_axis_angle(delta[:3, :3])
        if dx < self.keyframe_delta_trans and da < self.keyframe_delta_angle:  # :29-32
            return False
        self.accum_distance += dx
        self.prev_keypose = pose
        return True

    def get_accum_distance(self) -> float:
        return self.accum_distance


def others_positions_sensor(odom, map2odom, others_positions) -> np.ndarray:
    """:397-404: ``map2sensor = odom.inverse() * map2odom`` in double, every position ``(map2sensor * p).cast<float>()`` — the cast comes after
    the product.  Returns [K, 3] float32."""
    map2sensor = isometry_inverse(odom) @ np.asarray(map2odom, dtype=np.float64)
    pos = np.asarray(others_positions, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(pos), 3), dtype=np.float32)
    for i, p in enumerate(pos):
        out[i] = (map2sensor[:3, :3] @ p + map2sensor[:3, 3]).astype(np.float32)
    return out


def robot_radius_sqr(radius: float) -> float:
    """:406-407: ``float robot_radius_sqr = r * r`` with the product in double."""
    return float(np.float32(float(radius) * float(radius)))


class HipOps:
    """The point operations on the GPU in one call (``mrgfe_keyframe_callback``, or ``mrgfe_keyframe_callback_device`` for a cloud that is already in
    HBM): the kept cloud becomes keyframe ``key`` of ``store``."""

    def __init__(self, store):
        self.store = store

    def keyframe(self, key, msg, centres_sensor, radius, want_removed, records: int = 0):
        return self.store.keyframe_callback(key, msg, centres_sensor, radius, want_kept=len(centres_sensor) > 0, want_removed=want_removed, records=records)

    def keyframe_device(self, key, dev_ptr, n, centres_sensor, radius, want_removed, records: int = 0):
        return self.store.keyframe_callback_device(key, dev_ptr, n, centres_sensor, radius, want_kept=len(centres_sensor) > 0, want_removed=want_removed, records=records)


@dataclasses.dataclass
class KeyframeResult:
    """What ``cloud_callback`` hands to ``add_odom_keyframe`` (:446) and publishes (:437-443)."""
    key: int
    accum_distance: float
    odom: np.ndarray
    kept: np.ndarray | None     # the keyframe's cloud; None: no other robot, the message's own cloud is the keyframe's (:373,396)
    removed: np.ndarray | None  # the points that hit other robots; None unless asked for (get_subscription_count() > 0, :437)
    # (with ``records`` both are the ``data`` of the messages of :432-443 instead: uint8 records written on the device)
    centres_sensor: np.ndarray = None


class KeyframeCallback:
    def __init__(self, params: dict | None = None, ops=None, store=None, updater: KeyframeUpdater | None = None):
        self.p = dict(DEFAULTS)
        self.p.update(params or {})
        if ops is None:
            if store is None:
                raise ValueError("give the point operations (ops=) or the MapCloudStore the keyframes go into (store=)")
            ops = HipOps(store)
        self.ops = ops
        self.updater = updater or KeyframeUpdater(self.p["keyframe_delta_trans"], self.p["keyframe_delta_angle"])
        self.trans_odom2map = np.eye(4)  # trans_odom2map_ (set by the optimisation), :379-384
        self.others_odom_poses: dict = {}  # robot name -> position x, y, z in the map frame (others_odom_poses_), :386-393
        self.next_key = 1

    def _keyframe(self, odom, key, removed_points_wanted, point_work, records: int = 0):
        """:358-447 around the point work: ``point_work(key, centres, radius, want_removed)`` returns ``(kept, removed)``."""
        odom = np.array(odom, dtype=np.float64)
        update_required = self.updater.update(odom)  # :367
        accum_d = self.updater.get_accum_distance()
        if not update_required:
            return None
        # :380-384, trans_odom2map_.isApprox(Identity): [UPSTREAM-RECALL] Eigen 3.3 Core/Fuzzy.h on the 4 x 4 matrices,
        # |a - b|^2 <= prec^2 * min(|a|^2, |b|^2) with prec = NumTraits<double>::dummy_precision() = 1e-12
        m = np.asarray(self.trans_odom2map, dtype=np.float64)
        if float(np.sum((m - np.eye(4)) ** 2)) <= 1e-24 * min(float(np.sum(m * m)), 4.0):
            map2odom = np.eye(4)
        else:
            map2odom = isometry_inverse(self.trans_odom2map)
        others = [np.asarray(p, dtype=np.float64).reshape(3) for p in self.others_odom_poses.values()]
        centres = others_positions_sensor(odom, map2odom, others) if others else np.zeros((0, 3), dtype=np.float32)  # :396-404
        if key is None:
            key, self.next_key = self.next_key, self.next_key + 1
        kept, removed = point_work(key, centres, self.p["robot_remove_points_radius"], bool(removed_points_wanted))
        if not len(centres):
            kept = None
            if removed_points_wanted and removed is None:
                removed = np.empty(0, dtype=np.uint8) if records else np.empty((0, 4), dtype=np.float32)  # removed_cloud stays empty, :395
        return KeyframeResult(key, accum_d, odom, kept, removed if removed_points_wanted else None, centres)

    def cloud_callback(self, odom, msg, key: int | None = None, removed_points_wanted: bool = False, records: int = 0):
        """:358-447.  Returns a :class:`KeyframeResult`, or None when the pose starts no keyframe.  ``records`` 32 or 16 (default 0: off; needs ops that
        take it, :class:`HipOps`): ``kept`` and ``removed`` come back as the ``data`` of ``cloud_msg_filtered`` and ``other_robots_removed_points``
        (:432-443), written on the device (``mrgfe_keyframe_callback_records``)."""
        if records:
            return self._keyframe(odom, key, removed_points_wanted, lambda k, centres, radius, want_removed: self.ops.keyframe(k, msg, centres, radius, want_removed, records),
                                  records)
        return self._keyframe(odom, key, removed_points_wanted, lambda k, centres, radius, want_removed: self.ops.keyframe(k, msg, centres, radius, want_removed))

    def cloud_callback_device(self, odom, dev_ptr: int, n: int, key: int | None = None, removed_points_wanted: bool = False, records: int = 0):
        """The same callback — the same :class:`KeyframeUpdater` decision, the same centres — for a filtered scan that is already in HBM (all
        components in one container): ``n`` packed float4 points at ``dev_ptr`` on the store's device (``ops.keyframe_device``)."""
        if records:
            return self._keyframe(odom, key, removed_points_wanted,
                                  lambda k, centres, radius, want_removed: self.ops.keyframe_device(k, dev_ptr, n, centres, radius, want_removed, records), records)
        return self._keyframe(odom, key, removed_points_wanted, lambda k, centres, radius, want_removed: self.ops.keyframe_device(k, dev_ptr, n, centres, radius, want_removed))


__all__ = ["DEFAULTS", "KeyframeUpdater", "KeyframeCallback", "KeyframeResult", "HipOps", "angle_axis_angle", "isometry_inverse", "others_positions_sensor", "robot_radius_sqr"]
