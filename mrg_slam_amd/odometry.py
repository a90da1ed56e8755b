"""Host mirror of ``ScanMatchingOdometryComponent::matching`` (/root/reference/apps/scan_matching_odometry_component.cpp:195-350): the
caller of the hot path in the odometry component — first frame becomes the keyframe (``setInputTarget``), every later frame is
``setInputSource`` + ``align(prev_trans * msf_delta)`` against it, the keyframe is replaced when the motion since it exceeds
``keyframe_delta_translation`` / ``keyframe_delta_angle`` / ``keyframe_delta_time`` (:326-339), optional transform thresholding with
``max_consecutive_rejections`` (:278-318).  ``registration`` is anything with the ``pcl::Registration`` call surface the reference uses
(``setInputTarget`` / ``setInputSource`` / ``align(guess)`` / ``hasConverged`` / ``getFinalTransformation``): a HIP registration
(``mrg_slam_amd.registration``) or the CPU oracle's classes — the parity tests run the SAME loop over both.

Arithmetic as in the reference: poses are float 4 x 4 matrices (``Eigen::Matrix4f``), products in float; the rotation angle is
``acos(Quaternionf(R).w())`` (Eigen's matrix -> quaternion conversion, restated in ``quat_w``)."""
from __future__ import annotations

import numpy as np

DEFAULTS = {  # config/mrg_slam.yaml:77-86 (the component's own declare_parameter defaults differ: 0.25 / 0.15 / 1.0, :103-105)
    "keyframe_delta_translation": 1.0,
    "keyframe_delta_angle": 0.5236,
    "keyframe_delta_time": 10000.0,
    "enable_transform_thresholding": False,
    "max_acceptable_translation": 1.0,
    "max_acceptable_angle": 1.0,
    "max_consecutive_rejections": 5,
}


def quat_w(R) -> np.float32:
    """w of Eigen::Quaternionf(R) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl for a 3 x 3 matrix), in float."""
    R = np.asarray(R, dtype=np.float32)
    t = np.float32(R[0, 0] + R[1, 1] + R[2, 2])
    if t > np.float32(0):
        return np.float32(0.5) * np.sqrt(t + np.float32(1.0), dtype=np.float32)
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    tt = np.sqrt(np.float32(R[i, i] - R[j, j] - R[k, k] + np.float32(1.0)), dtype=np.float32)
    return np.float32((R[k, j] - R[j, k]) * (np.float32(0.5) / tt))


def rotation_angle(T) -> float:
    """``std::acos(Eigen::Quaternionf(T.block<3,3>(0,0)).w())`` (:281,327), promoted to double like the reference's ``double da``."""
    w = float(quat_w(np.asarray(T)[:3, :3]))
    return float(np.arccos(np.float32(min(1.0, max(-1.0, w)))))


class ScanMatchingOdometry:
    """State and decisions of ``ScanMatchingOdometryComponent::matching``; ``downsample`` is the component's own downsample step
    (default NONE, config/mrg_slam.yaml:95: the cloud passes through)."""

    def __init__(self, registration, params: dict | None = None, downsample=None, set_target=None, set_source=None):
        """``set_target`` / ``set_source`` override how a cloud is handed to the registration (e.g. device-resident clouds through
        ``setInputTargetDevice``); by default ``registration.setInputTarget(cloud)`` / ``setInputSource(cloud)``."""
        self.reg = registration
        self.p = dict(DEFAULTS)
        self.p.update(params or {})
        self._downsample = downsample or (lambda c: c)
        self._promote = set_target is None and set_source is None and hasattr(registration, "sourceBecomesTarget") and self.p.get("promote_source_to_keyframe", True)
        self._set_target = set_target or (lambda c: registration.setInputTarget(c))
        self._set_source = set_source or (lambda c: registration.setInputSource(c))
        self.keyframe_cloud = None
        self.keyframe_pose = np.eye(4, dtype=np.float32)
        self.keyframe_stamp = 0.0
        self.prev_time = None
        self.prev_trans = np.eye(4, dtype=np.float32)
        self.consecutive_rejections = 0
        self.keyframes = 0  # how many times a cloud became the keyframe
        self.last_converged = True

    def status(self, msf_delta=None, max_correspondence_dist: float = 0.5):
        """``publish_scan_matching_status`` (:391-431) for the last ``matching()`` frame through the registration's ``matchingStatus`` (one device pass);
        ``msf_delta`` is the prediction that frame was given.  The component publishes right after ``align`` (:268), before the keyframe decision; this reads
        the registration as ``matching()`` left it, so for a frame that became the keyframe (``keyframes`` grew) the matching error and the inliers are
        taken against the new keyframe.  The registration raises when no source has been set yet."""
        if not hasattr(self.reg, "matchingStatus"):
            raise NotImplementedError("the registration has no matchingStatus()")
        return self.reg.matchingStatus(max_correspondence_dist, None if msf_delta is None else np.asarray(msf_delta, dtype=np.float32))

    def matching(self, stamp: float, cloud, msf_delta=None) -> np.ndarray:
        """Returns the odometry pose (float 4 x 4) of this frame."""
        if self.keyframe_cloud is None:  # :197-205
            self.prev_time = None
            self.prev_trans = np.eye(4, dtype=np.float32)
            self.keyframe_pose = np.eye(4, dtype=np.float32)
            self.keyframe_stamp = stamp
            self.keyframe_cloud = self._downsample(cloud)
            self._set_target(self.keyframe_cloud)
            self.keyframes += 1
            return np.eye(4, dtype=np.float32)
        filtered = self._downsample(cloud)
        self._set_source(filtered)
        delta = np.eye(4, dtype=np.float32) if msf_delta is None else np.asarray(msf_delta, dtype=np.float32)
        self.reg.align((self.prev_trans @ delta).astype(np.float32))  # :265-266
        self.last_converged = bool(self.reg.hasConverged())
        if not self.last_converged:  # :270-273
            return (self.keyframe_pose @ self.prev_trans).astype(np.float32)
        trans = np.asarray(self.reg.getFinalTransformation(), dtype=np.float32)
        odom = (self.keyframe_pose @ trans).astype(np.float32)
        if self.p["enable_transform_thresholding"]:  # :278-318
            d = (np.linalg.inv(self.prev_trans).astype(np.float32) @ trans).astype(np.float32)
            dx = float(np.linalg.norm(d[:3, 3].astype(np.float32)))
            da = rotation_angle(d)
            if dx > self.p["max_acceptable_translation"] or da > self.p["max_acceptable_angle"]:
                self.consecutive_rejections += 1
                if self.consecutive_rejections >= self.p["max_consecutive_rejections"]:
                    self._new_keyframe(filtered, odom, stamp)
                    self.consecutive_rejections = 0
                    return self.keyframe_pose
                self.prev_time = stamp
                return (self.keyframe_pose @ self.prev_trans).astype(np.float32)
            self.consecutive_rejections = 0
        self.prev_time = stamp
        self.prev_trans = trans
        delta_translation = float(np.linalg.norm(trans[:3, 3]))
        delta_angle = rotation_angle(trans)
        delta_time = stamp - self.keyframe_stamp
        if (delta_translation > self.p["keyframe_delta_translation"] or delta_angle > self.p["keyframe_delta_angle"]
                or delta_time > self.p["keyframe_delta_time"]):  # :326-339
            self._new_keyframe(filtered, odom, stamp)
        return odom

    def _new_keyframe(self, filtered, odom, stamp):
        # (`filtered` is the cloud that has just been aligned as the source, :208 -> :333: a HIP registration takes it over with what it computed for it)
        self.keyframe_cloud = filtered
        if self._promote:
            self.reg.sourceBecomesTarget()
        else:
            self._set_target(filtered)
        self.keyframe_pose = odom
        self.keyframe_stamp = stamp
        self.prev_time = stamp
        self.prev_trans = np.eye(4, dtype=np.float32)
        self.keyframes += 1


# ---- the same frame as ONE library call (include/mrgfe.h mrgfe_odom_frame): the state machine above lives in csrc/odom_ctl.h ----------------------
OUTCOMES = ("first_frame", "accepted", "not_converged", "rejected", "rejected_reset")  # enum mrgfe_odom_outcome
_DOWNSAMPLE = {"NONE": 0, "VOXELGRID": 1, "APPROX_VOXELGRID": 2}


class OdomFrame:
    """One ``mrgfe_odom_result``: matrices as row-major 4 x 4 float arrays, ``status`` a ``registration.MatchingStatus`` or None, ``aligned`` the whole
    input cloud moved by ``odom`` (N x 4) when it was asked for and the frame was accepted, else None; ``raw`` is the ctypes record itself."""

    def __init__(self, raw, aligned):
        from .registration import MatchingStatus

        self.raw = raw
        self.outcome = OUTCOMES[raw.outcome]
        self.new_keyframe = bool(raw.new_keyframe)
        self.consecutive_rejections = int(raw.consecutive_rejections)
        self.converged = bool(raw.converged)
        self.iterations = int(raw.iterations)
        self.n_source = int(raw.n_source)
        self.odom = np.array(raw.odom, dtype=np.float32).reshape(4, 4).T.copy()
        self.keyframe_pose = np.array(raw.keyframe_pose, dtype=np.float32).reshape(4, 4).T.copy()
        self.trans = np.array(raw.trans, dtype=np.float32).reshape(4, 4).T.copy()
        s = raw.status
        self.status = None
        if raw.has_status:
            self.status = MatchingStatus(bool(s.has_converged), int(s.n_points), int(s.num_inliers), np.float32(s.inlier_fraction), float(s.matching_error),
                                         np.array(s.relative_pose, dtype=np.float64), np.array(s.prediction_error, dtype=np.float64) if s.has_prediction else None)
        self.aligned = aligned


class HipOdometry:
    """``ScanMatchingOdometryComponent::cloud_callback`` -> ``matching()`` in one call per frame over a HIP registration (``mrgfe_odom_*``): the message's
    bytes go up once, the cloud becomes the keyframe (first frame) or the source, is aligned from ``prev_trans * msf_delta``, and the decisions of
    :270-339 are made by the library's controller.  ``params``: the keys of ``DEFAULTS`` plus ``downsample_method`` ("NONE" / "VOXELGRID" /
    "APPROX_VOXELGRID"), ``downsample_resolution``, ``downsample_min_points_per_voxel`` and ``status_max_correspondence_dist``.  The registration must
    outlive this object (it is kept referenced here)."""

    def __init__(self, registration, params: dict | None = None):
        import ctypes as C

        from . import _lib

        self.reg = registration
        p = _lib.OdomParams()
        _lib.lib().mrgfe_odom_default_params(C.byref(p))
        for k, v in (params or {}).items():
            if k == "downsample_method":
                v = _DOWNSAMPLE[v] if isinstance(v, str) else int(v)
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        self.params = p
        self._h = C.c_void_p()
        _lib.check(_lib.lib().mrgfe_odom_create(registration._h, C.byref(p), C.byref(self._h)))

    def close(self):
        from . import _lib

        if getattr(self, "_h", None):
            # the handle borrows the registration and its context: when the collector has finalised one of them first (members of a reference cycle are
            # finalised in no particular order) the library call would touch freed memory, so the handle is dropped unfreed instead
            reg = getattr(self, "reg", None)
            if reg is not None and getattr(reg, "_h", None) and getattr(getattr(reg, "_ctx", None), "_h", None):
                _lib.lib().mrgfe_odom_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _handle(self):
        from . import _lib

        if not getattr(self, "_h", None):
            raise _lib.MrgfeError(_lib.ERR_INVALID, "the odometry handle has been destroyed")
        return self._h

    def reset(self):
        """Forgets the keyframe: the next frame is a first frame."""
        from . import _lib

        _lib.check(_lib.lib().mrgfe_odom_reset(self._handle()))

    def stats(self) -> dict:
        """What the last completed frame's downsample did (``mrgfe_odom_stats``, no GPU work): ``route`` 0 none or host-driven, 1 device-driven (one wait),
        2 device-driven attempted and handed back; ``anomaly`` the stage's word (``_lib.PF_ANOMALY_*``); ``points_in``; ``points_out`` handed to the
        registration; ``boxed`` the source grid was built in a box the frame handed over; ``served`` frames served device-driven so far."""
        import ctypes as C

        from . import _lib

        v = (C.c_int64 * 6)()
        _lib.check(_lib.lib().mrgfe_odom_stats(self._handle(), v))
        return {"route": int(v[0]), "anomaly": int(v[1]), "points_in": int(v[2]), "points_out": int(v[3]), "boxed": bool(v[4]), "served": int(v[5])}

    def state(self):
        """The controller's state (``_lib.OdomState``: keyframe pose and stamp, prev_trans, the rejection counter)."""
        import ctypes as C

        from . import _lib

        s = _lib.OdomState()
        _lib.check(_lib.lib().mrgfe_dbg_odom_state_of(self._handle(), C.byref(s)))
        return s

    @staticmethod
    def _delta(msf_delta):
        import ctypes as C

        if msf_delta is None:
            return None, None
        d = np.ascontiguousarray(np.asarray(msf_delta, dtype=np.float32).T)
        return d, d.ctypes.data_as(C.POINTER(C.c_float))

    def frame(self, msg_or_cloud, stamp: float, msf_delta=None, want_status: bool = False, want_aligned: bool = False, aligned_records: int = 0,
              records_out=None) -> OdomFrame:
        """One frame from a PointCloud2 dict (``data``, ``width``, ``height``, ``point_step``, ``row_step``, ``fields``: name -> offset, or the
        message's field list as ``io.layout_from_fields`` takes it) or from an
        N x 4 float32 cloud (sent as the packed 16-byte message).
        ``aligned_records`` 32 or 16 (default 0: off): the frame to its publish (``mrgfe_odom_frame_records``, :341-347) — on an accepted frame
        ``OdomFrame.aligned`` is the ``data`` of ``scan_matching_odometry/aligned_points`` (uint8, ``n * aligned_records`` bytes, written on the device; a
        view of ``records_out`` when the caller gives its own, ideally page-locked, buffer), else None."""
        import ctypes as C

        from . import _lib

        h = self._handle()
        lay = _lib.KeyframeParams()
        if isinstance(msg_or_cloud, dict):
            m = msg_or_cloud
            from .io import layout_from_fields

            data = m["data"]
            row_step = int(m.get("row_step", 0) or 0)  # (a field list whose layout needs it switches the registration's context to byte layouts)
            lay, _ = layout_from_fields(m["fields"], m["width"], m["height"], m["point_step"], row_step, m.get("is_bigendian", False), ctx=getattr(self.reg, "_ctx", None))
            lay.row_step = row_step
        else:
            c = np.ascontiguousarray(msg_or_cloud, dtype=np.float32)
            if c.ndim != 2 or c.shape[1] != 4:
                raise ValueError("clouds are N x 4 float32 arrays (x, y, z, intensity)")
            data = c.tobytes()
            _lib.lib().mrgfe_keyframe_default_params(C.byref(lay))
            lay.width = len(c)
        n = lay.width * lay.height
        aligned = np.empty((n, 4), dtype=np.float32) if want_aligned else None
        keep, dptr = self._delta(msf_delta)
        out = _lib.OdomResult()
        buf = (C.c_char * len(data)).from_buffer_copy(data) if len(data) else None
        if aligned_records:
            from .filters import _records_destination

            rec, m = _records_destination(n, aligned_records, records_out), C.c_size_t(0)
            _lib.check(_lib.lib().mrgfe_odom_frame_records(h, C.byref(lay), C.cast(buf, C.c_void_p) if buf is not None else None, len(data), float(stamp), dptr,
                                                             int(bool(want_status)), int(aligned_records), rec.ctypes.data_as(C.c_void_p), rec.nbytes, C.byref(m), C.byref(out)))
            return OdomFrame(out, rec[: m.value * aligned_records] if out.outcome == _lib.ODOM_ACCEPTED else None)
        _lib.check(_lib.lib().mrgfe_odom_frame(h, C.byref(lay), C.cast(buf, C.c_void_p) if buf is not None else None, len(data), float(stamp), dptr, int(bool(want_status)),
                                                 None if aligned is None else aligned.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)))
        return OdomFrame(out, aligned if (aligned is not None and out.outcome == _lib.ODOM_ACCEPTED) else None)

    def frame_device(self, dev_ptr: int, n: int, stamp: float, msf_delta=None, want_status: bool = False, want_aligned: bool = False, aligned_records: int = 0,
                     records_out=None) -> OdomFrame:
        """One frame from a packed cloud of ``n`` points already in HBM at ``dev_ptr`` (the output of ``scan_callback_to_device`` / ``prefilter_to_device``
        on the registration's context); the buffer may be overwritten as soon as this returns.  ``aligned_records``: as :meth:`frame`
        (``mrgfe_odom_frame_records_device``)."""
        import ctypes as C

        from . import _lib

        h = self._handle()
        aligned = np.empty((int(n), 4), dtype=np.float32) if want_aligned else None
        keep, dptr = self._delta(msf_delta)
        out = _lib.OdomResult()
        if aligned_records:
            from .filters import _records_destination

            rec, m = _records_destination(int(n), aligned_records, records_out), C.c_size_t(0)
            _lib.check(_lib.lib().mrgfe_odom_frame_records_device(h, C.c_void_p(dev_ptr), int(n), float(stamp), dptr, int(bool(want_status)), int(aligned_records),
                                                                    rec.ctypes.data_as(C.c_void_p), rec.nbytes, C.byref(m), C.byref(out)))
            return OdomFrame(out, rec[: m.value * aligned_records] if out.outcome == _lib.ODOM_ACCEPTED else None)
        _lib.check(_lib.lib().mrgfe_odom_frame_device(h, C.c_void_p(dev_ptr), int(n), float(stamp), dptr, int(bool(want_status)),
                                                        None if aligned is None else aligned.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)))
        return OdomFrame(out, aligned if (aligned is not None and out.outcome == _lib.ODOM_ACCEPTED) else None)

    def source(self):
        """(cloud N x 4, box of 6 floats, finite count or None) of the last frame: ``mrgfe_dbg_odom_source``."""
        import ctypes as C

        from . import _lib

        n = C.c_size_t(0)
        box = np.zeros(6, dtype=np.float32)
        nf = C.c_uint32(0)
        fp = C.POINTER(C.c_float)
        _lib.check(_lib.lib().mrgfe_dbg_odom_source(self._handle(), None, C.byref(n), box.ctypes.data_as(fp), C.byref(nf)))
        cloud = np.empty((n.value, 4), dtype=np.float32)
        _lib.check(_lib.lib().mrgfe_dbg_odom_source(self._handle(), cloud.ctypes.data_as(fp), C.byref(n), box.ctypes.data_as(fp), C.byref(nf)))
        return cloud, box, (None if nf.value == 0xFFFFFFFF else int(nf.value))
