"""Floor detection on the GPU: ``FloorDetectionComponent::detect`` (the reference's apps/floor_detection_component.cpp:100-183) — tilt compensation,
the height band, the k = 10 normal filter and the RANSAC plane fit — through ``mrgfe_floor_detect`` (csrc/floor.hip), on a host cloud, on a packed
cloud in device memory or, in one call, on the bytes of the sensor_msgs/PointCloud2 (``mrgfe_floor_callback``), and a host mirror of the
component's ``cloud_callback`` (:69-95).

Parameter names and defaults are the component's (:55-62) and config/mrg_slam.yaml:113-122.  The reference declares ``enable_normal_filtering``
(:61) but reads ``use_normal_filtering`` (:120); here both names set the one switch."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import Context, check, default_context, lib

_fp = C.POINTER(C.c_float)

DEFAULTS = {"tilt_deg": 0.0, "sensor_height": 2.0, "height_clip_range": 1.0, "floor_pts_thresh": 512, "floor_normal_thresh_deg": 10.0,
            "use_normal_filtering": True, "normal_filter_thresh_deg": 20.0}


def _params(p: dict) -> _lib.FloorParams:
    q = _lib.FloorParams()
    lib().mrgfe_floor_default_params(C.byref(q))
    q.tilt_deg, q.sensor_height, q.height_clip_range = float(p["tilt_deg"]), float(p["sensor_height"]), float(p["height_clip_range"])
    q.floor_pts_thresh = int(p["floor_pts_thresh"])
    q.floor_normal_thresh_deg = float(p["floor_normal_thresh_deg"])
    q.use_normal_filtering = int(bool(p["use_normal_filtering"]))
    q.normal_filter_thresh_deg = float(p["normal_filter_thresh_deg"])
    return q


def _merge(params: dict | None) -> dict:
    p = dict(DEFAULTS)
    params = dict(params or {})
    if "enable_normal_filtering" in params:  # the declared name (:61)
        params.setdefault("use_normal_filtering", params.pop("enable_normal_filtering"))
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"unknown floor detection parameters {sorted(unknown)}")
    p.update(params)
    return p


@dataclass
class FloorRecord:
    """``mrgfe_floor_result`` with the two published clouds."""

    found: bool
    reason: str
    coeffs: np.ndarray | None  # float32 [4] when found
    n_clipped: int
    n_filtered: int
    n_inliers: int
    iterations: int
    skipped: int
    filtered: np.ndarray | None = None  # floor_filtered_points [n_filtered, 4]
    inliers: np.ndarray | None = None   # floor_points [n_inliers, 4] (found only)


def _record(r: _lib.FloorResult, filt, inl) -> FloorRecord:
    found = bool(r.found)
    return FloorRecord(found, _lib.FLOOR_REASONS[r.reason], np.array(r.coeffs, dtype=np.float32) if found else None, r.n_clipped, r.n_filtered, r.n_inliers,
                       r.iterations, r.skipped, None if filt is None else filt[: r.n_filtered].copy(),
                       None if inl is None or not found else inl[: r.n_inliers].copy())


class FloorDetection:
    """``detect()`` on the GPU.  ``detect(cloud)`` returns the plane (float32 a, b, c, d, normal up) or None, like the reference's
    ``boost::optional<Eigen::Vector4f>``; ``last`` holds the :class:`FloorRecord` of the call (reason, stage counts, RANSAC iterations, clouds)."""

    def __init__(self, ctx: Context | None = None, **params):
        self.p = _merge(params)
        self.ctx = ctx
        self.last: FloorRecord | None = None

    def detect(self, cloud, want_clouds: bool = True):
        ctx = self.ctx or default_context()
        c = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 4))
        q, r = _params(self.p), _lib.FloorResult()
        filt = np.empty((max(len(c), 1), 4), dtype=np.float32) if want_clouds else None
        inl = np.empty((max(len(c), 1), 4), dtype=np.float32) if want_clouds else None
        check(lib().mrgfe_floor_detect(ctx._h, C.byref(q), c.ctypes.data_as(_fp), len(c), 16, C.byref(r), None if filt is None else filt.ctypes.data_as(_fp),
                                       None if inl is None else inl.ctypes.data_as(_fp)))
        self.last = _record(r, filt, inl)
        return self.last.coeffs

    def detect_device(self, dev_ptr: int, n: int, want_clouds: bool = True):
        """The same on a packed float4 cloud in device memory (``mrgfe_prefilter_device``'s output)."""
        ctx = self.ctx or default_context()
        q, r = _params(self.p), _lib.FloorResult()
        filt = np.empty((max(n, 1), 4), dtype=np.float32) if want_clouds else None
        inl = np.empty((max(n, 1), 4), dtype=np.float32) if want_clouds else None
        check(lib().mrgfe_floor_detect_device(ctx._h, C.byref(q), C.c_void_p(dev_ptr), int(n), C.byref(r), None if filt is None else filt.ctypes.data_as(_fp),
                                              None if inl is None else inl.ctypes.data_as(_fp)))
        self.last = _record(r, filt, inl)
        return self.last.coeffs

    def detect_pointcloud2(self, data, width: int, height: int, point_step: int, fields, row_step: int = 0, want_clouds: bool = True):
        """``cloud_callback`` (:69-93) on the bytes of the sensor_msgs/PointCloud2 in one call (``mrgfe_floor_callback``): the payload goes up once and
        the first kernel reads the records.  ``fields``: as ``io.layout_from_fields`` takes them (a field list whose layout needs it switches the
        context to byte layouts).  Same plane, record and clouds as ``io.ingest_pointcloud2`` followed by :meth:`detect_device`; an empty message
        gives None with ``last.reason == "empty_input"``."""
        from .io import layout_from_fields, pointcloud2_payload

        ctx = self.ctx or default_context()
        buf = pointcloud2_payload(data, width, height, point_step, row_step)
        lay, _ = layout_from_fields(fields, width, height, point_step, row_step, ctx=ctx)
        n = int(width) * int(height)
        q, r = _params(self.p), _lib.FloorResult()
        filt = np.empty((max(n, 1), 4), dtype=np.float32) if want_clouds else None
        inl = np.empty((max(n, 1), 4), dtype=np.float32) if want_clouds else None
        check(lib().mrgfe_floor_callback(ctx._h, C.byref(q), C.byref(lay), buf.ctypes.data_as(C.c_void_p) if buf.nbytes else None, buf.nbytes, C.byref(r),
                                         None if filt is None else filt.ctypes.data_as(_fp), None if inl is None else inl.ctypes.data_as(_fp)))
        self.last = _record(r, filt, inl)
        return self.last.coeffs

    def stage_times(self) -> dict:
        """HIP-event milliseconds of the stages of the last detection on the context, its host waits and RANSAC waves (``mrgfe_dbg_floor_stats``)."""
        ctx = self.ctx or default_context()
        v = (C.c_double * 8)()
        check(lib().mrgfe_dbg_floor_stats(ctx._h, v))
        return dict(zip(("band_ms", "normals_ms", "ransac_ms", "inliers_ms", "host_waits", "ransac_waves", "hypotheses"), [float(x) for x in v]))


def floor_ransac(cloud, threshold: float = 0.1, ctx: Context | None = None) -> dict:
    """Diagnostic (``mrgfe_dbg_floor_ransac``): RandomSampleConsensus<SampleConsensusModelPlane> alone."""
    ctx = ctx or default_context()
    c = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 4))
    has, coeffs, inl = C.c_int(0), (C.c_float * 4)(), np.empty(max(len(c), 1), dtype=np.int32)
    m, it, sk = C.c_size_t(0), C.c_int32(0), C.c_int32(0)
    check(lib().mrgfe_dbg_floor_ransac(ctx._h, c.ctypes.data_as(_fp), len(c), 16, float(threshold), C.byref(has), coeffs, inl.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.byref(m), C.byref(it), C.byref(sk)))
    return {"has_model": bool(has.value), "coeffs": np.array(coeffs, dtype=np.float32) if has.value else None, "inliers": inl[: m.value].copy(),
            "iterations": it.value, "skipped": sk.value}


def floor_normals(cloud, normal_filter_thresh_deg: float = 20.0, ctx: Context | None = None):
    """Diagnostic (``mrgfe_dbg_floor_normals``): the k = 10 normals [n, 3] (NaN with fewer than three neighbours) and the keep flags [n]."""
    ctx = ctx or default_context()
    c = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 4))
    nr, keep = np.empty((max(len(c), 1), 3), dtype=np.float32), np.empty(max(len(c), 1), dtype=np.uint8)
    check(lib().mrgfe_dbg_floor_normals(ctx._h, c.ctypes.data_as(_fp), len(c), 16, float(normal_filter_thresh_deg), nr.ctypes.data_as(_fp),
                                        keep.ctypes.data_as(C.POINTER(C.c_uint8))))
    return nr[: len(c)].copy(), keep[: len(c)].astype(bool)


class HipOps:
    """``detect`` on the GPU (``libmrgfe``)."""

    def __init__(self, ctx: Context | None = None):
        self.ctx = ctx

    def detect(self, cloud, p: dict):
        fd = FloorDetection(ctx=self.ctx, **p)
        return fd.detect(cloud, want_clouds=False)

    def detect_pointcloud2(self, msg: dict, p: dict):
        """The message's bytes in one call (``mrgfe_floor_callback``)."""
        fd = FloorDetection(ctx=self.ctx, **p)
        return fd.detect_pointcloud2(msg["data"], msg["width"], msg.get("height", 1), msg["point_step"], msg["fields"], int(msg.get("row_step", 0) or 0), want_clouds=False)


class FloorDetectionComponent:
    """Host mirror of ``FloorDetectionComponent::cloud_callback`` (:69-95).  ``ops.detect(cloud, params)`` supplies ``detect()``: by default the HIP
    path; the parity tests pass a CPU restatement — the SAME control flow runs over both.  Returns the ``FloorCoeffs`` message's ``coeffs`` (a list
    of four floats, empty when no floor was found), or None where the reference returns without publishing (empty cloud, :74-77)."""

    def __init__(self, params: dict | None = None, ops=None):
        self.p = _merge(params)
        self.ops = ops or HipOps()

    def cloud_callback(self, cloud):
        c = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 4))
        if len(c) == 0:
            return None
        floor = self.ops.detect(c, self.p)
        return [] if floor is None else [float(v) for v in np.asarray(floor, dtype=np.float32)]

    def pointcloud2_callback(self, msg: dict):
        """The same callback on the sensor_msgs/PointCloud2 itself — a dict with ``data``, ``width``, ``height``, ``point_step``, ``fields`` and
        optionally ``row_step``: ``ops.detect_pointcloud2(msg, params)`` gets its bytes in one call (``pcl::fromROSMsg``, :72, runs on the device)."""
        if int(msg["width"]) * int(msg.get("height", 1)) == 0:  # :74-77
            return None
        floor = self.ops.detect_pointcloud2(msg, self.p)
        return [] if floor is None else [float(v) for v in np.asarray(floor, dtype=np.float32)]
