"""Host mirror of ``PrefilteringComponent`` (/root/reference/apps/prefiltering_component.cpp:114-292): the caller of the prefilter rows of
the hot path — ``cloud_callback`` = ``deskewing`` (:231-292, with the IMU queue of ``imu_callback`` :114) -> transform into
``base_link_frame`` (:126-146, ``pcl_ros::transformPointCloud``) -> ``distance_filter`` (:207-229) -> ``downsample`` (:151-174) ->
``outlier_removal`` (:176-205).  ``ops`` supplies the point operations: by default the HIP path (``mrg_slam_amd``), for the parity tests the
CPU oracle — the SAME control flow runs over both.

What the ROS side does around it (``pcl::fromROSMsg`` / ``toROSMsg``, tf lookup, publishers) stays with the caller: ``cloud_callback``
takes the cloud as an ``[n, 4]`` float array (``mrg_slam_amd.io.ingest_pointcloud2`` makes one from a PointCloud2 payload on the GPU) and
``lookup_transform(base_link_frame, frame_id)`` stands for ``tf_buffer_->lookupTransform`` (returns a 4 x 4 matrix, or raises)."""
from __future__ import annotations

import numpy as np

DEFAULTS = {  # config/mrg_slam.yaml:43-68 (the component's declare_parameter defaults differ: STATISTICAL 20 / 1.0, radius 0.8, near 1.0; :98-111)
    "base_link_frame": "base_link",
    "downsample_method": "VOXELGRID",
    "downsample_resolution": 0.1,
    "downsample_min_points_per_voxel": 1,
    "outlier_removal_method": "RADIUS",
    "statistical_mean_k": 30,
    "statistical_stddev": 1.2,
    "radius_radius": 0.5,
    "radius_min_neighbors": 2,
    "enable_distance_filter": True,
    "distance_near_thresh": 0.1,
    "distance_far_thresh": 35.0,
    "enable_deskewing": False,
    "scan_period": 0.1,
}


class HipOps:
    """The point operations on the GPU (``libmrgfe``).  ``scan`` is the whole callback in one call (``mrgfe_scan_callback``: one upload, one
    kernel for deskewing + transform + the distance test, one download); ``deskew`` / ``transform`` / ``filters`` are the same steps as
    separate calls, the three filters through one fused call."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def scan(self, cloud, ang_v, scan_period, T, p, dev_ptr: int = 0):
        """deskew (``ang_v`` None: not) -> transform (``T`` None: not) -> filters of a packed [n, 4] cloud; with ``dev_ptr`` (room for n points)
        the result stays on the device and the count is returned."""
        return self.scan_pointcloud2(memoryview(cloud).cast("B"), len(cloud), 1, 16, {"x": 0, "y": 4, "z": 8, "intensity": 12}, 0, ang_v, scan_period, T, p, dev_ptr)

    def scan_pointcloud2(self, data, width, height, point_step, fields, row_step, ang_v, scan_period, T, p, dev_ptr: int = 0, records: int = 0, records_out=None,
                         colored: bool = False, colored_out=None):
        """``records`` 32 or 16 (default 0: off): the filtered scan as the message the component publishes (``mrgfe_scan_callback_records``, the
        ``pcl::toROSMsg`` + publish of :152-155) — a dict with the message's ``data`` (uint8; a view of ``records_out`` when given), ``point_step``, ``fields``
        (name -> offset), ``width``, ``height`` 1, ``row_step``, ``is_dense`` False, ``is_bigendian`` False; with ``dev_ptr`` the packed scan stays on the
        device as well.
        ``colored`` (needs ``records`` or ``dev_ptr``): the call also makes ``prefiltering/colored_points`` (:239-257, ``mrgfe_scan_callback_outputs``) and
        returns ``(result, colored message)``: ``width`` / ``height`` the input's, ``point_step`` 32, ``fields`` x y z rgb, ``data`` the raw scan's coloured
        records (a view of ``colored_out`` when given)."""
        from .filters import COLORED_FIELDS, RECORD_FIELDS, scan_callback, scan_callback_outputs, scan_callback_records, scan_callback_to_device

        if colored:
            if not (records or dev_ptr):
                raise ValueError("colored: with records or dev_ptr")
            rec, col, m = scan_callback_outputs(data, width, height, point_step, fields, records or 32, records_out, colored_out, dev_ptr, row_step, ang_v, scan_period, T, p,
                                             records=bool(records), ctx=self.ctx)
            cmsg = {"height": int(height), "width": int(width), "is_dense": False, "is_bigendian": False, "point_step": 32, "row_step": 32 * int(width),
                    "fields": dict(COLORED_FIELDS), "data": col}
            if not records:
                return m, cmsg
            return {"height": 1, "width": len(rec) // records, "is_dense": False, "is_bigendian": False, "point_step": records, "row_step": len(rec),
                    "fields": dict(RECORD_FIELDS[records]), "data": rec}, cmsg
        if records:
            rec = scan_callback_records(data, width, height, point_step, fields, records, records_out, dev_ptr, row_step, ang_v, scan_period, T, p, ctx=self.ctx)
            return {"height": 1, "width": len(rec) // records, "is_dense": False, "is_bigendian": False, "point_step": records, "row_step": len(rec),
                    "fields": dict(RECORD_FIELDS[records]), "data": rec}
        if dev_ptr:
            return scan_callback_to_device(data, width, height, point_step, fields, dev_ptr, int(width) * int(height), row_step, ang_v, scan_period, T, p, ctx=self.ctx)
        return scan_callback(data, width, height, point_step, fields, row_step, ang_v, scan_period, T, p, ctx=self.ctx)

    def deskew(self, cloud, ang_v, scan_period):
        from .map_cloud import deskew

        return deskew(cloud, ang_v, scan_period, ctx=self.ctx)

    def transform(self, cloud, T):
        from .map_cloud import transform_cloud

        return transform_cloud(cloud, T, ctx=self.ctx)

    def filters(self, cloud, p):
        from .filters import prefilter

        return prefilter(cloud, p, ctx=self.ctx)


class OracleOps:
    """The same operations by the CPU oracle, one after the other as the reference calls them (tests only)."""

    def __init__(self, orc):
        self.orc = orc

    def deskew(self, cloud, ang_v, scan_period):
        return self.orc.deskew(cloud, ang_v, scan_period)

    def transform(self, cloud, T):
        return self.orc.transform_points(np.asarray(T, dtype=np.float32), cloud)

    def filters(self, cloud, p):
        c = cloud
        if p["enable_distance_filter"]:
            c = self.orc.distance_filter(c, p["distance_near_thresh"], p["distance_far_thresh"])
        if p["downsample_method"] == "VOXELGRID":
            c = self.orc.voxelgrid(c, p["downsample_resolution"], p["downsample_min_points_per_voxel"])[0]
        elif p["downsample_method"] == "APPROX_VOXELGRID":
            c = self.orc.approx_voxelgrid(c, p["downsample_resolution"])
        if p["outlier_removal_method"] == "RADIUS":
            c = self.orc.radius_outlier(c, p["radius_radius"], p["radius_min_neighbors"])[0]
        elif p["outlier_removal_method"] == "STATISTICAL":
            c = self.orc.statistical_outlier(c, p["statistical_mean_k"], p["statistical_stddev"])[0]
        return c


class PrefilteringComponent:
    def __init__(self, params: dict | None = None, ops=None, lookup_transform=None, statistical_chains: bool = False, wide_statistical_chains: bool = False):
        """``statistical_chains``: switch the ops' context to serve ``outlier_removal_method: STATISTICAL`` behind ``downsample_method`` NONE /
        APPROX_VOXELGRID with one device wait (``Context.set_statistical_chains``; same output).  ``wide_statistical_chains``: the same for
        ``statistical_mean_k`` 64..255 wherever 1..63 is served that way (``Context.set_wide_statistical_chains``; same output).  Ops that hold no context
        (default: the shared one) get one of their own, so the shared context stays as it is; on ops without a context (the oracle's) the options do nothing."""
        self.p = dict(DEFAULTS)
        self.p.update(params or {})
        if self.p["downsample_method"] not in ("VOXELGRID", "APPROX_VOXELGRID", "NONE"):
            raise ValueError(f"unknown downsample_method {self.p['downsample_method']!r}")
        if self.p["outlier_removal_method"] not in ("RADIUS", "STATISTICAL", "NONE"):
            raise ValueError(f"unknown outlier_removal_method {self.p['outlier_removal_method']!r}")
        self.ops = ops or HipOps()
        if (statistical_chains or wide_statistical_chains) and hasattr(self.ops, "ctx"):
            if self.ops.ctx is None:
                from ._lib import Context

                self.ops.ctx = Context()
            if statistical_chains:
                self.ops.ctx.set_statistical_chains(True)
            if wide_statistical_chains:
                self.ops.ctx.set_wide_statistical_chains(True)
        self.lookup_transform = lookup_transform
        self.imu_queue: list[tuple[float, np.ndarray]] = []  # (stamp, angular velocity): imu_queue_

    def imu_callback(self, stamp: float, angular_velocity) -> None:
        """:114 — the subscription exists only with enable_deskewing (:61-64)."""
        if self.p["enable_deskewing"]:
            self.imu_queue.append((float(stamp), np.asarray(angular_velocity, dtype=np.float32).reshape(3)))

    def _take_imu(self, stamp: float):
        """The angular velocity ``deskewing`` uses for a scan stamped ``stamp`` (:234-270), or None when the queue is empty (the cloud is not
        deskewed).  The IMU message used is the first one newer than the scan, or the last one of the queue when none is; everything before it
        leaves the queue (:262-270)."""
        if not self.imu_queue:
            return None
        loc = 0
        ang_v = self.imu_queue[0][1]
        while loc < len(self.imu_queue):
            ang_v = self.imu_queue[loc][1]
            if self.imu_queue[loc][0] > stamp:
                break
            loc += 1
        del self.imu_queue[:loc]
        return ang_v

    def deskewing(self, cloud: np.ndarray, stamp: float) -> np.ndarray:
        """:231-292."""
        ang_v = self._take_imu(stamp)
        return cloud if ang_v is None else self.ops.deskew(cloud, ang_v, self.p["scan_period"])

    def _lookup(self, frame_id: str):
        """(ok, T): the transform into base_link_frame (:126-146) — T None when there is none to apply, ok False where the reference warns and
        returns early (tf2::TransformException, :133-138)."""
        if not (self.p["base_link_frame"] and self.lookup_transform is not None):
            return True, None
        try:
            return True, self.lookup_transform(self.p["base_link_frame"], frame_id)
        except Exception:  # noqa: BLE001
            return False, None

    def cloud_callback(self, cloud, stamp: float = 0.0, frame_id: str = ""):
        """:116-149.  Returns the filtered cloud (what ``points_pub_`` publishes), or None where the reference returns early (empty input,
        no transform into base_link_frame)."""
        src = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32).reshape(-1, 4))
        if len(src) == 0:
            return None
        if hasattr(self.ops, "scan"):  # the point operations of the whole callback in one call; the control flow around them is the same
            ang_v = self._take_imu(stamp)
            ok, T = self._lookup(frame_id)
            return self.ops.scan(src, ang_v, self.p["scan_period"], T, self.p) if ok else None
        src = self.deskewing(src, stamp)
        ok, T = self._lookup(frame_id)
        if not ok:
            return None
        if T is not None:
            src = self.ops.transform(src, T)
        return self.ops.filters(src, self.p)

    def pointcloud2_callback(self, data, width: int, height: int, point_step: int, fields, row_step: int = 0, stamp: float = 0.0, frame_id: str = "",
                             dev_ptr: int = 0, records: int = 0, records_out=None, colored: bool = False, colored_out=None):
        """``cloud_callback`` from the wire message (the payload and layout of a sensor_msgs/PointCloud2): pcl::fromROSMsg happens in the same
        GPU call as the rest.  ``fields``: a ``{name: offset}`` dict or the message's field list ``(name, offset, datatype, count)``, as
        ``io.layout_from_fields`` takes them (the list switches the context to byte layouts when the records need it: Velodyne's 22-byte points).  Returns the filtered cloud, or — with ``dev_ptr`` (device memory for width * height packed points) — leaves it
        there and returns its point count; None where the reference returns early.  Needs point operations with ``scan_pointcloud2`` (HipOps).
        ``records`` 32 or 16 (default 0: off): the callback to its publish (:152-155) — returns the filtered message (``HipOps.scan_pointcloud2``: its
        ``data``, ``point_step`` and ``fields``; ``records_out``: the caller's, ideally page-locked, buffer) and, with ``dev_ptr``, leaves the device cloud too.
        ``colored`` (a subscriber on ``prefiltering/colored_points``; with ``records`` or ``dev_ptr``): returns ``(result, colored message)`` — the second the
        message of :239-257 from the same GPU call (``HipOps.scan_pointcloud2``), or None when the IMU queue was empty: the reference returns from
        ``deskewing`` before it colours (:234-236)."""
        if int(width) * int(height) == 0:
            return None
        ang_v = self._take_imu(stamp)
        ok, T = self._lookup(frame_id)
        if not ok:
            return None
        if colored:
            if ang_v is None:
                return self.ops.scan_pointcloud2(data, width, height, point_step, fields, row_step, ang_v, self.p["scan_period"], T, self.p, dev_ptr, records, records_out), None
            return self.ops.scan_pointcloud2(data, width, height, point_step, fields, row_step, ang_v, self.p["scan_period"], T, self.p, dev_ptr, records, records_out, True,
                                             colored_out)
        if records:
            return self.ops.scan_pointcloud2(data, width, height, point_step, fields, row_step, ang_v, self.p["scan_period"], T, self.p, dev_ptr, records, records_out)
        return self.ops.scan_pointcloud2(data, width, height, point_step, fields, row_step, ang_v, self.p["scan_period"], T, self.p, dev_ptr)
