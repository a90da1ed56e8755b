"""Host-side mirror of the per-point passes around the scan-matching path, bound to
libmrgfe.so:

* :class:`MapCloudGenerator` — mrg_slam::MapCloudGenerator (/root/reference/src/mrg_slam/map_cloud_generator.cpp:14-86,
  called from apps/mrg_slam_component.cpp:727,781,1097) with its pcl::ApproximateMeanVoxelGrid pass;
* :func:`remove_points_near` — the other-robot point removal of apps/mrg_slam_component.cpp:396-429;
* :func:`deskew` — PrefilteringComponent::deskewing (apps/prefiltering_component.cpp:231-292);
* :meth:`MapCloudStore.publish` / :meth:`MapCloudStore.read` and :class:`MapPublisher` — the map as the message or file its three callers make of
  it (update_map_cloud_msg, publish_map_service, save_map_service: apps/mrg_slam_component.cpp:712-740, 764-796, 1078-1144) and stored keyframes
  read back as records (KeyFrame::save, the cloud_msg of publish_graph_service: src/mrg_slam/keyframe.cpp:109, 200);
* :func:`fill_ground_plane` and :meth:`MapCloudStore.fill_ground` — the ground fill of the first keyframe
  (src/mrg_slam/graph_database.cpp:114-129, src/pcl/fill_ground_plane.cpp).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from ._lib import (Context, GraphEdge, GroundFillParams, GroundFillResult, KeyframeMsg, KeyframeParams, MapPublishParams, MapPublishResult, MrgfeError, check, default_context,
                   lib)
from .filters import _cloud
from .io import pcd_binary_header, pointcloud2_from_xyzi

_fp = C.POINTER(C.c_float)
ERR_EMPTY = -4  # MRGFE_ERR_EMPTY (include/mrgfe.h)


@dataclass
class KeyFrameSnapshot:
    """The two members of mrg_slam::KeyFrameSnapshot the generator reads, plus the first_keyframe flag."""

    pose: np.ndarray  # 4 x 4, Eigen::Isometry3d
    cloud: np.ndarray  # N x 4 float32 (x, y, z, intensity)
    first_keyframe: bool = False


def keyframe_params(msg: dict, ctx: Context | None = None) -> KeyframeParams:
    """struct mrgfe_keyframe_params of a PointCloud2 given as a dict (``width``, ``height``, ``point_step``, ``fields``, optionally ``row_step``,
    ``is_bigendian``).  ``fields``: a ``{name: offset}`` dict or the message's field list, as ``io.layout_from_fields`` takes them; with ``ctx`` a
    field list whose layout needs it switches that context to byte layouts."""
    from .io import layout_from_fields

    row_step = int(msg.get("row_step", 0) or 0)
    p, _ = layout_from_fields(msg["fields"], msg["width"], msg.get("height", 1), msg["point_step"], row_step, msg.get("is_bigendian", False), ctx=ctx)
    p.row_step = row_step  # (0 stays 0: the call fills it in)
    return p


def _ground_fill_args(radius: float, map_resolution: float, simple: bool, estimate):
    """The parameter record, the column-major estimate (or None) and the two loop counts (``mrgfe_ground_fill_counts``: refuses what the library refuses)."""
    p = GroundFillParams(float(radius), float(map_resolution), int(bool(simple)), 0)
    est = None if estimate is None else np.ascontiguousarray(np.asarray(estimate, dtype=np.float64).reshape(4, 4).T)
    rings, angles = ground_fill_counts(radius, map_resolution)
    return p, est, rings * angles


def _ground_fill_info(r: GroundFillResult) -> dict:
    return {"has_model": bool(r.has_model), "ransac_iterations": int(r.ransac_iterations), "coeffs": np.array(r.coeffs[:], dtype=np.float32), "n_before": int(r.n_before),
            "n_rings": int(r.n_rings), "n_angles": int(r.n_angles), "n_added": int(r.n_added)}


def ground_fill_counts(radius: float, map_resolution: float):
    """``mrgfe_ground_fill_counts``: (rings, angles) of the disc, the accumulated loops of fill_cloud (src/pcl/fill_ground_plane.cpp:53-56); host only."""
    p = GroundFillParams(float(radius), float(map_resolution), 0, 0)
    rings, angles = C.c_uint32(0), C.c_uint32(0)
    check(lib().mrgfe_ground_fill_counts(C.byref(p), C.byref(rings), C.byref(angles)))
    return rings.value, angles.value


def fill_ground_plane(cloud, radius: float = 5.0, map_resolution: float = 0.05, simple: bool = False, estimate=None, ctx: Context | None = None, stride_bytes: int = 16):
    """``mrgfe_fill_ground_plane``: mrg_slam_pcl::fill_ground_plane_ransac / _simple (src/pcl/fill_ground_plane.cpp:21-47) on a host cloud.  ``estimate``:
    the 4 x 4 pose of the simple variant.  ``stride_bytes``: 16 for an [n, 4] cloud, or a ``_lib.layout`` descriptor for an array whose rows are such records
    (``io.pcl_xyzi_records``).  Returns ``(filled, info)``; ``filled`` is None when RANSAC found no model (``info["has_model"]`` False)."""
    ctx = ctx or default_context()
    c = _cloud(cloud) if stride_bytes == 16 else np.ascontiguousarray(cloud)  # (records of any dtype: their bytes are what is read)
    p, est, added = _ground_fill_args(radius, map_resolution, simple, estimate)
    cap = len(c) + added
    out = np.empty((max(cap, 1), 4), dtype=np.float32)
    r = GroundFillResult()
    check(lib().mrgfe_fill_ground_plane(ctx._h, C.byref(p), est.ctypes.data_as(C.POINTER(C.c_double)) if est is not None else None, C.cast(c.ctypes.data, _fp), len(c),
                                        int(stride_bytes), out.ctypes.data_as(_fp), cap, C.byref(r)))
    info = _ground_fill_info(r)
    return (out[: r.n_before + r.n_added] if r.has_model else None), info


class MapCloudStore:
    """Keyframe clouds resident in HBM (mrgfe_map_store): the map is regenerated from all keyframes every time it is
    published, and between two calls only the poses change."""

    def __init__(self, ctx: Context | None = None):
        self._ctx = ctx or default_context()
        self._h = C.c_void_p()
        check(lib().mrgfe_map_store_create(self._ctx._h, C.byref(self._h)))

    def _release_out(self):
        if getattr(self, "_out", None) is not None and getattr(self, "_out_pinned", False):
            lib().mrgfe_unpin_host_buffer(self._ctx._h, self._out.ctypes.data_as(C.c_void_p))
        self._out, self._out_pinned = None, False

    def _download_buffer(self, rows: int) -> np.ndarray:
        """The buffer the store keeps between calls for what comes down, with room for ``rows`` 16-byte rows: grown with a quarter of headroom, touched
        once and page-locked where the runtime allows it (the download is then direct DMA)."""
        if getattr(self, "_out", None) is None or len(self._out) < rows:
            self._release_out()
            self._out = np.empty((rows + rows // 4, 4), dtype=np.float32)
            self._out[:] = 0  # (touch the pages once, here)
            try:  # page-locked: the download is direct DMA
                check(lib().mrgfe_pin_host_buffer(self._ctx._h, self._out.ctypes.data_as(C.c_void_p), self._out.nbytes))
                self._out_pinned = True
            except MrgfeError:
                self._out_pinned = False
        return self._out

    def __del__(self):
        try:
            self._release_out()
            if getattr(self, "_h", None):
                # the store borrows its context: when the collector has finalised that first (members of a reference cycle are finalised in no particular
                # order) the library call would touch freed memory, so the handle is dropped unfreed instead (as OdomHandle.close does)
                if getattr(getattr(self, "_ctx", None), "_h", None):
                    lib().mrgfe_map_store_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass

    def add(self, key: int, cloud) -> None:
        c = _cloud(cloud)
        check(lib().mrgfe_map_store_add(self._h, key, c.ctypes.data_as(_fp), len(c), 16))

    def keyframe_callback(self, key: int, payload_or_msg, centres_sensor=None, radius: float = 2.0, want_kept: bool = True, want_removed: bool = True, records: int = 0,
                          kept_out=None, removed_out=None):
        """``mrgfe_keyframe_callback``: the point work of MrgSlamComponent::cloud_callback (apps/mrg_slam_component.cpp:372, 396-430) on a
        sensor_msgs/PointCloud2 — a dict with ``data``, ``width``, ``height``, ``point_step``, ``fields`` (name -> byte offset) and optionally
        ``row_step``, or a packed [n, 4] float32 cloud — in one call: the payload goes up once, every point closer than ``radius`` to one of
        ``centres_sensor`` (K x 3, sensor frame, K <= 64; robot_radius_sqr is float(radius * radius), :406-407) is split off, and the kept cloud
        becomes keyframe ``key`` of this store.  Returns ``(kept, removed)``; an output that is not wanted is None and is not downloaded.
        ``records`` 32 or 16 (default 0: off): the callback to its publishes (``mrgfe_keyframe_callback_records``, :432-443) — ``kept`` and ``removed`` are
        the ``data`` of ``cloud_msg_filtered`` and ``other_robots_removed_points`` (uint8, ``count * records`` bytes, written on the device; views of
        ``kept_out`` / ``removed_out`` when the caller gives its own, ideally page-locked, buffers)."""
        msg = payload_or_msg if isinstance(payload_or_msg, dict) else pointcloud2_from_xyzi(payload_or_msg)
        p = keyframe_params(msg, self._ctx)
        n = int(p.width) * int(p.height)
        buf = np.frombuffer(msg["data"], dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
        ctr = np.ascontiguousarray(np.asarray(centres_sensor if centres_sensor is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3))
        if records:
            return self._callback_records(n, records, want_kept, want_removed, kept_out, removed_out, lambda *tail: lib().mrgfe_keyframe_callback_records(
                self._h, int(key), C.byref(p), buf.ctypes.data_as(C.c_void_p) if n else None, buf.nbytes, ctr.ctypes.data_as(_fp) if len(ctr) else None, len(ctr),
                float(np.float32(float(radius) * float(radius))), *tail))
        kept = np.empty((n, 4), dtype=np.float32) if want_kept else None
        removed = np.empty((n, 4), dtype=np.float32) if want_removed and len(ctr) else None
        nk, nr = C.c_size_t(0), C.c_size_t(0)
        check(lib().mrgfe_keyframe_callback(self._h, int(key), C.byref(p), buf.ctypes.data_as(C.c_void_p) if n else None, buf.nbytes,
                                            ctr.ctypes.data_as(_fp) if len(ctr) else None, len(ctr), float(np.float32(float(radius) * float(radius))),
                                            kept.ctypes.data_as(_fp) if kept is not None else None, C.byref(nk),
                                            removed.ctypes.data_as(_fp) if removed is not None else None, C.byref(nr)))
        if want_removed and removed is None:
            removed = np.empty((0, 4), dtype=np.float32)  # (no other robot: nothing was removed)
        return (kept[: nk.value] if kept is not None else None), (removed[: nr.value] if removed is not None else None)

    def _callback_records(self, n, records, want_kept, want_removed, kept_out, removed_out, call):
        """the record tail of both callback forms: ``call(point_step, kept, kept capacity, n_kept, removed, removed capacity, n_removed)``"""
        from .filters import _records_destination

        kept = _records_destination(n, records, kept_out) if want_kept else None
        removed = _records_destination(n, records, removed_out) if want_removed else None
        nk, nr = C.c_size_t(0), C.c_size_t(0)
        check(call(int(records), kept.ctypes.data_as(C.c_void_p) if kept is not None else None, kept.nbytes if kept is not None else 0, C.byref(nk),
                   removed.ctypes.data_as(C.c_void_p) if removed is not None else None, removed.nbytes if removed is not None else 0, C.byref(nr)))
        return (kept[: nk.value * records] if kept is not None else None), (removed[: nr.value * records] if removed is not None else None)

    def keyframe_callback_device(self, key: int, dev_ptr: int, n: int, centres_sensor=None, radius: float = 0.0, want_kept: bool = True, want_removed: bool = False,
                                 records: int = 0, kept_out=None, removed_out=None):
        """``mrgfe_keyframe_callback_device``: :meth:`keyframe_callback` for a filtered scan that is already in HBM (all components in one container) —
        ``n`` packed float4 points at ``dev_ptr`` on the store's device, complete when the call is made (``scan_callback_to_device`` and the other
        ``*_device`` producers return only after their wait).  No upload: the same kernels read the buffer where it is; it is only read and is free
        on return.  Returns ``(kept, removed)`` as :meth:`keyframe_callback` does; ``records``: as there (``mrgfe_keyframe_callback_records_device``)."""
        n = int(n)
        ctr = np.ascontiguousarray(np.asarray(centres_sensor if centres_sensor is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3))
        if records:
            return self._callback_records(n, records, want_kept, want_removed, kept_out, removed_out, lambda *tail: lib().mrgfe_keyframe_callback_records_device(
                self._h, int(key), C.c_void_p(int(dev_ptr)) if dev_ptr else None, n, ctr.ctypes.data_as(_fp) if len(ctr) else None, len(ctr),
                float(np.float32(float(radius) * float(radius))), *tail))
        kept = np.empty((n, 4), dtype=np.float32) if want_kept else None
        removed = np.empty((n, 4), dtype=np.float32) if want_removed and len(ctr) else None
        nk, nr = C.c_size_t(0), C.c_size_t(0)
        check(lib().mrgfe_keyframe_callback_device(self._h, int(key), C.c_void_p(int(dev_ptr)) if dev_ptr else None, n, ctr.ctypes.data_as(_fp) if len(ctr) else None, len(ctr),
                                                   float(np.float32(float(radius) * float(radius))), kept.ctypes.data_as(_fp) if kept is not None else None, C.byref(nk),
                                                   removed.ctypes.data_as(_fp) if removed is not None else None, C.byref(nr)))
        if want_removed and removed is None:
            removed = np.empty((0, 4), dtype=np.float32)  # (no other robot: nothing was removed)
        return (kept[: nk.value] if kept is not None else None), (removed[: nr.value] if removed is not None else None)

    def fill_ground(self, src_key: int, dst_key: int, radius: float = 5.0, map_resolution: float = 0.05, simple: bool = False, estimate=None, want_cloud: bool = True):
        """``mrgfe_map_store_fill_ground``: the ground fill of the first keyframe (src/mrg_slam/graph_database.cpp:114-129) for the stored keyframe
        ``src_key``.  The filled cloud becomes the NEW keyframe ``dst_key`` — name the first keyframe by it from then on —; ``src_key`` stays as it was.
        ``estimate``: the 4 x 4 ``keyframe->node->estimate()`` of the simple variant.  Returns ``(filled, info)``: ``filled`` is the filled cloud
        (``keyframe->cloud = cloud_filled``) or None when it was not wanted or RANSAC found no model — then ``info["has_model"]`` is False and there is
        no ``dst_key``."""
        p, est, added = _ground_fill_args(radius, map_resolution, simple, estimate)
        cap = (self.has(int(src_key)) or 0) + added
        out = np.empty((max(cap, 1), 4), dtype=np.float32) if want_cloud else None
        r = GroundFillResult()
        check(lib().mrgfe_map_store_fill_ground(self._h, int(src_key), int(dst_key), C.byref(p), est.ctypes.data_as(C.POINTER(C.c_double)) if est is not None else None,
                                                out.ctypes.data_as(_fp) if out is not None else None, cap, C.byref(r)))
        info = _ground_fill_info(r)
        return (out[: r.n_before + r.n_added] if out is not None and r.has_model else None), info

    def add_keyframes(self, items) -> np.ndarray:
        """``mrgfe_map_store_add_keyframes``: the point work of GraphDatabase::add_static_keyframes / flush_graph_queue / load_graph
        (src/mrg_slam/graph_database.cpp:181-182, 294-295, 449-461) for a whole list of keyframe messages — one arena block, the payloads up behind
        one another, ONE launch, ONE wait.  ``items``: ``(key, payload_or_msg)`` pairs, each as :meth:`keyframe_callback` takes it; layouts may
        differ.  Returns the added flags (uint8 [n]): 0 for a key that was already stored, or came earlier in the list, with the same point count."""
        items = list(items)
        n = len(items)
        msgs = (KeyframeMsg * max(n, 1))()
        keep = []  # the payload buffers stay alive until the call has returned
        for i, (key, payload_or_msg) in enumerate(items):
            msg = payload_or_msg if isinstance(payload_or_msg, dict) else pointcloud2_from_xyzi(payload_or_msg)
            buf = np.frombuffer(msg["data"], dtype=np.uint8)
            keep.append(buf)
            msgs[i].key = int(key)
            msgs[i].layout = keyframe_params(msg, self._ctx)
            msgs[i].data = buf.ctypes.data if buf.nbytes else None
            msgs[i].data_bytes = buf.nbytes
        added = np.zeros(n, dtype=np.uint8)
        check(lib().mrgfe_map_store_add_keyframes(self._h, n, msgs, added.ctypes.data_as(C.POINTER(C.c_uint8))))
        return added

    def information_matrices(self, params, edges):
        """``mrgfe_map_store_edges``: InformationMatrixCalculator::calc_information_matrix for every edge ``(key1, key2, relpose)`` of a list (the
        loops of GraphDatabase::flush_keyframe_queue :139-142 and insert_loops :579-581) — one grouped grid build for the key1 clouds that have
        none, one batch of the fitness passes.  ``params``: a ``_lib.InfParams``.  Returns ``(inf [n, 6, 6], fitness [n])``."""
        edges = list(edges)
        n = len(edges)
        rec = (GraphEdge * max(n, 1))()
        for i, (key1, key2, relpose) in enumerate(edges):
            rec[i].key1, rec[i].key2 = int(key1), int(key2)
            rec[i].relpose[:] = np.asarray(relpose, dtype=np.float64).T.reshape(16).tolist()  # column-major
        inf, fit = np.zeros((n, 6, 6)), np.zeros(n)
        dp = C.POINTER(C.c_double)
        check(lib().mrgfe_map_store_edges(self._h, C.byref(params), n, rec, inf.ctypes.data_as(dp), fit.ctypes.data_as(dp)))
        return inf, fit

    def has(self, key: int):
        n = C.c_size_t(0)
        return n.value if lib().mrgfe_map_store_has(self._h, key, C.byref(n)) else None

    def bytes(self) -> int:
        return int(lib().mrgfe_map_store_bytes(self._h))

    def fitness(self, key1: int, key2: int, relpose, max_range: float = float("inf")) -> float:
        """InformationMatrixCalculator::calc_fitness_score(cloud1 = keyframe key1, cloud2 = keyframe key2, relpose) on the resident clouds."""
        T = np.ascontiguousarray(np.asarray(relpose, dtype=np.float64).T)
        out = C.c_double(0)
        check(lib().mrgfe_map_store_fitness(self._h, int(key1), int(key2), T.ctypes.data_as(C.POINTER(C.c_double)), max_range, C.byref(out)))
        return out.value

    def generate(self, keys, poses, first_keyframe=None, resolution: float = 0.1, min_points_per_voxel: int = 1, distance_far_thresh: float = 10000.0,
                 skip_first_cloud: bool = False, copy: bool = True):
        """MapCloudGenerator.generate over the stored keyframes ``keys`` with their current ``poses`` (4 x 4 each).
        The download lands in a buffer the store keeps between calls (a fresh 100 MB array per call costs more in page faults than the
        kernels and the copy together); ``copy=False`` returns a view of it that the next call overwrites."""
        K = len(keys)
        ks = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
        P = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64).T.reshape(16) for p in poses])) if K else np.zeros((0, 16))
        first = np.ascontiguousarray(np.asarray(first_keyframe if first_keyframe is not None else np.zeros(K), dtype=np.uint8))
        cap = max(sum(self.has(int(k)) or 0 for k in keys), 1)
        out = self._download_buffer(cap)
        m = C.c_size_t(0)
        try:
            check(lib().mrgfe_map_store_generate(self._h, K, ks.ctypes.data_as(C.POINTER(C.c_uint64)), P.ctypes.data_as(C.POINTER(C.c_double)),
                                                 first.ctypes.data_as(C.POINTER(C.c_uint8)), float(resolution), int(min_points_per_voxel), float(distance_far_thresh),
                                                 int(bool(skip_first_cloud)), out.ctypes.data_as(_fp), cap, C.byref(m)))
        except MrgfeError as e:
            if e.status == ERR_EMPTY:
                return None
            raise
        return out[: m.value].copy() if copy else out[: m.value]

    def _publish_args(self, keys, poses, first_keyframe, resolution, min_points_per_voxel, distance_far_thresh, skip_first_cloud, point_step, offsets):
        K = len(keys)
        ks = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
        P = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64).T.reshape(16) for p in poses])) if K else np.zeros((0, 16))
        first = np.ascontiguousarray(np.asarray(first_keyframe if first_keyframe is not None else np.zeros(K), dtype=np.uint8))
        offs = [np.asarray(o, dtype=np.float64).reshape(3).astype(np.float32) for o in offsets]  # (*zero_utm).cast<float>()
        p = MapPublishParams(float(resolution), int(min_points_per_voxel), float(distance_far_thresh), int(bool(skip_first_cloud)), int(point_step), len(offs))
        for i, o in enumerate(offs[:2]):  # (a third offset: n_offsets = 3, which the library refuses)
            p.offsets[3 * i:3 * i + 3] = [float(v) for v in o]
        return K, ks, P, first, p

    def publish(self, keys, poses, first_keyframe=None, resolution: float = 0.1, min_points_per_voxel: int = 1, distance_far_thresh: float = 10000.0,
                skip_first_cloud: bool = False, point_step: int = 32, offsets=(), copy: bool = True):
        """``mrgfe_map_store_publish``: the map of :meth:`generate` — same points, order and bits — as the records its callers send or save, written on the
        device: ``point_step`` 32 gives the ``pcl::toROSMsg`` records (x, y, z, 1.0f, intensity, three zero words), 16 the packed points of a binary PCD's
        body; ``offsets``: up to two (x, y, z) added in f32 one after the other behind the voxel filter (zero_utm, then zero_enu:
        apps/mrg_slam_component.cpp:1104-1116).  Returns the message as a dict — ``data`` (uint8), ``width``, ``height``, ``point_step``, ``row_step``,
        ``fields``, ``is_dense``, ``is_bigendian``, and ``n_unfiltered`` (the points before the voxel filter) — which ``io.xyzi_from_pointcloud2``,
        ``io.layout_from_fields`` and :meth:`keyframe_callback` take back, or None where the reference returns nullptr.  The download lands in the
        buffer :meth:`generate` uses; ``copy=False`` returns a view of it that the next call overwrites."""
        K, ks, P, first, p = self._publish_args(keys, poses, first_keyframe, resolution, min_points_per_voxel, distance_far_thresh, skip_first_cloud, point_step, offsets)
        cap = max(sum(self.has(int(k)) or 0 for k in keys), 1)
        out = self._download_buffer(cap * (2 if int(point_step) == 32 else 1)).reshape(-1).view(np.uint8)
        r = MapPublishResult()
        try:
            check(lib().mrgfe_map_store_publish(self._h, K, ks.ctypes.data_as(C.POINTER(C.c_uint64)), P.ctypes.data_as(C.POINTER(C.c_double)),
                                                first.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(p), out.ctypes.data_as(C.c_void_p), cap * int(point_step), C.byref(r)))
        except MrgfeError as e:
            if e.status == ERR_EMPTY:
                return None
            raise
        data = out[: r.data_bytes]
        return _map_message(data.copy() if copy else data, r)

    def publish_device(self, keys, poses, first_keyframe=None, resolution: float = 0.1, min_points_per_voxel: int = 1, distance_far_thresh: float = 10000.0,
                       skip_first_cloud: bool = False, point_step: int = 32, offsets=()):
        """``mrgfe_map_store_publish_device``: :meth:`publish` with the records left in the store's workspace.  Returns the message dict with ``data`` None and
        ``dev_ptr`` (0 for an empty map): device memory that is complete on return and valid until the next publish, read or the end of this store."""
        K, ks, P, first, p = self._publish_args(keys, poses, first_keyframe, resolution, min_points_per_voxel, distance_far_thresh, skip_first_cloud, point_step, offsets)
        r, d = MapPublishResult(), C.c_void_p()
        try:
            check(lib().mrgfe_map_store_publish_device(self._h, K, ks.ctypes.data_as(C.POINTER(C.c_uint64)), P.ctypes.data_as(C.POINTER(C.c_double)),
                                                       first.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(p), C.byref(d), C.byref(r)))
        except MrgfeError as e:
            if e.status == ERR_EMPTY:
                return None
            raise
        msg = _map_message(None, r)
        msg["dev_ptr"] = int(d.value or 0)
        return msg

    def read(self, keys, point_step: int = 32):
        """``mrgfe_map_store_read``: the stored clouds of ``keys`` (a key may repeat) as records — ``uint8 [n_i, point_step]`` arrays, views of one buffer —
        with ``point_step`` 32 (``io.pcl_xyzi_records``: the cloud_msg of publish_graph_service) or 16 (the packed points: a binary PCD's body).  One
        launch at most and one wait for the whole list."""
        keys = [int(k) for k in keys]
        step = int(point_step)
        ks = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
        cap = sum(self.has(k) or 0 for k in keys) * (step if step in (16, 32) else 0)
        data = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(len(keys) + 1, dtype=np.uint64)
        check(lib().mrgfe_map_store_read(self._h, len(keys), ks.ctypes.data_as(C.POINTER(C.c_uint64)), step, data.ctypes.data_as(C.c_void_p), cap,
                                         offs.ctypes.data_as(C.POINTER(C.c_uint64))))
        return [data[int(offs[i]):int(offs[i + 1])].reshape(-1, step) for i in range(len(keys))]

    def egress_stats(self) -> dict:
        """``mrgfe_map_store_egress_stats``: what the last :meth:`publish` / :meth:`read` did — kernel launches of its record stage, host waits of the whole
        call, bytes brought down, device bytes its workspace grew by."""
        v = (C.c_int64 * 4)()
        check(lib().mrgfe_map_store_egress_stats(self._h, v))
        return dict(zip(("launches", "host_waits", "bytes_down", "workspace_grown"), [int(x) for x in v]))


def _map_message(data, r) -> dict:
    """The sensor_msgs/PointCloud2 members of a published map: what pcl::toROSMsg fills for an unorganised pcl::PointXYZI cloud (four FLOAT32 fields; the
    padding words of the record are no fields), or the packed layout of ``io.pointcloud2_from_xyzi``."""
    return {"height": 1, "width": int(r.n_points), "is_dense": False, "is_bigendian": False, "point_step": int(r.point_step), "row_step": int(r.data_bytes),
            "fields": {"x": 0, "y": 4, "z": 8, "intensity": int(r.off_intensity)}, "data": data, "n_unfiltered": int(r.n_unfiltered)}


@dataclass
class MapRequest:
    """The members of mrg_slam_msgs/srv/PublishMap and SaveMap the two services read; the defaults are the "not set" values of
    apps/mrg_slam_component.cpp:774-779 / 1087-1092."""

    resolution: float = 0.0  # 0: map_cloud_resolution
    min_points_per_voxel: int = -1  # < 0: map_cloud_min_points_per_voxel
    distance_far_thresh: float = 0.0  # 0: map_cloud_distance_far_thresh
    skip_first_cloud: bool = False
    frame_id: str = ""  # empty: map_frame_id
    utm: bool = False  # SaveMap: add zero_utm to the points


class MapPublisher:
    """Host mirror of the three callers of MapCloudGenerator::generate in MrgSlamComponent over a map store (anything with :meth:`MapCloudStore.publish`'s
    signature: the logic runs on the CPU against a stand-in):

    * :meth:`update` — update_map_cloud_msg (apps/mrg_slam_component.cpp:712-740) behind ``map_cloud_msg_update_required_``;
    * :meth:`publish_map` — publish_map_service (:764-796);
    * :meth:`save_map` — save_map_service (:1078-1144): the PCD and the ``.utm`` file.

    ``set_snapshot`` is what the optimisation timer does at :880-890: the new ``(key, pose, first_keyframe)`` list and the flag."""

    def __init__(self, store, map_cloud_resolution: float = 0.05, map_cloud_min_points_per_voxel: int = 2, map_cloud_distance_far_thresh: float = 10000.0,
                 map_frame_id: str = "map", zero_utm=None, zero_enu=None):
        self.store = store
        self.resolution, self.min_points_per_voxel, self.distance_far_thresh = float(map_cloud_resolution), int(map_cloud_min_points_per_voxel), float(map_cloud_distance_far_thresh)
        self.map_frame_id = map_frame_id
        self.zero_utm, self.zero_enu = zero_utm, zero_enu  # GpsProcessor::zero_utm() / zero_enu(): (x, y, z) doubles or None
        self.snapshot: list = []
        self.update_required = False
        self.map_cloud_msg = None
        self.updated = False  # what the last update_map_cloud_msg returned

    def set_snapshot(self, snapshot) -> None:
        self.snapshot = [(int(k), np.asarray(T, dtype=np.float64), bool(f)) for k, T, f in snapshot]
        self.update_required = True

    def _request(self, req):
        """(resolution, min_points_per_voxel, distance_far_thresh, frame_id) of a request: the config values where it sets none (:774-779)."""
        resolution = self.resolution if req.resolution == 0 else req.resolution
        min_points = self.min_points_per_voxel if req.min_points_per_voxel < 0 else req.min_points_per_voxel
        far = self.distance_far_thresh if req.distance_far_thresh == 0 else req.distance_far_thresh
        return float(np.float32(resolution)), int(min_points), float(np.float32(far)), (req.frame_id or self.map_frame_id)

    def _publish(self, snapshot, **kw):
        return self.store.publish([k for k, _, _ in snapshot], [T for _, T, _ in snapshot], [f for _, _, f in snapshot], **kw)

    def update(self):
        """update_map_cloud_msg: regenerates ``map_cloud_msg`` when the snapshot has changed since the last call, and returns it — the cached message
        otherwise, and after a generation that gave no cloud; ``updated`` is the reference's return value."""
        self.updated = False
        if not self.update_required:
            return self.map_cloud_msg
        snapshot, self.update_required = self.snapshot, False
        msg = self._publish(snapshot, resolution=self.resolution, min_points_per_voxel=self.min_points_per_voxel, distance_far_thresh=self.distance_far_thresh,
                            skip_first_cloud=False, point_step=32)
        if msg is None:
            return self.map_cloud_msg
        msg["frame_id"] = self.map_frame_id
        self.map_cloud_msg, self.updated = msg, True
        return msg

    def publish_map(self, req=None):
        """publish_map_service: the message to publish, or None (``res->success = false``)."""
        req = req or MapRequest()
        resolution, min_points, far, frame_id = self._request(req)
        msg = self._publish(self.snapshot, resolution=resolution, min_points_per_voxel=min_points, distance_far_thresh=far, skip_first_cloud=bool(req.skip_first_cloud),
                            point_step=32)
        if msg is not None:
            msg["frame_id"] = frame_id
        return msg

    def save_map(self, req, path: str) -> bool:
        """save_map_service: the map with zero_utm (only when ``req.utm``) and zero_enu (whenever set) added, as a binary PCD at ``path`` — the header of
        ``io.write_pcd_binary`` and the 16-byte records as they came down — and ``path + ".utm"`` whenever zero_utm is set (:1121-1124).  The directory
        is made first (the reference makes it after the ``.utm`` file).  Returns ``res->success``."""
        resolution, min_points, far, _ = self._request(req)
        offsets = []
        if self.zero_utm is not None and req.utm:
            offsets.append(self.zero_utm)
        if self.zero_enu is not None:
            offsets.append(self.zero_enu)
        msg = self._publish(self.snapshot, resolution=resolution, min_points_per_voxel=min_points, distance_far_thresh=far, skip_first_cloud=bool(req.skip_first_cloud),
                            point_step=16, offsets=offsets, copy=False)
        if msg is None:
            return False
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        if self.zero_utm is not None:
            with open(path + ".utm", "w") as f:
                f.write("%.6f %.6f %.6f\n" % tuple(float(v) for v in self.zero_utm))
        with open(path, "wb") as f:
            f.write(pcd_binary_header(msg["width"]))
            f.write(memoryview(msg["data"]))
        return True


class MapCloudGenerator:
    def __init__(self, ctx: Context | None = None):
        self._ctx = ctx or default_context()

    def generate(self, keyframes, resolution: float, min_points_per_voxel: int = 1, distance_far_thresh: float = 10000.0, skip_first_cloud: bool = False):
        """Returns the map cloud (voxels in ascending voxel index; the reference's order is its hash map's), or None where
        the reference returns nullptr (no keyframes, or an empty cloud from more than one keyframe)."""
        kfs = list(keyframes)
        K = len(kfs)
        clouds = [_cloud(k.cloud) for k in kfs]
        ptrs = (_fp * max(K, 1))(*[c.ctypes.data_as(_fp) for c in clouds])
        ns = (C.c_size_t * max(K, 1))(*[len(c) for c in clouds])
        poses = np.ascontiguousarray(np.stack([np.asarray(k.pose, dtype=np.float64).T.reshape(16) for k in kfs])) if K else np.zeros((0, 16))
        first = np.ascontiguousarray(np.array([1 if k.first_keyframe else 0 for k in kfs], dtype=np.uint8))
        cap = max(int(sum(len(c) for c in clouds)), 1)
        out = np.empty((cap, 4), dtype=np.float32)
        m = C.c_size_t(0)
        try:
            check(lib().mrgfe_map_cloud_generate(self._ctx._h, K, ptrs, ns, 16, poses.ctypes.data_as(C.POINTER(C.c_double)), first.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 float(resolution), int(min_points_per_voxel), float(distance_far_thresh), int(bool(skip_first_cloud)),
                                                 out.ctypes.data_as(_fp), cap, C.byref(m)))
        except MrgfeError as e:
            if e.status == ERR_EMPTY:
                return None
            raise
        return out[: m.value].copy()


def remove_points_near(cloud, centres_sensor, radius: float, ctx: Context | None = None):
    """Returns (kept, removed): every point closer than ``radius`` to one of ``centres_sensor`` (K x 3, sensor frame) goes to
    ``removed``.  robot_radius_sqr is float(radius * radius), as at mrg_slam_component.cpp:405-406."""
    ctx = ctx or default_context()
    c = _cloud(cloud)
    ctr = np.ascontiguousarray(np.asarray(centres_sensor, dtype=np.float32).reshape(-1, 3))
    kept, removed = np.empty_like(c), np.empty_like(c)
    nk, nr = C.c_size_t(0), C.c_size_t(0)
    check(lib().mrgfe_remove_points_near(ctx._h, c.ctypes.data_as(_fp), len(c), 16, ctr.ctypes.data_as(_fp), len(ctr), float(np.float32(float(radius) * float(radius))),
                                         kept.ctypes.data_as(_fp), C.byref(nk), removed.ctypes.data_as(_fp), C.byref(nr)))
    return kept[: nk.value].copy(), removed[: nr.value].copy()


def deskew(cloud, angular_velocity, scan_period: float = 0.1, ctx: Context | None = None) -> np.ndarray:
    ctx = ctx or default_context()
    c = _cloud(cloud)
    out = np.empty_like(c)
    av = np.ascontiguousarray(np.asarray(angular_velocity, dtype=np.float32).reshape(3))
    check(lib().mrgfe_deskew(ctx._h, c.ctypes.data_as(_fp), len(c), 16, av.ctypes.data_as(_fp), float(scan_period), out.ctypes.data_as(_fp)))
    return out


def transform_cloud(cloud, T, ctx: Context | None = None) -> np.ndarray:
    """pcl::transformPointCloud(cloud, out, Matrix4f(T)) (the base_link transform of PrefilteringComponent::cloud_callback,
    apps/prefiltering_component.cpp:141): float arithmetic, non-finite points unchanged, intensity copied."""
    ctx = ctx or default_context()
    c = _cloud(cloud)
    out = np.empty_like(c)
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float32).T)
    check(lib().mrgfe_transform_cloud(ctx._h, c.ctypes.data_as(_fp), len(c), 16, Tc.ctypes.data_as(_fp), out.ctypes.data_as(_fp)))
    return out
