"""Host-side mirror of the per-point passes around the scan-matching path, bound to
libmrgfe.so:

* :class:`MapCloudGenerator` — mrg_slam::MapCloudGenerator (/root/reference/src/mrg_slam/map_cloud_generator.cpp:14-86,
  called from apps/mrg_slam_component.cpp:727,781,1097) with its pcl::ApproximateMeanVoxelGrid pass;
* :func:`remove_points_near` — the other-robot point removal of apps/mrg_slam_component.cpp:396-429;
* :func:`deskew` — PrefilteringComponent::deskewing (apps/prefiltering_component.cpp:231-292);
* :func:`fill_ground_plane` and :meth:`MapCloudStore.fill_ground` — the ground fill of the first keyframe
  (src/mrg_slam/graph_database.cpp:114-129, src/pcl/fill_ground_plane.cpp).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import Context, GraphEdge, GroundFillParams, GroundFillResult, KeyframeMsg, KeyframeParams, MrgfeError, check, default_context, lib
from .filters import _cloud
from .io import pointcloud2_from_xyzi

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

    def __del__(self):
        try:
            self._release_out()
            if getattr(self, "_h", None):
                lib().mrgfe_map_store_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass

    def add(self, key: int, cloud) -> None:
        c = _cloud(cloud)
        check(lib().mrgfe_map_store_add(self._h, key, c.ctypes.data_as(_fp), len(c), 16))

    def keyframe_callback(self, key: int, payload_or_msg, centres_sensor=None, radius: float = 2.0, want_kept: bool = True, want_removed: bool = True):
        """``mrgfe_keyframe_callback``: the point work of MrgSlamComponent::cloud_callback (apps/mrg_slam_component.cpp:372, 396-430) on a
        sensor_msgs/PointCloud2 — a dict with ``data``, ``width``, ``height``, ``point_step``, ``fields`` (name -> byte offset) and optionally
        ``row_step``, or a packed [n, 4] float32 cloud — in one call: the payload goes up once, every point closer than ``radius`` to one of
        ``centres_sensor`` (K x 3, sensor frame, K <= 64; robot_radius_sqr is float(radius * radius), :406-407) is split off, and the kept cloud
        becomes keyframe ``key`` of this store.  Returns ``(kept, removed)``; an output that is not wanted is None and is not downloaded."""
        msg = payload_or_msg if isinstance(payload_or_msg, dict) else pointcloud2_from_xyzi(payload_or_msg)
        p = keyframe_params(msg, self._ctx)
        n = int(p.width) * int(p.height)
        buf = np.frombuffer(msg["data"], dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
        ctr = np.ascontiguousarray(np.asarray(centres_sensor if centres_sensor is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3))
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

    def keyframe_callback_device(self, key: int, dev_ptr: int, n: int, centres_sensor=None, radius: float = 0.0, want_kept: bool = True, want_removed: bool = False):
        """``mrgfe_keyframe_callback_device``: :meth:`keyframe_callback` for a filtered scan that is already in HBM (all components in one container) —
        ``n`` packed float4 points at ``dev_ptr`` on the store's device, complete when the call is made (``scan_callback_to_device`` and the other
        ``*_device`` producers return only after their wait).  No upload: the same kernels read the buffer where it is; it is only read and is free
        on return.  Returns ``(kept, removed)`` as :meth:`keyframe_callback` does."""
        n = int(n)
        ctr = np.ascontiguousarray(np.asarray(centres_sensor if centres_sensor is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3))
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
        if getattr(self, "_out", None) is None or len(self._out) < cap:
            self._release_out()
            self._out = np.empty((cap + cap // 4, 4), dtype=np.float32)
            self._out[:] = 0  # (touch the pages once, here)
            try:  # page-locked: the download is direct DMA
                check(lib().mrgfe_pin_host_buffer(self._ctx._h, self._out.ctypes.data_as(C.c_void_p), self._out.nbytes))
                self._out_pinned = True
            except MrgfeError:
                self._out_pinned = False
        out = self._out
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
