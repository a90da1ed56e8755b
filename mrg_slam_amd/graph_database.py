"""Host mirror of the edge-producing parts of ``GraphDatabase`` (``src/mrg_slam/graph_database.cpp`` of the reference): the odometry edges of
``flush_keyframe_queue`` (:65-157) and the loop edges of ``insert_loops`` (:578-590), both of which run inside every optimisation tick
(apps/mrg_slam_component.cpp:802-914), and the information matrices they ask ``InformationMatrixCalculator`` for.

The reference asks for one matrix per edge, inside the loop that makes the edge.  Here the loop makes the LIST of edges (keys and relative poses,
no point work) and one function sends the list through the edge operations: by default ``mrgfe_map_store_edges`` — one grouped grid build, one
batch of the fitness passes — over the keyframes' clouds in the shared :class:`MapCloudStore`; a test injects a per-edge route or the CPU oracle,
and the SAME lists run over all of them, as with ``keyframes.py``.

The ground fill of the first keyframe (:114-129, ``enable_fill_first_cloud``; off by default as in apps/mrg_slam_component.cpp:270) goes through an
injected operation in the same way: by default ``mrgfe_map_store_fill_ground`` over the store, which stores the filled cloud under a NEW key
and leaves the keyframe's old cloud as it was.

What stays with the caller: the g2o nodes and edges, robust kernels, uuids and the anchor node (:84-112).  A keyframe is any object with ``odom`` (4 x 4 float64, ``Eigen::Isometry3d``) and the key of its cloud (``key``, or
``store_key()`` as ``loop_detector.KeyFrame`` has it); a loop is any object with ``key1``, ``key2`` and ``relative_pose`` (float 4 x 4)."""
from __future__ import annotations

import dataclasses

import numpy as np

from .keyframes import isometry_inverse

DEFAULTS = {"max_keyframes_per_update": 10,  # apps/mrg_slam_component.cpp:279 (config/mrg_slam.yaml:162 sets 10000: the whole queue)
            # the ground fill of the first keyframe, apps/mrg_slam_component.cpp:270-272 and :245 (config/mrg_slam_ouster.yaml:158-160 turns it on, radius 7.5)
            "enable_fill_first_cloud": False, "fill_first_cloud_radius": 5.0, "fill_first_cloud_simple": False, "map_cloud_resolution": 0.05}

# mrgfe_map_store_edges against mrgfe_map_store_information_matrix in a loop (profiles/graph_update_summary.md): lists shorter than this go edge by edge
MIN_EDGES_ONE_CALL = 1


def cloud_key(keyframe) -> int:
    key = getattr(keyframe, "key", None)
    return int(key if key is not None else keyframe.store_key())


@dataclasses.dataclass
class GraphEdge:
    """What add_se3_edge and calc_information_matrix are given for one edge: ``key1`` --relative_pose--> ``key2``."""
    key1: object
    key2: object
    relative_pose: np.ndarray  # 4 x 4 float64
    kind: str = "odom"         # Edge::TYPE_ODOM / TYPE_LOOP
    information: np.ndarray | None = None
    fitness: float | None = None

    def keyed(self):
        return cloud_key(self.key1), cloud_key(self.key2), self.relative_pose


def odometry_edges(queue, prev_robot_keyframe, keyframes_empty: bool, max_keyframes_per_update: int = DEFAULTS["max_keyframes_per_update"]):
    """flush_keyframe_queue :65-158 without the graph: returns ``(edges, prev_robot_keyframe, n_taken)``.  The first ``min(len(queue),
    max_keyframes_per_update)`` keyframes are taken (:65, :158: the caller erases ``queue[:n_taken]``); the very first keyframe of an empty graph
    gets no edge and becomes ``prev`` (:133-136); every other one gets ``keyframe -> prev`` with ``keyframe.odom.inverse() * prev.odom`` (:139),
    and ``prev`` advances (:156)."""
    edges = []
    n_taken = min(len(queue), int(max_keyframes_per_update))
    for i in range(n_taken):
        keyframe = queue[i]
        if i == 0 and keyframes_empty:
            prev_robot_keyframe = keyframe
            continue
        relative_pose = isometry_inverse(keyframe.odom) @ np.asarray(prev_robot_keyframe.odom, dtype=np.float64)
        edges.append(GraphEdge(keyframe, prev_robot_keyframe, relative_pose, "odom"))
        prev_robot_keyframe = keyframe
    return edges, prev_robot_keyframe, max(n_taken, 0)


def loop_edges(loops):
    """insert_loops :578-581: ``relpose = loop->relative_pose.cast<double>()``, edge ``key1 -> key2``."""
    return [GraphEdge(loop.key1, loop.key2, np.asarray(loop.relative_pose).astype(np.float64), "loop") for loop in loops]


class HipEdgeOps:
    """The edge operations on the GPU over the clouds of ``store``: the whole list in one call (``mrgfe_map_store_edges``); lists shorter than
    ``min_edges_one_call`` go edge by edge through ``mrgfe_map_store_information_matrix``."""

    def __init__(self, store, calculator=None, min_edges_one_call: int = MIN_EDGES_ONE_CALL):
        from .filters import InformationMatrixCalculator

        self.store = store
        self.calc = calculator or InformationMatrixCalculator()
        self.min_edges_one_call = int(min_edges_one_call)

    def information_matrices(self, edges):
        keyed = [e.keyed() for e in edges]
        if len(keyed) >= self.min_edges_one_call:
            inf = self.calc.calc_information_matrices_keyed(self.store, keyed)
            return inf, np.array(self.calc.last_fitness_scores, dtype=np.float64)
        inf, fit = np.zeros((len(keyed), 6, 6)), np.zeros(len(keyed))
        for i, (k1, k2, rel) in enumerate(keyed):
            inf[i] = self.calc.calc_information_matrix_keyed(self.store, k1, k2, rel)
            fit[i] = self.calc.last_fitness_score
        return inf, fit


class HipGroundFillOps:
    """The ground fill on the GPU over the clouds of ``store`` (``mrgfe_map_store_fill_ground``).  The store is append-only, so the filled cloud
    becomes a NEW keyframe: ``filled_key(keyframe)`` names it (the integrator's own rule, any non-zero key the store does not hold yet), and the
    keyframe is renamed to it — ``keyframe.key`` is what ``cloud_key`` reads first — so every later edge, loop candidate and map names the filled
    cloud.  With ``want_cloud`` the keyframe's host cloud is replaced too (``keyframe->cloud = cloud_filled``, :125).  Without a RANSAC model
    nothing changes (the reference would read an empty coefficient vector there)."""

    def __init__(self, store, filled_key, want_cloud: bool = True):
        self.store, self.filled_key, self.want_cloud = store, filled_key, bool(want_cloud)
        self.last_info = None

    def fill_first_cloud(self, keyframe, radius, map_resolution, simple, estimate):
        dst = int(self.filled_key(keyframe))
        filled, self.last_info = self.store.fill_ground(cloud_key(keyframe), dst, radius, map_resolution, simple=simple, estimate=estimate, want_cloud=self.want_cloud)
        if self.last_info["has_model"]:
            keyframe.key = dst
            if filled is not None:
                keyframe.cloud = filled
        return self.last_info


def fill_first_cloud(keyframe, params: dict, fill_ops, odom2map=None):
    """:114-129 for the first keyframe of an empty graph: ``fill_ops.fill_first_cloud(keyframe, radius, map_resolution, simple, estimate)`` with
    ``estimate`` = ``keyframe->node->estimate()`` = ``odom2map * keyframe->odom`` (:73-74) in the simple variant (:119-121) and None in the RANSAC
    variant (:123), which does not read it."""
    simple = bool(params["fill_first_cloud_simple"])
    estimate = None
    if simple:
        odom = np.asarray(keyframe.odom, dtype=np.float64)
        estimate = odom if odom2map is None else np.asarray(odom2map, dtype=np.float64) @ odom
    return fill_ops.fill_first_cloud(keyframe, float(params["fill_first_cloud_radius"]), float(params["map_cloud_resolution"]), simple, estimate)


def add_information(edges, ops):
    """Send a list of edges through the edge operations (``ops.information_matrices(edges) -> (inf [n, 6, 6], fitness [n])``) and leave every
    edge's matrix and score with it.  Returns the list."""
    edges = list(edges)
    if edges:
        inf, fit = ops.information_matrices(edges)
        for e, m, f in zip(edges, inf, fit):
            e.information, e.fitness = np.array(m, dtype=np.float64), float(f)
    return edges


class GraphDatabaseEdges:
    """The state the two loops share (``keyframe_queue_``, ``new_keyframes_``, ``keyframes_``, ``prev_robot_keyframe_``) and the two calls of an
    optimisation tick."""

    def __init__(self, params: dict | None = None, ops=None, store=None, fill_ops=None):
        """``fill_ops``: the ground-fill operation (``fill_first_cloud(keyframe, radius, map_resolution, simple, estimate)``), needed only with
        ``enable_fill_first_cloud``: a :class:`HipGroundFillOps` (it needs the integrator's rule for the filled cloud's key), or a test's fake."""
        self.p = dict(DEFAULTS)
        self.p.update(params or {})
        if ops is None:
            if store is None:
                raise ValueError("give the edge operations (ops=) or the MapCloudStore the keyframes' clouds are in (store=)")
            ops = HipEdgeOps(store)
        self.ops = ops
        if self.p["enable_fill_first_cloud"] and fill_ops is None:
            raise ValueError("enable_fill_first_cloud needs the ground-fill operation (fill_ops=): the filled cloud is stored under a key the integrator chooses")
        self.fill_ops = fill_ops
        self.keyframe_queue: list = []
        self.new_keyframes: list = []
        self.keyframes: list = []
        self.prev_robot_keyframe = None
        self.edges: list = []

    def add_odom_keyframe(self, keyframe) -> None:
        self.keyframe_queue.append(keyframe)

    def flush_keyframe_queue(self, odom2map=None):
        """:48-161.  Returns the new odometry edges with their information matrices, or None where the reference returns false (empty queue).
        ``odom2map`` (4 x 4, the identity when None) enters only the estimate the simple ground fill is given (:73-74, :120)."""
        if not self.keyframe_queue:
            return None
        # :79, :114: keyframes_.empty() && new_keyframes_.size() == 1 — the first keyframe taken into an empty graph, before its edges name its cloud
        if self.p["enable_fill_first_cloud"] and not self.keyframes and not self.new_keyframes and int(self.p["max_keyframes_per_update"]) > 0:
            fill_first_cloud(self.keyframe_queue[0], self.p, self.fill_ops, odom2map)
        edges, self.prev_robot_keyframe, n = odometry_edges(self.keyframe_queue, self.prev_robot_keyframe, not self.keyframes, self.p["max_keyframes_per_update"])
        self.new_keyframes.extend(self.keyframe_queue[:n])  # :70
        del self.keyframe_queue[:n]                         # :158
        add_information(edges, self.ops)
        self.edges.extend(edges)
        return edges

    def insert_loops(self, loops):
        """:571-595."""
        edges = add_information(loop_edges(loops), self.ops)
        self.edges.extend(edges)
        self.keyframes.extend(self.new_keyframes)  # :593-594
        self.new_keyframes.clear()
        return edges


__all__ = ["DEFAULTS", "GraphEdge", "GraphDatabaseEdges", "HipEdgeOps", "HipGroundFillOps", "add_information", "cloud_key", "fill_first_cloud", "loop_edges", "odometry_edges"]
