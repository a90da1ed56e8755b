"""Host mirror of the edge-producing parts of ``GraphDatabase`` (``src/mrg_slam/graph_database.cpp`` of the reference): the odometry edges of
``flush_keyframe_queue`` (:65-157) and the loop edges of ``insert_loops`` (:578-590), both of which run inside every optimisation tick
(apps/mrg_slam_component.cpp:802-914), and the information matrices they ask ``InformationMatrixCalculator`` for.

The reference asks for one matrix per edge, inside the loop that makes the edge.  Here the loop makes the LIST of edges (keys and relative poses,
no point work) and one function sends the list through the edge operations: by default ``mrgfe_map_store_edges`` — one grouped grid build, one
batch of the fitness passes — over the keyframes' clouds in the shared :class:`MapCloudStore`; a test injects a per-edge route or the CPU oracle,
and the SAME lists run over all of them, as with ``keyframes.py``.

What stays with the caller: the g2o nodes and edges, robust kernels, uuids, the anchor node and the ground fill of the first keyframe
(:84-129).  A keyframe is any object with ``odom`` (4 x 4 float64, ``Eigen::Isometry3d``) and the key of its cloud (``key``, or
``store_key()`` as ``loop_detector.KeyFrame`` has it); a loop is any object with ``key1``, ``key2`` and ``relative_pose`` (float 4 x 4)."""
from __future__ import annotations

import dataclasses

import numpy as np

from .keyframes import isometry_inverse

DEFAULTS = {"max_keyframes_per_update": 10}  # apps/mrg_slam_component.cpp:279 (config/mrg_slam.yaml:162 sets 10000: the whole queue)

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

    def __init__(self, params: dict | None = None, ops=None, store=None):
        self.p = dict(DEFAULTS)
        self.p.update(params or {})
        if ops is None:
            if store is None:
                raise ValueError("give the edge operations (ops=) or the MapCloudStore the keyframes' clouds are in (store=)")
            ops = HipEdgeOps(store)
        self.ops = ops
        self.keyframe_queue: list = []
        self.new_keyframes: list = []
        self.keyframes: list = []
        self.prev_robot_keyframe = None
        self.edges: list = []

    def add_odom_keyframe(self, keyframe) -> None:
        self.keyframe_queue.append(keyframe)

    def flush_keyframe_queue(self):
        """:48-161.  Returns the new odometry edges with their information matrices, or None where the reference returns false (empty queue)."""
        if not self.keyframe_queue:
            return None
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


__all__ = ["DEFAULTS", "GraphEdge", "GraphDatabaseEdges", "HipEdgeOps", "add_information", "cloud_key", "loop_edges", "odometry_edges"]
