"""GPU: mrgfe_map_store_edges — the information matrices of a whole list of graph edges in one call (one grouped grid build, one batch of the
fitness passes) — against the CPU oracle's calc_information_matrix and against mrgfe_map_store_information_matrix edge by edge; independence from
what the grid caches hold; the edge cases of the single call; and the graph-database mirror's lists through the store and through the oracle."""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [(1, 0), (2, 1), (3, 2), (3, 0), (3, 1), (0, 3), (3, 0)]  # odometry edges, loop edges, a reversed one and a repeated (3, 0)
DBL_MAX = np.finfo(np.float64).max


@functools.lru_cache(maxsize=None)
def scene():
    """Four prefiltered VLP-16 scans on an arc (the clouds of test_gpu_filters.py's information-matrix test), the perturbed relative poses of the
    edge list, and the oracle's matrices and scores: computed once, shared, never written to."""
    from mrg_slam_amd import prefilter, synth
    from oracle import oracle as orc

    sc = synth.street_scene()
    poses = synth.arc_trajectory(4)
    clouds = [prefilter(synth.synth_lidar(sc, poses[k], "VLP16", 900 + k)) for k in range(4)]
    rng = np.random.default_rng(1)
    edges, o_inf, o_fit = [], [], []
    for e, (a, b) in enumerate(PAIRS):
        rel = edges[3][2] if e == 6 else synth.perturb_pose(np.linalg.inv(poses[a]) @ poses[b], rng, (0.05, 0.05, 0.02), (0.2, 0.2, 0.5))  # (the repeat: the same edge again)
        edges.append((a + 1, b + 1, rel))
        m, f = orc.calc_information_matrix(clouds[a], clouds[b], rel)
        o_inf.append(m)
        o_fit.append(f)
    for c in clouds:
        c.setflags(write=False)
    return clouds, poses, edges, np.stack(o_inf), np.array(o_fit)


def fresh_store():
    from mrg_slam_amd import MapCloudStore

    store = MapCloudStore()
    for k, c in enumerate(scene()[0]):
        store.add(k + 1, c)
    return store


def test_against_the_oracle_and_against_the_single_call():
    from mrg_slam_amd import InformationMatrixCalculator

    clouds, _, edges, o_inf, o_fit = scene()
    assert all(2000 < len(c) < 20000 for c in clouds)
    calc = InformationMatrixCalculator()
    inf = calc.calc_information_matrices_keyed(fresh_store(), edges)
    fit = calc.last_fitness_scores
    assert inf.shape == (7, 6, 6) and fit.shape == (7,) and calc.last_fitness_score == fit[-1]
    print("fitness", fit, "oracle", o_fit, "rel", np.abs(fit - o_fit) / o_fit)
    np.testing.assert_allclose(fit, o_fit, rtol=1e-9, atol=0)
    np.testing.assert_allclose(inf, o_inf, rtol=1e-9, atol=0)
    assert (fit > 0).all() and fit[3] == fit[6] and np.array_equal(inf[3], inf[6])  # the repeated edge
    # edge by edge on another store: the single calls build key1's grid alone and score one job per launch
    single = fresh_store()
    s_inf, s_fit = [], []
    for k1, k2, rel in edges:
        s_inf.append(calc.calc_information_matrix_keyed(single, k1, k2, rel))
        s_fit.append(calc.last_fitness_score)
    s_inf, s_fit = np.stack(s_inf), np.array(s_fit)
    print("one call - single", fit - s_fit)
    assert np.array_equal(fit.view(np.uint64), s_fit.view(np.uint64)) and np.array_equal(inf.view(np.uint64), s_inf.view(np.uint64))
    np.testing.assert_allclose(fit, s_fit, rtol=1e-12, atol=0)
    np.testing.assert_allclose(inf, s_inf, rtol=1e-12, atol=0)
    # the same call with E = 1 per edge, on a third store
    one = fresh_store()
    for e, edge in enumerate(edges):
        m = calc.calc_information_matrices_keyed(one, [edge])
        assert m.shape == (1, 6, 6) and np.array_equal(m[0].view(np.uint64), inf[e].view(np.uint64))
        assert calc.last_fitness_scores[0] == fit[e] == calc.last_fitness_score


def test_results_do_not_depend_on_what_the_caches_hold():
    from mrg_slam_amd import InformationMatrixCalculator

    _, _, edges, _, _ = scene()
    calc = InformationMatrixCalculator()

    def run(store, es=edges):
        m = calc.calc_information_matrices_keyed(store, es)
        return m.view(np.uint64).copy(), calc.last_fitness_scores.view(np.uint64).copy()

    ref = run(fresh_store())
    store = fresh_store()
    for again in range(2):  # the second call finds every grid in the set the first one left
        got = run(store)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    warm = fresh_store()
    warm.fitness(4, 1, edges[3][2])  # the single calls' cache holds key1 = 4 and 2, not 3 and 1
    warm.fitness(2, 1, edges[0][2])
    got = run(warm)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # a list whose grids partly sit in the set of the call before, partly have to be built: the set is rebuilt
    part = fresh_store()
    a = run(part, edges[:2])
    b = run(part, edges[1:])
    assert np.array_equal(a[0], ref[0][:2]) and np.array_equal(b[0], ref[0][1:]) and np.array_equal(b[1], ref[1][1:])
    # ... and the single call after the one call still gives its own bits
    for e in (0, 5):
        assert np.float64(part.fitness(*edges[e])).view(np.uint64) == ref[1][e]


def test_edge_cases_of_the_single_call():
    from mrg_slam_amd import InformationMatrixCalculator, MrgfeError, _lib

    clouds, _, edges, _, _ = scene()
    store = fresh_store()
    store.add(9, np.zeros((0, 4), np.float32))  # an empty keyframe
    calc = InformationMatrixCalculator()
    inf = calc.calc_information_matrices_keyed(store, [(2, 2, np.eye(4)), (9, 1, np.eye(4)), (1, 9, np.eye(4)), (9, 9, np.eye(4)), edges[0]])
    fit = calc.last_fitness_scores
    assert fit[0] == 0.0  # key1 == key2 with the identity: every point is its own nearest neighbour
    assert fit[1] == fit[2] == fit[3] == DBL_MAX
    for e in (1, 2, 3):
        np.testing.assert_array_equal(inf[e], calc.from_fitness(DBL_MAX))
        np.testing.assert_array_equal(inf[e], calc.calc_information_matrix_keyed(store, *[(9, 1), (1, 9), (9, 9)][e - 1], np.eye(4)))
    np.testing.assert_array_equal(inf[0], calc.from_fitness(0.0))
    np.testing.assert_array_equal(inf[4], calc.calc_information_matrix_keyed(store, *edges[0]))
    assert len(calc.calc_information_matrices_keyed(store, [])) == 0
    # use_const_inf_matrix: no GPU work, the keys need not exist
    const = InformationMatrixCalculator({"use_const_inf_matrix": True, "const_stddev_x": 0.25})
    m = const.calc_information_matrices_keyed(store, [(77, 78, np.eye(4)), (1, 2, np.eye(4))])
    for k in range(2):
        np.testing.assert_array_equal(m[k], np.diag([4.0] * 3 + [10.0] * 3))
    assert (const.last_fitness_scores == 0.0).all()
    # a missing key: the error names it, and nothing is written
    p = calc._p
    rec = (_lib.GraphEdge * 2)()
    for i, (k1, k2) in enumerate(((2, 1), (1, 4242))):
        rec[i].key1, rec[i].key2 = k1, k2
        rec[i].relpose[:] = np.eye(4).reshape(16).tolist()
    out, f = np.full((2, 36), -7.0), np.full(2, -7.0)
    import ctypes as C

    dp = C.POINTER(C.c_double)
    assert _lib.lib().mrgfe_map_store_edges(store._h, C.byref(p), 2, rec, out.ctypes.data_as(dp), f.ctypes.data_as(dp)) == _lib.ERR_INVALID
    assert "4242" in _lib.last_error() and (out == -7.0).all() and (f == -7.0).all()
    with pytest.raises(MrgfeError, match="4243"):
        calc.calc_information_matrices_keyed(store, [(4243, 1, np.eye(4))])


@dataclasses.dataclass
class KF:
    key: int
    odom: np.ndarray
    cloud: np.ndarray


@dataclasses.dataclass
class Lp:
    key1: KF
    key2: KF
    relative_pose: np.ndarray


def test_the_mirrors_lists_through_the_store_and_through_the_oracle():
    """GraphDatabaseEdges over the store (one call per list) and over the oracle edge by edge: flush_keyframe_queue with max_keyframes_per_update 3
    (two flushes), then insert_loops with two loops whose float relative poses are widened."""
    from mrg_slam_amd import synth
    from mrg_slam_amd.graph_database import GraphDatabaseEdges
    from oracle import oracle as orc

    clouds, poses, _, _, _ = scene()
    rng = np.random.default_rng(7)
    kfs = [KF(k + 1, synth.perturb_pose(poses[k], rng, (0.03, 0.03, 0.01), (0.1, 0.1, 0.3)), clouds[k]) for k in range(4)]

    class OracleOps:
        def information_matrices(self, edges):
            out = [orc.calc_information_matrix(e.key1.cloud, e.key2.cloud, e.relative_pose) for e in edges]
            return np.stack([m for m, _ in out]), np.array([f for _, f in out])

    results = []
    for db in (GraphDatabaseEdges({"max_keyframes_per_update": 3}, store=fresh_store()), GraphDatabaseEdges({"max_keyframes_per_update": 3}, ops=OracleOps())):
        for k in kfs:
            db.add_odom_keyframe(k)
        got = list(db.flush_keyframe_queue())
        got += db.insert_loops([Lp(kfs[2], kfs[0], (np.linalg.inv(kfs[2].odom) @ kfs[0].odom).astype(np.float32))])
        got += db.flush_keyframe_queue()
        got += db.insert_loops([Lp(kfs[3], kfs[0], (np.linalg.inv(kfs[3].odom) @ kfs[0].odom).astype(np.float32)),
                                Lp(kfs[3], kfs[1], (np.linalg.inv(kfs[3].odom) @ kfs[1].odom).astype(np.float32))])
        results.append(got)
    a, b = results
    assert [(e.key1.key, e.key2.key, e.kind) for e in a] == [(e.key1.key, e.key2.key, e.kind) for e in b] == [
        (2, 1, "odom"), (3, 2, "odom"), (3, 1, "loop"), (4, 3, "odom"), (4, 1, "loop"), (4, 2, "loop")]
    for ea, eb in zip(a, b):
        np.testing.assert_array_equal(ea.relative_pose, eb.relative_pose)
        assert ea.fitness == pytest.approx(eb.fitness, rel=1e-9) and eb.fitness > 0
        np.testing.assert_allclose(ea.information, eb.information, rtol=1e-9, atol=0)
