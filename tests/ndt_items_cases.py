"""Inputs and the lock-step replay shared by tests/test_gpu_ndt_items.py (the HIP kernels) and tests/test_ndt_items_cpu.py (its CPU twin).

The NDT derivative kernels work in ITEMS: `ppt` consecutive 256-point tiles of one pair, one partial record each, and a pair's records are added in a fixed
order (four interleaved slices).  A round picks ppt per kernel variant (0 score + gradient + Hessian, 1 score + gradient, 2 f64 Hessian) as

    ppt = clamp(tiles of all pairs busy in that variant // wg_target, 1, max_ppt)        wg_target = CUs * 4, max_ppt = 8

so a pair's f64 sums depend on its own points and on the round's ppt — and through ppt on who else is in its batch, which round the others are in and how many
CUs the device has.  `lockstep_replay` restates that rule (from the sentence above, not from the code) around one hand-stepped optimiser per pair, with an
evaluator that adds in the kernels' order for a given ppt: what a batch must reproduce bit for bit."""
import ctypes as C
import functools

import numpy as np

from oracle.replay import small_cloud

PPTS = (2, 3, 8, 64)
SEARCHES = ("DIRECT7", "DIRECT1", "DIRECT26", "KDTREE")
LEAVES = (1.0, 0.37)  # the kernels take another path when the leaf is not 1
REDUCE_RECORDS = {1: (4, 5, 28, 29, 32, 33, 124, 125, 128, 129, 157), 3: (29, 33, 125, 129)}  # ppt -> records per pair around the 8- and 32-load loops of the reduction

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)


def sizes(ppt):
    """source sizes around the item boundaries: one point, a ragged single tile, one item less / exactly / plus one point, two items plus one point, and a
    last item of ppt - 1 tiles and seven points"""
    return (1, 255, 256 * ppt - 1, 256 * ppt, 256 * ppt + 1, 512 * ppt + 1, 256 * (3 * ppt - 1) + 7)


@functools.lru_cache(maxsize=None)
def target():
    """5000 points in 6 m x 4 m x 3 m: at leaf 0.37 the ground and the walls still hold a dozen points per voxel"""
    t = small_cloud(5000, 41, extent=(3.0, 2.0, 1.5))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def relative_pose():
    from mrg_slam_amd import synth

    return synth.make_pose([0.12, -0.08, 0.03], synth.rot_xyz(0.01, -0.015, 0.02))


@functools.lru_cache(maxsize=None)
def source(n):
    """n target points drawn with replacement, 1 cm of noise, moved by the inverse of relative_pose(); never written to"""
    from oracle import oracle as orc

    rng = np.random.default_rng(7000 + n)
    pts = target()[rng.integers(0, len(target()), n)].copy()
    pts[:, :3] += rng.normal(0, 0.01, (n, 3)).astype(np.float32)
    src = orc.transform_points(np.linalg.inv(relative_pose()), pts)
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def pose():
    """(T, p): where the evaluations are taken, a few centimetres and milliradians off the true pose"""
    from oracle import oracle as orc

    rel = relative_pose()
    p = np.concatenate([rel[:3, 3] + [0.04, -0.03, 0.02], [0.013, -0.011, 0.026]])
    return orc.pose_to_matrix(p), p


@functools.lru_cache(maxsize=None)
def oracle_sums(n, search, leaf, ppt, modes=(0, 1, 2)):
    """{mode: (score, gradient, Hessian)} of the GPU-order oracle for source(n) at pose(): computed once, shared, never written to"""
    from oracle import oracle as orc

    o = orc.Ndt(resolution=leaf, search=search, num_threads=8, gpu_order_ppt=ppt)  # (items in parallel: the sums keep their order)
    assert o.setInputTarget(target()) == 0
    o.setInputSource(source(n))
    T, p = pose()
    out = {}
    for mode in modes:
        s, g, H = o.evaluate(T, p, mode)
        g.setflags(write=False)
        H.setflags(write=False)
        out[mode] = (s, g, H)
    return out


def same_bits(a, b):
    """equal as bit patterns (array_equal would take -0.0 for 0.0 and never a NaN for itself)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


# ------------------------------------------------------------------------------------------------------------------------
# the round plan and the lock-step replay
# ------------------------------------------------------------------------------------------------------------------------
def tiles_of(n):
    return (n + 255) // 256


def ppt_rule(tiles, wg_target, max_ppt):
    return max(1, min(tiles // wg_target, max_ppt))


def ndt_params(eps=1e-3, resolution=1.0, search="DIRECT7", maximum_iterations=64):
    from mrg_slam_amd._lib import NDT_HIP, SEARCH
    from mrg_slam_amd.registration import default_params

    p = default_params(NDT_HIP)
    p.resolution, p.transformation_epsilon, p.maximum_iterations, p.nn_search_method = resolution, eps, maximum_iterations, SEARCH[search]
    return p


def oracle_evaluators(targets, pairs, resolution=1.0, search="DIRECT7", num_threads=8):
    """evaluate(pair, T, p, mode, ppt) over one GPU-order oracle per pair of `pairs` = [(target index, source, guess)]"""
    from oracle import oracle as orc

    objs = []
    for ti, src, _ in pairs:
        o = orc.Ndt(resolution=resolution, search=search, num_threads=num_threads, gpu_order_ppt=1)
        assert o.setInputTarget(targets[ti]) == 0
        o.setInputSource(src)
        objs.append(o)

    def evaluate(i, T, p, mode, ppt):
        objs[i].set_gpu_order_ppt(ppt)
        return objs[i].evaluate(T, p, mode)

    return evaluate


def lockstep_replay(params, n_src, guesses, evaluate, wg_target, max_ppt, forced_ppt=0):
    """The rounds of a batch replayed on the CPU: one hand-stepped optimiser (mrgfe_dbg_ctl_*) per pair; per round every busy pair's requested kind is read,
    each kind's tiles are summed over its busy pairs, ppt comes from the rule (or is `forced_ppt`), and `evaluate(pair, T, p, mode, ppt)` answers.
    Returns (records, schedule): records[i] = dict(T, converged, iterations, evaluations, H, trans_probability, modes); schedule[r] = dict(n_pairs, n_items, ppt),
    three entries each, ppt 0 for a kind without a busy pair."""
    from mrg_slam_amd._lib import check, lib

    L = lib()
    P = len(n_src)
    handles = []
    try:
        for i in range(P):
            h = C.c_void_p()
            g = np.ascontiguousarray(np.asarray(guesses[i], dtype=np.float32).T)
            check(L.mrgfe_dbg_ctl_create(C.byref(params), g.ctypes.data_as(_fp), int(n_src[i]), C.byref(h)))
            handles.append(h)
        modes = [[] for _ in range(P)]
        schedule = []
        while True:
            assert len(schedule) < 2000
            req = {}
            for i in range(P):
                mode, Tc, p = C.c_int(0), np.empty((4, 4), dtype=np.float32), np.empty(6)
                if L.mrgfe_dbg_ctl_request(handles[i], C.byref(mode), Tc.ctypes.data_as(_fp), p.ctypes.data_as(_dp)):
                    req[i] = (mode.value, Tc.T.copy(), p)
            if not req:
                break
            tiles = [sum(tiles_of(n_src[i]) for i, r in req.items() if r[0] == m) for m in range(3)]
            n_pairs = [sum(1 for r in req.values() if r[0] == m) for m in range(3)]
            ppt = [(forced_ppt or ppt_rule(tiles[m], wg_target, max_ppt)) if n_pairs[m] else 0 for m in range(3)]
            n_items = [sum(-(-tiles_of(n_src[i]) // ppt[m]) for i, r in req.items() if r[0] == m) for m in range(3)]
            schedule.append({"n_pairs": n_pairs, "n_items": n_items, "ppt": ppt})
            for i, (mode, T, p) in req.items():
                s, grad, H = evaluate(i, T, p, mode, ppt[mode])
                modes[i].append(mode)
                check(L.mrgfe_dbg_ctl_result(handles[i], s, np.ascontiguousarray(grad).ctypes.data_as(_dp), np.ascontiguousarray(H).ctypes.data_as(_dp), 0.0))
        records = []
        for i in range(P):
            Tc, conv, it, ev = np.empty((4, 4), dtype=np.float32), C.c_int(0), C.c_int(0), C.c_int(0)
            H, tp = np.empty((6, 6)), C.c_double(0)
            check(L.mrgfe_dbg_ctl_final(handles[i], Tc.ctypes.data_as(_fp), C.byref(conv), C.byref(it), C.byref(ev)))
            check(L.mrgfe_dbg_ctl_record(handles[i], H.ctypes.data_as(_dp), C.byref(tp)))
            records.append({"T": Tc.T.copy(), "converged": bool(conv.value), "iterations": it.value, "evaluations": ev.value, "H": H, "trans_probability": tp.value,
                            "modes": modes[i]})
        return records, schedule
    finally:
        for h in handles:
            L.mrgfe_dbg_ctl_destroy(h)


def schedule_arrays(schedule):
    """(n_pairs, n_items) as the [rounds, 3] arrays of the products' getters"""
    return (np.array([r["n_pairs"] for r in schedule], dtype=np.uint32).reshape(-1, 3), np.array([r["n_items"] for r in schedule], dtype=np.uint32).reshape(-1, 3))


def record_of(rec):
    """a mrgfe_pair_result row as the dict lockstep_replay returns"""
    from mrg_slam_amd.registration import result_matrix

    return {"T": result_matrix(rec), "converged": bool(rec["converged"]), "iterations": int(rec["iterations"]), "evaluations": int(rec["evaluations"]),
            "H": np.array(rec["H"], dtype=np.float64).reshape(6, 6), "trans_probability": float(rec["trans_probability"])}


def f64_fields_equal(a, b):
    return same_bits(a["H"], b["H"]) and same_bits([a["trans_probability"]], [b["trans_probability"]])


def agreement(got, want, modes):
    """The acceptance rule of tests/test_gpu_soak.py::test_soak_all_methods for one alignment against its replay: "exact" — transform, flag, iteration and evaluation
    counts equal bit for bit — or, only where the replayed trajectory holds an f64 Hessian evaluation (kind 2: the device's exp and the C library's may
    differ in the last bit there), "near": within 1e-6 m / rad after the same counts.  Anything else: None."""
    from mrg_slam_amd import synth

    counts = (got["converged"], got["iterations"], got["evaluations"]) == (want["converged"], want["iterations"], want["evaluations"])
    if counts and np.array_equal(got["T"], want["T"]):
        return "exact"
    if counts and 2 in modes:
        dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - want["T"][:3, 3]))
        if dt <= 1e-6 and float(synth.rotation_angle(got["T"], want["T"])) <= 1e-6:
            return "near"
    return None


# ------------------------------------------------------------------------------------------------------------------------
# the batch of the round-plan tests
# ------------------------------------------------------------------------------------------------------------------------
BATCH_EPS = 1e-3  # the pairs leave in different rounds
ROUND_SHAPES = ((2, 8), (3, 5))  # (wg_target, max_ppt): 52 tiles in all, so the first rounds run at the cap and ppt falls as pairs finish


@functools.lru_cache(maxsize=None)
def batch_workload():
    """(targets, [(target index, source, guess)]): the seven pairs of tests/icp_cases.py, sources of 31 to 3000 points against two targets"""
    import icp_cases

    return icp_cases.batch_workload()


@functools.lru_cache(maxsize=None)
def batch_replay(wg_target, max_ppt, forced_ppt=0, first=0, count=None):
    """lockstep_replay of pairs [first, first + count) of batch_workload() as a batch of their own, the GPU-order oracle evaluating: computed once, shared"""
    targets, pairs = batch_workload()
    pairs = pairs[first:first + (len(pairs) - first if count is None else count)]
    evaluate = oracle_evaluators(targets, pairs)
    return lockstep_replay(ndt_params(BATCH_EPS), [len(s) for _, s, _ in pairs], [g for _, _, g in pairs], evaluate, wg_target, max_ppt, forced_ppt)


def schedule_is_live(schedule):
    """(distinct ppt values, rounds with two busy kinds at different ppt) of a replay's own schedule"""
    values = sorted({v for r in schedule for v in r["ppt"] if v})
    split = sum(1 for r in schedule if len({v for v in r["ppt"] if v}) > 1)
    return values, split
