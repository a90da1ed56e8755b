"""GPU: the registration handle (mrgfe_reg, the pcl::Registration stand-in) under the call orders its users make, not only
set target -> set source -> align.

PCL's contract: each setter replaces only its own cloud; align, getFitnessScore and the search object see the last target and the
last source that were set.  The odometry hands the aligned scan over as the keyframe (scan_matching_odometry_component.cpp:333,
mrgfe_reg_source_becomes_target) and the loop detector re-targets and re-sources one object many times.  Every result of a
sequence is checked against a fresh handle on a context of its own (bit for bit), against f64 / brute-force references
(fitness, 1-NN, aligned cloud) and, for one sequence per class, against the CPU oracle driven through the same calls.
Everything is drawn from fixed seeds."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSES = ["NdtHip", "PclNdtHip", "GicpHip", "SmallGicpHip", "VgicpHip", "IcpHip", "PclGicpHip"]
NDT_CLASSES = ("NdtHip", "PclNdtHip")
# pool of synthetic street scans (prefiltered, then thinned): sizes differ on purpose. [1] is a few hundred points, [5] is larger than
# every other one, so that a target upload after it has to grow the buffer it lands in.
SIZES = (2500, 300, 4500, 1500, 3500, 8000)
A, B, C_FIT, D, C_GROW = 2, 4, 0, 3, 5  # the named cases: source A, target B, re-target C (fits the spare buffer) or C_GROW (does not)
N_OPS, N_SEEDS = 14, 6
NN_QUERIES = 500
# the per-method oracle tests' bar (test_gpu_ndt.py / test_gpu_pclndt.py::test_align_matches_oracle TOL_T / TOL_R,
# test_gpu_fullsize.py::test_gicp_family_full_size_matches_oracle): 1e-4 m / 1e-4 rad, the same convergence flag and iteration count
TOL_T, TOL_R = 1e-4, 1e-4


def _guesses():
    from mrg_slam_amd import synth

    return [np.eye(4), synth.make_pose([0.2, 0.05, 0.0], synth.rot_xyz(0.0, 0.0, 0.01)), synth.make_pose([-0.3, 0.1, 0.02], synth.rot_xyz(0.002, -0.001, -0.015))]


def _key(cloud):
    return hashlib.sha1(np.ascontiguousarray(cloud).tobytes()).hexdigest() + str(len(cloud))


def _outcome(fn):
    from mrg_slam_amd import MrgfeError

    try:
        return "ok", fn()
    except MrgfeError as e:
        return "err", e.status


@pytest.fixture(scope="module")
def pool():
    import torch

    from mrg_slam_amd import synth
    from oracle import oracle as orc

    scene = synth.street_scene()
    poses = synth.arc_trajectory(len(SIZES) + 2, step=0.4)
    raw = [synth.synth_lidar(scene, poses[k], "VLP16", synth.BASE_SEED + k) for k in range(len(SIZES) + 2)]
    clouds = []
    for k, n in enumerate(SIZES):
        c = orc.distance_filter(raw[k], 0.1, 35.0)
        c, _ = orc.voxelgrid(c, 0.1, 1)
        c, _ = orc.radius_outlier(c, 0.5, 2)
        c, _ = orc.voxelgrid(c, 0.15, 1)
        assert len(c) >= n, (k, len(c), n)
        keep = np.sort(np.random.default_rng(100 + k).choice(len(c), n, replace=False))
        clouds.append(np.ascontiguousarray(c[keep]))
    assert len(clouds[C_GROW]) > max(len(c) for k, c in enumerate(clouds) if k != C_GROW)
    dev = [torch.from_numpy(c).to("cuda:0") for c in clouds]
    torch.cuda.synchronize()
    bad = {"overflow": clouds[D][:100].copy(), "nan": np.full((64, 4), np.nan, np.float32), "empty": np.zeros((0, 4), np.float32)}
    bad["overflow"][0, :3] = (2e5, 2e5, 2e3)  # more than INT32_MAX voxels of 1 m in its bounding box
    return {"clouds": clouds, "dev": dev, "raw": raw[len(SIZES):], "bad": bad}


class Fresh:
    """Fresh handles on a context of their own: what a sequence must reproduce. Align results are memoised per (class, target, source, guess)."""

    def __init__(self):
        from mrg_slam_amd import Context

        self.ctx = Context()
        self.memo = {}

    def handle(self, name, tgt=None, src=None):
        import mrg_slam_amd as M

        r = getattr(M, name)(transformation_epsilon=0.01, ctx=self.ctx)
        if tgt is not None:
            r.setInputTarget(tgt)
        if src is not None:
            r.setInputSource(src)
        return r

    def align(self, name, tgt, src, gi):
        key = (name, _key(tgt), _key(src), gi)
        if key not in self.memo:
            r = self.handle(name, tgt, src)
            aligned = r.align(_guesses()[gi], want_aligned=True)
            self.memo[key] = (r.getFinalTransformation(), r.hasConverged(), r.getFinalNumIteration(), r.getHessian(), aligned)
        return self.memo[key]


@pytest.fixture(scope="module")
def fresh():
    return Fresh()


def _same_align(got, exp, what):
    T, conv, iters, H, aligned = got
    np.testing.assert_array_equal(T, exp[0], err_msg=what)
    assert (conv, iters) == (exp[1], exp[2]), what
    np.testing.assert_array_equal(H, exp[3], err_msg=what)
    if aligned is not None:
        np.testing.assert_array_equal(aligned, exp[4], err_msg=what)


def _align_record(r, gi, want=True):
    aligned = r.align(_guesses()[gi], want_aligned=want)
    return r.getFinalTransformation(), r.hasConverged(), r.getFinalNumIteration(), r.getHessian(), aligned


class Seq:
    """One registration handle driven through a list of ops, with a model of what it must hold: the current target and source clouds
    and the last final transformation.  Every op is checked as it runs; ``log`` keeps what each op returned."""

    def __init__(self, name, ctx, pool, fresh):
        import mrg_slam_amd as M

        self.name, self.ctx, self.pool, self.fresh = name, ctx, pool, fresh
        self.reg = getattr(M, name)(transformation_epsilon=0.01, ctx=ctx)
        self.tgt = self.src = None
        self.T = np.eye(4, dtype=np.float32)
        self.keep = []    # device buffers the handle may still point at
        self.log = []

    def _expect_error(self, op_fn):
        """the outcome of the same call on a fresh handle holding the same inputs"""
        return _outcome(lambda: op_fn(self.fresh.handle(self.name, self.tgt, self.src)))

    def step(self, op):
        import torch

        from mrg_slam_amd import _lib, prefilter_to_device
        from mrg_slam_amd.io import pcl_xyzi_records
        from oracle import oracle as orc

        clouds, dev, reg = self.pool["clouds"], self.pool["dev"], self.reg
        kind, what = op[0], f"{self.name} {op}"
        res = None
        if kind == "tgt":
            _, k, mode = op
            if mode == "host":
                st = reg.setInputTarget(clouds[k])
            elif mode == "rec32":  # the reference's 32-byte pcl::PointXYZI records, gathered on the device
                rec = pcl_xyzi_records(clouds[k])
                st = _lib.check(_lib.lib().mrgfe_reg_set_target(reg._h, rec.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), len(rec), _lib.LAYOUT_PCL_XYZI))
                reg._n_tgt = len(rec)
            else:
                st = reg.setInputTargetDevice(dev[k].data_ptr(), len(clouds[k]))
            assert st == 0, what
            self.tgt = clouds[k]
            res = st
        elif kind == "src":
            _, k, mode = op
            if mode == "host":
                reg.setInputSource(clouds[k])
                self.src = clouds[k]
            elif mode == "device":
                reg.setInputSourceDevice(dev[k].data_ptr(), len(clouds[k]))
                self.src = clouds[k]
            else:  # the prefilter chain on this context leaves the cloud in HBM, the registration takes it with the chain's box
                buf = torch.empty((len(clouds[k]) + 16, 4), dtype=torch.float32, device="cuda:0")
                self.keep.append(buf)
                m = prefilter_to_device(clouds[k], buf.data_ptr(), buf.shape[0], ctx=self.ctx)
                reg.setInputSourceFromPrefilter(buf.data_ptr(), m)
                self.ctx.synchronize()
                self.src = buf[:m].cpu().numpy()
            res = len(self.src)
        elif kind == "promote":
            if self.src is None:
                res = _outcome(reg.sourceBecomesTarget)
                assert res[0] == "err" and res == self._expect_error(lambda r: r.sourceBecomesTarget()), what
            else:
                res = reg.sourceBecomesTarget()
                assert res == 0, what
                self.tgt = self.src
        elif kind == "align":
            _, gi, want = op
            if self.tgt is None or self.src is None:
                res = _outcome(lambda: reg.align(_guesses()[gi], want_aligned=want))
                assert res[0] == "err" and res == self._expect_error(lambda r: r.align(_guesses()[gi])), what
            else:
                res = _align_record(reg, gi, want)
                _same_align(res, self.fresh.align(self.name, self.tgt, self.src, gi), what)
                if want:
                    np.testing.assert_array_equal(res[4], orc.transform_points(res[0], self.src), err_msg=what)
                self.T = res[0]
        elif kind == "fit":
            _, max_range = op
            if self.tgt is None or self.src is None:
                res = _outcome(lambda: reg.getFitnessScore(max_range))
                assert res[0] == "err" and res == self._expect_error(lambda r: r.getFitnessScore(max_range)), what
            else:
                # PCL: mean of the squared 1-NN distances of T_last * source that are <= max_range (squared against un-squared), f64 sum;
                # the bar of test_gpu_fitness_passes.py
                res = reg.getFitnessScore(max_range)
                assert res == pytest.approx(orc.calc_fitness_score(self.tgt, self.src, self.T, max_range), rel=1e-12), what
        elif kind == "nn":
            _, qk = op
            q = orc.transform_points(_guesses()[1], clouds[qk][:NN_QUERIES])
            if self.tgt is None:
                res = _outcome(lambda: reg.nearestKSearch1(q))
                assert res[0] == "err" and res == self._expect_error(lambda r: r.nearestKSearch1(q)), what
            else:
                # exact search: brute force over the current target, a tie going to the lowest index on both sides
                res = reg.nearestKSearch1(q)
                bi, bd = orc.nn1_brute(self.tgt, q)
                np.testing.assert_array_equal(res[1], bd, err_msg=what)
                np.testing.assert_array_equal(res[0], bi, err_msg=what)
        else:
            raise ValueError(op)
        self.log.append((op, res))
        return res


def _ops(seed, n=N_OPS):
    """a seeded op list: set target (host / 32-byte records / device), set source (host / device / from the prefilter), hand-over, align,
    fitness, 1-NN search"""
    rng = np.random.default_rng(seed)
    kinds = ("tgt", "src", "promote", "align", "fit", "nn")
    ops = []
    for _ in range(n):
        kind = kinds[rng.choice(len(kinds), p=[0.2, 0.2, 0.12, 0.24, 0.12, 0.12])]
        k = int(rng.integers(len(SIZES)))
        if kind == "tgt":
            ops.append(("tgt", k, ("host", "rec32", "device")[rng.integers(3)]))
        elif kind == "src":
            ops.append(("src", k, ("host", "device", "prefilter")[rng.integers(3)]))
        elif kind == "promote":
            ops.append(("promote",))
        elif kind == "align":
            ops.append(("align", int(rng.integers(3)), bool(rng.integers(2))))
        elif kind == "fit":
            ops.append(("fit", (float("inf"), 1.0, 0.01)[rng.integers(3)]))
        else:
            ops.append(("nn", k))
    return ops


# ---- a. named regression cases -----------------------------------------------------------------------------------------------------
def _set_src(r, pool, k, resident):
    if resident:
        r.setInputSourceDevice(pool["dev"][k].data_ptr(), len(pool["clouds"][k]))
    else:
        r.setInputSource(pool["clouds"][k])


def _promoted(name, pool, resident):
    """S(A); T(B); align; sourceBecomesTarget — on a context of its own"""
    import mrg_slam_amd as M
    from mrg_slam_amd import Context

    r = getattr(M, name)(transformation_epsilon=0.01, ctx=Context())
    _set_src(r, pool, A, resident)
    assert r.setInputTarget(pool["clouds"][B]) == 0
    first = _align_record(r, 1)
    assert r.sourceBecomesTarget() == 0
    return r, first


@pytest.mark.parametrize("resident", [False, True], ids=["uploaded", "resident"])
@pytest.mark.parametrize("name", CLASSES)
def test_retarget_after_hand_over_keeps_the_source(pool, fresh, name, resident):
    """S(A); T(B); align; hand-over; T(C); align == a fresh handle with target C and source A — with a C that fits the buffer the old
    target left and with a C larger than any cloud the handle has held (its buffer is regrown: the source must not live there)."""
    from oracle import oracle as orc

    cl = pool["clouds"]
    for c in (C_FIT, C_GROW):
        r, first = _promoted(name, pool, resident)
        _same_align(first, fresh.align(name, cl[B], cl[A], 1), f"{name} first align")
        assert r.setInputTarget(cl[c]) == 0
        got = _align_record(r, 1)
        _same_align(got, fresh.align(name, cl[c], cl[A], 1), f"{name} after T({len(cl[c])})")
        np.testing.assert_array_equal(got[4], orc.transform_points(got[0], cl[A]))
        assert r.getFitnessScore() == pytest.approx(orc.calc_fitness_score(cl[c], cl[A], got[0]), rel=1e-12)


@pytest.mark.parametrize("resident", [False, True], ids=["uploaded", "resident"])
@pytest.mark.parametrize("name", CLASSES)
def test_hand_over_then_align_matches_the_source_onto_itself(pool, fresh, name, resident):
    """hand-over; align with no new source: the source aligns onto itself, as PCL does after setInputTarget(input_); twice in a row the
    same; then a device target and a host target after it each leave the source alone."""
    cl, dev = pool["clouds"], pool["dev"]
    r, _ = _promoted(name, pool, resident)
    _same_align(_align_record(r, 2), fresh.align(name, cl[A], cl[A], 2), f"{name} hand-over; align")
    assert r.sourceBecomesTarget() == 0
    _same_align(_align_record(r, 2), fresh.align(name, cl[A], cl[A], 2), f"{name} hand-over twice; align")
    r2, _ = _promoted(name, pool, resident)
    assert r2.sourceBecomesTarget() == 0
    assert r2.setInputTargetDevice(dev[C_FIT].data_ptr(), len(cl[C_FIT])) == 0
    _same_align(_align_record(r2, 1), fresh.align(name, cl[C_FIT], cl[A], 1), f"{name} hand-over; device target")
    assert r2.setInputTarget(cl[C_GROW]) == 0
    _same_align(_align_record(r2, 1), fresh.align(name, cl[C_GROW], cl[A], 1), f"{name} hand-over; device target; host target")


def _bad_targets(name):
    # NDT: PCL's "Leaf size is too small" index overflow and a cloud without a finite point; the GICP family has no failing target — the
    # empty cloud is its degenerate one (test_gpu_gicp.py::test_gicp_family_degenerate_inputs, test_icp_exact_copy_limits_and_degenerate_inputs)
    if name in NDT_CLASSES:
        return ("overflow", "nan")
    return ("empty",) if name != "PclGicpHip" else ()


@pytest.mark.parametrize("resident", [False, True], ids=["uploaded", "resident"])
@pytest.mark.parametrize("name", [c for c in CLASSES if _bad_targets(c)])
def test_failed_target_after_hand_over_keeps_the_source(pool, fresh, name, resident):
    """hand-over; a target that fails: the status and the align outcome a fresh handle gives; then a good target and the source is still A."""
    import mrg_slam_amd as M

    cl = pool["clouds"]
    for bad in _bad_targets(name):
        cloud = pool["bad"][bad]
        r, _ = _promoted(name, pool, resident)
        ref = fresh.handle(name)
        st_ref = ref.setInputTarget(cloud)
        if name in NDT_CLASSES:
            assert st_ref == {"overflow": M._lib.ERR_OVERFLOW, "nan": M._lib.ERR_EMPTY}[bad]
        assert r.setInputTarget(cloud) == st_ref, (name, bad)
        ref.setInputSource(cl[A])
        got, exp = _outcome(lambda: _align_record(r, 1, False)), _outcome(lambda: _align_record(ref, 1, False))
        assert got[0] == exp[0], (name, bad, got, exp)
        if exp[0] == "err":
            assert got == exp
        else:
            np.testing.assert_array_equal(got[1][0], exp[1][0])
            assert got[1][1:3] == exp[1][1:3]
        assert r.setInputTarget(cl[C_FIT]) == 0
        _same_align(_align_record(r, 1), fresh.align(name, cl[C_FIT], cl[A], 1), f"{name} {bad}; good target")


# ---- b. seeded sequences against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_seeded_sequences_follow_the_model(pool, fresh, name):
    from mrg_slam_amd import Context

    for s in range(N_SEEDS):
        seq = Seq(name, Context(), pool, fresh)
        for op in _ops([s, CLASSES.index(name)]):
            seq.step(op)


# ---- c. the oracle driven through the same sequence --------------------------------------------------------------------------------
def _oracle(name):
    from oracle import oracle as orc

    return {"NdtHip": lambda: orc.Ndt(transformation_epsilon=0.01, num_threads=4), "PclNdtHip": lambda: orc.PclNdt(transformation_epsilon=0.01),
            "GicpHip": lambda: orc.FastGicp(transformation_epsilon=0.01, num_threads=4), "SmallGicpHip": lambda: orc.SmallGicp(transformation_epsilon=0.01, num_threads=1),
            "VgicpHip": lambda: orc.FastVgicp(transformation_epsilon=0.01, num_threads=1), "IcpHip": lambda: orc.Icp(transformation_epsilon=0.01),
            "PclGicpHip": lambda: orc.PclGicp(transformation_epsilon=0.01, num_threads=4)}[name]()


@pytest.mark.parametrize("name", CLASSES)
def test_oracle_follows_the_same_sequence(pool, fresh, name):
    """A handle and a fresh handle could share one wrong answer: the oracle, driven through the same calls (a hand-over is
    setInputTarget(the current source)), must give each align's result at the per-method oracle tests' bar."""
    from mrg_slam_amd import Context, synth

    seq = Seq(name, Context(), pool, fresh)
    o = _oracle(name)
    have_t = have_s = False
    n_aligns = 0
    for op in _ops([0, CLASSES.index(name)]) + [("src", A, "host"), ("tgt", B, "host"), ("align", 1, False), ("promote",), ("align", 0, False)]:
        seq.step(op)
        if op[0] == "tgt" or (op[0] == "promote" and seq.src is not None):
            o.setInputTarget(seq.tgt)
            have_t = True
        elif op[0] == "src":
            o.setInputSource(seq.src)
            have_s = True
        elif op[0] == "align" and have_t and have_s:
            o.align(_guesses()[op[1]])
            T, conv, iters = seq.log[-1][1][:3]
            To = o.getFinalTransformation()
            assert np.linalg.norm(T[:3, 3].astype(np.float64) - To[:3, 3]) <= TOL_T and synth.rotation_angle(T, To) <= TOL_R, (name, op, T, To)
            assert (conv, iters) == (o.hasConverged(), o.getFinalNumIteration()), (name, op)
            n_aligns += 1
    assert n_aligns >= 2


# ---- d. handles that share a context -----------------------------------------------------------------------------------------------
SHARED = ("SmallGicpHip", "NdtHip", "PclGicpHip")


def _shared_ops(i):
    return [("src", A, "prefilter"), ("tgt", B, "device"), ("align", 1, True)] + _ops([50 + i, 7], N_OPS - 3)


def _same_log(a, b, what):
    assert len(a) == len(b), what
    for (op, x), (op2, y) in zip(a, b):
        assert op == op2
        if isinstance(x, tuple) and x and isinstance(x[0], np.ndarray):
            for u, v in zip(x, y):
                if isinstance(u, np.ndarray):
                    np.testing.assert_array_equal(u, v, err_msg=f"{what} {op}")
                else:
                    assert u == v, (what, op)
        else:
            assert x == y, (what, op, x, y)


def test_handles_sharing_a_context_answer_like_handles_alone(pool, fresh):
    """Three registrations on one Context (what the adapter's shared_context(device, role) gives every registration of a role), their
    sequences interleaved op by op, with a prefilter pass and a floor detection on that context between a set and an align: every result
    is bit-identical to the same sequence on a context of its own."""
    import torch

    from mrg_slam_amd import Context, FloorDetection, prefilter_to_device

    solo = []
    for i, name in enumerate(SHARED):
        s = Seq(name, Context(), pool, fresh)
        for op in _shared_ops(i):
            s.step(op)
        solo.append(s)
    ctx = Context()
    shared = [Seq(name, ctx, pool, fresh) for name in SHARED]
    raw = pool["raw"]
    scratch = torch.empty((max(len(x) for x in raw) + 16, 4), dtype=torch.float32, device="cuda:0")
    floor = FloorDetection(ctx=ctx)
    side = 0
    op_lists = [_shared_ops(i) for i in range(len(SHARED))]
    for j in range(N_OPS):
        for s, ops in zip(shared, op_lists):
            if ops[j][0] == "align":
                x = raw[side % len(raw)]
                side += 1
                prefilter_to_device(x, scratch.data_ptr(), scratch.shape[0], ctx=ctx)
                floor.detect(x, want_clouds=False)
            s.step(ops[j])
    assert side >= 3
    for a, b in zip(shared, solo):
        _same_log(a.log, b.log, a.name)
