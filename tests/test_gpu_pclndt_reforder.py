"""GPU: PCL_NDT_HIP (and NDT_HIP) with their sums in the REFERENCE's order, opened per context by ``mrgfe_ctx_set_ndt_reference_order``.

pcl::NormalDistributionsTransform (registration_method "NDT" and every unknown name, registrations.cpp:115-129) adds pair after pair on one thread, in
computeDerivatives and in computeHessian.  The default f64 kernels factor a point's voxel sums and add in a tree: 1e-16 relative per sum, which an optimisation
that does not settle amplifies past the 1e-4 bar on 2 of 1200 random scenes.  On a context with the switch on every evaluation and every alignment must equal
``orc.PclNdt(gpu_order=0)`` BIT FOR BIT — all 36 Hessian entries: the reference's Hessian is not symmetric in its last bits.  The switch is set on a context of
this file's own; the one test that needs the default context switches it back off."""
import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 5000)  # one tile of four points and less, around the 128- and 256-point boundaries, many workgroups
RESOLUTIONS = (1.0, 0.6, 2.0)
POSES = (np.array([0.2, -0.05, 0.01, 0.012, -0.006, 0.025]), np.zeros(6), np.array([-0.4, 0.3, 0.05, -0.02, 0.03, -0.1]),  # tests/test_gpu_ndt_reforder.py's three
         np.array([6.0, -4.0, 0.5, 0.0, 0.0, 0.3]))  # ... and one that moves small sources out of every voxel's reach


def _pair(n=6000, seed=0, noise=0.01, m=None):
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    tgt = small_cloud(n, seed)
    rel = synth.make_pose([0.25, -0.1, 0.03], synth.rot_xyz(0.01, -0.008, 0.03))
    src = orc.transform_points(np.linalg.inv(rel), tgt[: m or n])
    src[:, :3] += np.random.default_rng(seed + 1).normal(0, noise, (len(src), 3)).astype(np.float32)
    return tgt, src, rel


@pytest.fixture(scope="module")
def ref_ctx():
    """A context of this file's own with the switch on; switched off again and closed at the end."""
    from mrg_slam_amd import Context

    c = Context(0)
    c.set_ndt_reference_order(True)
    yield c
    c.set_ndt_reference_order(False)
    c.close()


@pytest.fixture(scope="module")
def plain_ctx():
    from mrg_slam_amd import Context

    c = Context(0)
    yield c
    c.close()


_ORACLE_EVALUATIONS = {}


def _oracle_evaluations():
    """{(res, m, pose index, mode): (score, grad, H, the oracle's running mean of neighbours per point after this evaluation)} for the first m points of the
    `_pair(12000, seed=3)` source: computed once for the whole file and never changed."""
    from oracle import oracle as orc

    if not _ORACLE_EVALUATIONS:
        tgt, src, _ = _pair(12000, seed=3)
        for res in RESOLUTIONS:
            for m in SIZES:
                o = orc.PclNdt(gpu_order=0, resolution=res)
                assert o.setInputTarget(tgt) == 0
                o.setInputSource(src[:m])
                for pi, p in enumerate(POSES):
                    T = orc.pose_to_matrix(p)
                    for mode in (0, 1, 2):
                        s, g, H = o.evaluate(T, p, mode)
                        _ORACLE_EVALUATIONS[(res, m, pi, mode)] = (s, g.copy(), H.copy(), o.mean_neighbours)
    return _ORACLE_EVALUATIONS


def _evaluations_not_vacuous(records, default_path_hessian):
    """The preconditions of the bit-identity test, on the oracle's side: without them it could pass on empty sums, on a symmetric Hessian that a mirrored upper
    triangle reproduces, or on a default path that already equals the oracle.  `default_path_hessian`: the 5000-point mode-0 Hessian at resolution 1.0, first
    pose, from a context with the switch OFF."""
    nb_first = {}  # neighbours per point of the first evaluation of each (res, m): the running mean after one evaluation is that evaluation's own
    for (res, m, pi, mode), (_, _, _, mean_nb) in records.items():
        if pi == 0 and mode == 0:
            nb_first[(res, m)] = mean_nb
    far = [records[(1.0, m, 3, 0)] for m in (1, 3, 4, 5)]
    assert all(s == 0.0 and not g.any() and not H.any() for s, g, H, _ in far), "the far pose leaves the small sources without a voxel at resolution 1.0"
    assert all(records[(1.0, m, 3, 0)][0] != 0.0 for m in SIZES if m >= 127), "... and the larger ones with some"
    assert max(nb_first[(res, 1)] for res in RESOLUTIONS) >= 3.0, "a single point with three voxels or more in reach"
    asym = [int((H != H.T).sum()) for (res, m, pi, mode), (_, _, H, _) in records.items() if mode != 1 and H.any()]
    assert asym and min(asym) > 0, "the reference's Hessian differs from its transpose in every evaluation that has a pair"
    oH = records[(1.0, 5000, 0, 0)][2]
    assert (default_path_hessian != oH).any(), "the default path already equals the oracle: the test below would show nothing"


@pytest.mark.parametrize("res", RESOLUTIONS)
@pytest.mark.parametrize("force_hash", ["0", "1"])
def test_every_evaluation_is_bit_identical_to_the_reference_order_oracle(res, force_hash, monkeypatch, ref_ctx, plain_ctx):
    from mrg_slam_amd import PclNdtHip
    from oracle import oracle as orc

    monkeypatch.setenv("MRGFE_FORCE_HASH", force_hash)
    records = _oracle_evaluations()
    tgt, src, _ = _pair(12000, seed=3)
    d = PclNdtHip(resolution=1.0, ctx=plain_ctx)
    assert d.setInputTarget(tgt) == 0
    d.setInputSource(src[:5000])
    _evaluations_not_vacuous(records, d.evaluate(orc.pose_to_matrix(POSES[0]), POSES[0], 0)[2])
    g = PclNdtHip(resolution=res, ctx=ref_ctx)
    assert g.setInputTarget(tgt) == 0
    for m in SIZES:
        g.setInputSource(src[:m])
        nb_sum, n_evals = 0.0, 0
        for pi, p in enumerate(POSES):
            T = orc.pose_to_matrix(p)
            for mode in (0, 1, 2):
                gs, gg, gH = g.evaluate(T, p, mode)
                os_, og, oH, o_mean_nb = records[(res, m, pi, mode)]
                what = (res, m, pi, mode)
                assert gs == os_, what
                np.testing.assert_array_equal(gg, og, err_msg=str(what))
                np.testing.assert_array_equal(gH, oH, err_msg=str(what))  # all 36 entries; zeros where the kind delivers none, on both sides
                nb_sum += g.eval_neighbours / m  # the oracle's own bookkeeping: nb_total / n per evaluation, averaged over the evaluations so far
                n_evals += 1
                assert nb_sum / n_evals == o_mean_nb, what


@pytest.mark.parametrize("eps", [0.1, 1e-4, 1e-6])
@pytest.mark.parametrize("guess_kind", ["identity", "warm", "far"])
def test_alignments_are_bit_identical(eps, guess_kind, ref_ctx):
    from mrg_slam_amd import PclNdtHip, synth
    from oracle import oracle as orc

    tgt, src, rel = _pair(9000, seed=5)
    g = PclNdtHip(transformation_epsilon=eps, maximum_iterations=40, ctx=ref_ctx)
    o = orc.PclNdt(gpu_order=0, transformation_epsilon=eps, maximum_iterations=40)
    assert g.setInputTarget(tgt) == 0 and o.setInputTarget(tgt) == 0
    g.setInputSource(src)
    o.setInputSource(src)
    guess = {"identity": np.eye(4), "warm": synth.warm_guess(rel, 3), "far": synth.make_pose([0.8, 0.5, 0.1], synth.rot_xyz(0.02, 0.01, -0.08)) @ rel}[guess_kind]
    aligned = g.align(guess, want_aligned=True)
    o.align(guess)
    print(eps, guess_kind, "iterations", g.getFinalNumIteration(), o.getFinalNumIteration(), "evaluations", g.evals, o.evals,
          "max |dT|", np.abs(g.getFinalTransformation().astype(np.float64) - o.getFinalTransformation()).max())
    np.testing.assert_array_equal(g.getFinalTransformation(), o.getFinalTransformation())
    assert (g.hasConverged(), g.getFinalNumIteration(), g.evals) == (o.hasConverged(), o.getFinalNumIteration(), o.evals)
    assert g.getTransformationLikelihood() == pytest.approx(o.getTransformationLikelihood(), rel=1e-12)
    # (the two JacobiSVD restatements are not pinned to each other: the pose vector carries ~1e-16 of difference, visible in the last bits of an f64 Hessian
    # evaluated with that pose's angle tables — the bar of tests/test_gpu_ndt_reforder.py)
    np.testing.assert_allclose(g.getHessian(), o.getHessian(), rtol=0, atol=1e-11 * np.abs(o.getHessian()).max())
    np.testing.assert_array_equal(aligned, orc.transform_points(g.getFinalTransformation(), src))


def test_batches_take_the_same_path_in_chunks(monkeypatch, ref_ctx):
    """A batch in reference order is host-stepped; a round's evaluations are cut into launches that fit the record workspace (MRGFE_REF_WORKSPACE_MB).  Nine pairs
    of different sizes against three targets: the records of single registrations, for a roomy workspace and for one that holds a single evaluation at a time."""
    from mrg_slam_amd import BatchMatcher, PclNdtHip, synth
    from mrg_slam_amd._lib import PCL_NDT_HIP
    from mrg_slam_amd.registration import default_params, result_matrix
    from oracle import oracle as orc

    rng = np.random.default_rng(7)
    targets = [small_cloud(5000 + 700 * k, 50 + k) for k in range(3)]
    pairs = []
    for k in range(9):
        t = k % 3
        rel = synth.make_pose(rng.normal(0, 0.25, 3), synth.rot_xyz(*rng.normal(0, 0.02, 3)))
        pairs.append((t, orc.transform_points(np.linalg.inv(rel), targets[t][: 3000 + 211 * k]), synth.perturb_pose(np.eye(4), rng)))
    singles = []
    for t, src, guess in pairs:
        r = PclNdtHip(transformation_epsilon=1e-5, maximum_iterations=30, ctx=ref_ctx)
        r.setInputTarget(targets[t])
        r.setInputSource(src)
        r.align(guess)
        singles.append((r.getFinalTransformation(), r.hasConverged(), r.getFinalNumIteration(), r.evals, r.getHessian(), r.getFitnessScore()))
    assert max(s[2] for s in singles) > 1  # more than PCL's one-iteration regime
    prm = default_params(PCL_NDT_HIP)
    prm.transformation_epsilon, prm.maximum_iterations = 1e-5, 30
    for ws in ("4096", "3"):  # 3 MiB: the smallest job (3000 points, score + gradient) is 750 tiles * 108 slots * 8 rows * 8 B = 5.2 MB -> one job per launch (a job always runs)
        monkeypatch.setenv("MRGFE_REF_WORKSPACE_MB", ws)
        bm = BatchMatcher(prm, ctx=ref_ctx)
        tid = [bm.add_target(t) for t in targets]
        for t, src, guess in pairs:
            bm.add_pair(tid[t], src, guess)
        res = bm.align(float("inf"))
        for r, (T, conv, it, ev, H, fit) in zip(res, singles):
            np.testing.assert_array_equal(result_matrix(r), T)
            assert (bool(r["converged"]), int(r["iterations"]), int(r["evaluations"])) == (conv, it, ev) and r["fitness"] == fit
            np.testing.assert_array_equal(r["H"].reshape(6, 6), H)


def test_the_switch_opens_the_mode_per_context_and_nothing_else_does(monkeypatch, ref_ctx, plain_ctx):
    from mrg_slam_amd import Context, NdtHip, PclNdtHip, synth
    from mrg_slam_amd._lib import lib
    from oracle import oracle as orc

    tgt, src, rel = _pair(6000, seed=5)
    p = POSES[0]
    T = orc.pose_to_matrix(p)
    guess = synth.warm_guess(rel, 3)

    def run(cls, ctx, **kw):
        r = cls(ctx=ctx, **kw)
        assert r.setInputTarget(tgt) == 0
        r.setInputSource(src)
        out = [r.evaluate(T, p, mode) for mode in (0, 1, 2)]
        r.align(guess)
        return out, r.getFinalTransformation(), r.getHessian(), (r.hasConverged(), r.getFinalNumIteration(), r.evals)

    def same(a, b):
        for (s0, g0, H0), (s1, g1, H1) in zip(a[0], b[0]):
            assert s0 == s1
            np.testing.assert_array_equal(g0, g1)
            np.testing.assert_array_equal(H0, H1)
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])
        assert a[3] == b[3]

    ndt_kw = dict(search="KDTREE", transformation_epsilon=0.001, maximum_iterations=64)
    pcl_kw = dict(transformation_epsilon=1e-5, maximum_iterations=30)
    ndt_default, pcl_default = run(NdtHip, plain_ctx, **ndt_kw), run(PclNdtHip, plain_ctx, **pcl_kw)
    # NDT_HIP: the switch is the debug setter's mode
    ndt_switched = run(NdtHip, ref_ctx, **ndt_kw)
    assert lib().mrgfe_dbg_set_ndt_reference_order(1) == 1
    try:
        ndt_dbg = run(NdtHip, plain_ctx, **ndt_kw)
        pcl_dbg = run(PclNdtHip, plain_ctx, **pcl_kw)  # the process-wide setting never touches PCL_NDT_HIP
    finally:
        assert lib().mrgfe_dbg_set_ndt_reference_order(0) == 0
    same(ndt_switched, ndt_dbg)
    assert any((a[2] != b[2]).any() for a, b in zip(ndt_switched[0], ndt_default[0]))  # (and the mode is not the default path)
    same(pcl_dbg, pcl_default)
    np.testing.assert_array_equal(pcl_default[0][0][2], pcl_default[0][0][2].T)  # the default f64 items: an upper triangle, mirrored
    pcl_switched = run(PclNdtHip, ref_ctx, **pcl_kw)
    assert (pcl_switched[0][0][2] != pcl_switched[0][0][2].T).any() and (pcl_switched[0][0][2] != pcl_default[0][0][2]).any()
    # on and off again: the default path's records; a context made like a switched one inherits the switch
    c = Context(0)
    try:
        c.set_ndt_reference_order(True)
        same(run(PclNdtHip, c, **pcl_kw), pcl_switched)
        c.set_ndt_reference_order(False)
        same(run(PclNdtHip, c, **pcl_kw), pcl_default)
        same(run(NdtHip, c, **ndt_kw), ndt_default)
    finally:
        c.close()


@pytest.fixture()
def default_context_in_reference_order():
    from mrg_slam_amd._lib import default_context

    default_context().set_ndt_reference_order(True)
    yield
    default_context().set_ndt_reference_order(False)


def test_reference_order_soak_is_bit_identical_and_inside_the_bar(default_context_in_reference_order):
    """Sixty random scenes (oracle/replay.py pclndt_soak: resolutions 0.5-2 m, eps 0.1-1e-7, 35 or 64 iterations, warm and identity guesses — the kind of scenes of
    which 2 in 1200 leave the bar under the default tree order): in reference order NONE may, and transformation, flags, iteration and evaluation counts must
    be the oracle's bit for bit."""
    from oracle.replay import pclndt_soak

    st = pclndt_soak(60, 31)
    print({k: v for k, v in st.items() if k != "over_bar_cases"})
    assert st["exact"] == st["cases"] and st["over_bar"] == 0, st["over_bar_cases"]
    assert st["flag_or_iteration_mismatch"] == 0 and st["evaluation_count_mismatch"] == 0
    assert st["iterations_total"] > 3 * st["cases"]  # long optimisations are in the sample
