"""GPU: what turns the kernels' sums into a pose — the trial cost of gicp_error_kernel (through mrgfe_gicp_error, the launch the LM loop makes),
gicp_reduce_record over 57 .. 130 block records, the accepted steps of GicpLmController, ICP_HIP's chain of float transformations and the Newton
step of csrc/ndt_ctl.h — against the first-principles models (tests/gicp_analytic.py, tests/ndt_analytic.py), with the inputs, preconditions and
bars of tests/optimiser_cases.py that tests/test_optimiser_steps_cpu.py applies to the oracle.  The parity tests hold kernels and oracle against
each other; a composition side, a re-linearised trial cost or a missing flip that the two share passes those and fails here.

Derived bars: trial costs and records 1e-12 max(|e|, 1) up to 800 terms, 1e-12 n / 800 beyond; descent of the frozen-term cost up to that e bar;
NDT step length in [eps / 2, step_size] (1e-3 relative), pose arithmetic 4 ulp_f32; prefixes and stepping modes exact.
Measured bars, ten times the oracle's figures against the models on the CPU (none is taken from this path):
  step equation  |(H + lambda I) d + b| / |b| per step   small 4.16e-8, 2.05e-6;  large 7.47e-7, 3.73e-5;
                                                         far 2.53e-6, 2.90e-4, 8.15e-3, -, -, 7.11e-3              -> bars 4.16e-7 ... 8.15e-2
                 (far, steps 3 and 4: the oracle's own 0.676 and 0.143 |b| say nothing — not asserted; prefix, descent and termination are)
  damping floor  -lambda / max diag H                    small 1.54e-10, large 9.85e-9, far 2.86e-10                -> bars 1.54e-9, 9.85e-8, 2.86e-9
  ICP chain      max|dT| for maximum_iterations 1 .. 6   4.77e-7, 2.38e-7, 2.38e-7, 4.77e-7, 2.38e-7, 4.77e-7        -> bars 4.77e-6, 2.38e-6 ...
  NDT direction  |delta / |delta| - Newton direction|    2.73e-6                                                    -> bar 2.73e-5
The interior of the More-Thuente line search and the BFGS of PCL_GICP_HIP stay with the oracle comparison (tests/optimiser_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import gicp_cases as gc
import optimiser_cases as oc

pytestmark = pytest.mark.gpu

HIP = gc.Backend("hip")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    oc.report("HIP path")


# ---- 1: the trial cost ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,res", oc.VARIANTS)
@pytest.mark.parametrize("pose", ["small", "large", "far"])
def test_trial_costs(variant, res, pose):
    """(a), (b): the cost at exp(d) T / T exp(d), |d| = 1e-3, 0.05, 0.5, over the terms frozen at T, every source size; at 0.5 the model's cost
    with the correspondences found again, or M frozen again, is another number"""
    for n in gc.SOURCE_SIZES:
        tgt, src, T = oc.pose_case(pose, n)
        oc.check_trial_costs(HIP, variant, tgt, src, T, f"{pose} n={n} res={res}", res=res)


@pytest.mark.parametrize("variant,res", oc.VARIANTS)
def test_trial_costs_with_dropouts(variant, res):
    """a third of the source without a correspondence, NaN and Inf in both clouds: the frozen -1 entries add nothing at any trial pose"""
    tgt, src, T = gc.pair_with_dropouts(res)
    oc.check_trial_costs(HIP, variant, tgt, src, T, f"dropouts res={res}", res=res)


@pytest.mark.parametrize("variant", ["fast", "vgicp"])
@pytest.mark.parametrize("n", oc.MANY_BLOCK_SIZES)
def test_many_block_records(variant, n):
    """(c) 57, 58, 65 and 130 block records: below, at and past the eight-loads-in-flight loop of gicp_reduce_record, linearize and error"""
    oc.check_many_blocks(HIP, variant, n)


def test_trial_cost_needs_a_linearisation():
    """MRGFE_ERR_STATE before anything was linearised and after either cloud was set again; the terms of an alignment serve as well as those of
    mrgfe_gicp_linearize; MRGFE_ERR_INVALID for ICP_HIP and PCL_GICP_HIP; the tap leaves the evaluation count alone"""
    import mrg_slam_amd as M
    from mrg_slam_amd import _lib

    tgt, src = gc.pair(257, gc.SMALL_POSE)
    T = gc.nudged(gc.SMALL_POSE)
    reg = gc.load(M.GicpHip(maximum_iterations=2), tgt, src)
    with pytest.raises(M.MrgfeError) as err:
        reg.error(T)
    assert err.value.status == _lib.ERR_STATE
    H, b, e, n = reg.linearize(T)
    assert reg.error(T) == (pytest.approx(e, rel=1e-13), n)
    for again in (reg.setInputSource, reg.setInputTarget):
        reg.linearize(T)
        again(src if again == reg.setInputSource else tgt)
        with pytest.raises(M.MrgfeError) as err:
            reg.error(T)
        assert err.value.status == _lib.ERR_STATE
    reg.align(T)
    evals = reg.evals
    e1, n1 = reg.error(T)
    assert n1 > 200 and e1 > 0 and reg.evals == evals
    Tc = np.ascontiguousarray(T.T)
    out, cnt = C.c_double(0), C.c_int(0)
    for other in (M.IcpHip(), M.PclGicpHip()):
        gc.load(other, tgt, src)
        other.align(T)
        assert _lib.lib().mrgfe_gicp_error(other._h, Tc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out), C.byref(cnt)) == _lib.ERR_INVALID


# ---- 2: the LM loops --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fast", "small", "vgicp"])
@pytest.mark.parametrize("name", ["small", "large", "far"])
@pytest.mark.parametrize("n", [257, 700])
def test_lm_trajectory(variant, name, n):
    """prefix, step equation, descent and termination over the alignments with maximum_iterations = 1, 2, 3 ..."""
    oc.check_trajectory(HIP, variant, name, n)


@pytest.mark.parametrize("variant", ["fast", "small", "vgicp"])
def test_model_tells_the_composition_sides_apart(variant):
    """from the model alone: the step read on the other side misses the step equation by more than a hundred bars"""
    oc.check_wrong_side_is_told_apart(variant)


@pytest.mark.parametrize("variant", ["fast", "small", "vgicp"])
def test_batch_records_after_three_iterations(variant):
    """pairs of 255, 256 and 257 source points, three outer iterations: the batch's records are the single registrations' bit for bit"""
    import mrg_slam_amd as M
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params, result_matrix

    cls, method = {"fast": (M.GicpHip, _lib.GICP_HIP), "small": (M.SmallGicpHip, _lib.SMALL_GICP_HIP), "vgicp": (M.VgicpHip, _lib.VGICP_HIP)}[variant]
    prm = default_params(method)
    prm.maximum_iterations, prm.transformation_epsilon, prm.rotation_epsilon = 3, 1e-6, 1e-6
    guess = oc.off_guess(gc.LARGE_POSE)
    bm = M.BatchMatcher(prm)
    pairs = [gc.pair(n, gc.LARGE_POSE) for n in (255, 256, 257)]
    t = bm.add_target(pairs[0][0])
    for k, (_, src) in enumerate(pairs):
        bm.add_pair(t, src, np.eye(4))
        bm.set_guess(k, guess)
    res = bm.align(fitness_max_range=float("inf"))
    for k, (tgt, src) in enumerate(pairs):
        reg = gc.load(cls(maximum_iterations=3, transformation_epsilon=1e-6, rotation_epsilon=1e-6), tgt, src)
        reg.align(guess)
        assert reg.getFinalNumIteration() == 2 and not reg.hasConverged()  # three outer iterations were run
        np.testing.assert_array_equal(result_matrix(res[k]), reg.getFinalTransformation())
        assert (int(res[k]["iterations"]), bool(res[k]["converged"]), int(res[k]["evaluations"])) == (2, False, reg.evals)
        np.testing.assert_array_equal(np.array(res[k]["H"]).reshape(6, 6), reg.getHessian())


# ---- 3: ICP -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["near", "changing"])
@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_chain(which, reciprocal):
    """IcpHip(maximum_iterations = m), m = 1 .. 6, against the model's own chain of float poses; "changing": another correspondence set at step 3"""
    oc.check_icp_chain(HIP, which, reciprocal)


# ---- 4: NDT -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,search,res", oc.NDT_CONFIGS)
def test_ndt_newton_steps(kind, search, res):
    """direction, length and pose arithmetic of every step between the alignments with maximum_iterations = 0 .. 5"""
    oc.check_ndt_steps(HIP, kind, search, res)


@pytest.mark.parametrize("kind,search,res", oc.NDT_CONFIGS)
def test_ndt_stepping_modes(kind, search, res):
    """host-stepped, device-stepped and as a 16-pair batch (whose controller runs in ndt_reduce_kernel): the single registration's matrices bit for bit"""
    import mrg_slam_amd as M
    from mrg_slam_amd import _lib
    from mrg_slam_amd.registration import default_params, result_matrix

    single, _ = oc.ndt_runs(HIP, kind, search, res)
    try:
        for host in (1, 0):
            _lib.lib().mrgfe_dbg_set_host_control(host)
            stepped, _ = oc.ndt_runs(HIP, kind, search, res)
            for m, (a, b) in enumerate(zip(single, stepped)):
                assert a[0] == b[0] and a[2] == b[2], f"host control {host}, maximum_iterations {m}: {b[0]} iterations, the single registration {a[0]}"
                np.testing.assert_array_equal(b[1], a[1], err_msg=f"host control {host}, maximum_iterations {m}")
    finally:
        _lib.lib().mrgfe_dbg_set_host_control(-1)
    tgt, src, guess, _ = oc.ndt_case(res)
    for m, (it, T, conv) in enumerate(single):
        prm = default_params(_lib.PCL_NDT_HIP if kind == "pcl" else _lib.NDT_HIP)
        prm.resolution, prm.transformation_epsilon, prm.step_size, prm.maximum_iterations = res, oc.NDT_EPS, oc.NDT_STEP, m
        if kind != "pcl":
            prm.nn_search_method = _lib.SEARCH[search]
        bm = M.BatchMatcher(prm)
        t = bm.add_target(tgt)
        for _ in range(16):
            bm.add_pair(t, src, guess)
        out = bm.align(float("inf"))
        for k in range(16):
            np.testing.assert_array_equal(result_matrix(out[k]), T, err_msg=f"batch pair {k}, maximum_iterations {m}")
            assert (int(out[k]["iterations"]), bool(out[k]["converged"])) == (it, conv)
