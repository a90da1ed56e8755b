"""CPU: the call surface of the statistical chains' switch — ``mrgfe_ctx_set_statistical_chains``, ``mrgfe_ctx_sor_grid_stats``,
``mrgfe_dbg_set_sor_grid_rule`` — declared, exported and bound; what they refuse; the switch and the statistics on a context made without a device
(``mrgfe_dbg_ctx_create_detached``); ``PrefilteringComponent(statistical_chains=...)`` over the oracle's operations."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def detached():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    h = C.c_void_p()
    assert L.mrgfe_dbg_ctx_create_detached(C.byref(h)) == 0 and h.value
    yield h
    L.mrgfe_ctx_destroy(h)


def test_the_symbols_are_declared_exported_and_bound():
    from mrg_slam_amd import Context, _lib

    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    want = {"mrgfe_ctx_set_statistical_chains": [C.c_void_p, C.c_int], "mrgfe_ctx_sor_grid_stats": [C.c_void_p, dp],
            "mrgfe_dbg_set_sor_grid_rule": [C.c_float, C.c_double, C.c_int]}
    for name, args in want.items():
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    assert "mrgfe_dbg_set_sor_grid_rule" in _lib.DEBUG_SIGNATURES
    pub = open(os.path.join(ROOT, "include", "mrgfe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "mrgfe_debug.h")).read()
    assert re.search(r"int\s+mrgfe_ctx_set_statistical_chains\(mrgfe_ctx\* ctx, int on\);", pub)
    assert re.search(r"int\s+mrgfe_ctx_sor_grid_stats\(mrgfe_ctx\* ctx, double out\[6\]\);", pub)
    assert re.search(r"int\s+mrgfe_dbg_set_sor_grid_rule\(float start_edge, double crowding_target, int max_halvings\);", dbg)
    assert "mrgfe_dbg_set_sor_grid_rule" not in pub
    assert inspect.signature(Context.set_statistical_chains).parameters["on"].default is True and callable(Context.sor_grid_stats)


def test_null_arguments_are_refused_with_the_entry_point_s_name(detached):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    out = (C.c_double * 6)(*([-7.0] * 6))
    for call, fn in ((lambda: L.mrgfe_ctx_set_statistical_chains(None, 1), "mrgfe_ctx_set_statistical_chains"),
                     (lambda: L.mrgfe_ctx_sor_grid_stats(None, out), "mrgfe_ctx_sor_grid_stats"), (lambda: L.mrgfe_ctx_sor_grid_stats(detached, None), "mrgfe_ctx_sor_grid_stats")):
        status = call()
        assert status == _lib.ERR_INVALID and _lib.last_error().startswith(fn + ":"), (fn, status, _lib.last_error())
    assert list(out) == [-7.0] * 6  # nothing is written by a refused call


def test_the_switch_and_the_statistics_touch_no_device(detached):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    out = (C.c_double * 6)(*([-7.0] * 6))
    assert L.mrgfe_ctx_sor_grid_stats(detached, out) == 0 and list(out) == [0.0] * 6
    for on in (1, 0, 5, 0):
        assert L.mrgfe_ctx_set_statistical_chains(detached, on) == 0
    try:
        assert L.mrgfe_dbg_set_sor_grid_rule(C.c_float(0.3), C.c_double(1.5), 2) == 0
    finally:
        assert L.mrgfe_dbg_set_sor_grid_rule(C.c_float(0.0), C.c_double(0.0), 0) == 0
    assert L.mrgfe_ctx_sor_grid_stats(detached, out) == 0 and list(out) == [0.0] * 6


def test_the_component_s_option_is_off_by_default_and_does_nothing_to_ops_without_a_context():
    from mrg_slam_amd.prefiltering import OracleOps, PrefilteringComponent
    from oracle import oracle as orc

    assert inspect.signature(PrefilteringComponent.__init__).parameters["statistical_chains"].default is False
    rng = np.random.default_rng(4)
    cloud = np.concatenate([rng.uniform(-6, 6, (1500, 3)), rng.uniform(0, 1, (1500, 1))], 1).astype(np.float32)
    p = {"downsample_method": "APPROX_VOXELGRID", "downsample_resolution": 0.25, "outlier_removal_method": "STATISTICAL", "statistical_mean_k": 20,
         "statistical_stddev": 1.0, "base_link_frame": ""}
    exp = orc.distance_filter(cloud, 0.1, 35.0)
    exp = orc.approx_voxelgrid(exp, 0.25)
    exp, _ = orc.statistical_outlier(exp, 20, 1.0)
    assert 0 < len(exp) < len(cloud)
    got = {}
    for on in (False, True):
        ops = OracleOps(orc)
        comp = PrefilteringComponent(p, ops=ops, statistical_chains=on)
        assert not hasattr(ops, "ctx")
        got[on] = comp.cloud_callback(cloud, 0.0, "velodyne")
        assert np.array_equal(np.asarray(got[on]).view(np.uint32), exp.view(np.uint32)), on
