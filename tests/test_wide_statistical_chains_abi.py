"""CPU: the call surface of the wide statistical chains' switch — ``mrgfe_ctx_set_wide_statistical_chains`` and its read-back
``mrgfe_dbg_wide_statistical_chains`` — declared, exported and bound; what they refuse; the switch set and read on a context made without a device
(``mrgfe_dbg_ctx_create_detached``); ``PrefilteringComponent(wide_statistical_chains=...)`` over the oracle's operations."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mrgfe_ctx_set_wide_statistical_chains"


@pytest.fixture()
def detached():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    h = C.c_void_p()
    assert L.mrgfe_dbg_ctx_create_detached(C.byref(h)) == 0 and h.value
    yield h
    L.mrgfe_ctx_destroy(h)


def test_the_symbol_is_declared_exported_and_bound():
    from mrg_slam_amd import Context, _lib

    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int]
    assert NAME in _lib.SIGNATURES and NAME not in _lib.DEBUG_SIGNATURES and "mrgfe_dbg_wide_statistical_chains" in _lib.DEBUG_SIGNATURES
    pub = open(os.path.join(ROOT, "include", "mrgfe.h")).read()
    dbg = open(os.path.join(ROOT, "include", "mrgfe_debug.h")).read()
    assert re.search(r"int\s+mrgfe_ctx_set_wide_statistical_chains\(mrgfe_ctx\* ctx, int on\);", pub)
    assert re.search(r"int\s+mrgfe_dbg_wide_statistical_chains\(mrgfe_ctx\* ctx, int\* on, int\* inherited\);", dbg)
    assert "mrgfe_dbg_wide_statistical_chains" not in pub
    assert inspect.signature(Context.set_wide_statistical_chains).parameters["on"].default is True


def test_a_null_context_is_refused_with_the_entry_point_s_name():
    from mrg_slam_amd import _lib

    status = _lib.lib().mrgfe_ctx_set_wide_statistical_chains(None, 1)
    assert status == _lib.ERR_INVALID and _lib.last_error().startswith(NAME + ":"), (status, _lib.last_error())


def test_the_switch_touches_no_device_and_leaves_its_neighbour_alone(detached):
    from mrg_slam_amd import _lib

    L = _lib.lib()

    def held():
        on = C.c_int(-7)
        assert L.mrgfe_dbg_wide_statistical_chains(detached, C.byref(on), None) == 0
        return on.value

    assert held() == 0  # off by default
    for on in (1, 0, 5, 0, 1):
        assert L.mrgfe_ctx_set_wide_statistical_chains(detached, on) == 0
        assert held() == (1 if on else 0), on
    assert L.mrgfe_ctx_set_statistical_chains(detached, 1) == 0 and L.mrgfe_ctx_set_statistical_chains(detached, 0) == 0
    assert held() == 1  # (the neighbouring switch is another one)
    out = (C.c_double * 6)(*([-7.0] * 6))
    assert L.mrgfe_ctx_sor_grid_stats(detached, out) == 0 and list(out) == [0.0] * 6
    assert L.mrgfe_dbg_wide_statistical_chains(None, C.byref(C.c_int()), None) == _lib.ERR_INVALID
    assert L.mrgfe_dbg_wide_statistical_chains(detached, None, None) == _lib.ERR_INVALID


def test_the_component_s_option_is_off_by_default_and_does_nothing_to_ops_without_a_context():
    from mrg_slam_amd.prefiltering import OracleOps, PrefilteringComponent
    from oracle import oracle as orc

    par = inspect.signature(PrefilteringComponent.__init__).parameters
    assert par["wide_statistical_chains"].default is False and par["statistical_chains"].default is False
    rng = np.random.default_rng(4)
    cloud = np.concatenate([rng.uniform(-6, 6, (1500, 3)), rng.uniform(0, 1, (1500, 1))], 1).astype(np.float32)
    p = {"downsample_method": "VOXELGRID", "downsample_resolution": 0.25, "outlier_removal_method": "STATISTICAL", "statistical_mean_k": 100,
         "statistical_stddev": 1.0, "base_link_frame": ""}
    exp = orc.distance_filter(cloud, 0.1, 35.0)
    exp, _ = orc.voxelgrid(exp, 0.25, 1)
    exp, _ = orc.statistical_outlier(exp, 100, 1.0)
    assert 0 < len(exp) < len(cloud)
    for on in (False, True):
        ops = OracleOps(orc)
        comp = PrefilteringComponent(p, ops=ops, wide_statistical_chains=on)
        assert not hasattr(ops, "ctx")
        got = comp.cloud_callback(cloud, 0.0, "velodyne")
        assert np.array_equal(np.asarray(got).view(np.uint32), exp.view(np.uint32)), on
