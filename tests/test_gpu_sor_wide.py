"""GPU: StatisticalOutlierRemoval with mean_k = 64 .. 255 (mean_k + 1 neighbours on the wide k-NN kernel) against the CPU oracle, bit for bit and in
order: the filter object, mrgfe_statistical_outlier, the prefilter chains (host-driven, route 0, at either setting of the device-driven switch) and
the scan callback.  mean_k = 256 is refused."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import small_cloud

pytestmark = pytest.mark.gpu

FIELDS = {"x": 0, "y": 4, "z": 8, "intensity": 12}
CHAIN = {"enable_distance_filter": True, "distance_near_thresh": 0.1, "distance_far_thresh": 35.0, "downsample_resolution": 0.1, "downsample_min_points_per_voxel": 1,
         "outlier_removal_method": "STATISTICAL", "statistical_mean_k": 100, "statistical_stddev": 1.0}


@pytest.fixture(scope="module")
def ctx():
    from mrg_slam_amd import Context

    return Context()


@functools.lru_cache(maxsize=None)
def displaced_cloud():
    c = small_cloud(6000, 13)
    c[:10, :3] += 60.0
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def quarter_scan():
    from mrg_slam_amd import synth

    c = np.ascontiguousarray(synth.synth_lidar(synth.street_scene(), np.eye(4), "VLP16", 4711)[::4])
    c.setflags(write=False)
    return c


def statistical_outlier_abi(ctx, c, mean_k, stddev):
    """mrgfe_statistical_outlier itself"""
    from mrg_slam_amd import _lib

    fp = C.POINTER(C.c_float)
    c = np.ascontiguousarray(c, dtype=np.float32)
    out, m = np.empty_like(c), C.c_size_t(0)
    _lib.check(_lib.lib().mrgfe_statistical_outlier(ctx._h, c.ctypes.data_as(fp), len(c), 16, mean_k, stddev, out.ctypes.data_as(fp), C.byref(m)))
    return out[: m.value].copy()


@pytest.mark.parametrize("mean_k,stddev", [(64, 1.2), (100, 1.0), (255, 0.5)])
def test_statistical_outlier_exact(ctx, mean_k, stddev):
    from mrg_slam_amd import StatisticalOutlierRemoval
    from oracle import oracle as orc

    c = displaced_cloud()
    exp, _ = orc.statistical_outlier(c, mean_k, stddev)
    assert 0 < len(exp) < len(c)
    so = StatisticalOutlierRemoval(ctx)
    so.setMeanK(mean_k)
    so.setStddevMulThresh(stddev)
    so.setInputCloud(c)
    np.testing.assert_array_equal(so.filter(), exp)
    np.testing.assert_array_equal(statistical_outlier_abi(ctx, c, mean_k, stddev), exp)


def test_nobody_has_enough_neighbours(ctx):
    """200 points, mean_k = 255: no row of 256 neighbours is complete — the oracle defines what comes out"""
    from mrg_slam_amd import StatisticalOutlierRemoval
    from oracle import oracle as orc

    c = small_cloud(200, 5)
    exp, _ = orc.statistical_outlier(c, 255, 1.0)
    so = StatisticalOutlierRemoval(ctx)
    so.setMeanK(255)
    so.setStddevMulThresh(1.0)
    so.setInputCloud(c)
    np.testing.assert_array_equal(so.filter(), exp)
    np.testing.assert_array_equal(statistical_outlier_abi(ctx, c, 255, 1.0), exp)


def oracle_chain(c, p):
    from oracle import oracle as orc

    c = orc.distance_filter(np.ascontiguousarray(c, dtype=np.float32), p["distance_near_thresh"], p["distance_far_thresh"])
    if p["downsample_method"] == "VOXELGRID":
        c, _ = orc.voxelgrid(c, p["downsample_resolution"], p["downsample_min_points_per_voxel"])
    c, _ = orc.statistical_outlier(c, p["statistical_mean_k"], p["statistical_stddev"])
    return c


@functools.lru_cache(maxsize=None)
def chain_expected(downsample):
    return oracle_chain(quarter_scan(), dict(CHAIN, downsample_method=downsample))


@pytest.mark.parametrize("downsample", ["VOXELGRID", "NONE"])
def test_prefilter_chain_is_host_driven_and_exact(ctx, downsample):
    from mrg_slam_amd import prefilter
    from mrg_slam_amd._lib import lib

    p = dict(CHAIN, downsample_method=downsample)
    exp = chain_expected(downsample)
    assert 1000 < len(exp) < len(quarter_scan())
    try:
        for mode in (1, 0):
            assert lib().mrgfe_dbg_set_prefilter_device_driven(mode) == mode
            got = prefilter(quarter_scan(), p, ctx=ctx)
            assert ctx.prefilter_stats()["route"] == 0, mode
            np.testing.assert_array_equal(got, exp, err_msg=f"switch at {mode}")
    finally:
        lib().mrgfe_dbg_set_prefilter_device_driven(1)


def test_scan_callback_on_the_same_chain(ctx):
    from mrg_slam_amd import scan_callback

    p = dict(CHAIN, downsample_method="VOXELGRID")
    scan = quarter_scan()
    data = memoryview(np.ascontiguousarray(scan)).cast("B")
    got = scan_callback(data, len(scan), 1, 16, FIELDS, 0, None, 0.1, None, p, ctx=ctx)
    assert ctx.prefilter_stats()["route"] == 0
    assert got.tobytes() == chain_expected("VOXELGRID").tobytes()


def test_mean_k_256_is_refused(ctx):
    from mrg_slam_amd import MrgfeError, StatisticalOutlierRemoval, _lib, prefilter

    so = StatisticalOutlierRemoval(ctx)
    so.setMeanK(256)
    so.setInputCloud(displaced_cloud())
    with pytest.raises(MrgfeError, match=r"\[1, 255\]") as e:
        so.filter()
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(MrgfeError, match=r"\[1, 255\]") as e:
        prefilter(quarter_scan(), dict(CHAIN, downsample_method="VOXELGRID", statistical_mean_k=256), ctx=ctx)
    assert e.value.status == _lib.ERR_INVALID
