"""CPU: what the scan egress calls refuse before they touch the device — ``mrgfe_scan_callback_records``, ``mrgfe_prefilter_records``,
``mrgfe_cloud_records_device``, ``mrgfe_ctx_egress_stats`` — held against a context made without a device (``mrgfe_dbg_ctx_create_detached``), and the
call surface of the bindings.  Every refusal is MRGFE_ERR_INVALID with a message and leaves the destination as it was."""
import ctypes as C
import inspect

import numpy as np
import pytest

SENTINEL = 0x5A
N = 10  # points of the stand-in message


@pytest.fixture()
def detached():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    h = C.c_void_p()
    assert L.mrgfe_dbg_ctx_create_detached(C.byref(h)) == 0 and h.value
    yield h
    L.mrgfe_ctx_destroy(h)


def _refused(status, fn):
    from mrg_slam_amd import _lib

    assert status == _lib.ERR_INVALID, status
    msg = _lib.last_error()
    assert fn in msg, msg
    return msg


def _scan_args(n=N):
    from mrg_slam_amd import _lib

    q = _lib.ScanParams()
    _lib.lib().mrgfe_scan_default_params(C.byref(q))
    q.width = n
    data = np.zeros(n * 16, dtype=np.uint8)
    return q, data, data.ctypes.data_as(C.POINTER(C.c_uint8))


def _prefilter_args(n=N):
    from mrg_slam_amd import _lib

    q = _lib.PrefilterParams()
    _lib.lib().mrgfe_prefilter_default_params(C.byref(q))
    cloud = np.ones((n, 4), dtype=np.float32)
    return q, cloud, cloud.ctypes.data_as(C.POINTER(C.c_float))


def _destination(n=N, step=32):
    buf = np.full(n * step, SENTINEL, dtype=np.uint8)
    return buf, buf.ctypes.data_as(C.c_void_p)


def test_the_four_exports_are_bound_and_struct_free():
    """plain pointers, sizes and ints: no structure of the ABI is new"""
    from mrg_slam_amd import Context, _lib, cloud_records_from_device, prefilter_records, scan_callback_records
    from mrg_slam_amd.prefiltering import HipOps, PrefilteringComponent

    L = _lib.lib()
    vp, szp = C.c_void_p, C.POINTER(C.c_size_t)
    want = {"mrgfe_scan_callback_records": [vp, C.POINTER(_lib.ScanParams), C.POINTER(C.c_uint8), C.c_int, vp, C.c_size_t, vp, szp],
            "mrgfe_prefilter_records": [vp, C.POINTER(_lib.PrefilterParams), C.POINTER(C.c_float), C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, vp, szp],
            "mrgfe_cloud_records_device": [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t],
            "mrgfe_ctx_egress_stats": [vp, C.POINTER(C.c_int64)]}
    for name, args in want.items():
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    assert callable(Context.egress_stats)
    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert names(scan_callback_records)[:8] == ["data", "width", "height", "point_step", "fields", "record_step", "out", "dev_ptr"]
    assert names(prefilter_records) == ["cloud", "record_step", "out", "dev_ptr", "params", "ctx"]
    assert names(cloud_records_from_device) == ["dev_ptr", "n", "record_step", "out", "ctx"]
    for f in (HipOps.scan_pointcloud2, PrefilteringComponent.pointcloud2_callback):  # opt-in, default off
        assert inspect.signature(f).parameters["records"].default == 0 and inspect.signature(f).parameters["records_out"].default is None


def test_egress_stats_of_a_fresh_context_are_zero(detached):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    out = (C.c_int64 * 6)(*([7] * 6))
    assert L.mrgfe_ctx_egress_stats(detached, out) == 0 and list(out) == [0] * 6
    out = (C.c_int64 * 6)(*([7] * 6))
    _refused(L.mrgfe_ctx_egress_stats(None, out), "mrgfe_ctx_egress_stats")
    assert list(out) == [7] * 6
    _refused(L.mrgfe_ctx_egress_stats(detached, None), "mrgfe_ctx_egress_stats")
    _refused(L.mrgfe_dbg_ctx_create_detached(None), "mrgfe_dbg_ctx_create_detached")


def test_null_arguments_are_refused(detached):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    q, data, dp = _scan_args()
    buf, bp = _destination()
    m = C.c_size_t(99)
    fn = "mrgfe_scan_callback_records"
    _refused(L.mrgfe_scan_callback_records(None, C.byref(q), dp, 32, bp, buf.nbytes, None, C.byref(m)), fn)
    _refused(L.mrgfe_scan_callback_records(detached, None, dp, 32, bp, buf.nbytes, None, C.byref(m)), fn)
    _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), None, 32, bp, buf.nbytes, None, C.byref(m)), fn)
    _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), dp, 32, None, buf.nbytes, None, C.byref(m)), fn)
    _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), dp, 32, bp, buf.nbytes, None, None), fn)
    p, cloud, cp = _prefilter_args()
    _refused(L.mrgfe_prefilter_records(None, C.byref(p), cp, N, 16, 32, bp, buf.nbytes, None, C.byref(m)), "mrgfe_prefilter")
    _refused(L.mrgfe_prefilter_records(detached, None, cp, N, 16, 32, bp, buf.nbytes, None, C.byref(m)), "mrgfe_prefilter")
    _refused(L.mrgfe_prefilter_records(detached, C.byref(p), None, N, 16, 32, bp, buf.nbytes, None, C.byref(m)), "mrgfe_prefilter")
    _refused(L.mrgfe_prefilter_records(detached, C.byref(p), cp, N, 16, 32, None, buf.nbytes, None, C.byref(m)), "mrgfe_prefilter_records")
    _refused(L.mrgfe_prefilter_records(detached, C.byref(p), cp, N, 16, 32, bp, buf.nbytes, None, None), "mrgfe_prefilter")
    fn = "mrgfe_cloud_records_device"
    stand_in = C.c_void_p(0x1000)  # (never followed: the refusals come first)
    _refused(L.mrgfe_cloud_records_device(None, stand_in, N, 32, bp, buf.nbytes), fn)
    _refused(L.mrgfe_cloud_records_device(detached, None, N, 32, bp, buf.nbytes), fn)
    _refused(L.mrgfe_cloud_records_device(detached, stand_in, N, 32, None, buf.nbytes), fn)
    assert (buf == SENTINEL).all()
    del data, cloud


@pytest.mark.parametrize("step", [0, 8, 24, 64, -32])
def test_other_point_steps_are_refused(detached, step):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    q, data, dp = _scan_args()
    p, cloud, cp = _prefilter_args()
    buf, bp = _destination(step=64)
    m = C.c_size_t(99)
    assert "point_step" in _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), dp, step, bp, buf.nbytes, None, C.byref(m)), "mrgfe_scan_callback_records")
    assert "point_step" in _refused(L.mrgfe_prefilter_records(detached, C.byref(p), cp, N, 16, step, bp, buf.nbytes, None, C.byref(m)), "mrgfe_prefilter_records")
    assert "point_step" in _refused(L.mrgfe_cloud_records_device(detached, C.c_void_p(0x1000), N, step, bp, buf.nbytes), "mrgfe_cloud_records_device")
    assert (buf == SENTINEL).all()
    del data, cloud


@pytest.mark.parametrize("step", [16, 32])
def test_a_capacity_one_byte_short_is_refused_and_the_destination_untouched(detached, step):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    q, data, dp = _scan_args()
    p, cloud, cp = _prefilter_args()
    buf, bp = _destination(step=step)
    m = C.c_size_t(99)
    short = N * step - 1
    assert "capacity_bytes" in _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), dp, step, bp, short, None, C.byref(m)), "mrgfe_scan_callback_records")
    assert "capacity_bytes" in _refused(L.mrgfe_prefilter_records(detached, C.byref(p), cp, N, 16, step, bp, short, None, C.byref(m)), "mrgfe_prefilter_records")
    assert "capacity_bytes" in _refused(L.mrgfe_cloud_records_device(detached, C.c_void_p(0x1000), N, step, bp, short), "mrgfe_cloud_records_device")
    assert (buf == SENTINEL).all()
    del data, cloud


def test_the_refusals_of_the_underlying_calls_are_kept(detached):
    from mrg_slam_amd import _lib

    L = _lib.lib()
    buf, bp = _destination()
    m = C.c_size_t(99)
    q, data, dp = _scan_args()
    q.filters.downsample_method = 7
    assert "unknown method" in _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), dp, 32, bp, buf.nbytes, None, C.byref(m)), "mrgfe_scan_callback_records")
    q, data, dp = _scan_args()
    q.point_step = 18  # not a multiple of 4 on a context without byte layouts
    _refused(L.mrgfe_scan_callback_records(detached, C.byref(q), dp, 32, bp, buf.nbytes, None, C.byref(m)), "mrgfe_scan_callback_records")
    p, cloud, cp = _prefilter_args()
    p.downsample_resolution = 0.0
    assert "downsample_resolution" in _refused(L.mrgfe_prefilter_records(detached, C.byref(p), cp, N, 16, 32, bp, buf.nbytes, None, C.byref(m)), "mrgfe_prefilter")
    # an empty message is MRGFE_OK before anything is asked of the device: *out_n = 0, nothing written, no call counted
    q, data, dp = _scan_args(0)
    assert L.mrgfe_scan_callback_records(detached, C.byref(q), None, 32, bp, 0, None, C.byref(m)) == 0 and m.value == 0
    assert L.mrgfe_cloud_records_device(detached, None, 0, 32, bp, 0) == 0  # (n = 0 asks nothing of the device either)
    assert (buf == SENTINEL).all()
    del data, cloud


def test_the_bindings_refuse_a_bad_destination_before_the_library_sees_it():
    from mrg_slam_amd import cloud_records_from_device, prefilter_records

    class NoCtx:  # nothing of the context is touched
        pass

    cloud = np.ones((N, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="16 or 32"):
        prefilter_records(cloud, 24, ctx=NoCtx())
    with pytest.raises(ValueError, match="records buffer too small"):
        prefilter_records(cloud, 32, np.zeros(N * 32 - 1, dtype=np.uint8), ctx=NoCtx())
    with pytest.raises(ValueError, match="uint8"):
        cloud_records_from_device(0x1000, N, 32, np.zeros((N, 8), dtype=np.float32), ctx=NoCtx())
