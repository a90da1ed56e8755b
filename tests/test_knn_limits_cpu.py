"""CPU: the refusals around the k-NN list's limit of 256 entries that need no device — the C ABI checks these ranges before it touches the context, so
a context that is never dereferenced (a zeroed block of memory) is enough to reach them.  The messages name the accepted range."""
import ctypes as C

import numpy as np
import pytest

FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def untouched_ctx():
    block = C.create_string_buffer(4096)  # only its address is used: every call below returns before the context is read
    return C.cast(block, C.c_void_p), block


def reg_params(method, k):
    from mrg_slam_amd import _lib

    p = _lib.RegParams()
    _lib.lib().mrgfe_reg_default_params(method, C.byref(p))
    p.correspondence_randomness = k
    return p


@pytest.mark.parametrize("method", ["GICP_HIP", "SMALL_GICP_HIP", "VGICP_HIP", "PCL_GICP_HIP", "PCL_GICP_OMP_HIP"])
@pytest.mark.parametrize("k", [257, 3, 0, 1 << 20])
def test_correspondence_randomness_outside_4_256_is_refused(untouched_ctx, method, k):
    from mrg_slam_amd import MrgfeError, _lib

    p = reg_params(getattr(_lib, method), k)
    for create in (_lib.lib().mrgfe_reg_create, _lib.lib().mrgfe_batch_create):
        h = C.c_void_p()
        with pytest.raises(MrgfeError, match=r"correspondence_randomness must be in \[4, 256\]") as e:
            _lib.check(create(untouched_ctx[0], C.byref(p), C.byref(h)))
        assert e.value.status == _lib.ERR_INVALID and not h.value


@pytest.mark.parametrize("k", [257, 3])
def test_methods_without_neighbour_lists_do_not_care(k):
    """ICP_HIP and the NDTs have no covariances: the controllers that run without a device accept any value, as before"""
    from mrg_slam_amd import _lib

    guess = np.eye(4, dtype=np.float32)
    h = C.c_void_p()
    p = reg_params(_lib.ICP_HIP, k)
    assert _lib.lib().mrgfe_dbg_icp_ctl_create(C.byref(p), guess.ctypes.data_as(FP), 10, 10, C.byref(h)) == 0 and h.value
    _lib.lib().mrgfe_dbg_icp_ctl_destroy(h)


@pytest.mark.parametrize("mean_k", [256, 0, -1, 1 << 20])
def test_statistical_outlier_mean_k_outside_1_255_is_refused(untouched_ctx, mean_k):
    from mrg_slam_amd import MrgfeError, _lib

    m = C.c_size_t(7)
    with pytest.raises(MrgfeError, match=r"mean_k must be in \[1, 255\]") as e:
        _lib.check(_lib.lib().mrgfe_statistical_outlier(untouched_ctx[0], None, 0, 16, mean_k, 1.0, None, C.byref(m)))
    assert e.value.status == _lib.ERR_INVALID


@pytest.mark.parametrize("k", [257, 0, -5])
def test_knn_k_outside_1_256_is_refused(untouched_ctx, k):
    from mrg_slam_amd import MrgfeError, _lib

    with pytest.raises(MrgfeError, match=r"k must be in \[1, 256\]") as e:
        _lib.check(_lib.lib().mrgfe_knn(untouched_ctx[0], None, 0, None, 0, 16, k, None, None))
    assert e.value.status == _lib.ERR_INVALID


def test_chain_parameters_name_the_limit(untouched_ctx):
    """statistical_mean_k = 256 in the prefilter parameters: refused by the parameter check of every chain entry point"""
    from mrg_slam_amd import MrgfeError, _lib

    p = _lib.PrefilterParams()
    _lib.lib().mrgfe_prefilter_default_params(C.byref(p))
    p.outlier_removal_method = 2
    p.statistical_mean_k = 256
    m = C.c_size_t(0)
    with pytest.raises(MrgfeError, match=r"statistical_mean_k must be in \[1, 255\]") as e:
        _lib.check(_lib.lib().mrgfe_prefilter(untouched_ctx[0], C.byref(p), None, 0, 16, None, C.byref(m)))
    assert e.value.status == _lib.ERR_INVALID
