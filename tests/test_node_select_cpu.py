"""CPU: the bounded selection's new entry points (mrgfe_node_align_best, mrgfe_node_select_stats, mrgfe_dbg_node_fit_bounds,
mrgfe_batch_align_best_async) refuse NULL arguments with MRGFE_ERR_INVALID and a message, and the Python call surface has the documented shape."""
import ctypes as C
import inspect

import numpy as np


def _arrays(n=2):
    from mrg_slam_amd import _lib

    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    res = (_lib.PairResult * n)()
    i32 = [np.zeros(n, dtype=np.int32) for _ in range(3)]
    f64 = np.zeros(8)
    return res, [a.ctypes.data_as(ip) for a in i32], f64.ctypes.data_as(dp), (i32, f64)


def _refused(status):
    from mrg_slam_amd import _lib

    assert status == _lib.ERR_INVALID
    assert _lib.last_error()
    return _lib.last_error()


def test_null_node_is_refused_by_the_three_node_calls():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    res, (group, state, best), score, keep = _arrays()
    assert "mrgfe_node_align_best" in _refused(L.mrgfe_node_align_best(None, float("inf"), 1.0, group, 1, res, state, best, score))
    assert "mrgfe_node_select_stats" in _refused(L.mrgfe_node_select_stats(None, score))
    assert "mrgfe_dbg_node_fit_bounds" in _refused(L.mrgfe_dbg_node_fit_bounds(None, score, score))
    del keep


def test_null_arguments_are_refused_without_a_gpu():
    """(a node or a batch cannot be made without a GPU: a handle that is never followed stands in where another argument is the NULL one)"""
    from mrg_slam_amd import _lib

    L = _lib.lib()
    res, (group, state, best), score, keep = _arrays()
    fake = C.c_void_p(0x1000)
    assert "mrgfe_node_select_stats" in _refused(L.mrgfe_node_select_stats(fake, None))
    assert "mrgfe_dbg_node_fit_bounds" in _refused(L.mrgfe_dbg_node_fit_bounds(fake, None, score))
    assert "mrgfe_dbg_node_fit_bounds" in _refused(L.mrgfe_dbg_node_fit_bounds(fake, score, None))
    # n_groups > 0 without best / best_score, and a negative n_groups: checked before the node is looked at
    assert "mrgfe_node_align_best" in _refused(L.mrgfe_node_align_best(fake, float("inf"), 1.0, group, 1, res, state, None, score))
    assert "mrgfe_node_align_best" in _refused(L.mrgfe_node_align_best(fake, float("inf"), 1.0, group, 1, res, state, best, None))
    assert "mrgfe_node_align_best" in _refused(L.mrgfe_node_align_best(fake, float("inf"), 1.0, group, -1, res, state, best, score))
    assert "mrgfe_batch_align_best" in _refused(L.mrgfe_batch_align_best_async(None, float("inf"), 1.0, group, 1, res, state, best, score))
    del keep


def test_the_matchers_have_the_documented_methods():
    from mrg_slam_amd import BatchMatcher, NodeMatcher

    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(NodeMatcher.align_best) == names(BatchMatcher.align_best) == ["self", "max_range", "group", "score_cap"]
    assert names(BatchMatcher.align_best_async) == ["self", "max_range", "group", "score_cap"]
    for f in (NodeMatcher.align_best, BatchMatcher.align_best_async):
        assert inspect.signature(f).parameters["score_cap"].default is None
    assert names(NodeMatcher.select_stats) == names(NodeMatcher.fit_bounds) == ["self"]
    assert callable(BatchMatcher.wait)
