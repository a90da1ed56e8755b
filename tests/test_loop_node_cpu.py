"""CPU: the refusals and no-GPU paths of the node's store calls and of mrgfe_loop_create_node.  mrgfe_node_create opens a device, so nothing here has a real
node: the detector only BORROWS its node and store (it reads neither before a stage runs), which is what lets the paths that queue nothing be checked
with two stand-in addresses.  The checks that need a node are in tests/test_gpu_node_store.py and tests/test_gpu_loop_detect_node.py."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from mrg_slam_amd import _lib

    _lib.build()
    return _lib.lib()


def _loop_params(L, selection=0):
    from mrg_slam_amd import _lib

    cp = _lib.LoopParams()
    L.mrgfe_loop_default_params(C.byref(cp))
    cp.fitness_selection = selection
    return cp


def test_the_new_symbols_resolve_with_their_prototypes(L):
    from mrg_slam_amd import _lib

    for name in ("mrgfe_node_add_target_from_store", "mrgfe_node_add_pair_from_store", "mrgfe_node_clear_pairs", "mrgfe_node_store_stats", "mrgfe_loop_create_node",
                 "mrgfe_dbg_node_set_store_copy"):
        sig = _lib.SIGNATURES.get(name) or _lib.DEBUG_SIGNATURES[name]
        assert getattr(L, name).argtypes == sig[1] and getattr(L, name).restype == sig[0], name


def test_null_handles_are_invalid_arguments(L):
    from mrg_slam_amd import _lib

    out = (C.c_int64 * 4)(7, 7, 7, 7)
    g = np.eye(4, dtype=np.float32)
    fp = g.ctypes.data_as(C.POINTER(C.c_float))
    stand_in = C.create_string_buffer(64)
    some = C.cast(stand_in, C.c_void_p)
    assert L.mrgfe_node_clear_pairs(None) == _lib.ERR_INVALID and b"NULL" in L.mrgfe_last_error()
    assert L.mrgfe_node_store_stats(None, out) == _lib.ERR_INVALID
    assert L.mrgfe_node_store_stats(some, None) == _lib.ERR_INVALID and list(out) == [7, 7, 7, 7]
    assert L.mrgfe_node_add_target_from_store(None, some, 1) == _lib.ERR_INVALID
    assert L.mrgfe_node_add_target_from_store(some, None, 1) == _lib.ERR_INVALID
    assert L.mrgfe_node_add_pair_from_store(None, 0, some, 1, fp) == _lib.ERR_INVALID
    assert L.mrgfe_node_add_pair_from_store(some, 0, None, 1, fp) == _lib.ERR_INVALID
    assert L.mrgfe_node_add_pair_from_store(some, 0, some, 1, None) == _lib.ERR_INVALID
    assert L.mrgfe_dbg_node_set_store_copy(None, 0) == _lib.ERR_INVALID


def test_loop_create_node_refuses_null_arguments_and_a_bad_selection(L):
    from mrg_slam_amd import _lib

    stand_in = C.create_string_buffer(64)
    some = C.cast(stand_in, C.c_void_p)
    cp = _loop_params(L)
    # (unlike mrgfe_loop_create there is no detector over a node without a node and a store)
    for node, store, with_params, with_out in ((None, some, True, True), (some, None, True, True), (some, some, False, True), (some, some, True, False), (None, None, True, True)):
        h = C.c_void_p(1)
        assert L.mrgfe_loop_create_node(node, store, C.byref(cp) if with_params else None, C.byref(h) if with_out else None) == _lib.ERR_INVALID
        assert b"mrgfe_loop_create_node" in L.mrgfe_last_error()
        assert h.value is None or not with_out  # *out is NULL after a refusal
    for bad in (-1, 2, 7):
        cp = _loop_params(L, bad)
        h = C.c_void_p(1)
        assert L.mrgfe_loop_create_node(some, some, C.byref(cp), C.byref(h)) == _lib.ERR_INVALID
        assert b"fitness_selection" in L.mrgfe_last_error() and h.value is None


@pytest.mark.parametrize("selection", [0, 1])
def test_a_detector_over_a_node_without_new_keyframes_finds_nothing_and_queues_nothing(L, selection):
    """n_new == 0, no keyframes, or no candidates: MRGFE_OK with 0 loops before the node is reached"""
    from mrg_slam_amd import _lib

    stand_in = C.create_string_buffer(64)
    some = C.cast(stand_in, C.c_void_p)
    cp = _loop_params(L, selection)
    h = C.c_void_p()
    assert L.mrgfe_loop_create_node(some, some, C.byref(cp), C.byref(h)) == _lib.MRGFE_OK and h.value
    try:
        kf = (_lib.LoopKeyframe * 2)()
        for i, k in enumerate(kf):
            k.key, k.slam_id, k.accum_distance = 11 + i, 1, 100.0 * i
            k.estimate[0] = k.estimate[5] = k.estimate[10] = k.estimate[15] = 1.0
            k.estimate[12] = 1000.0 * i  # 1 km apart: no candidates
        out = (_lib.LoopResult * 2)()
        n = C.c_int(5)
        assert L.mrgfe_loop_detect(h, 1, kf, 0, None, 0, None, out, 2, C.byref(n)) == _lib.MRGFE_OK and n.value == 0
        n = C.c_int(5)
        assert L.mrgfe_loop_detect(h, 0, None, 1, kf, 0, None, out, 2, C.byref(n)) == _lib.MRGFE_OK and n.value == 0
        n = C.c_int(5)
        assert L.mrgfe_loop_detect(h, 1, kf, 1, C.byref(kf[1]), 0, None, out, 2, C.byref(n)) == _lib.MRGFE_OK and n.value == 0
        st = (C.c_int64 * 5)()
        assert L.mrgfe_loop_stats(h, st) == _lib.MRGFE_OK and list(st) == [0, 0, 0, 1, 0]
        assert L.mrgfe_loop_reset(h) == _lib.MRGFE_OK
        assert bytes(stand_in.raw) == bytes(64)  # the stand-ins were never written
    finally:
        L.mrgfe_loop_destroy(h)
