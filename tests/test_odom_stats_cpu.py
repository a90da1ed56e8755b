"""CPU: mrgfe_odom_stats — the symbol is exported and bound, and NULL arguments are refused before anything is touched (the call needs no GPU)."""
import ctypes as C


def test_the_symbol_is_bound():
    from mrg_slam_amd import HipOdometry, _lib

    fn = _lib.lib().mrgfe_odom_stats
    assert fn.restype is C.c_int and len(fn.argtypes) == 2
    assert callable(HipOdometry.stats)


def test_null_arguments_are_invalid():
    from mrg_slam_amd import _lib

    L = _lib.lib()
    out = (C.c_int64 * 6)(*([7] * 6))
    assert L.mrgfe_odom_stats(None, out) == _lib.ERR_INVALID
    assert list(out) == [7] * 6
    # (a handle needs a registration and so a GPU: the NULL test comes before the handle is read, so any non-NULL address stands for one here)
    stand_in = (C.c_char * 4096)()
    assert L.mrgfe_odom_stats(C.cast(stand_in, C.c_void_p), None) == _lib.ERR_INVALID
    assert b"mrgfe_odom_stats" in L.mrgfe_last_error()
