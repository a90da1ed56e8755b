"""GPU: exp_float_arg (csrc/dev_exp.h), the exp of the float path of the default NDT derivative kernels, against the device library's exp(double) it restates.

The kernels call it on a float converted to double, so its domain is the 2^32 float bit patterns and the proof is exhaustive: mrgfe_dbg_exp_float_args sweeps
a range of patterns on the device and counts those for which the two doubles differ in any bit (two NaNs are equal).  Sixteen chunks of 2^28 patterns, about
10 ms of device work in all.  The entry point also says how many of its results were zero, subnormal, infinite and NaN, so the test can tell that the sweep
went through every branch of the routine and not, say, sixteen times through one chunk."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNKS, CHUNK = 16, 1 << 28


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


# the regions the sweep must cross, each by one pattern inside it (what the routine does there)
REGIONS = {
    "zero": (_bits(0.0), _bits(-0.0)),                              # t = 0: the polynomial's constant term, exp = 1
    "denormal results": (_bits(-710.0), _bits(-745.0)),             # ldexp into the subnormals (-745.13 < x < -708.39)
    "overflow to infinity": (_bits(710.0), _bits(1025.0), _bits(3.0e38)),  # by ldexp (x > 709.78) and by the x > 1024 select
    "negative arguments below -745": (_bits(-746.0), _bits(-1076.0), _bits(-3.0e38)),  # zero by ldexp and by the x < -1075 select
    "NaN and infinity inputs": (0x7FC00000, 0xFFC00001, 0x7F800001, _bits(np.inf), _bits(-np.inf)),
}


def _count_between(lo, hi):
    """float bit patterns of one sign from pattern lo to pattern hi inclusive (same sign: patterns order like magnitudes)"""
    return hi - lo + 1


def test_exp_float_arg_equals_the_library_exp_on_every_float():
    from mrg_slam_amd import Context
    from mrg_slam_amd._lib import lib

    ctx = Context()
    swept = []
    mismatches, classes = 0, np.zeros(4, dtype=np.uint64)
    first_bad = None
    for c in range(CHUNKS):
        first = c * CHUNK
        bad, where, cls = C.c_uint64(0), C.c_uint32(0), (C.c_uint64 * 4)()
        assert lib().mrgfe_dbg_exp_float_args(ctx._h, first, CHUNK, C.byref(bad), C.byref(where), cls) == 0
        swept.append((first, first + CHUNK - 1))
        mismatches += bad.value
        if bad.value and first_bad is None:
            first_bad = where.value
        classes += np.array(list(cls), dtype=np.uint64)
    zeros, subnormals, infs, nans = (int(v) for v in classes)
    print(f"exp_float_arg vs exp over {CHUNKS} x 2^28 patterns: {mismatches} mismatches; results zero {zeros}, subnormal {subnormals}, infinite {infs}, NaN {nans}")
    assert mismatches == 0, f"first offending float pattern 0x{first_bad:08x}"
    # the chunks tile the 2^32 patterns, and every named region lies inside them
    assert swept[0][0] == 0 and swept[-1][1] == 0xFFFFFFFF and all(a[1] + 1 == b[0] for a, b in zip(swept, swept[1:]))
    for name, patterns in REGIONS.items():
        for p in patterns:
            assert any(lo <= p <= hi for lo, hi in swept), (name, hex(p))
    # ... and the results say the branches were taken.  NaN: exactly the NaN inputs.  The others between what follows from the size of a double alone:
    # exp(x) is zero for every x <= -746 (e^-746 < 2^-1075) and for no x >= -745; infinite for every x >= 710 and no x <= 709; subnormal for every x in
    # [-745, -709] and for no x outside (-746, -708)
    assert nans == 2 * ((1 << 23) - 1)
    neg_inf, pos_inf = _bits(-np.inf), _bits(np.inf)
    assert _count_between(_bits(-746.0), neg_inf) <= zeros <= _count_between(_bits(-745.0), neg_inf) - 1
    assert _count_between(_bits(710.0), pos_inf) <= infs <= _count_between(_bits(709.0), pos_inf) - 1
    assert _count_between(_bits(-709.0), _bits(-745.0)) <= subnormals <= _count_between(_bits(-708.0), _bits(-746.0)) - 2
