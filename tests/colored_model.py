"""The bytes of ``prefiltering/colored_points`` (apps/prefiltering_component.cpp:239-257) written down twice, for tests/test_colored_model_cpu.py and
tests/test_gpu_colored_records.py.

The record is the ``pcl::PointXYZRGB`` in memory, which ``pcl::toROSMsg`` copies as it is (fields x@0 y@4 z@8 rgb@16, point_step 32):
bytes 0..11 the bits of x, y, z; 12..15 ``1.0f``; 16 b, 17 g = 128, 18 r, 19 a = 255; 20..31 zero — with ``t = (double)i / (double)n``,
``r = (uint8_t)(255 * t)``, ``b = (uint8_t)(255 * (1 - t))`` in IEEE f64, truncated toward zero.

``colour_bytes`` is the numpy spelling (f64 ``i / n``, ``np.trunc``).  ``colour_bytes_integer`` uses no floating point at all: every f64 operation of
the loop — the division, the subtraction, the two products — is rounded to nearest-even by hand on Python integers, so it holds the first one."""
import numpy as np

SIZES = (1, 2, 51, 255, 256, 257, 765, 4097)
RECORD = 32


def colour_bytes(n):
    """(r, b) of the n points, uint8 arrays"""
    t = np.arange(n, dtype=np.float64) / np.float64(n)
    return np.trunc(255.0 * t).astype(np.uint8), np.trunc(255.0 * (1.0 - t)).astype(np.uint8)


def colour_bytes_reciprocal(n):
    """what multiplying by 1 / n in place of the division gives: NOT the reference's bytes (the CPU test counts where it differs)"""
    t = np.arange(n, dtype=np.float64) * (np.float64(1.0) / np.float64(n))
    return np.trunc(255.0 * t).astype(np.uint8), np.trunc(255.0 * (1.0 - t)).astype(np.uint8)


def _round(num, den):
    """num / den (integers, num >= 0, den > 0) rounded to the nearest f64, ties to even: (q, s) with value q / 2**s, 2**52 <= q < 2**53, or (0, 0).
    Every value here lies in [2**-13, 256], so no overflow, no denormal."""
    if num == 0:
        return 0, 0
    s = 52 - (num.bit_length() - den.bit_length())
    while (num << s if s >= 0 else num >> -s) // den >= 1 << 53:
        s -= 1
    while (num << s) // den < 1 << 52:
        s += 1
    assert s >= 0
    q, rem = divmod(num << s, den)
    if 2 * rem > den or (2 * rem == den and q & 1):
        q += 1
    if q == 1 << 53:
        q, s = q >> 1, s - 1
    return q, s


def _trunc(q, s):
    return q >> s if s >= 0 else q << -s


def colour_bytes_integer(n):
    r, b = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for i in range(n):
        q, s = _round(i, n)                          # t = i / n
        r[i] = _trunc(*_round(255 * q, 1 << s))      # 255 * t
        u, us = _round((1 << s) - q, 1 << s)         # 1 - t
        b[i] = _trunc(*_round(255 * u, 1 << us))     # 255 * (1 - t)
    return r, b


def colored_records(xyz_bits):
    """the n records as bytes; xyz_bits: [n, 3] uint32, the bits of x, y, z as the message holds them"""
    xyz_bits = np.ascontiguousarray(xyz_bits, dtype=np.uint32).reshape(-1, 3)
    n = len(xyz_bits)
    rec = np.zeros((n, RECORD), dtype=np.uint8)
    if n == 0:
        return rec.reshape(-1)
    r, b = colour_bytes(n)
    rec[:, 0:12] = xyz_bits.view(np.uint8).reshape(n, 12)
    rec[:, 12:16] = np.frombuffer(np.float32(1.0).tobytes(), dtype=np.uint8)
    rec[:, 16], rec[:, 17], rec[:, 18], rec[:, 19] = b, 128, r, 255
    return rec.reshape(-1)
