"""CPU: the yardstick of tests/test_gpu_colored_records.py is itself held — the numpy model of the colour bytes of ``prefiltering/colored_points``
(tests/colored_model.py: f64 ``i / n``, ``np.trunc``) against a second spelling that uses no floating point (every f64 operation rounded to
nearest-even on integers), and against the exact quotient wherever truncation cannot depend on the rounding."""
import numpy as np
import pytest

import colored_model as cm


@pytest.mark.parametrize("n", cm.SIZES + (85, 510))
def test_numpy_model_equals_the_integer_spelling(n):
    r, b = cm.colour_bytes(n)
    ri, bi = cm.colour_bytes_integer(n)
    assert np.array_equal(r, ri) and np.array_equal(b, bi)
    assert r[0] == 0 and b[0] == 255 and int(r.max()) <= 254
    # where 255 * i / n is no integer it is at least 1 / n away from one, the two roundings move it by 2^-44 at the most: the byte is the exact floor
    i = np.arange(n, dtype=np.int64)
    inexact = (255 * i) % n != 0
    assert np.array_equal(r[inexact], ((255 * i) // n)[inexact].astype(np.uint8))
    # where it is an integer k the byte is k or k - 1 (the rounded quotient may lie below i / n)
    k = ((255 * i) // n)[~inexact]
    assert ((r[~inexact] == k) | (r[~inexact] == k - 1)).all()


def test_a_reciprocal_is_not_the_division():
    """multiplying by 1 / n changes red bytes: the kernel must divide"""
    changed = {n: int((cm.colour_bytes(n)[0] != cm.colour_bytes_reciprocal(n)[0]).sum()) for n in (51, 85, 255, 510, 765)}
    assert changed == {51: 3, 85: 9, 255: 24, 510: 24, 765: 103}, changed


def test_record_layout():
    bits = np.array([[0x3F800000, 0x7FC01234, 0xFF800000], [1, 2, 3]], dtype=np.uint32)
    rec = cm.colored_records(bits).reshape(2, 32)
    assert rec[:, 0:12].tobytes() == bits.tobytes()
    assert rec[:, 12:16].tobytes() == np.array([1.0, 1.0], dtype=np.float32).tobytes()
    assert rec[0, 16:20].tolist() == [255, 128, 0, 255] and rec[1, 16:20].tolist() == [127, 128, 127, 255]
    assert not rec[:, 20:].any()
    assert cm.colored_records(np.zeros((0, 3), dtype=np.uint32)).size == 0
