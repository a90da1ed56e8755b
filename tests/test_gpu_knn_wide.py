"""GPU: the wide k-NN search, 65 <= k <= 256 (nn_knn_wide_kernel<R>, R = ceil(k / 64) list entries per lane), against a full sort of all squared
distances by (distance, index) — the library's float expression ((dx*dx + dy*dy) + dz*dz) in numpy, indices and distances compared exactly.  The k
values are the register boundaries; k = 63 and 64 run the narrow kernel on the same clouds under the same assertion."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["clusters", "plane_and_specks", "line", "duplicates", "tiny"]
WIDE_K = [65, 128, 129, 192, 193, 255, 256]
NARROW_K = [63, 64]
K_MAX = 256


def _adversarial_target(rng, kind):
    """the five kinds of tests/test_gpu_filters.py at a few thousand points each"""
    if kind == "clusters":  # dense blobs metres apart: most of the bounding box is empty, far queries cross many empty bricks
        centres = rng.uniform(-40, 40, (12, 3)) * [1, 1, 0.1]
        pts = np.concatenate([c + rng.normal(0, 0.15, (300, 3)) for c in centres])
    elif kind == "plane_and_specks":  # one dense sheet plus isolated points far above it
        sheet = np.c_[rng.uniform(-30, 30, (4000, 2)), rng.normal(0, 0.01, 4000)]
        specks = rng.uniform(-30, 30, (40, 3)) + [0, 0, 45]
        pts = np.concatenate([sheet, specks])
    elif kind == "line":  # degenerate extent along two axes
        pts = np.c_[rng.uniform(-50, 50, 3000), np.zeros(3000), np.zeros(3000)]
    elif kind == "duplicates":  # every point four times: ties must resolve to the lowest index
        base = rng.uniform(-10, 10, (750, 3))
        pts = np.concatenate([base, base, base, base])
    else:  # "tiny"
        pts = rng.uniform(-1, 1, (3, 3))
    out = np.zeros((len(pts), 4), np.float32)
    out[:, :3] = pts
    return out


def full_sort(t, q, ids=None):
    """(indices [nq, K_MAX], squared distances likewise) of the K_MAX nearest of every query by (distance, index), -1 / -1.0 beyond the cloud's size;
    `ids`: the rows of t that count (the finite ones)"""
    ids = np.arange(len(t)) if ids is None else ids
    tx, ty, tz = (t[ids, a].astype(np.float32) for a in range(3))
    idx, sqd = np.full((len(q), K_MAX), -1, np.int32), np.full((len(q), K_MAX), -1.0, np.float32)
    for i in range(len(q)):
        dx, dy, dz = tx - q[i, 0], ty - q[i, 1], tz - q[i, 2]
        d = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((ids, d))[:K_MAX]
        idx[i, : len(order)] = ids[order]
        sqd[i, : len(order)] = d[order]
    return idx, sqd


def assert_rows(got, want, k, rows=None):
    """the first k columns of the full sort, exactly; a row of the full sort ends in -1 / -1.0 where the cloud does"""
    (idx, sqd), (wi, wd) = got, want
    assert idx.shape == sqd.shape and idx.shape[1] == k
    if rows is not None:
        idx, sqd = idx[rows], sqd[rows]
    np.testing.assert_array_equal(idx, wi[:, :k])
    np.testing.assert_array_equal(sqd, wd[:, :k])


@functools.lru_cache(maxsize=None)
def adversarial_case(kind):
    """(cloud, 600 queries, their full sort), computed once for every k"""
    rng = np.random.default_rng({"clusters": 111, "plane_and_specks": 112, "line": 113, "duplicates": 114, "tiny": 115}[kind])
    t = _adversarial_target(rng, kind)
    lo, hi = t[:, :3].min(0), t[:, :3].max(0)
    q = np.zeros((600, 4), np.float32)
    q[:300, :3] = t[rng.integers(0, len(t), 300), :3]                # the cloud's own points (self k-NN)
    q[300:500, :3] = rng.uniform(lo - 1, hi + 1, (200, 3))           # near the box
    q[500:, :3] = rng.uniform(lo - 40, hi + 40, (100, 3))            # far: they climb rings and levels
    for a in (t, q):
        a.setflags(write=False)
    return t, q, full_sort(t, q)


@pytest.mark.parametrize("k", WIDE_K + NARROW_K)
@pytest.mark.parametrize("kind", KINDS)
def test_knn_exact_on_adversarial_clouds(kind, k):
    from mrg_slam_amd import knn

    t, q, want = adversarial_case(kind)
    assert_rows(knn(t, q, k), want, k)


@pytest.mark.parametrize("n,k", [(40, 100), (70, 65), (64, 65), (65, 65), (256, 256), (257, 256), (129, 129), (40, 64)])
def test_clouds_around_k_points(n, k):
    """fewer points than k: rows end in -1 / -1.0; just over k: the list fills exactly once"""
    from mrg_slam_amd import knn

    rng = np.random.default_rng(1000 * n + k)
    t = np.zeros((n, 4), np.float32)
    t[:, :3] = rng.uniform(-3, 3, (n, 3))
    q = np.concatenate([t, np.float32([[50, -20, 3, 0], [0, 0, 0, 0]])])
    got = knn(t, q, k)
    assert_rows(got, full_sort(t, q), k)
    if n < k:
        assert (got[0][:, n:] == -1).all() and (got[1][:, n:] == -1.0).all() and (got[0][:, :n] >= 0).all()


@pytest.mark.parametrize("k", [128, 65, 256, 64])
def test_identical_points_tie_by_index_across_the_register_boundary(k):
    """300 copies of one point: every distance is 0, so a row is 0, 1, 2, ... k - 1 — decided by the index alone, past entry 63 as before it"""
    from mrg_slam_amd import knn

    t = np.tile(np.float32([1.5, -2.25, 0.75, 0.0]), (300, 1))
    q = np.concatenate([t[:5], np.float32([[1.5, -2.25, 0.5, 0], [30, 30, 30, 0]])])
    idx, sqd = knn(t, q, k)
    np.testing.assert_array_equal(idx, np.tile(np.arange(k, dtype=np.int32), (len(q), 1)))
    assert_rows((idx, sqd), full_sort(t, q), k)
    assert (sqd[:5] == 0.0).all()


@functools.lru_cache(maxsize=None)
def scan_case():
    """a quarter of the street scan with specks far from everything, NaN and Inf points; a sample of its own points as rows, fully sorted once"""
    from mrg_slam_amd import synth

    rng = np.random.default_rng(4242)
    t = np.ascontiguousarray(synth.scan_pair(0, "VLP16", synth.street_scene())[0][::4]).copy()
    t[:40, :3] += rng.uniform(-300, 300, (40, 3)).astype(np.float32)
    t[::13, 2] = np.nan
    t[7::101, 0] = np.inf
    fin = np.isfinite(t[:, :3]).all(1)
    ids = np.nonzero(fin)[0]
    sample = np.unique(np.concatenate([rng.choice(ids, 250, replace=False), ids[ids < 40]]))
    t.setflags(write=False)
    return t, fin, sample, full_sort(t, t[sample], ids)


@pytest.mark.parametrize("k", [65, 128, 193, 256, 64])
def test_self_knn_of_a_scan_with_non_finite_points(k):
    from mrg_slam_amd import knn

    t, fin, sample, want = scan_case()
    assert len(t) > 3000 and (~fin).sum() > 100
    idx, sqd = knn(t, t, k)
    assert (idx[~fin] == -1).all() and (sqd[~fin] == -1.0).all()  # non-finite queries get empty rows
    assert (idx[fin][:, 0] >= 0).all()
    assert_rows((idx, sqd), want, k, rows=sample)


@pytest.mark.parametrize("k", [65, 256])
def test_empty_cloud_and_no_queries(k):
    from mrg_slam_amd import knn

    t, q, _ = adversarial_case("line")
    none = np.zeros((0, 4), np.float32)
    idx, sqd = knn(none, q[:70], k)
    assert idx.shape == (70, k) and (idx == -1).all() and (sqd == -1.0).all()
    idx, sqd = knn(t, none, k)
    assert idx.shape == (0, k) and sqd.shape == (0, k)


@pytest.mark.parametrize("k", [257, 0])
def test_k_outside_the_lists_is_refused(k):
    from mrg_slam_amd import MrgfeError, _lib, knn
    from mrg_slam_amd.filters import grid_set_query

    t, q, _ = adversarial_case("tiny")
    for call in (lambda: knn(t, q[:4], k), lambda: grid_set_query([t, t], q[:4], k)):
        with pytest.raises(MrgfeError, match=r"\[1, 256\]") as e:
            call()
        assert e.value.status == _lib.ERR_INVALID


@pytest.mark.parametrize("k", [65, 200])
def test_grids_built_together_answer_wide_queries(k):
    """mrgfe_dbg_grid_set_query: NnGridSet's grids go through the same dispatch"""
    from mrg_slam_amd.filters import grid_set_query

    ta, q, want_a = adversarial_case("clusters")
    tb, _, _ = adversarial_case("duplicates")
    idx, sqd = grid_set_query([ta, tb], q, k)
    assert_rows((idx[0], sqd[0]), want_a, k)
    assert_rows((idx[1], sqd[1]), full_sort(tb, q[:150]), k, rows=np.arange(150))
