"""Placements and a brute-force numpy model for the uniform-grid layer (csrc/nn_grid.hip, nn_device.h, cellsort.hip and the voxel keys of
csrc/filters.hip): searches, the fitness score, the outlier filters and the two voxel grids, restated without any grid.

Nothing here imports the oracle or the product: tests/test_grid_placements_cpu.py holds the oracle to this model, tests/test_gpu_grid_placements.py
the kernels, and tests/test_oracle_filters.py uses the same restatements on ``small_cloud``.

The placements move the four quantities of that layer that scale with coordinate size or extent away from their comfortable values: the binning
slack ``1e-6 (extent + cell)``, the float ``floorf((q - origin) / cell)`` of a query's cell, the 2^24-cell cap with its edge doublings, and the float
product ``floor(x * inv_leaf)`` of the voxel keys.  Each placement is a deterministic function of its seed and returns ``(cloud, queries)``, read-only."""
import functools

import numpy as np

from conftest import small_cloud

DBL_MAX = np.finfo(np.float64).max
INT32_MAX = 2**31 - 1
INT32_MIN = -(2**31)


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def finite_rows(c):
    return np.isfinite(c[:, :3]).all(1)


def sqdist(a, b):
    """float32 squared distances [len(a), len(b)] in FLANN's L2_Simple order: (dx*dx + dy*dy) + dz*dz."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        dz = a[:, None, 2] - b[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def knn(target, queries, k):
    """The k nearest target points of every query by a full sort on (distance, index): (indices int32 [nq, k], squared distances float32 [nq, k]).
    Non-finite target points are no candidates; a row ends in (-1, -1.0) where the target has fewer than k finite points, and a non-finite query's
    row is all (-1, -1.0)."""
    ids = np.nonzero(finite_rows(target))[0]
    qf = finite_rows(queries)
    idx = np.full((len(queries), k), -1, dtype=np.int32)
    sqd = np.full((len(queries), k), -1.0, dtype=np.float32)
    m = min(k, len(ids))
    if m and qf.any():
        D = sqdist(queries[qf], target[ids])
        order = np.argsort(D, axis=1, kind="stable")[:, :m]  # stable: ties go to the lowest index (ids ascends)
        idx[qf, :m] = ids[order]
        sqd[qf, :m] = np.take_along_axis(D, order, 1)
    return idx, sqd


def nn1(target, queries):
    """Exact nearest neighbour: (index, squared distance); (-1, -1.0) for a non-finite query or a target without a finite point."""
    idx, sqd = knn(target, queries, 1)
    return idx[:, 0], sqd[:, 0]


def radius_count(c, radius):
    """Points within the radius of every point, inclusive (sqdist <= r*r in double) and counting the point itself."""
    with np.errstate(invalid="ignore"):
        return (sqdist(c, c).astype(np.float64) <= float(radius) * float(radius)).sum(1)


def radius_outlier(c, radius, min_neighbors):
    """pcl::RadiusOutlierRemoval: (kept cloud, keep mask); non-finite points go."""
    keep = finite_rows(c) & (radius_count(c, radius) >= min_neighbors + 1)
    return c[keep], keep


def statistical_outlier(c, mean_k, stddev_mul):
    """pcl::StatisticalOutlierRemoval with the arithmetic of the reference: float sqrt of the float squared distances of the mean_k nearest other
    points, added in double in neighbour order, the mean rounded to float; float squares, double sums over the cloud in point order; points without a
    search result (non-finite ones) keep distance 0 and pass.  Returns (kept cloud, keep mask, mean distances, threshold)."""
    n = len(c)
    ids = np.nonzero(finite_rows(c))[0]
    dist = np.zeros(n, dtype=np.float32)
    valid = 0
    if len(ids) >= mean_k + 1:
        D = np.sort(np.partition(sqdist(c[ids], c[ids]), mean_k, axis=1)[:, :mean_k + 1], axis=1)[:, 1:]  # (the point itself comes first)
        dist[ids] = (np.cumsum(np.sqrt(D).astype(np.float64), axis=1)[:, -1] / mean_k).astype(np.float32)
        valid = len(ids)
    s = float(np.cumsum(dist.astype(np.float64))[-1]) if n else 0.0
    ss = float(np.cumsum((dist * dist).astype(np.float64))[-1]) if n else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = np.float64(s) / valid + stddev_mul * np.sqrt((np.float64(ss) - np.float64(s) * s / valid) / (np.float64(valid) - 1))
    keep = ~(dist.astype(np.float64) > thr)
    return c[keep], keep, dist, float(thr)


def statistical_margin(c, mean_k, stddev_mul):
    """The smallest relative distance of a finite point's mean distance from the threshold: the model adds in numpy's order, a kernel in its own, so a
    placement is only usable with StatisticalOutlierRemoval when this is well above the rounding of those sums."""
    _, _, dist, thr = statistical_outlier(c, mean_k, stddev_mul)
    if np.isnan(thr):  # fewer than mean_k + 1 finite points: no search succeeds, every distance stays 0 and every point passes
        return float("inf")
    return float(np.abs(dist[finite_rows(c)].astype(np.float64) - thr).min() / thr)


def voxel_cells(c, leaf):
    """floor(x * inverse_leaf) with both in float, as pcl::VoxelGrid and pcl::ApproximateVoxelGrid compute their cells (finite coordinates)."""
    inv = np.float32(1.0) / np.float32(leaf)
    return np.floor(np.asarray(c, dtype=np.float32)[:, :3] * inv).astype(np.int64)


def voxelgrid(c, leaf, min_points=1):
    """pcl::VoxelGrid as a dictionary: (cloud, overflow).  Non-finite points are dropped; centroids are float running sums in point order divided by
    the float count, voxels ascend by their linear index.  Overflow is PCL's 'leaf size is too small' test — dx * dy * dz > INT32_MAX with
    d = int64((max - min) * inverse_leaf) + 1 from the float product, taken here in exact integers — and passes the input through."""
    inv = np.float32(1.0) / np.float32(leaf)
    f = c[finite_rows(c)]
    if len(f) == 0:
        return np.zeros((0, 4), np.float32), False
    lo, hi = f[:, :3].min(0), f[:, :3].max(0)
    d = [int(np.int64((hi[a] - lo[a]) * inv)) + 1 for a in range(3)]
    if d[0] * d[1] * d[2] > INT32_MAX:
        return c.copy(), True
    ijk = voxel_cells(f, leaf)
    mn, mx = np.floor(lo * inv).astype(np.int64), np.floor(hi * inv).astype(np.int64)
    div = mx - mn + 1
    lin = (ijk - mn) @ np.array([1, div[0], div[0] * div[1]])
    cells = {}
    for i, k in enumerate(lin):
        cells.setdefault(int(k), []).append(i)
    out = []
    for k in sorted(cells):
        idx = cells[k]
        if len(idx) < min_points:
            continue
        acc = np.zeros(4, dtype=np.float32)
        for i in idx:
            acc = acc + f[i]  # float32 running sum in point order
        out.append(acc / np.float32(len(idx)))
    return np.asarray(out, dtype=np.float32).reshape(-1, 4), False


def approx_voxelgrid(c, leaf):
    """pcl::ApproximateVoxelGrid as the plain sequential loop over a dict-backed 512-entry history: a point whose entry holds another cell flushes
    that entry's centroid and takes the entry over; the occupied entries are flushed in entry order at the end.  A coordinate that is non-finite or
    beyond the int range after the product gives the cell INT_MIN (the x86 conversion's answer)."""
    inv = np.float32(1.0) / np.float32(leaf)
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor(c[:, :3] * inv).astype(np.float64)
    ok = (fl >= -2147483648.0) & (fl < 2147483648.0)  # (false for NaN)
    cell = np.where(ok, fl, float(INT32_MIN)).astype(np.int64)
    hashes = (cell[:, 0] * 7171 + cell[:, 1] * 3079 + cell[:, 2] * 4231) & 511  # (the low bits of the unsigned 32-bit sum)
    hist, out = {}, []
    for p, ijk, h in zip(c, map(tuple, cell.tolist()), hashes.tolist()):
        e = hist.get(h)
        if e is not None and e[0] != ijk:
            out.append(e[1] / np.float32(e[2]))
            e = None
        if e is None:
            e = [ijk, np.zeros(4, np.float32), 0]
        with np.errstate(invalid="ignore"):  # (inf + -inf in a cell of non-finite points)
            e[1] = e[1] + p
        e[2] += 1
        hist[h] = e
    for h in sorted(hist):
        out.append(hist[h][1] / np.float32(hist[h][2]))
    return np.array(out, dtype=np.float32).reshape(-1, 4)


def distance_filter(c, near, far):
    """PrefilteringComponent::distance_filter: the float norm promoted to double, strictly between the thresholds (a non-finite norm fails both)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(np.float64)
        return c[(d > near) & (d < far)]


def downsample(c, method, leaf):
    if method == "VOXELGRID":
        return voxelgrid(c, leaf, 1)[0]
    if method == "APPROX_VOXELGRID":
        return approx_voxelgrid(c, leaf)
    assert method == "NONE"
    return c


def outlier_removal(c, method, radius=0.5, min_neighbors=2, mean_k=30, stddev_mul=1.0):
    if method == "RADIUS":
        return radius_outlier(c, radius, min_neighbors)[0]
    if method == "STATISTICAL":
        return statistical_outlier(c, mean_k, stddev_mul)[0]
    assert method == "NONE"
    return c


def transform(T, c):
    """The cloud under the pose cast to float, each coordinate ((m2 * z + t) + m1 * y) + m0 * x in float without contraction."""
    M = np.asarray(T, dtype=np.float64).astype(np.float32)
    out = np.array(c, dtype=np.float32)
    x, y, z = (np.asarray(c, dtype=np.float32)[:, a] for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = ((M[r, 2] * z + M[r, 3]) + M[r, 1] * y) + M[r, 0] * x
    return out


def fitness(target, queries, T, max_range=float("inf")):
    """InformationMatrixCalculator::calc_fitness_score: the mean, in double, of the float nearest squared distances of the transformed queries over
    those with d <= max_range — the squared distance against the UN-squared range, the reference's quirk; DBL_MAX when there is none."""
    idx, d = nn1(target, transform(T, queries))
    sel = (idx >= 0) & (d.astype(np.float64) <= max_range)
    return float(d[sel].astype(np.float64).sum() / sel.sum()) if sel.any() else DBL_MAX


def matching_status(target, source, max_correspondence_dist):
    """publish_scan_matching_status for an identity final transformation: (matching error, inlier count, float inlier fraction).  The count is
    strict: sqd < dist * dist with the float distance promoted to double."""
    idx, d = nn1(target, source)
    found = idx >= 0
    err = float(d[found].astype(np.float64).sum() / found.sum()) if found.any() else DBL_MAX
    inliers = int(np.count_nonzero(found & (d.astype(np.float64) < float(max_correspondence_dist) * float(max_correspondence_dist))))
    return err, inliers, np.float32(inliers) / np.float32(len(source))


def voxel_changes(c, leaf):
    """How many finite points fall into another voxel when the float product floor(x * inverse_leaf) is replaced by double arithmetic,
    floor(x / leaf): the sensitivity of a cloud to a kernel that divides instead of multiplying, or that contracts the product into an FMA."""
    f = c[finite_rows(c)]
    exact = np.floor(f[:, :3].astype(np.float64) / float(leaf)).astype(np.int64)
    return int((voxel_cells(f, leaf) != exact).any(1).sum())


# ------------------------------------------------------------------------------------------------------------------------
# the placements
# ------------------------------------------------------------------------------------------------------------------------
N_TARGET, N_QUERY, N_BAD_ROWS = 3000, 300, 20
CROSS_FAR = 2.0e5
# 5e3 m, not 2e4: the 1-NN search of the query midway along the needle walks shells of 64-cell blocks (nn_pyramid_walk, level C) until one reaches the
# blob, and nn_shell_walk enumerates all ~24 s^2 nodes of shell s whatever the grid's width — about s^3 / 2 trips of a lane group for s shells.  The edge
# is 0.25 m here (the 2^24-cell cap is not reached), a block 16 m: 156 shells and 2e6 trips at 5e3 m (1.5 s measured), 625 shells and 1e8 trips at 2e4 m.
# The walk is right, it merely needs longer.  (The k-NN ring walk had the same shape — 12 s per call for the point at the tip — and now skips the slabs of a
# ring above and below the grid: csrc/nn_grid.hip, nn_knn_walk_list.)
NEEDLE_FAR = 5.0e3


def _finish(xyz, seed, extra_queries=()):
    """xyz [n, 3] float32, finite -> (cloud, queries): the first N_TARGET rows give the queries — 100 with 0.3 m of noise, 50 one float up on every
    axis, 50 one float down, 100 exact copies — two queries are made non-finite, N_BAD_ROWS other rows of the cloud get a NaN or an inf."""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, dtype=np.float32)
    assert np.isfinite(xyz).all() and len(xyz) >= N_TARGET
    cloud = np.empty((len(xyz), 4), dtype=np.float32)
    cloud[:, :3] = xyz
    cloud[:, 3] = rng.uniform(0, 1, len(xyz)).astype(np.float32)
    rows = rng.permutation(N_TARGET)
    picks, bad = rows[:N_QUERY], rows[N_QUERY:N_QUERY + N_BAD_ROWS]
    q = cloud[picks].copy()
    q[:100, :3] += rng.normal(0, 0.3, (100, 3)).astype(np.float32)
    q[100:150, :3] = np.nextafter(q[100:150, :3], np.float32(np.inf))
    q[150:200, :3] = np.nextafter(q[150:200, :3], np.float32(-np.inf))
    q[7, 0] = np.nan
    q[93, 1] = np.inf
    if len(extra_queries):
        e = np.zeros((len(extra_queries), 4), dtype=np.float32)
        e[:, :3] = np.asarray(extra_queries, dtype=np.float32)
        q = np.concatenate([q, e])
    cloud[bad, rng.integers(0, 3, N_BAD_ROWS)] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), N_BAD_ROWS)
    cloud.setflags(write=False)
    q.setflags(write=False)
    return cloud, q


def _offset(origin, seed):
    xyz = (small_cloud(N_TARGET, 5)[:, :3].astype(np.float64) + np.asarray(origin, dtype=np.float64)).astype(np.float32)
    return _finish(xyz, seed)


def _lattice(s, shifted, seed):
    """Integer triples in [0, 14)^3 times float32 s: 2000 distinct lattice points and 1000 repeats of them, in random order."""
    rng = np.random.default_rng(seed)
    triples = rng.permutation(14 ** 3)[:2000]
    triples = np.concatenate([triples, rng.choice(triples, N_TARGET - 2000)])[rng.permutation(N_TARGET)]
    ijk = np.stack([triples % 14, (triples // 14) % 14, triples // 196], 1).astype(np.float32)
    xyz = ijk * np.float32(s)
    if shifted:
        xyz = xyz + np.float32(0.1) * np.float32(7)
    return _finish(xyz, seed + 1)


def _lattice_leaf(s, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(-20, 20, (N_TARGET, 3)).astype(np.float32) * np.float32(s)
    return _finish(xyz, seed + 1)


def _blob(sigma, seed):
    return np.random.default_rng(seed).normal(0, sigma, (N_TARGET, 3))


def _cross(seed):
    F = CROSS_FAR
    far = np.array([[F, 0, 0], [-F, 0, 0], [0, F, 0], [0, -F, 0], [0, 0, F], [0, 0, -F]])
    mid = np.array([[F / 2, 0, 0], [0, -F / 2, 0], [0, 0, F / 2]])
    return _finish(np.concatenate([_blob(0.5, seed), far]), seed + 1, np.concatenate([far, mid]))


def _needle(seed):
    far = np.array([[NEEDLE_FAR, 0, 0]])
    return _finish(np.concatenate([_blob(0.5, seed), far]), seed + 1, np.concatenate([far, far / 2]))


def _speck(origin, seed):
    return _finish((_blob(5e-4, seed) + np.asarray(origin, dtype=np.float64)).astype(np.float32), seed + 1)


UTM = (364000.25, 5621000.5, 31.125)
_PLACEMENTS = {
    "offset_utm": lambda: _offset(UTM, 101),
    "offset_neg": lambda: _offset((-1e5, 3e4, 2e3), 102),
    "offset_pow2": lambda: _offset((1024, -2048, 512), 103),
    "lattice_0.5": lambda: _lattice(0.5, False, 111),
    "lattice_0.5_shifted": lambda: _lattice(0.5, True, 113),
    "lattice_0.125": lambda: _lattice(0.125, False, 115),
    "lattice_0.125_shifted": lambda: _lattice(0.125, True, 117),
    "lattice_0.03125": lambda: _lattice(0.03125, False, 119),
    "lattice_0.03125_shifted": lambda: _lattice(0.03125, True, 121),
    "lattice_leaf_0.1": lambda: _lattice_leaf(0.1, 131),
    "lattice_leaf_0.05": lambda: _lattice_leaf(0.05, 133),
    "lattice_leaf_0.025": lambda: _lattice_leaf(0.025, 135),
    "cross": lambda: _cross(141),
    "needle": lambda: _needle(143),
    "speck_origin": lambda: _speck((0, 0, 0), 151),
    "speck_offset": lambda: _speck((100, -50, 20), 153),
}

OFFSETS = ["offset_utm", "offset_neg", "offset_pow2"]
LATTICES = [f"lattice_{s}{t}" for s in ("0.5", "0.125", "0.03125") for t in ("", "_shifted")]
LATTICE_LEAVES = ["lattice_leaf_0.1", "lattice_leaf_0.05", "lattice_leaf_0.025"]
FULL = OFFSETS + LATTICES + ["cross"]                    # every case
SEARCH = FULL + ["needle", "speck_origin", "speck_offset"]  # 1-NN, k-NN, radius and statistical outlier removal
VOXEL = FULL + LATTICE_LEAVES                            # the two voxel grids
# needle is left to brute force alone: the oracle's ring walk visits every cell of every ring along such a grid (minutes once the needle is long)
ORACLE_SEARCH = [p for p in SEARCH if p != "needle"]

KNN_K = [1, 5, 20, 64, 65, 256]
RADIUS_PARAMS = [(0.5, 2), (0.125, 8)]
STATISTICAL_PARAMS = [(10, 1.2), (30, 1.0), (100, 1.0)]
LEAVES = [0.1, 0.37, 0.5]
MIN_POINTS = [1, 3]
MAX_RANGES = [float("inf"), 0.01, 1e-9]
STATISTICAL_MARGIN = 1e-9
# the fused chain: distance filter wide open, the default leaf, the outlier stages' usual parameters
CHAIN_NEAR, CHAIN_FAR, CHAIN_LEAF, CHAIN_STDDEV = 0.0, 1e9, 0.1, 1.0
CHAIN_DOWNSAMPLE = ["VOXELGRID", "APPROX_VOXELGRID", "NONE"]
CHAIN_OUTLIER = [("RADIUS", 30), ("STATISTICAL", 30), ("STATISTICAL", 100), ("NONE", 30)]  # (method, statistical_mean_k)


@functools.lru_cache(maxsize=None)
def placement(name):
    return _PLACEMENTS[name]()


@functools.lru_cache(maxsize=None)
def chain_downsampled(name, method):
    """The placement's cloud after the chain's distance filter and downsample stage (read-only, shared by the outlier cases)."""
    c = downsample(distance_filter(placement(name)[0], CHAIN_NEAR, CHAIN_FAR), method, CHAIN_LEAF)
    c.setflags(write=False)
    return c
