"""First-principles model of the NDT target build (pcl / pclomp VoxelGridCovariance) in numpy — an INDEPENDENT check of the voxel
statistics, written from the definition and not from oracle/ndt.cpp or csrc/ndt_build.hip:

* the cell of a point: PCL's VoxelGrid indexing, the ONE place where float arithmetic is part of the specification (``cell_of``);
* per leaf: count, mean and covariance, centred and two-pass in longdouble, the covariance scaled by (n-1)/n after the 1/n form (PCL's
  stated quirk), eigenvalues from np.linalg.eigh floored at 0.01 * lambda_max, the rebuilt covariance and its inverse;
* a class per leaf that says what the model can predict about the library's accept / reject decision (``CLASSES``);
* the reference's own error (``single_pass_reference``): the single-pass formula (sum xx^T - 2 sum x mean^T) / n + mean mean^T in plain
  float64, sums added in point order, put through the same eigh / floor / inverse — its deviation from the centred model is what the
  tolerances of tests/test_ndt_leaves_cpu.py and tests/test_gpu_ndt_leaves.py are taken from;
* ``scene``: constructed clouds with one voxel per leaf kind (regular, thin plane, exact plane, exact line, duplicates) and size.
"""
import numpy as np

MIN_POINTS = 6            # pclomp / PCL min_points_per_voxel_
EIG_FLOOR = 0.01          # min_covar_eigvalue_mult_
PCL_NEG_EIG_TOL = 1e-12   # pcl::VoxelGridCovariance (PCL 1.12) tolerates eigenvalues down to -1e-12 (the libraries: or the covariance's rounding noise, if
                          # that is larger); pclomp's fork tests w < 0

# class -> what the model predicts for (pclomp rule, PCL rule): True accepted, False rejected, None no prediction
CLASSES = {
    "few": (False, False),            # n < 6: zero inverse covariance, never in the voxel lookup
    "regular": (True, True),          # lambda_min >= 0.01 lambda_max: accepted, the floor is inactive
    "thin": (True, True),             # 1e-9 lambda_max < lambda_min < 0.01 lambda_max: accepted, compared against the floored rebuild
    "point": (False, False),          # lambda_max == 0 (all points equal): rejected (lambda_max <= 0)
    "rank_deficient": (None, True),   # exact plane / line, lambda_min <= 1e-12 lambda_max: the sign of a rounding-noise eigenvalue decides under
                                      # pclomp's rule (w < 0), PCL's tolerance accepts; an accepted one is compared against the floored rebuild,
                                      # which is unique (every null direction gets the same floor)
    "marginal": (None, None),         # 1e-12 < lambda_min / lambda_max <= 1e-9: no prediction (the scenes hold none)
}


def cell_of(xyz, leaf, rule="build"):
    """(float-rule cell, exact-arithmetic cell) of each point, N x 3 int64 each.

    THE NAMED QUIRK: PCL computes the cell in FLOAT arithmetic.  The leaf size is a float; the build (applyFilter) multiplies the float coordinate by
    the float inverse leaf size, floor(f32(p) * f32(1 / leaf)); the neighbourhood lookup of a query point (getNeighborhoodAtPoint, rule="lookup")
    divides instead, floor(f32(p) / f32(leaf)).  Either can differ from the exact cell floor(p / leaf) (p and leaf the float values, the quotient in
    exact arithmetic) for a point on or next to a cell face when the leaf is no power of two — the second value returned, so that a test can count
    such points."""
    x = np.asarray(xyz, dtype=np.float32)
    lf = np.float32(leaf)
    if rule == "build":
        fl = np.floor(x * (np.float32(1.0) / lf))
    else:
        fl = np.floor(x / lf)
    assert fl.dtype == np.float32
    # exact: floor(p / leaf) with a correction by exact products (k * leaf is exact in float64 for |k| < 2^29: 24 + 29 bits)
    p, l = x.astype(np.float64), float(lf)
    with np.errstate(invalid="ignore"):
        k = np.floor(p / l)
        k = np.where(k * l > p, k - 1, k)
        k = np.where((k + 1) * l <= p, k + 1, k)
        fin = np.isfinite(x)
        return np.where(fin, fl, 0).astype(np.int64), np.where(fin, k, 0).astype(np.int64)


def grid_of(xyz, leaf):
    """finite mask, cells (float rule), min_b, max_b, div_b, linear key of every finite point"""
    x = np.asarray(xyz, dtype=np.float32)[:, :3]
    fin = np.isfinite(x).all(1)
    ijk, _ = cell_of(x[fin], leaf)
    min_b, max_b = ijk.min(0), ijk.max(0)
    div_b = max_b - min_b + 1
    key = (ijk - min_b) @ np.array([1, div_b[0], div_b[0] * div_b[1]], dtype=np.int64)
    return fin, ijk, min_b, max_b, div_b, key


def _floored_inverse(cov):
    """eigenvalues (ascending, unfloored), floored rebuild V D V^T and its inverse V D^-1 V^T"""
    w, V = np.linalg.eigh(cov)
    if w[2] <= 0:
        return w, np.zeros((3, 3)), np.zeros((3, 3))
    wf = np.maximum(w, EIG_FLOOR * w[2])
    return w, (V * wf) @ V.T, (V / wf) @ V.T


def _classify(n, w):
    if n < MIN_POINTS:
        return "few"
    if w[2] <= 0:
        return "point"
    r = w[0] / w[2]
    if r <= 1e-12:
        return "rank_deficient"
    if r <= 1e-9:
        return "marginal"
    return "thin" if r < EIG_FLOOR else "regular"


class Leaves:
    """keys ascending; n; mean (float64 of the longdouble mean); cov (centred, (n-1)/n scaled, unfloored); lam (its eigenvalues); cov_reg / icov
    (floored rebuild and inverse; zero for `few` and `point`); cls; centroid (the FLOAT centroid the radius search sees: float sum in point order
    over float(n)); grid = (min_b, max_b, div_b); point_key (key of every input point, -1 for a skipped one)."""

    def accepted_prediction(self, pcl_rule=False):
        return [CLASSES[c][1 if pcl_rule else 0] for c in self.cls]

    def for_evaluate(self, accepted=None):
        """(keys, npts, mean, icov) as tests/ndt_analytic.evaluate takes them: npts = -1 where `accepted` (default: every leaf of a class that must be
        accepted) is false"""
        if accepted is None:
            accepted = np.array([a is True for a in self.accepted_prediction()])
        return self.keys, np.where(accepted, self.n, np.where(self.n >= MIN_POINTS, -1, self.n)), self.mean, self.icov


def build(cloud, leaf):
    """the target build of `cloud` (N x 3 or N x 4 float32) at leaf size `leaf` (the library holds it as a float)"""
    pts = np.asarray(cloud, dtype=np.float32)[:, :3]
    fin, _, min_b, max_b, div_b, key = grid_of(pts, leaf)
    L = Leaves()
    L.grid = (min_b, max_b, div_b)
    L.point_key = np.full(len(pts), -1, dtype=np.int64)
    L.point_key[fin] = key
    idx = np.flatnonzero(fin)
    order = np.argsort(key, kind="stable")  # point order inside a leaf is kept
    ks, starts, counts = np.unique(key[order], return_index=True, return_counts=True)
    m = len(ks)
    L.keys, L.n = ks, counts.astype(np.int64)
    L.mean, L.cov, L.lam = np.zeros((m, 3)), np.zeros((m, 3, 3)), np.zeros((m, 3))
    L.cov_reg, L.icov, L.centroid, L.cls = np.zeros((m, 3, 3)), np.zeros((m, 3, 3)), np.zeros((m, 3), dtype=np.float32), []
    L.members = []
    for i in range(m):
        sel = idx[order[starts[i]:starts[i] + counts[i]]]
        L.members.append(sel)
        p32 = pts[sel]
        n = len(sel)
        L.centroid[i] = np.cumsum(p32, axis=0, dtype=np.float32)[-1] / np.float32(n)
        x = p32.astype(np.longdouble)
        mean = x.sum(0) / n
        L.mean[i] = mean.astype(np.float64)
        if n < MIN_POINTS:
            L.cls.append("few")
            continue
        d = x - mean
        cov = ((d.T @ d) / n * ((n - 1) / np.longdouble(n))).astype(np.float64)
        cov = (cov + cov.T) / 2
        w, cov_reg, icov = _floored_inverse(cov)
        L.cov[i], L.lam[i] = cov, w
        c = _classify(n, w)
        L.cls.append(c)
        if c != "point":
            L.cov_reg[i], L.icov[i] = cov_reg, icov
    L.cls = np.array(L.cls)
    return L


def single_pass_reference(cloud, model):
    """(mean, icov) of every leaf of `model` by the single-pass formula in plain float64, the sums added in point order, then the same eigh / floor /
    inverse as the model: the reference's OWN rounding error against the centred longdouble form (eps |mean|^2 / lambda_max) — what a correct
    implementation of the single-pass build may differ from the model by."""
    pts = np.asarray(cloud, dtype=np.float32)[:, :3].astype(np.float64)
    m = len(model.keys)
    mean, icov = np.zeros((m, 3)), np.zeros((m, 3, 3))
    for i, sel in enumerate(model.members):
        x = pts[sel]
        n = len(sel)
        s = np.cumsum(x, axis=0)[-1]
        mean[i] = s / n
        if model.cls[i] in ("few", "point"):
            continue
        xx = np.cumsum(x[:, :, None] * x[:, None, :], axis=0)[-1]
        cov = (xx - 2 * np.outer(s, mean[i])) / n + np.outer(mean[i], mean[i])
        cov *= (n - 1.0) / n
        icov[i] = _floored_inverse((cov + cov.T) / 2)[2]
    return mean, icov


def rel_dev(a, b):
    """per leaf: max |a - b| over max |b| (0 where b is all zero and a equals it)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ax = tuple(range(1, a.ndim))
    den = np.abs(b).max(axis=ax)
    num = np.abs(a - b).max(axis=ax)
    return np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0.0))


TOL_FACTOR, TOL_FLOOR = 8.0, 1e-12


def tolerances(cloud, model):
    """{"mean", "icov", "icov_rank_deficient"}: the worst relative deviation of ``single_pass_reference`` from the model over the leaves of the scene
    (rank-deficient leaves apart), times TOL_FACTOR (the eigen-solver's and the 3 x 3 inverse's own operation order), floored at TOL_FLOOR;
    "measured" holds the raw figures."""
    sp_mean, sp_icov = single_pass_reference(cloud, model)
    rd = model.cls == "rank_deficient"
    full = np.isin(model.cls, ("regular", "thin"))
    meas = {
        "mean": float(rel_dev(sp_mean, model.mean).max()),
        "icov": float(rel_dev(sp_icov[full], model.icov[full]).max()) if full.any() else 0.0,
        "icov_rank_deficient": float(rel_dev(sp_icov[rd], model.icov[rd]).max()) if rd.any() else 0.0,
    }
    tol = {k: max(TOL_FACTOR * v, TOL_FLOOR) for k, v in meas.items()}
    tol["measured"] = meas
    return tol


# ---- constructed scenes -----------------------------------------------------------------------------------------------------------------------------
KINDS = ("regular", "thin_plane", "plane_x", "plane_y", "plane_z", "line_a", "line_b", "duplicates")
SIZES = (5, 6, 7, 30, 200)
_Q = 2.0 ** -12  # every coordinate of an exact line is a multiple of this: exact in float32 below 4096, so the points are EXACTLY collinear


def scene(leaf, origin=(0.0, 0.0, 0.0), seed=0):
    """(cloud N x 4 float32, info) — one voxel per (kind, size), KINDS x SIZES = 40 voxels two cells apart (no two share a cell, no two are DIRECT7 or
    radius neighbours), every point at least 0.1 leaf inside its cell, the cloud in a shuffled order with a few NaN / inf points.  info: a list of
    (kind, size, cell) in construction order.  Deterministic in (leaf, origin, seed)."""
    rng = np.random.default_rng([seed, int(round(leaf * 1000))])
    lf = float(np.float32(leaf))
    base = np.floor(np.asarray(origin, dtype=np.float64) / lf).astype(np.int64)
    pts, info = [], []
    for k, (kind, n) in enumerate((kd, s) for kd in KINDS for s in SIZES):
        cell = base + 2 * np.array([k % 7, (k // 7) % 6, k % 3])
        u = 0.1 + 0.8 * rng.random((n, 3))  # in-cell coordinates
        if kind == "thin_plane":  # oblique thin plane through the cell centre, sigma = 1e-3 leaf along its normal
            nrm = np.array([0.36, -0.48, 0.8])
            v = (u - 0.5) * 0.7
            v -= np.outer(v @ nrm, nrm)
            u = 0.5 + v + np.outer(rng.normal(0, 1e-3, n), nrm)
        p = (cell + u) * lf
        if kind.startswith("plane_"):  # exact axis-aligned plane: one coordinate is ONE float for all points (a generic one: the sums round)
            a = "xyz".index(kind[-1])
            p[:, a] = np.float32((cell[a] + 0.1 + 0.8 * rng.random()) * lf)
        elif kind.startswith("line_"):  # exact oblique line: p0 + t d on the 2^-12 lattice
            d = np.array([3, -2, 1] if kind == "line_a" else [1, 2, -3]) * _Q
            p0 = np.round((cell + 0.5) * lf / _Q) * _Q
            tmax = int(0.38 * lf / (3 * _Q))
            p = p0 + np.outer(rng.integers(-tmax, tmax + 1, n), d)
        elif kind == "duplicates":
            p[:] = p[0]
        pts.append(p)
        info.append((kind, n, cell))
    xyz = np.concatenate(pts).astype(np.float32)
    bad = np.tile(xyz[:6], (1, 1))
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, :], bad[5, 1] = np.nan, np.inf, -np.inf, np.inf, np.nan, np.nan
    xyz = np.concatenate([xyz, bad])
    xyz = xyz[rng.permutation(len(xyz))]
    cloud = np.empty((len(xyz), 4), dtype=np.float32)
    cloud[:, :3] = xyz
    cloud[:, 3] = rng.random(len(xyz)).astype(np.float32)
    return cloud, info


def face_cloud(leaf, n_cells=40, seed=0):
    """points on and next to cell faces (k * leaf and the floats around it, k positive and negative, per axis) — the inputs at which the float rule and
    the exact cell can part.  N x 4 float32."""
    rng = np.random.default_rng([seed, int(round(leaf * 1000))])
    lf = np.float32(leaf)
    ks = np.concatenate([np.arange(-n_cells, n_cells + 1), rng.integers(-3000, 3000, 3 * n_cells)])
    face = (ks.astype(np.float32) * lf).astype(np.float32)
    near = [face]
    for _ in range(2):
        near.append(np.nextafter(near[-1], np.float32(np.inf)))
    lo = face
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf))
        near.append(lo)
    v = np.concatenate(near)
    xyz = np.stack([v, rng.permutation(v), rng.uniform(-1, 1, len(v)).astype(np.float32)], 1).astype(np.float32)
    return np.concatenate([xyz, rng.random((len(xyz), 1)).astype(np.float32)], 1)
