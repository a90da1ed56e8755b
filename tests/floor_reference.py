"""Test-side restatement of FloorDetectionComponent::detect (the reference's apps/floor_detection_component.cpp:100-183) in numpy float32, in the
reference's order of operations: tilt (:103-109), height band (:110-118, plane_clip :192-208), normal filter (:120-122, normal_filtering :216-243),
transform back (:124), RANSAC (:139-167).  The product never imports this file (tests/test_abi.py: it lives under tests/).

The upstream arithmetic is restated from recall, PCL 1.12.1 / Eigen 3.3 [UPSTREAM-RECALL]; csrc/floor.hip lists the same points.  Unpinned: no PCL
build exists to hold it against.  Every float32 operation below is one IEEE operation (numpy does not contract), so a difference from the GPU is an
arithmetic difference, except in the normals: float atan2 / sin / cos are libm's here and the device's there."""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = _libm.atan2f.restype = ctypes.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [ctypes.c_float]
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]

MAX_ITERATIONS = 10000
PROBABILITY = 0.99
MAX_SKIP = 10 * MAX_ITERATIONS
MAX_SAMPLE_CHECKS = 1000
INT_MAX = 2**31 - 1


# ---- MT19937 (boost::mt19937 == std::mt19937) --------------------------------------------------------------------------------------------------
class MT19937:
    def __init__(self, seed: int = 5489):
        mt = [0] * 624
        mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.mt, self.i = mt, 624

    def _twist(self):
        mt = self.mt
        for kk in range(624):
            y = (mt[kk] & 0x80000000) | (mt[(kk + 1) % 624] & 0x7FFFFFFF)
            mt[kk] = mt[(kk + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.i = 0

    def __call__(self) -> int:
        if self.i >= 624:
            self._twist()
        y = self.mt[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


# ---- tilt, band, transforms -------------------------------------------------------------------------------------------------------------------
def tilt_rotations(tilt_deg: float):
    """AngleAxisf(tilt_deg * M_PI / 180.0f, UnitY).toRotationMatrix() (:103-106) and the inverse this port uses (its transpose)."""
    a = f32(tilt_deg * math.pi / 180.0)
    s, c = f32(_libm.sinf(float(a))), f32(_libm.cosf(float(a)))
    r11 = (f32(1) - c) * f32(1) + c
    z = f32(0)
    R = np.array([[c, z, s], [z, r11, z], [-s, z, c]], dtype=f32)
    return R, R.T.copy()


def transform(R, cloud):
    """pcl::transformPointCloud with [R | 0] (SSE order: m00 x + (m01 y + (m02 z + m03)))."""
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    out = cloud.copy()
    for r in range(3):
        t = R[r, 2] * z + f32(0)
        t = R[r, 1] * y + t
        out[:, r] = R[r, 0] * x + t
    return out


def band_flags(tilted, sensor_height, height_clip_range):
    """plane_clip twice (:111-112): keep z >= -(h + r), then drop z >= -(h - r); PlaneClipper3D's (0 x + 0 y) + 1 z."""
    lo, hi = -f32(sensor_height + height_clip_range), -f32(sensor_height - height_clip_range)
    hz = (f32(0) * tilted[:, 0] + f32(0) * tilted[:, 1]) + f32(1) * tilted[:, 2]
    return (hz >= lo) & ~(hz >= hi)


# ---- normals ------------------------------------------------------------------------------------------------------------------------------------
def knn10(cloud):
    """k = 10 nearest neighbours ascending by (float squared distance ((dx^2 + dy^2) + dz^2), index); -1 where the cloud has fewer points."""
    n, k = len(cloud), 10
    out = np.full((n, k), -1, dtype=np.int64)
    if n == 0:
        return out
    p = cloud[:, :3].astype(f32)
    try:
        from scipy.spatial import cKDTree

        cand = min(n, 24)
        _, ci = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=cand)
        ci = np.asarray(ci).reshape(n, cand)
    except ImportError:  # pragma: no cover
        ci = None
    for s in range(0, n, 2048):
        q = p[s: s + 2048]
        if ci is None:
            idx = np.broadcast_to(np.arange(n), (len(q), n))
        else:
            idx = ci[s: s + 2048]
        d = q[:, None, :] - p[idx]
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.lexsort((idx, sq), axis=-1)[:, :k]
        out[s: s + len(q), : order.shape[1]] = np.take_along_axis(np.asarray(idx), order, axis=1)
        if ci is not None:  # a candidate list can miss ties at the 10th distance: check against the full cloud for those rows
            kth = np.take_along_axis(sq, order[:, -1:], axis=1)[:, 0]
            far = np.take_along_axis(sq, np.argsort(sq, axis=1)[:, -1:], axis=1)[:, 0]
            for r in np.nonzero(far <= kth)[0]:
                dd = p - q[r]
                s2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
                out[s + r, :] = np.lexsort((np.arange(n), s2))[:k] if n >= k else np.concatenate([np.lexsort((np.arange(n), s2)), -np.ones(k - n, np.int64)])
    return out


def _roots2(b, c):
    d = f32(float(b * b) - 4.0 * float(c))
    if d < 0:
        d = f32(0)
    sd = f32(math.sqrt(d))
    return [f32(0), f32(0.5) * (b - sd), f32(0.5) * (b + sd)]


def eigen33_smallest(m):
    """pcl::eigen33(mat, eigenvalue, eigenvector): float32 throughout."""
    m = np.asarray(m, dtype=f32).reshape(3, 3)
    scale = f32(np.abs(m).max())
    if scale <= np.finfo(f32).tiny:
        scale = f32(1)
    s = m / scale
    m00, m01, m02, m11, m12, m22 = s[0, 0], s[0, 1], s[0, 2], s[1, 1], s[1, 2], s[2, 2]
    two = f32(2)
    c0 = m00 * m11 * m22 + two * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
    c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
    c2 = m00 + m11 + m22
    if abs(c0) < np.finfo(f32).eps:
        r = _roots2(c2, c1)
    else:
        s_inv3 = f32(1.0 / 3.0)
        s_sqrt3 = f32(math.sqrt(3.0))
        c2_over_3 = c2 * s_inv3
        a_over_3 = (c1 - c2 * c2_over_3) * s_inv3
        if a_over_3 > 0:
            a_over_3 = f32(0)
        half_b = f32(0.5) * (c0 + c2_over_3 * (two * c2_over_3 * c2_over_3 - c1))
        q = half_b * half_b + a_over_3 * a_over_3 * a_over_3
        if q > 0:
            q = f32(0)
        rho = f32(math.sqrt(-a_over_3))
        theta = f32(_libm.atan2f(float(f32(math.sqrt(-q))), float(half_b))) * s_inv3
        ct, st = f32(_libm.cosf(float(theta))), f32(_libm.sinf(float(theta)))
        r = [c2_over_3 + two * rho * ct, c2_over_3 - rho * (ct + s_sqrt3 * st), c2_over_3 - rho * (ct - s_sqrt3 * st)]
        if r[0] >= r[1]:
            r[0], r[1] = r[1], r[0]
        if r[1] >= r[2]:
            r[1], r[2] = r[2], r[1]
            if r[0] >= r[1]:
                r[0], r[1] = r[1], r[0]
        if r[0] <= 0:
            r = _roots2(c2, c1)
    s = s.copy()
    for i in range(3):
        s[i, i] = s[i, i] - r[0]
    vecs = []
    for a, b in ((s[0], s[1]), (s[0], s[2]), (s[1], s[2])):
        v = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)
        vecs.append((v, (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
    (v1, l1), (v2, l2), (v3, l3) = vecs
    if l1 >= l2 and l1 >= l3:
        v, ln = v1, l1
    elif l2 >= l1 and l2 >= l3:
        v, ln = v2, l2
    else:
        v, ln = v3, l3
    return v / f32(math.sqrt(ln))


def point_normal(cloud, nbrs):
    """NormalEstimation::computePointNormal: computeMeanAndCovarianceMatrix (shifted by the first neighbour, neighbour order) + eigen33."""
    nbrs = [int(j) for j in nbrs if j >= 0]
    if len(nbrs) < 3:
        return np.full(3, np.nan, dtype=f32)
    K = cloud[nbrs[0], :3]
    acc = np.zeros(9, dtype=f32)
    for j in nbrs:
        x, y, z = cloud[j, 0] - K[0], cloud[j, 1] - K[1], cloud[j, 2] - K[2]
        acc += np.array([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z], dtype=f32)
    acc = acc / f32(len(nbrs))
    m = np.empty(9, dtype=f32)
    m[0] = acc[0] - acc[6] * acc[6]
    m[1] = acc[1] - acc[6] * acc[7]
    m[2] = acc[2] - acc[6] * acc[8]
    m[4] = acc[3] - acc[7] * acc[7]
    m[5] = acc[4] - acc[7] * acc[8]
    m[8] = acc[5] - acc[8] * acc[8]
    m[3], m[6], m[7] = m[1], m[2], m[5]
    return eigen33_smallest(m)


def normal_keep(normals, thresh_deg):
    """|normalized(n) . z| > cos(thresh) in double; NaN fails.  Also returns |n_z| / |n| for the boundary test."""
    n = normals.astype(f32)
    sq = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(sq)
        u = np.where((sq > 0)[:, None], n / np.where(sq > 0, r, f32(1))[:, None], n)
    dot = (u[:, 0] * f32(0) + u[:, 1] * f32(0)) + u[:, 2] * f32(1)
    a = np.abs(dot.astype(np.float64))
    cos_t = math.cos(thresh_deg * math.pi / 180.0)
    with np.errstate(invalid="ignore"):
        return a > cos_t, a


def normals(cloud, thresh_deg=20.0):
    nb = knn10(cloud)
    nr = np.stack([point_normal(cloud, nb[i]) for i in range(len(cloud))]) if len(cloud) else np.zeros((0, 3), f32)
    keep, a = normal_keep(nr, thresh_deg)
    return nr, keep, a


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------------------
def _sample_good(p0, p1, p2):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (p1 - p0) / (p2 - p0)
    return bool(d[0] != d[1] or d[2] != d[1])


def plane_from_sample(p0, p1, p2):
    """computeModelCoefficients: None when the cross product's stableNorm < 1e-5."""
    a, b = p1 - p0, p2 - p0
    c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)
    mx = f32(np.abs(c).max())
    scale, inv = f32(0), f32(1)
    if mx > 0:
        tmp = f32(1) / mx
        if tmp > np.finfo(f32).max:
            inv = np.finfo(f32).max
            scale = f32(1) / inv
        elif mx > np.finfo(f32).max:
            inv, scale = f32(1), mx
        else:
            scale, inv = mx, tmp
    elif mx != mx:
        scale = mx
    ssq = f32(0)
    if scale > 0:
        s = c * inv
        ssq = ssq + ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    norm = scale * f32(math.sqrt(ssq))
    if norm < f32(1e-5):  # (a NaN norm passes, as upstream)
        return None
    n = c / norm
    d = f32(-1) * ((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])
    return np.array([n[0], n[1], n[2], d], dtype=f32)


def plane_dist(c, cloud):
    """|c . (x, y, z, 1)| in Eigen's SSE Vector4f order: (c0 x + c2 z) + (c1 y + c3)."""
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    return np.abs((c[0] * x + c[2] * z) + (c[1] * y + c[3] * f32(1)))


def ransac(cloud, threshold=0.1):
    """RandomSampleConsensus<SampleConsensusModelPlane>::computeModel + getInliers on a fresh model.  Returns dict(has_model, coeffs, inliers,
    iterations, skipped)."""
    pts = np.ascontiguousarray(np.asarray(cloud, dtype=f32).reshape(-1, 4))
    n = len(pts)
    xyz = pts[:, :3]
    rng = MT19937(12345)
    shuffled = list(range(n))
    iterations, skipped, best, k = 0, 0, 0, float("inf")
    model = None
    log_probability = math.log(1.0 - PROBABILITY)
    one_over_indices = 1.0 / n if n else float("inf")
    eps = np.finfo(np.float64).eps
    k = 1.7976931348623157e308
    while iterations < k and skipped < MAX_SKIP:
        if n < 3:
            iterations = INT_MAX - 1
            break
        sample = None
        for _ in range(MAX_SAMPLE_CHECKS):
            for i in range(3):
                j = i + (rng() >> 1) % (n - i)
                shuffled[i], shuffled[j] = shuffled[j], shuffled[i]
            s = shuffled[:3]
            if _sample_good(xyz[s[0]], xyz[s[1]], xyz[s[2]]):
                sample = s
                break
        if sample is None:
            break
        c = plane_from_sample(xyz[sample[0]], xyz[sample[1]], xyz[sample[2]])
        if c is None:
            skipped += 1
            continue
        cnt = int(np.count_nonzero(plane_dist(c, xyz).astype(np.float64) < threshold))
        if cnt > best:
            best, model = cnt, c
            w = best * one_over_indices
            p_no = 1.0 - math.pow(w, 3.0)
            p_no = min(1.0 - eps, max(eps, p_no))
            k = log_probability / math.log(p_no)
        iterations += 1
        if iterations > MAX_ITERATIONS:
            break
    if model is None:
        return {"has_model": False, "coeffs": None, "inliers": np.zeros(0, np.int64), "iterations": iterations, "skipped": skipped}
    inl = np.nonzero(plane_dist(model, xyz).astype(np.float64) < threshold)[0]
    return {"has_model": True, "coeffs": model, "inliers": inl, "iterations": iterations, "skipped": skipped}


# ---- detect() -----------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = {"tilt_deg": 0.0, "sensor_height": 2.0, "height_clip_range": 1.0, "floor_pts_thresh": 512, "floor_normal_thresh_deg": 10.0,
            "use_normal_filtering": True, "normal_filter_thresh_deg": 20.0}


def detect(cloud, params=None, keep_override=None):
    """Returns a dict: found, reason, coeffs, filtered (floor_filtered_points), inliers (floor_points), n_clipped, iterations, skipped, keep / a (the
    normal filter's flags and |n_z| of the band cloud).  keep_override: use these normal keep-flags instead of the restated ones (to hold the RANSAC
    stage against the GPU's when only a boundary flag differs)."""
    p = dict(DEFAULTS)
    p.update(params or {})
    c = np.ascontiguousarray(np.asarray(cloud, dtype=f32).reshape(-1, 4))
    out = {"found": False, "coeffs": None, "filtered": np.zeros((0, 4), f32), "inliers": np.zeros((0, 4), f32), "n_clipped": 0, "iterations": 0, "skipped": 0,
           "keep": None, "a": None}
    if len(c) == 0:
        out["reason"] = "empty_input"
        return out
    R, Ri = tilt_rotations(p["tilt_deg"])
    t = transform(R, c)
    band = t[band_flags(t, p["sensor_height"], p["height_clip_range"])]
    out["n_clipped"] = len(band)
    if len(band) == 0:
        out["reason"] = "none_after_clip"
        return out
    if p["use_normal_filtering"]:
        _, keep, a = normals(band, p["normal_filter_thresh_deg"])
        out["keep"], out["a"] = keep, a
        if keep_override is not None:
            keep = np.asarray(keep_override, dtype=bool)
        band = band[keep]
    filt = transform(Ri, band)
    out["filtered"] = filt
    if len(filt) < p["floor_pts_thresh"]:
        out["reason"] = "too_few_filtered"
        return out
    r = ransac(filt, 0.1)
    out["iterations"], out["skipped"] = r["iterations"], r["skipped"]
    if not r["has_model"]:
        out["reason"] = "no_model"
        return out
    coeffs = r["coeffs"].copy()
    out["coeffs"] = coeffs
    if len(r["inliers"]) < p["floor_pts_thresh"]:
        out["reason"] = "too_few_inliers"
        return out
    ref = Ri[:, 2]
    dot = float((coeffs[0] * ref[0] + coeffs[1] * ref[1]) + coeffs[2] * ref[2])
    if abs(dot) < math.cos(p["floor_normal_thresh_deg"] * math.pi / 180.0):
        out["reason"] = "not_vertical"
        return out
    if (coeffs[0] * f32(0) + coeffs[1] * f32(0)) + coeffs[2] * f32(1) < 0:
        coeffs = coeffs * f32(-1)
    out.update(found=True, reason="found", coeffs=coeffs, inliers=filt[r["inliers"]])
    return out


class ReferenceOps:
    """``ops`` of mrg_slam_amd.floor_detection.FloorDetectionComponent backed by this restatement."""

    def detect(self, cloud, p):
        r = detect(cloud, p)
        return r["coeffs"] if r["found"] else None
