"""First-principles model of the GICP family in numpy float64 — an INDEPENDENT check of the covariance, Mahalanobis, Jacobian and
voxel-map arithmetic of GICP_HIP / SMALL_GICP_HIP / VGICP_HIP / PCL_GICP_HIP / ICP_HIP, not a restatement of the oracle or of the kernels.
Everything follows from the cost of Segal et al. 2009 ("Generalized-ICP", eq. 2)

    e(T)  = sum_i  w_i r_i^T M_i r_i,       r_i = m_B(i) - T a_i,      M_i = (C_B(i) + R C_A(i) R^T)^-1  frozen at the linearisation pose,
    b     = sum_i  w_i J_i^T M_i r_i,       H   = sum_i w_i J_i^T M_i J_i        (so  d e / d xi = 2 b,  Gauss-Newton Hessian 2 H)

DERIVED here:
  * the regularised covariance of the k nearest neighbours: mean and centred second moment over k (both / k), np.linalg.eigh,
    E diag(1e-3, 1, 1) E^T with the eigenvalues ascending (fast_gicp's PLANE form); and pcl::GICP's form: raw second moments minus
    mean mean^T, the value gicp_epsilon on the direction of the smallest |eigenvalue|;
  * M by np.linalg.inv; the residual and the cost;
  * the Jacobian from the six generator matrices G_i of se(3), rotations first: J[:, i] = -(G_i T a)[:3] for the left perturbation
    exp(xi) T (fast_gicp, VGICP), -(T G_i a)[:3] for the right one T exp(xi) (small_gicp) — no skew-symmetric tables;
  * VGICP's voxel map: per voxel the mean of its points and the mean of their covariances, weight sqrt(points in the voxel), one
    correspondence per source point: the voxel its transformed position falls in;
  * pcl::GICP's functor: f = 1/m sum d^T M d, d = R(x) a + t - b, and its gradient in x = (t, phi, theta, psi) for
    R = Rz(psi) Ry(theta) Rx(phi), from products of elementary rotations and their derivatives;
  * one ICP step: Kabsch (np.linalg.svd of the cross-covariance) over brute-force correspondences, composed onto the guess; a chain of them,
    every step from the float pose the one before it left (icp_chain);
  * the se(3) logarithm (se3_log): the matrix logarithm by inverse scaling and squaring (Denman-Beavers square roots, then the power series of
    log(I + X)), read off along the six generators — the inverse of se3_exp, with no closed form of either.

TAKEN AS GIVEN (conventions, not arithmetic that could be wrong in an interesting way):
  * which neighbours / which correspondence: float32 squared distances in the kernels' order ((dx dx + dy dy) + dz dz), ascending by
    (distance, index) — brute_knn below restates _brute_knn of tests/test_gpu_primitives.py; a GICP correspondence holds iff that float
    distance, as a double, is < max_correspondence_distance^2 (strict); an ICP one iff it is not > (pcl::IterativeClosestPoint);
  * the float query point of GICP, pcl::GICP and ICP: T cast to float, ((m0 x + m1 y) + m2 z) + m3 in float;
  * the double query point of VGICP and its voxel index floor(x / res - 0.5);
  * the order of the 6-vectors: rotation first for H / b, (t, phi, theta, psi) for pcl::GICP;
  * the scaling of pcl::GICP's cost as its functor defines it (f / m, gradient 2 / m), its Mahalanobis rotation (the rotation of the
    float transformation the correspondences were found at) and the float products in its raw moments;
  * with fewer than k neighbours in the cloud the sums run over those there are and are still divided by k;
  * pcl::IterativeClosestPoint's cumulative FLOAT transformation: the pose an ICP iteration starts from is the float matrix the one before left.
"""
import numpy as np


# ---- given: selection -------------------------------------------------------------------------------------------------------------
def brute_knn(cloud, q, k):
    """(index, squared distance) of the k nearest finite points, ascending by (distance, index); -1 where there is none"""
    c, qq = np.asarray(cloud)[:, :3].astype(np.float32), np.asarray(q)[:, :3].astype(np.float32)
    idx = np.full((len(qq), k), -1, dtype=np.int64)
    sqd = np.full((len(qq), k), np.inf, dtype=np.float32)
    ids = np.nonzero(np.isfinite(c).all(axis=1))[0]
    for i, p in enumerate(qq):
        if not np.isfinite(p).all() or len(ids) == 0:
            continue
        d = c[ids] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        o = np.lexsort((ids, d2))[:k]
        idx[i, : len(o)] = ids[o]
        sqd[i, : len(o)] = d2[o]
    return idx, sqd


def transform_float(T, pts):
    """The float query points: T cast to float times (x, y, z, 1), accumulated left to right in float"""
    Tf = np.asarray(T).astype(np.float32)
    p = np.asarray(pts)[:, :3].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        cols = []
        for r in range(3):
            s = Tf[r, 0] * p[:, 0]
            s = s + Tf[r, 1] * p[:, 1]
            s = s + Tf[r, 2] * p[:, 2]
            cols.append(s + Tf[r, 3])
    return np.stack(cols, 1)


def nearest(target, queries, max_distance, strict=True):
    """index of the nearest target point per query, -1 where the float distance is not < max^2 (strict) / is > max^2 (not strict)"""
    idx, sqd = brute_knn(target, queries, 1)
    idx, d = idx[:, 0].copy(), sqd[:, 0].astype(np.float64)
    thr = float(max_distance) * float(max_distance)
    idx[(idx >= 0) & (~(d < thr) if strict else (d > thr))] = -1
    return idx, d


# ---- se(3) ------------------------------------------------------------------------------------------------------------------------
def generators():
    """The six generator matrices of se(3): rotations about x, y, z, then translations along x, y, z"""
    G = np.zeros((6, 4, 4))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        G[i, k, j], G[i, j, k] = 1.0, -1.0  # d/da of the rotation about axis i at a = 0
        G[3 + i, i, 3] = 1.0
    return G


def se3_exp(xi):
    """exp(sum xi_i G_i) by scaling and squaring of the power series"""
    A = np.tensordot(np.asarray(xi, dtype=np.float64), generators(), 1)
    s = max(0, int(np.ceil(np.log2(max(np.abs(A).sum(), 1e-300)))) + 4)
    A = A / 2.0 ** s
    E, term = np.eye(4), np.eye(4)
    for n in range(1, 20):
        term = term @ A / n
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def se3_log(T):
    """xi with exp(sum xi_i G_i) = T (rotation angle below pi): square roots until T^(1 / 2^s) is within 0.25 of I, the series of log(I + X) there,
    times 2^s, projected on the generators (what a float matrix has off se(3) — its rounding — is dropped by the projection)"""
    A = np.asarray(T, dtype=np.float64)
    s = 0
    while np.abs(A - np.eye(4)).sum(1).max() > 0.25 and s < 40:
        Y, Z = A, np.eye(4)  # Denman-Beavers: Y -> A^(1/2), Z -> A^(-1/2)
        for _ in range(50):
            Yn, Zn = 0.5 * (Y + np.linalg.inv(Z)), 0.5 * (Z + np.linalg.inv(Y))
            done = np.abs(Yn - Y).max() <= 4e-16 * np.abs(Yn).max()
            Y, Z = Yn, Zn
            if done:
                break
        A = Y
        s += 1
    X = A - np.eye(4)
    L, P = np.zeros((4, 4)), np.eye(4)
    for n in range(1, 40):
        P = P @ X
        L = L + (P / n if n % 2 else -P / n)
    L = L * 2.0 ** s
    G = generators()
    return np.array([(L * G[i]).sum() / (G[i] * G[i]).sum() for i in range(6)])


def adjoint(T):
    """Ad with exp(Ad xi) T = T exp(xi), rotation block first"""
    R, t = T[:3, :3], T[:3, 3]
    tx = np.tensordot(t, generators()[:3, :3, :3], 1)
    return np.block([[R, np.zeros((3, 3))], [tx @ R, R]])


def _rot(axis, a, order=0):
    """order-th derivative with respect to the angle of the rotation about `axis` by a"""
    c, s = np.cos(a), np.sin(a)
    cc, ss = [(c, s), (-s, c)][order]
    d = 1.0 if order == 0 else 0.0
    if axis == 0:
        return np.array([[d, 0, 0], [0, cc, -ss], [0, ss, cc]])
    if axis == 1:
        return np.array([[cc, 0, ss], [0, d, 0], [-ss, 0, cc]])
    return np.array([[cc, -ss, 0], [ss, cc, 0], [0, 0, d]])


# ---- covariances ------------------------------------------------------------------------------------------------------------------
def _neighbourhoods(cloud, k):
    idx, _ = brute_knn(cloud, cloud, k)
    X = np.asarray(cloud)[:, :3].astype(np.float64)[np.maximum(idx, 0)]  # n x k x 3
    return X, (idx >= 0)


def covariances_fast(cloud, k=20, eps=1e-3):
    """fast_gicp / small_gicp: (C[n, 3, 3], w[n, 3]) — the regularised covariances and the ascending eigenvalues of the sample ones"""
    X, ok = _neighbourhoods(cloud, k)
    X = np.where(ok[:, :, None], X, 0.0)
    mean = X.sum(1) / k
    D = np.where(ok[:, :, None], X - mean[:, None, :], 0.0)
    S = np.einsum("nka,nkb->nab", D, D) / k
    w, E = np.linalg.eigh(S)
    vals = np.array([eps, 1.0, 1.0])
    return np.einsum("nam,m,nbm->nab", E, vals, E), w


def covariances_pcl(cloud, k=20, gicp_epsilon=1e-3):
    """pcl::GICP: raw second moments (float products, added in neighbour order) / k minus mean mean^T; gicp_epsilon on the direction of
    the smallest |eigenvalue|.  Returns (C, w) with w the eigenvalues ordered by descending magnitude."""
    idx, _ = brute_knn(cloud, cloud, k)
    P = np.asarray(cloud)[:, :3].astype(np.float32)
    n = len(P)
    raw, mean = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for j in range(k):
        ok = idx[:, j] >= 0
        p = P[np.maximum(idx[:, j], 0)]
        mean += np.where(ok[:, None], p.astype(np.float64), 0.0)
        prod = (p[:, :, None] * p[:, None, :]).astype(np.float64)  # float products
        raw += np.where(ok[:, None, None], prod, 0.0)
    mean /= k
    S = raw / k - mean[:, :, None] * mean[:, None, :]
    w, E = np.linalg.eigh(S)
    order = np.argsort(-np.abs(w), axis=1, kind="stable")
    w = np.take_along_axis(w, order, 1)
    E = np.take_along_axis(E, order[:, None, :], 2)
    vals = np.array([1.0, 1.0, gicp_epsilon])
    return np.einsum("nam,m,nbm->nab", E, vals, E), w


# ---- the GICP factor --------------------------------------------------------------------------------------------------------------
class Terms:
    """The correspondences of one linearisation: source points a, target means m_B, frozen Mahalanobis matrices M, weights w"""

    def __init__(self, a, mB, M, w):
        self.a = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, 3), np.ones((len(a), 1))], 1)
        self.mB, self.M, self.w = np.asarray(mB, dtype=np.float64).reshape(-1, 3), np.asarray(M, dtype=np.float64).reshape(-1, 3, 3), np.asarray(w, dtype=np.float64)

    def __len__(self):
        return len(self.w)

    def residuals(self, T):
        return self.mB - (self.a @ T.T)[:, :3]

    def cost(self, T):
        r = self.residuals(T)
        return float(np.einsum("n,na,nab,nb->", self.w, r, self.M, r))

    def jacobians(self, T, side):
        G = generators()
        if side == "left":
            return -np.einsum("iab,bc,nc->nai", G, T, self.a)[:, :3, :]
        return -np.einsum("ab,ibc,nc->nai", T, G, self.a)[:, :3, :]

    def linearize(self, T, side):
        """(H, b, e, number of correspondences)"""
        T = np.asarray(T, dtype=np.float64)
        r, J = self.residuals(T), self.jacobians(T, side)
        H = np.einsum("n,nai,nab,nbj->ij", self.w, J, self.M, J)
        b = np.einsum("n,nai,nab,nb->i", self.w, J, self.M, r)
        return H, b, self.cost(T), len(self)


def mahalanobis(C_B, C_A, R):
    return np.linalg.inv(C_B + R @ C_A @ R.T)


def gicp_terms(target, source, cov_target, cov_source, T, max_distance=2.0):
    """GICP / small_gicp: the nearest target point of the float query, within the distance (strict)"""
    T = np.asarray(T, dtype=np.float64)
    j, _ = nearest(target, transform_float(T, source), max_distance, strict=True)
    keep = np.nonzero(j >= 0)[0]
    R = T[:3, :3]
    M = [mahalanobis(cov_target[j[i]], cov_source[i], R) for i in keep]
    return Terms(np.asarray(source)[keep, :3], np.asarray(target)[j[keep], :3], M, np.ones(len(keep))), j


def voxel_map(target, cov_target, resolution):
    """{voxel coordinate: (points, mean, mean covariance)} over the finite target points"""
    P = np.asarray(target)[:, :3].astype(np.float64)
    members = {}
    for i, p in enumerate(P):
        if np.isfinite(p).all():
            members.setdefault(tuple(np.floor(p / resolution - 0.5).astype(np.int64)), []).append(i)
    return {c: (len(m), P[m].mean(0), np.asarray(cov_target)[m].mean(0)) for c, m in members.items()}


def voxel_coords(T, source, resolution):
    """The double query points T a of VGICP and x / res - 0.5, whose floor is the voxel coordinate"""
    a = np.asarray(source)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        tA = a @ np.asarray(T, dtype=np.float64)[:3, :3].T + np.asarray(T, dtype=np.float64)[:3, 3]
        return tA, tA / resolution - 0.5


def vgicp_terms(target, source, cov_target, cov_source, T, resolution):
    T = np.asarray(T, dtype=np.float64)
    vox = voxel_map(target, cov_target, resolution)
    tA, u = voxel_coords(T, source, resolution)
    a, mB, M, w, hit = [], [], [], [], np.full(len(tA), False)
    for i in range(len(tA)):
        if not np.isfinite(tA[i]).all():
            continue
        v = vox.get(tuple(np.floor(u[i]).astype(np.int64)))
        if v is None:
            continue
        hit[i] = True
        a.append(np.asarray(source)[i, :3])
        mB.append(v[1])
        M.append(mahalanobis(v[2], cov_source[i], T[:3, :3]))
        w.append(np.sqrt(v[0]))
    return Terms(np.reshape(a, (-1, 3)), mB, M, w), hit


# ---- pcl::GICP's functor ------------------------------------------------------------------------------------------------------------
def pcl_cost(target, source, cov_target, cov_source, T, x, max_distance=2.0):
    """(f, g[6], correspondences) at x = (t, phi, theta, psi) over the correspondences found at the float transformation T"""
    Tf = np.asarray(T).astype(np.float32).astype(np.float64)
    j, _ = nearest(target, transform_float(T, source), max_distance, strict=True)
    keep = np.nonzero(j >= 0)[0]
    m = len(keep)
    if m == 0:
        return 0.0, np.zeros(6), 0
    M = np.array([mahalanobis(cov_target[j[i]], cov_source[i], Tf[:3, :3]) for i in keep])
    a = np.asarray(source)[keep, :3].astype(np.float64)
    b = np.asarray(target)[j[keep], :3].astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    ang = [(2, x[5]), (1, x[4]), (0, x[3])]  # R = Rz(psi) Ry(theta) Rx(phi)

    def prod(which):
        out = np.eye(3)
        for axis, v in ang:
            out = out @ _rot(axis, v, int(axis == which))
        return out

    d = a @ prod(-1).T + x[:3] - b
    Md = np.einsum("nab,nb->na", M, d)
    f = float(np.einsum("na,na->", d, Md)) / m
    g = np.zeros(6)
    g[:3] = 2.0 / m * Md.sum(0)
    for i in range(3):
        g[3 + i] = 2.0 / m * float(np.einsum("na,na->", a @ prod(i).T, Md))
    return f, g, m


# ---- ICP ----------------------------------------------------------------------------------------------------------------------------
def icp_correspondences(target, source, pose, max_distance=2.0, reciprocal=False):
    """(float query points at `pose`, index of the target point per source point or -1)"""
    cur = transform_float(pose, source)
    j, _ = nearest(target, cur, max_distance, strict=False)
    if reciprocal:
        back, _ = nearest(cur, np.asarray(target)[np.maximum(j, 0)], max_distance, strict=False)  # the target point's nearest source point
        j[back != np.arange(len(cur))] = -1
    return cur, j


def icp_step(target, source, guess, max_distance=2.0, reciprocal=False):
    """One iteration of point-to-point ICP from `guess`: (T_step guess as float64 4 x 4, correspondences)"""
    cur, j = icp_correspondences(target, source, guess, max_distance, reciprocal)
    keep = np.nonzero(j >= 0)[0]
    P, Q = cur[keep].astype(np.float64), np.asarray(target)[j[keep], :3].astype(np.float64)
    mp, mq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - mq).T @ (P - mp) / len(keep))
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U) * np.linalg.det(Vt)]) @ Vt
    step = np.eye(4)
    step[:3, :3], step[:3, 3] = R, mq - R @ mp
    return step @ np.asarray(guess).astype(np.float32).astype(np.float64), len(keep)


def icp_chain(target, source, guess, steps, max_distance=2.0, reciprocal=False):
    """`steps` iterations, each from the pose the one before left CAST TO FLOAT (the cumulative float transformation): the float poses
    T_0 = float(guess), T_1, ... T_steps"""
    poses = [np.asarray(guess).astype(np.float32)]
    for _ in range(steps):
        poses.append(icp_step(target, source, poses[-1], max_distance, reciprocal)[0].astype(np.float32))
    return poses
