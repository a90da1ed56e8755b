"""Inputs, preconditions and bars of the GICP family's first-principles checks, shared by tests/test_gicp_analytic_cpu.py (the oracle
against tests/gicp_analytic.py) and tests/test_gpu_gicp_analytic.py (the HIP kernels against it): a `Backend` puts the oracle's classes and
the product's behind one face, and every check here takes one.

Bars (none of them comes from what the code under test gives):
  H, b, e      1e-12 max|.| (+ 1e-9 absolute on b): both sides are f64 on f32 inputs, cond(C_B + R C_A R^T) <= 2 / 2e-3, n <= 800 terms
               -> n 1e3 2^-53 ~ 1e-13 at worst;
  covariances  |dC| <= 1e-13 w2 / (w1 - w0) per point — first-order perturbation of the projector on the regularised direction;
               precondition (w1 - w0) / w2 >= 1e-3 on every neighbourhood of a generic cloud;
  planes       against the hand-written I - (1 - 1e-3) n n^T: 1e-12 + 2 d / sqrt(w1), d the largest distance of the float points from the
               plane (a least-squares plane through points that far off tilts by at most d / sigma_1);
  pcl f, g and the ICP step pass through float matrices: ten times the oracle-against-model figure measured on the CPU (PCL_F_BAR ...).
Preconditions on the inputs, asserted and never skipped over: no query with its two nearest target distances (or its nearest and the
threshold) within 1e-5 relative, no VGICP query within 1e-9 res of a voxel face."""
import numpy as np

import gicp_analytic as ga
from conftest import small_cloud

SOURCE_SIZES = (1, 255, 256, 257, 513, 700)
FAR = np.array([300.0, -200.0, 50.0])
SMALL_POSE = ga.se3_exp([0.01, -0.008, 0.03, 0.2, -0.1, 0.03])
LARGE_POSE = ga.se3_exp(np.concatenate([1.2 * np.array([2.0, -1.0, 2.0]) / 3.0, [3.0, -2.0, 0.5]]))  # 1.2 rad about a skew axis

# oracle against model, measured by tests/test_gicp_analytic_cpu.py (see its docstring), times ten
PCL_F_BAR = 10 * 6.52e-6  # |df| / |f|
PCL_G_BAR = 10 * 6.51e-6  # max|dg| / max|g|
ICP_T_BAR = 10 * 5.79e-7  # max|dT|, metres (translation column) and 1 (rotation block)



def nudged(T, centre=(0.0, 0.0, 0.0)):
    """T moved by 3 cm / 7 mrad about `centre`: the pose the linearisations are taken at, off the one the clouds meet at"""
    C = np.eye(4)
    C[:3, 3] = centre
    return C @ ga.se3_exp([0.004, -0.003, 0.005, 0.03, -0.02, 0.01]) @ np.linalg.inv(C) @ T


MEASURED = {}  # quantity -> largest discrepancy seen in this process, in units of its bar's scale


def note(quantity, value):
    MEASURED[quantity] = max(MEASURED.get(quantity, 0.0), float(value))


def report(title):
    print(f"\n{title}: largest discrepancy against tests/gicp_analytic.py per quantity")
    for q in sorted(MEASURED):
        print(f"  {q:28s} {MEASURED[q]:.3g}")


# ---- the two implementations behind one face ----------------------------------------------------------------------------------------
class Backend:
    def __init__(self, name):
        self.name = name

    def _mod(self):
        if self.name == "oracle":
            from oracle import oracle as m
        else:
            import mrg_slam_amd as m
        return m

    def lm(self, variant, **kw):
        names = {"fast": ("FastGicp", "GicpHip"), "small": ("SmallGicp", "SmallGicpHip"), "vgicp": ("FastVgicp", "VgicpHip")}[variant]
        if self.name == "oracle":
            kw["num_threads"] = 1
        return getattr(self._mod(), names[self.name != "oracle"])(**kw)

    def pcl(self, **kw):
        return getattr(self._mod(), "PclGicp" if self.name == "oracle" else "PclGicpHip")(**kw)

    def icp(self, **kw):
        return getattr(self._mod(), "Icp" if self.name == "oracle" else "IcpHip")(**kw)

    def linearize(self, reg, T):
        """(H, b, e, n) whichever order the implementation returns them in"""
        out = reg.linearize(np.asarray(T, dtype=np.float64))
        if self.name == "oracle":
            e, H, b, n = out
            return H, b, e, n
        return out


def load(reg, target, source):
    reg.setInputTarget(target)
    reg.setInputSource(source)
    return reg


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def cloud4(xyz):
    out = np.zeros((len(xyz), 4), dtype=np.float32)
    out[:, :3] = xyz
    return out


def pair(n, T, seed=7, n_target=800, noise=0.05, offset=None):
    """A target of n_target points and a source of n: target points moved by `noise` and taken back through T, so that the clouds
    overlap at the pose T however large its rotation is; `offset` moves the whole scene."""
    tgt = small_cloud(n_target, seed)
    rng = np.random.default_rng(seed + 1000)
    world = tgt[rng.permutation(n_target)[:n], :3].astype(np.float64) + rng.normal(0, noise, (n, 3))
    if offset is not None:
        tgt[:, :3] = (tgt[:, :3].astype(np.float64) + offset).astype(np.float32)
        world = world + offset
    return tgt, cloud4((world - T[:3, 3]) @ T[:3, :3])


def lattice(normal_tilt=(0.0, 0.0), offset=(0.0, 0.0, 0.0), m=13, step=0.5):
    """m x m points on a plane through `offset`, the plane z = 0 tilted about x and then y: (cloud, unit normal, a point of it)"""
    u = (np.arange(m) - m // 2) * step
    flat = np.stack([np.repeat(u, m), np.tile(u, m), np.zeros(m * m)], 1)
    R = ga._rot(1, normal_tilt[1]) @ ga._rot(0, normal_tilt[0])
    return cloud4(flat @ R.T + np.asarray(offset)), R[:, 2], np.asarray(offset, dtype=np.float64)


def line_cloud(n=40):
    d = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    return cloud4(np.array([1.0, -2.0, 0.5]) + 0.1 * np.arange(n)[:, None] * d), d


def copies_cloud(n=25):
    return cloud4(np.tile([1.5, -2.25, 0.75], (n, 1)))


def octahedron_cloud():
    """24 points +-r e_i, r in (0.5, 1, 2, 4): mean 0 and second moment 5.3125 / 3 I, exactly"""
    return cloud4(np.concatenate([s * r * np.eye(3) for r in (0.5, 1.0, 2.0, 4.0) for s in (1, -1)]))


VOXEL_FILL = {(0, 0, 0): 1, (2, 3, 0): 2, (0, 3, 0): 9, (3, 3, 0): 100}


def voxel_pair(res, T, seed=3):
    """Target: voxels of 1, 2, 9 and 100 points by construction ((2, 3, 0) and (3, 3, 0) share a face).  Source: points in every one of them,
    1e-3 m on either side of that face and of the outer face of the 100-point voxel (behind which the map is empty), one far outside
    the grid; taken back through T."""
    rng = np.random.default_rng(seed)
    tgt, world = [], []
    for c, cnt in VOXEL_FILL.items():
        lo = (np.array(c) + 0.5) * res  # the voxel of x is floor(x / res - 0.5)
        tgt.append(lo + rng.uniform(0.05, 0.95, (cnt, 3)) * res)
        world.append(lo + rng.uniform(0.05, 0.95, (3, 3)) * res)
    y, z = 3.5 * res + 0.41 * res, 0.5 * res + 0.63 * res
    for face in (3.5 * res, 4.5 * res):
        world.append(np.array([[face - 1e-3, y, z], [face + 1e-3, y, z]]))
    world.append(np.array([[50.0, 50.0, 50.0], [1.5 * res + 0.5 * res, 1.5 * res + 0.5 * res, z]]))  # outside the grid; an empty voxel inside it
    world = np.concatenate(world)
    return cloud4(np.concatenate(tgt)), cloud4((world - T[:3, 3]) @ T[:3, :3])


# ---- preconditions ------------------------------------------------------------------------------------------------------------------
def assert_unambiguous(target, source, T, max_distance):
    q = ga.transform_float(T, source).astype(np.float64)
    t = np.asarray(target)[:, :3].astype(np.float64)
    t = t[np.isfinite(t).all(1)]
    q = q[np.isfinite(q).all(1)]
    d = np.sort(np.sqrt(((q[:, None, :] - t[None, :, :]) ** 2).sum(2)), axis=1)
    assert (d[:, 1] - d[:, 0] > 1e-5 * d[:, 1]).all(), "a query with two nearest target points at equal distance: choose another seed"
    assert (np.abs(d[:, 0] - max_distance) > 1e-5 * max_distance).all(), "a correspondence on the threshold: choose another seed"


def assert_off_the_faces(source, T, res):
    _, u = ga.voxel_coords(T, source, res)
    u = u[np.isfinite(u).all(1)]
    f = u - np.floor(u)
    assert (np.minimum(f, 1 - f) > 1e-9).all(), "a query on a voxel face: choose another seed"


# ---- checks -------------------------------------------------------------------------------------------------------------------------
def compare_hbe(got, want, tag):
    (H, b, e, n), (Hm, bm, em, nm) = got, want
    assert n == nm, f"{tag}: {n} correspondences, the model has {nm}"
    sH, sb, se = np.abs(Hm).max(initial=0.0), np.abs(bm).max(initial=0.0), abs(em)
    dH, db, de = np.abs(H - Hm).max(), np.abs(b - bm).max(), abs(e - em)
    if nm:
        note("H  |dH| / max|H|", dH / sH)
        note("b  |db| / max|b|", db / sb)
        note("e  |de| / |e|", de / se)
    print(f"{tag}: n {n}  dH/max|H| {dH / sH if sH else dH:.2e}  db/max|b| {db / sb if sb else db:.2e}  de/|e| {de / se if se else de:.2e}")
    assert dH <= 1e-12 * sH, f"{tag}: H differs by {dH / sH if sH else dH:.3g} max|H|"
    assert db <= 1e-12 * sb + 1e-9, f"{tag}: b differs by {db:.3g}, max|b| {sb:.3g}"
    assert de <= 1e-12 * se, f"{tag}: e differs by {de / se if se else de:.3g} |e|"


def check_linearize(be, variant, target, source, T, tag, max_distance=2.0, res=1.0, ambiguity_exempt=False):
    """One update_correspondences + linearize of the implementation against the model fed with the implementation's own covariances (so
    that this isolates the linearisation).  Returns the model's (H, b, e, n) and the number of source points."""
    kw = {"resolution": res} if variant == "vgicp" else {"max_correspondence_distance": max_distance}
    reg = load(be.lm(variant, **kw), target, source)
    Ct, Cs = reg.covariances("target"), reg.covariances("source")
    if variant == "vgicp":
        assert_off_the_faces(source, T, res)
        terms, _ = ga.vgicp_terms(target, source, Ct, Cs, T, res)
    else:
        if not ambiguity_exempt:
            assert_unambiguous(target, source, T, max_distance)
        terms, _ = ga.gicp_terms(target, source, Ct, Cs, T, max_distance)
    want = terms.linearize(T, "right" if variant == "small" else "left")
    compare_hbe(be.linearize(reg, T), want, f"{be.name} {variant} {tag}")
    return want, terms


def spectral_gap(w, form):
    """distance of the regularised direction's eigenvalue from the other two over the largest magnitude"""
    if form == "fast":  # ascending: the direction of w0
        return (w[:, 1] - w[:, 0]) / w[:, 2]
    return np.minimum(np.abs(w[:, 0] - w[:, 2]), np.abs(w[:, 1] - w[:, 2])) / np.abs(w[:, 0])  # by descending magnitude: that of the last


def covariances_of(be, form, cloud, k):
    reg = be.lm("fast", correspondence_randomness=k) if form == "fast" else be.pcl(correspondence_randomness=k)
    return load(reg, cloud, cloud).covariances("target")


def check_covariances(be, form, cloud, k, tag):
    """The regularised covariances of a cloud whose neighbourhoods all have a direction of their own to regularise"""
    C = covariances_of(be, form, cloud, k)
    Cm, w = (ga.covariances_fast if form == "fast" else ga.covariances_pcl)(cloud, k)
    gap = spectral_gap(w, form)
    assert gap.min() >= 1e-3, f"{tag}: a neighbourhood with a relative eigen-gap of {gap.min():.3g}: choose another seed"
    worst = (np.abs(C - Cm).max(axis=(1, 2)) * gap).max()
    note(f"C ({form})  |dC| gap", worst)
    print(f"{be.name} {form} covariances {tag}: max |dC| (w1 - w0) / w2 = {worst:.2e}, smallest gap {gap.min():.3g}")
    assert np.isfinite(C).all() and worst <= 1e-13, f"{tag}: |dC| gap = {worst:.3g}"
    return C, Cm


def check_plane(be, form, cloud, normal, origin, k, tag):
    """A planar neighbourhood against the hand-written answer"""
    C = covariances_of(be, form, cloud, k)
    Cm, w = (ga.covariances_fast if form == "fast" else ga.covariances_pcl)(cloud, k)
    want = np.eye(3) - (1 - 1e-3) * np.outer(normal, normal)
    off = np.abs((cloud[:, :3].astype(np.float64) - origin) @ normal).max()
    w1 = np.sort(np.abs(w), axis=1)[:, 1].min()
    bar = 1e-12 + 2 * off / np.sqrt(w1)
    for name, got in ((be.name, C), ("model", Cm)):
        d = np.abs(got - want).max()
        print(f"{name} {form} plane {tag}: |C - (I - (1 - 1e-3) n n^T)| = {d:.2e}, bar {bar:.2e}")
        assert d <= bar, f"{name} {tag}: {d:.3g} > {bar:.3g}"
    return C, Cm, w


def check_degenerate(be, form, cloud, k, tag, direction=None):
    """Neighbourhoods whose regularised matrix is not unique: invariants only"""
    C = covariances_of(be, form, cloud, k)
    assert np.isfinite(C).all(), f"{tag}: non-finite covariance"
    np.testing.assert_array_equal(C, C.transpose(0, 2, 1), err_msg=tag)
    ev = np.linalg.eigvalsh(C)
    d = np.abs(ev - [1e-3, 1.0, 1.0]).max()
    note(f"C ({form}) degenerate |d eig|", d)
    print(f"{be.name} {form} {tag}: eigenvalues off (1e-3, 1, 1) by {d:.2e}")
    assert d <= 1e-12, f"{tag}: eigenvalues off by {d:.3g}"
    if direction is not None:
        q = np.abs(np.einsum("a,nab,b->n", direction, C, direction) - 1.0).max()
        print(f"{be.name} {form} {tag}: |d^T C d - 1| = {q:.2e}")
        assert q <= 1e-9, f"{tag}: d^T C d off 1 by {q:.3g}"


def check_pcl_evaluate(be, target, source, T, x, tag):
    reg = load(be.pcl(), target, source)
    assert_unambiguous(target, source, T, 2.0)
    fm, gm, nm = ga.pcl_cost(target, source, reg.covariances("target"), reg.covariances("source"), T, x)
    f, g, n = reg.evaluate(T, x)
    df, dg = abs(f - fm) / abs(fm), np.abs(g - gm).max() / np.abs(gm).max()
    note("pcl f  |df| / |f|", df)
    note("pcl g  |dg| / max|g|", dg)
    print(f"{be.name} pcl evaluate {tag}: n {n}  df/|f| {df:.2e}  dg/max|g| {dg:.2e}")
    assert n == nm and nm > 0.5 * len(source)
    assert df <= PCL_F_BAR and dg <= PCL_G_BAR, f"{tag}: df {df:.3g} (bar {PCL_F_BAR:.3g}), dg {dg:.3g} (bar {PCL_G_BAR:.3g})"


def check_icp_step(be, target, source, guess, reciprocal, tag):
    reg = load(be.icp(maximum_iterations=1, transformation_epsilon=1e-12, use_reciprocal_correspondences=reciprocal), target, source)
    reg.align(guess)
    want, m = ga.icp_step(target, source, guess, 2.0, reciprocal)
    d = np.abs(reg.getFinalTransformation().astype(np.float64) - want).max()
    note("ICP step  max|dT|", d)
    print(f"{be.name} ICP step {tag}: {m} correspondences, max|dT| {d:.2e}")
    assert reg.getFinalNumIteration() == 1 and m >= 3
    assert d <= ICP_T_BAR, f"{tag}: max|dT| {d:.3g} (bar {ICP_T_BAR:.3g})"
    return want, m


# ---- the cases both files run ---------------------------------------------------------------------------------------------------------
def generic_cloud(n):
    """small_cloud: a ground plane, two walls and clutter — every neighbourhood has a direction of its own (check_covariances asserts it)"""
    return small_cloud(n, {20: 2, 21: 3, 257: 7}.get(n, 7))


def pair_with_dropouts(res):
    """A third of the source 50 m above the scene (beyond max_correspondence_distance; outside the voxel grid), NaN and Inf among the
    source and the target points: (target, source, pose)"""
    T = nudged(LARGE_POSE)
    tgt, src = pair(513, LARGE_POSE)
    third = np.arange(0, len(src), 3)
    src[third, :3] = (src[third, :3].astype(np.float64) + np.array([0, 0, 50.0]) @ LARGE_POSE[:3, :3]).astype(np.float32)  # + 50 m in z of the target frame
    src[[1, 100], 0], src[200, 1], src[301, 2] = np.nan, np.inf, -np.inf
    tgt[[5, 400], 2], tgt[77, 0] = np.nan, np.inf
    return tgt, src, T


def check_threshold(be):
    """A pair at exactly max_correspondence_distance, in floats that square exactly (an offset of 2.0 along x, identity pose): dropped by
    the model and by the implementation; the float below 2.0 is kept."""
    tgt = np.concatenate([small_cloud(600, 5), cloud4([[0.0, 0.25, 64.0], [0.0, 40.25, 64.0], [0.0, 80.25, 64.0]])])  # three points on their own
    below = np.nextafter(np.float32(2.0), np.float32(0.0))
    src = np.concatenate([cloud4([[2.0, 0.25, 64.0], [below, 40.25, 64.0], [0.0, 81.25, 64.0]]), small_cloud(40, 6)])
    for variant in ("fast", "small"):
        (H, b, e, n), terms = check_linearize(be, variant, tgt, src, np.eye(4), "at the threshold", ambiguity_exempt=True)
        j, d = ga.nearest(tgt, ga.transform_float(np.eye(4), src), 2.0)
        assert d[0] == 4.0 and j[0] == -1 and d[1] < 4.0 and j[1] == 601 and j[2] == 602  # exactly on it: dropped; one float below, and well inside: kept


def check_voxel_weights(be, res):
    T = nudged(LARGE_POSE)
    tgt, src = voxel_pair(res, LARGE_POSE)
    (H, b, e, n), terms = check_linearize(be, "vgicp", tgt, src, LARGE_POSE, f"voxel weights res={res}", res=res)
    # by construction: three points in every voxel, and of the two pairs across a face 1e-3 m apart one point each side
    assert sorted(np.round(terms.w ** 2).astype(int)) == sorted([1] * 3 + [2] * 4 + [9] * 3 + [100] * 5)
    check_linearize(be, "vgicp", tgt, src, T, f"voxel weights, off the pose, res={res}", res=res)


def check_planes(be, form):
    """z = 0, a plane tilted by (0.3, 0.4) rad, and the tilted one 360 m away (there pcl::GICP's raw float moments no longer hold the
    plane: the implementation is held against the model, which restates those float products, and not against the hand-written matrix)"""
    for tilt, offset, tag in (((0.0, 0.0), (0, 0, 0), "z=0"), ((0.3, 0.4), (0.25, -0.5, 1.0), "tilted"), ((0.3, 0.4), tuple(FAR), "tilted, far")):
        cloud, normal, origin = lattice(tilt, offset)
        if form == "pcl" and tag == "tilted, far":
            C = covariances_of(be, form, cloud, 20)
            Cm, w = ga.covariances_pcl(cloud, 20)
        else:
            C, Cm, w = check_plane(be, form, cloud, normal, origin, 20, tag)
        gap = spectral_gap(w, form)
        worst = (np.abs(C - Cm).max(axis=(1, 2)) * gap).max()
        note(f"C ({form})  |dC| gap", worst)
        print(f"{be.name} {form} plane {tag}: against the model |dC| gap = {worst:.2e}, smallest gap {gap.min():.3g}")
        assert gap.min() >= 1e-3 and worst <= 1e-13, f"{tag}: |dC| gap = {worst:.3g}"


def check_degenerates(be, form):
    line, d = line_cloud()
    check_degenerate(be, form, line, 20, "points on a line", direction=d)
    check_degenerate(be, form, copies_cloud(), 20, "copies of one point")
    check_degenerate(be, form, octahedron_cloud(), 24, "octahedral blob")


def check_pcl(be):
    """f and g at x with angles of 0.8 - 0.9 rad, a few mm / mrad off the pose the clouds meet at, where the correspondences are found"""
    x0 = np.array([3.0, -2.0, 0.5, 0.9, -0.8, 0.85])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ga._rot(2, x0[5]) @ ga._rot(1, x0[4]) @ ga._rot(0, x0[3]), x0[:3]
    tgt, src = pair(700, T)
    check_pcl_evaluate(be, tgt, src, T, x0 + [0.02, -0.03, 0.01, 0.004, -0.003, 0.005], "large rotation")


def check_icp(be, reciprocal):
    tgt, src = pair(513, LARGE_POSE)
    guess = ga.se3_exp([0.01, -0.005, 0.008, 0.05, -0.03, 0.02]) @ LARGE_POSE
    want, m = check_icp_step(be, tgt, src, guess, reciprocal, "reciprocal" if reciprocal else "plain")
    plain_m = ga.icp_step(tgt, src, guess, 2.0, False)[1]
    assert m == plain_m == len(src) if not reciprocal else m < plain_m  # the mutual test prunes
