"""GPU: ``mrgfe_reg_matching_status`` — ScanMatchingOdometryComponent::publish_scan_matching_status
(apps/scan_matching_odometry_component.cpp:391-431) as one device pass — gives the bits of the two calls it replaces
(``getFitnessScore()`` and the count over ``nearestKSearch`` of the aligned cloud), counts strictly, agrees with a brute-force search,
and follows the registration's target through the keyframe hand-over.

Targets are 4096 points on three noisy planes (a floor and two walls, dense enough for 1 m NDT voxels); sources are perturbed subsets
of them, moved by the inverse of a small pose so that ``align`` has something to find.  Everything is drawn from fixed seeds."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ["NDT_OMP", "FAST_GICP"]
DBL_MAX = np.finfo(np.float64).max


def _planes(n, seed, shift=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    n_floor = n * 55 // 100
    n_wall = (n - n_floor) // 2
    c = np.zeros((n, 4), dtype=np.float32)
    c[:n_floor, 0] = rng.uniform(-6, 6, n_floor)
    c[:n_floor, 1] = rng.uniform(-6, 6, n_floor)
    c[n_floor:n_floor + n_wall, 0] = 6.0
    c[n_floor:n_floor + n_wall, 1] = rng.uniform(-6, 6, n_wall)
    c[n_floor:n_floor + n_wall, 2] = rng.uniform(0, 3, n_wall)
    rest = n - n_floor - n_wall
    c[n_floor + n_wall:, 0] = rng.uniform(-6, 6, rest)
    c[n_floor + n_wall:, 1] = -6.0
    c[n_floor + n_wall:, 2] = rng.uniform(0, 3, rest)
    c[:, :3] += rng.normal(0, 0.02, (n, 3))
    c[:, :3] += np.float32(shift)
    c[:, 3] = rng.uniform(0, 255, n)
    return rng.permutation(c).astype(np.float32)


def _true_pose():
    from mrg_slam_amd import synth

    return synth.make_pose([0.15, -0.1, 0.03], synth.rot_xyz(0.002, -0.001, 0.01))


def _guess():
    from mrg_slam_amd import synth

    return synth.make_pose([0.13, -0.08, 0.02], synth.rot_xyz(0.0, 0.0, 0.008))


def _into_source_frame(pts):
    """The cloud ``pts`` (target frame) as the sensor would see it from ``_true_pose()``."""
    Ti = np.linalg.inv(_true_pose())
    out = pts.copy()
    out[:, :3] = (pts[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return out


def _source(target, n, seed, offsets=None):
    """n points of the target with 1 cm of noise (``offsets``: per-point displacement added on top), in the source frame."""
    rng = np.random.default_rng(seed)
    s = target[rng.choice(len(target), n, replace=n > len(target))].copy()
    s[:, :3] += rng.normal(0, 0.01, (n, 3)).astype(np.float32)
    if offsets is not None:
        s[:, :3] += offsets.astype(np.float32)
    return _into_source_frame(s)


def _make(method, ctx=None, **kw):
    from mrg_slam_amd import select_registration_method

    return select_registration_method({"registration_method": method, **kw}, ctx=ctx)


@pytest.fixture(scope="module")
def target():
    return _planes(4096, 1)


@pytest.fixture(scope="module")
def delta():
    from mrg_slam_amd import synth

    return synth.make_pose([0.2, -0.05, 0.01], synth.rot_xyz(0.0, 0.001, 0.012)).astype(np.float32)


def _relations(reg, aligned, dist=0.5, delta=None):
    """Case 1's relations between the status and the calls it replaces; returns the record."""
    from mrg_slam_amd.registration import status_poses

    n = len(aligned)
    st = reg.matchingStatus(dist, delta)
    fit = reg.getFitnessScore()
    _, sqd = reg.nearestKSearch1(aligned)
    inliers = int(np.count_nonzero(sqd.astype(np.float64) < dist * dist))
    print(f"n {n} dist {dist}: matching_error {st.matching_error!r} fitness {fit!r} inliers {st.num_inliers} expected {inliers}")
    assert np.float64(st.matching_error).tobytes() == np.float64(fit).tobytes(), (st.matching_error, fit)
    assert st.num_inliers == inliers
    assert st.n_points == n
    assert np.float32(st.inlier_fraction).tobytes() == (np.float32(inliers) / np.float32(n)).tobytes()
    assert st.has_converged == reg.hasConverged()
    rel, err = status_poses(reg.getFinalTransformation(), delta)
    assert st.relative_pose.tobytes() == rel.tobytes()
    if delta is None:
        assert st.prediction_error is None
    else:
        assert st.prediction_error.tobytes() == err.tobytes()
    return st


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_same_bits_as_fitness_and_the_nearest_search(target, delta, method, n):
    """One below, at and one above the workgroup (256) and the sum slice (1024), then three slices."""
    reg = _make(method)
    reg.setInputTarget(target)
    reg.setInputSource(_source(target, n, 100 + n))
    aligned = reg.align(_guess(), want_aligned=True)
    st = _relations(reg, aligned, 0.5, delta)
    _relations(reg, aligned, 0.5, None)
    if n >= 255:
        assert st.num_inliers > n // 2 and st.matching_error < 0.05  # the pair does match: the counts are not trivially zero


@pytest.mark.parametrize("method", METHODS)
def test_every_pass_reaches_the_count(target, method):
    """A third of the source 0.3 m, a third 3 m and a third 40 m off the target: the block pass, the seed + sweep and the walk each settle some."""
    from mrg_slam_amd import Context

    ctx = Context()
    n = 1536
    off = np.zeros((n, 3))
    off[0::3, 2] = 0.3
    off[1::3, 2] = 3.0
    off[2::3, 2] = 40.0
    reg = _make(method, ctx=ctx)
    reg.setInputTarget(target)
    reg.setInputSource(_source(target, n, 7, off))
    aligned = reg.align(_guess(), want_aligned=True)
    counts = []
    for dist in (0.5, 5.0, 100.0):
        calls = ctx.fitness_stats()["calls"]
        st = reg.matchingStatus(dist)
        stats = ctx.fitness_stats()
        assert stats["calls"] == calls + 1  # one set of fitness passes per status
        assert stats["queries"] == n and stats["queued"] > 0, stats  # the sweep or the walk saw queries
        counts.append(_relations(reg, aligned, dist).num_inliers)
        assert st.num_inliers == counts[-1]
    print("inliers at 0.5 / 5 / 100 m:", counts)
    assert counts[0] <= counts[1] <= counts[2] == n


@pytest.mark.parametrize("method", METHODS)
def test_the_comparison_is_strict(method):
    """sqd < max_correspondence_dist^2 with the float distance promoted to double: 0.25f < 0.25 is false."""
    rng = np.random.default_rng(5)
    tgt = np.zeros((41, 4), dtype=np.float32)
    ang = rng.uniform(0, 2 * np.pi, 40)
    rad = rng.uniform(10, 20, 40)
    tgt[1:, 0], tgt[1:, 1], tgt[1:, 2] = rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1, 1, 40)
    src = np.zeros((3, 4), dtype=np.float32)
    src[0, 0] = 0.5
    src[1, 0] = np.float32(0.49999997)
    src[2, 1] = np.float32(0.5000001)
    reg = _make(method)  # freshly created: the final transformation is the identity
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    _, sqd = reg.nearestKSearch1(src)
    assert sqd[0] == np.float32(0.25) and sqd[1] < np.float32(0.25) < sqd[2]
    st = reg.matchingStatus(0.5)
    assert (st.n_points, st.num_inliers) == (3, 1)
    assert st.inlier_fraction == np.float32(1) / np.float32(3)
    assert st.matching_error == reg.getFitnessScore()
    assert st.relative_pose.tolist() == [0, 0, 0, 0, 0, 0, 1] and not st.has_converged


@pytest.mark.parametrize("method", METHODS)
def test_against_brute_force(target, method):
    n = 1500
    rng = np.random.default_rng(9)
    off = np.zeros((n, 3))
    # 60 % on the surfaces, the rest 0.3 m or 0.7 m off them along z, up and down alike so that the alignment is not biased
    off[:, 2] = rng.choice([0.0, 0.0, 0.0, 0.3, -0.3, 0.7, -0.7, 0.0, 0.0, 0.0], n)
    reg = _make(method)
    reg.setInputTarget(target)
    reg.setInputSource(_source(target, n, 10, off))
    aligned = reg.align(_guess(), want_aligned=True)
    a, t = aligned[:, :3], target[:, :3]
    d = np.empty(n, dtype=np.float32)
    for i in range(0, n, 250):
        diff = a[i:i + 250, None, :] - t[None, :, :]
        d[i:i + 250] = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]).min(axis=1)
    margin = np.abs(d.astype(np.float64) - 0.25).min() / 0.25
    print(f"{method}: closest brute-force distance to the threshold, relative {margin:.3g}")
    assert margin > 1e-4, "the generator put a distance on the threshold"
    want_inliers = int(np.count_nonzero(d.astype(np.float64) < 0.25))
    want_error = float(d.astype(np.float64).mean())
    st = reg.matchingStatus(0.5)
    print(f"{method}: inliers {st.num_inliers} / {want_inliers}, matching_error {st.matching_error!r} / {want_error!r}")
    assert st.num_inliers == want_inliers and 0 < want_inliers < n
    assert abs(st.matching_error - want_error) <= 1e-6 * want_error


def test_large_launch_form(target):
    """2^20 + 1025 queries: above the size at which the passes leave their many-small-workgroups form."""
    n = (1 << 20) + 1025
    rng = np.random.default_rng(13)
    reps = (n + len(target) - 1) // len(target)
    src = np.tile(target, (reps, 1))[:n].copy()
    src[:, :3] += rng.normal(0, 0.02, (n, 3)).astype(np.float32)
    reg = _make("NDT_OMP", reg_maximum_iterations=2)
    reg.setInputTarget(target)
    reg.setInputSource(_into_source_frame(src))
    aligned = reg.align(_guess(), want_aligned=True)
    st = _relations(reg, aligned, 0.5)
    assert st.num_inliers > n // 2


@pytest.mark.parametrize("method", METHODS)
def test_empty_clouds_and_state(target, method):
    from mrg_slam_amd import MrgfeError, _lib

    reg = _make(method)
    reg.setInputTarget(target)
    s = _lib.MatchingStatus()
    assert _lib.lib().mrgfe_reg_matching_status(reg._h, 0.5, None, C.byref(s)) == _lib.ERR_STATE  # before set_source
    with pytest.raises(MrgfeError) as e:
        reg.matchingStatus()
    assert e.value.status == _lib.ERR_STATE
    reg.setInputSource(np.zeros((0, 4), dtype=np.float32))
    st = reg.matchingStatus()
    assert (st.n_points, st.num_inliers) == (0, 0) and np.isnan(st.inlier_fraction) and st.matching_error == DBL_MAX
    empty_target = _make(method)
    assert _lib.lib().mrgfe_reg_matching_status(empty_target._h, 0.5, None, C.byref(s)) == _lib.ERR_STATE  # no target either
    empty_target.setInputTarget(np.zeros((0, 4), dtype=np.float32))
    empty_target.setInputSource(target[:100])
    st = empty_target.matchingStatus()
    assert (st.n_points, st.num_inliers) == (100, 0) and st.inlier_fraction == 0 and st.matching_error == DBL_MAX


@pytest.mark.parametrize("method", METHODS)
def test_after_the_source_became_the_target(target, method):
    """The hand-over of the keyframe update (:333): the status searches the grid of the NEW target."""
    reg = _make(method)
    reg.setInputTarget(target)
    other = _planes(3000, 2, shift=(2.0, 1.0, 0.0))  # overlaps the first scene in part only
    reg.setInputSource(other)
    reg.align(np.eye(4))
    reg.sourceBecomesTarget()
    n = 1025
    reg.setInputSource(_source(other, n, 21))
    aligned = reg.align(_guess(), want_aligned=True)
    st = _relations(reg, aligned, 0.5)
    a = aligned[:, :3].astype(np.float64)
    d_new = np.array([((other[:, :3] - p) ** 2).sum(axis=1).min() for p in a])
    d_old = np.array([((target[:, :3] - p) ** 2).sum(axis=1).min() for p in a])
    print(f"{method}: matching_error {st.matching_error!r}, brute force on the new target {d_new.mean()!r}, on the old one {d_old.mean()!r}")
    assert d_old.mean() > 10 * d_new.mean()  # the two targets tell the cases apart
    assert abs(st.matching_error - d_new.mean()) <= 1e-5 * d_new.mean()  # (f64 distances here against the kernel's float ones)


@pytest.mark.parametrize("method", METHODS)
def test_odometry_status_is_the_last_frame(target, delta, method):
    from mrg_slam_amd.odometry import ScanMatchingOdometry
    from mrg_slam_amd.registration import status_poses

    reg = _make(method)
    odo = ScanMatchingOdometry(reg)
    odo.matching(0.0, target)
    frames = [_source(target, n, 30 + k) for k, n in enumerate((2000, 1500, 1777))]
    small = np.eye(4, dtype=np.float32)
    for k, f in enumerate(frames):
        odo.matching(0.1 * (k + 1), f, msf_delta=small if k < 2 else delta)
    assert odo.keyframes == 1  # 0.18 m of motion: the first cloud is still the keyframe
    st = odo.status(msf_delta=delta)
    assert st.n_points == 1777 and st.has_converged == odo.last_converged
    assert st.matching_error == reg.getFitnessScore()
    rel, err = status_poses(reg.getFinalTransformation(), delta)
    assert st.relative_pose.tobytes() == rel.tobytes() and st.prediction_error.tobytes() == err.tobytes()
    direct = reg.matchingStatus(0.5, delta)
    assert (direct.num_inliers, direct.matching_error) == (st.num_inliers, st.matching_error) and st.num_inliers > 1000
    assert odo.status().prediction_error is None
