"""CPU: the ICP loop of the product (csrc/gicp_engine.h IcpController — the one controller behind IcpHip and the ICP batches) stepped by hand through
mrgfe_dbg_icp_ctl_*, no GPU involved.  The 17 moment sums it asks for are computed here in numpy (brute-force float32 nearest neighbour, pcl's
`distance > max_dist^2` rule, f64 sums) and every returned step is applied to the working copy in float32; the loop must end where the CPU
oracle's pcl::IterativeClosestPoint ends."""
import ctypes as C

import numpy as np
import pytest

from conftest import small_cloud
from icp_cases import icp_params, make_pairs, pose_errors

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _move(T, xyz):
    """pcl::transformPointCloud's float path: x' = m0 x + (m1 y + (m2 z + m3))"""
    T = np.asarray(T, dtype=np.float32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([T[r, 0] * x + (T[r, 1] * y + (T[r, 2] * z + T[r, 3])) for r in range(3)], 1).astype(np.float32)


def _sums(cur, tgt, max_dist, reciprocal=False):
    """the record of one correspondence round: count, sum src, sum dst, sum dst src^T (row-major), sum of squared distances"""
    out = np.zeros(17)
    if len(cur) == 0 or len(tgt) == 0:
        return out
    d = cur[:, None, :] - tgt[None, :, :]  # float32
    sq = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    j = np.argmin(sq, axis=1)  # ties: the lowest index
    dist = sq[np.arange(len(cur)), j]
    keep = ~(dist.astype(np.float64) > max_dist * max_dist)
    if reciprocal:
        back = np.argmin(sq, axis=0)
        keep &= (back[j] == np.arange(len(cur))) & ~(sq[back[j], j].astype(np.float64) > max_dist * max_dist)
    s, t = cur[keep].astype(np.float64), tgt[j[keep]].astype(np.float64)
    out[0] = keep.sum()
    out[1:4], out[4:7] = s.sum(0), t.sum(0)
    out[7:16] = (t.T @ s).reshape(-1)
    out[16] = dist[keep].astype(np.float64).sum()
    return out


class Ctl:
    def __init__(self, params, guess, n_src, n_tgt):
        from mrg_slam_amd._lib import check, lib

        self._lib, self._check = lib(), check
        self._h = C.c_void_p()
        g = np.ascontiguousarray(np.asarray(guess, dtype=np.float32).T)
        check(self._lib.mrgfe_dbg_icp_ctl_create(C.byref(params), g.ctypes.data_as(_fp), n_src, n_tgt, C.byref(self._h)))

    def result(self, sums):
        """-> (done, row-major Tm)"""
        s = np.ascontiguousarray(sums, dtype=np.float64)
        done, Tm = C.c_int(0), np.empty((4, 4), dtype=np.float32)
        self._check(self._lib.mrgfe_dbg_icp_ctl_result(self._h, s.ctypes.data_as(_dp), C.byref(done), Tm.ctypes.data_as(_fp)))
        return bool(done.value), Tm.T.copy()

    def final(self):
        T, conv, it, ev = np.empty((4, 4), dtype=np.float32), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.mrgfe_dbg_icp_ctl_final(self._h, T.ctypes.data_as(_fp), C.byref(conv), C.byref(it), C.byref(ev)))
        return T.T.copy(), bool(conv.value), it.value, ev.value

    def close(self):
        self._lib.mrgfe_dbg_icp_ctl_destroy(self._h)
        self._h = None


def _drive(params, tgt, src, guess, max_steps=200):
    ctl = Ctl(params, guess, len(src), len(tgt))
    cur = _move(guess, src[:, :3]) if len(src) else src[:, :3]
    try:
        for _ in range(max_steps):
            done, Tm = ctl.result(_sums(cur, tgt[:, :3], params.max_correspondence_distance, bool(params.use_reciprocal_correspondences)))
            if done:
                return ctl.final()
            cur = _move(Tm, cur)
        raise AssertionError("the controller did not end")
    finally:
        ctl.close()


def _pair():
    tgt = small_cloud(300, 300)
    (_, src, guess), = make_pairs([tgt], [200])
    return tgt, src, guess


@pytest.mark.parametrize("reciprocal", [False, True])
def test_hand_stepped_controller_ends_where_the_oracle_ends(reciprocal):
    from oracle import oracle as orc

    tgt, src, guess = _pair()
    p = icp_params(reciprocal)
    T, conv, it, ev = _drive(p, tgt, src, guess)
    o = orc.Icp(transformation_epsilon=p.transformation_epsilon, use_reciprocal_correspondences=reciprocal)
    o.setInputTarget(tgt)
    o.setInputSource(src)
    o.align(guess)
    print(f"reciprocal={reciprocal}: controller {it} iterations converged={conv}, oracle {o.getFinalNumIteration()} converged={o.hasConverged()}, "
          f"errors {pose_errors(T, o.getFinalTransformation())}")
    assert conv == o.hasConverged() and it == o.getFinalNumIteration()
    assert it >= 3 and ev == it  # several steps, one correspondence round each
    dt, dr = pose_errors(T, o.getFinalTransformation())
    assert dt <= 1e-4 and dr <= 1e-4


def test_fewer_than_three_correspondences_end_the_loop_unconverged():
    tgt, src, guess = _pair()
    p = icp_params()
    for n_src, n_tgt, sums in ((200, 300, None), (0, 300, np.zeros(17)), (200, 0, np.zeros(17))):
        ctl = Ctl(p, guess, n_src, n_tgt)
        if sums is None:  # two correspondences only: the sums of a 2-point source
            sums = _sums(_move(guess, src[:2, :3]), tgt[:, :3], p.max_correspondence_distance)
            assert sums[0] == 2
        done, Tm = ctl.result(sums)
        T, conv, it, ev = ctl.final()
        assert done and not conv and it == 0 and ev == 1
        np.testing.assert_array_equal(Tm, np.eye(4, dtype=np.float32))
        np.testing.assert_array_equal(T, np.asarray(guess, dtype=np.float32))
        from mrg_slam_amd import MrgfeError

        with pytest.raises(MrgfeError):  # the loop has ended
            ctl.result(sums)
        ctl.close()


def test_the_iteration_limit_counts_as_converged():
    tgt, src, guess = _pair()
    T, conv, it, ev = _drive(icp_params(eps=1e-12, maximum_iterations=1), tgt, src, guess)
    assert conv and it == 1 and ev == 1
    assert not np.array_equal(T, np.asarray(guess, dtype=np.float32))
    T2, conv2, it2, _ = _drive(icp_params(eps=1e-12, maximum_iterations=2), tgt, src, guess)
    assert conv2 and it2 == 2


def test_an_unchanged_mean_squared_error_ends_the_loop():
    """An exact rigid copy with transformation_epsilon = -1, which pcl takes as it comes: the rotation test wants a cosine >= 2 and the translation test a
    square <= -1, so no step meets them, and what ends the loop — long before the iteration limit — is |mse - previous mse| < 1e-12 once the distances have
    vanished.  The oracle does the same."""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    tgt = small_cloud(300, 300)
    rel = synth.make_pose([0.05, -0.03, 0.01], synth.rot_xyz(0.004, -0.002, 0.006))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:200])
    p = icp_params(eps=-1.0)
    ctl = Ctl(p, np.eye(4), len(src), len(tgt))
    cur, mses = src[:, :3].copy(), []
    for _ in range(64):
        sums = _sums(cur, tgt[:, :3], p.max_correspondence_distance)
        mses.append(sums[16] / sums[0])
        done, Tm = ctl.result(sums)
        if done:
            break
        cur = _move(Tm, cur)
    T, conv, it, ev = ctl.final()
    ctl.close()
    assert conv and 2 <= it < 64 and ev == it
    assert abs(mses[-1] - mses[-2]) < 1e-12 and all(abs(a - b) >= 1e-12 for a, b in zip(mses[:-2], mses[1:-1]))  # the mse rule fired, at its first chance
    dt, dr = pose_errors(T, rel)
    assert dt <= 1e-4 and dr <= 1e-4
    o = orc.Icp(transformation_epsilon=-1.0)
    o.setInputTarget(tgt)
    o.setInputSource(src)
    o.align(np.eye(4))
    assert o.hasConverged() and o.getFinalNumIteration() == it
