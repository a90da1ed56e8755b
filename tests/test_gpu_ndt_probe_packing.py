"""GPU: the one-lane-per-point kinds of the NDT derivative kernels (1 score + gradient, 2 f64 Hessian) on a scene where the lanes of a wavefront disagree
on which of their seven DIRECT7 probes are occupied.

Those kinds walk a point's occupied voxels in probe order, every lane for itself, and each lane's f64 sums must keep their operands and their order whatever
its neighbours in the wavefront see — which a street scene, where consecutive points lie on one surface, hardly probes.  Here the target is a 6 x 6 x 3 m box
whose 1 m voxels are occupied in a checkerboard (so a point's probes alternate between hit and miss and two points one voxel apart see complementary
subsets), with one cell filled in to give a point all seven, four cells cleared to give a point none, and a voxel of five points that must not count
(pclomp's minimum is six).  The 300 source points — two tiles, the second partial — sit close to voxel faces in random order.  Kinds 1 and 2 at two poses
are held bit for bit against the GPU-order oracle at one and at two tiles per item (one item of two tiles, two items)."""
import functools

import numpy as np
import pytest

import ndt_items_cases as K

pytestmark = pytest.mark.gpu

N_SRC = 300
FILLED = (1, 1, 1)  # an odd cell, occupied on top of the checkerboard: it and its six neighbours are occupied
ISOLATED = (5, 5, 1)  # an odd cell whose in-box neighbours are cleared
CLEARED = ((4, 5, 1), (5, 4, 1), (5, 5, 0), (5, 5, 2))
SPARSE = (0, 1, 0)  # an odd cell with five points
OFF7 = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))  # the probe order of the kernels
POSES = ((0.03, -0.02, 0.01, 0.004, -0.003, 0.005), (-0.04, 0.05, -0.02, -0.006, 0.002, -0.004))


def _occupied_cells():
    cells = {(i, j, k) for i in range(6) for j in range(6) for k in range(3) if (i + j + k) % 2 == 0}
    return (cells | {FILLED}) - set(CLEARED)


@functools.lru_cache(maxsize=None)
def target():
    rng = np.random.default_rng(9107)
    pts = [np.array(c) + rng.uniform(0.05, 0.95, (12, 3)) for c in sorted(_occupied_cells())]
    pts.append(np.array(SPARSE) + rng.uniform(0.05, 0.95, (5, 3)))
    t = np.zeros((sum(len(p) for p in pts), 4), dtype=np.float32)
    t[:, :3] = np.concatenate(pts)
    t = t[rng.permutation(len(t))]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def source():
    rng = np.random.default_rng(9108)
    xyz = rng.uniform([0.2, 0.2, 0.2], [5.8, 5.8, 2.8], (N_SRC, 3))
    axis = rng.integers(0, 3, N_SRC)
    face = np.where(axis == 2, rng.integers(1, 3, N_SRC), rng.integers(1, 6, N_SRC))
    xyz[np.arange(N_SRC), axis] = face + rng.choice([-1.0, 1.0], N_SRC) * rng.uniform(0.07, 0.12, N_SRC)  # a step or two of the poses' motion from a face
    xyz[0] = np.array(FILLED) + 0.5
    xyz[1] = np.array(ISOLATED) + 0.5
    xyz[2] = (9.0, 9.0, 9.0)  # outside the grid's box: no probe is even looked up
    xyz[N_SRC - 1] = np.array(FILLED) + (0.5, 0.5, 0.4)  # all seven again, in the partial tile
    s = np.zeros((N_SRC, 4), dtype=np.float32)
    s[:, :3] = xyz
    s.setflags(write=False)
    return s


def _probe_masks(T):
    """per source point the 7-bit mask of its occupied probes at pose T, from the scene as it was laid out (cells of at least six points)"""
    from oracle import oracle as orc

    cells, counts = np.unique(np.floor(target()[:, :3]).astype(int), axis=0, return_counts=True)
    occupied = {tuple(c) for c, n in zip(cells, counts) if n >= 6}
    assert occupied == _occupied_cells() and SPARSE not in occupied
    ijk = np.floor(orc.transform_points(T, source())[:, :3]).astype(int)
    return np.array([sum(1 << n for n, o in enumerate(OFF7) if (c[0] + o[0], c[1] + o[1], c[2] + o[2]) in occupied) for c in ijk])


@functools.lru_cache(maxsize=None)
def _want(pose, ppt):
    from oracle import oracle as orc

    o = orc.Ndt(resolution=1.0, search="DIRECT7", num_threads=8, gpu_order_ppt=ppt)
    assert o.setInputTarget(target()) == 0
    o.setInputSource(source())
    p = np.array(POSES[pose])
    return {mode: o.evaluate(orc.pose_to_matrix(p), p, mode) for mode in (1, 2)}


@pytest.mark.parametrize("pose", [0, 1])
def test_the_scene_has_wavefronts_whose_lanes_disagree(pose):
    """CPU side of the case: without this the comparison below proves nothing.  In every wavefront of the two tiles some probe is occupied for one lane and
    empty for another, a wavefront visits more probes than its busiest lane has voxels, and the source holds a point with all seven and points with none."""
    from oracle import oracle as orc

    masks = _probe_masks(orc.pose_to_matrix(np.array(POSES[pose])))
    count = np.array([bin(m).count("1") for m in masks])
    assert (masks == 0x7F).sum() >= 2 and masks[0] == 0x7F and masks[N_SRC - 1] == 0x7F
    assert masks[1] == 0 and masks[2] == 0
    waves = [masks[a:a + 64] for tile in (0, 256) for a in range(tile, min(tile + 256, N_SRC), 64)]
    assert len(waves) == 5 and len(waves[-1]) == N_SRC - 256
    shorter = 0
    for w in waves:
        union, common = np.bitwise_or.reduce(w), np.bitwise_and.reduce(w)
        assert union != common  # some probe splits the wavefront
        visited, busiest = bin(union).count("1"), max(bin(m).count("1") for m in w)
        assert busiest <= visited
        shorter += int(busiest < visited)
    print(f"pose {pose}: mean occupied probes {count.mean():.2f}, wavefronts whose busiest lane has fewer voxels than the wavefront visits probes: {shorter} of 5")
    assert shorter >= 1


@pytest.mark.parametrize("ppt", [1, 2])
@pytest.mark.parametrize("pose", [0, 1])
def test_point_per_lane_kinds_equal_the_gpu_order_oracle(pose, ppt):
    from mrg_slam_amd import NdtHip
    from oracle import oracle as orc

    g = NdtHip(resolution=1.0, search="DIRECT7")
    assert g.setInputTarget(target()) == 0
    g.setInputSource(source())
    p = np.array(POSES[pose])
    T = orc.pose_to_matrix(p)
    want = _want(pose, ppt)
    assert abs(want[1][0]) > 1.0 and np.abs(want[2][2]).max() > 1.0  # there is something to add up
    for mode in (1, 2):
        sg, gg, Hg = g.evaluate(T, p, mode, ppt=ppt)
        so, go, Ho = want[mode]
        if mode == 1:
            assert K.same_bits([sg], [so]) and K.same_bits(gg, go), (pose, ppt, sg, so, np.abs(gg - go).max())
        else:
            assert K.same_bits(Hg, Ho), (pose, ppt, np.abs(Hg - Ho).max() / np.abs(Ho).max())
