"""What tests/test_ndt_leaves_cpu.py (the oracle) and tests/test_gpu_ndt_leaves.py (the HIP kernels) both assert of a library's NDT leaves against
tests/ndt_leaves_model.py: the scenes (one per leaf size and origin, computed once), the tolerances measured on the reference alone, the checks.  The
figures and their derivation are in the docstring of tests/test_ndt_leaves_cpu.py."""
import functools

import numpy as np
import ndt_leaves_model as M

RESOLUTIONS = [1.0, 0.5, 0.37, 2.0]
ORIGINS = [(0.0, 0.0, 0.0), (-37.3, 12.9, -2.2), (2500.0, -1800.0, 40.0)]
ORIGIN_IDS = ["origin", "near", "far"]


@functools.lru_cache(maxsize=None)
def case(res, origin, seed=0):
    """(cloud, model leaves, tolerances) of one scene: computed once, shared, never written to"""
    cloud, _ = M.scene(res, origin, seed)
    cloud.setflags(write=False)
    model = M.build(cloud, res)
    return cloud, model, M.tolerances(cloud, model)


def check_scene_is_live(model):
    cnt = dict(zip(*np.unique(model.cls, return_counts=True)))
    assert 40 <= len(model.keys) <= 60 and model.n.sum() < 5000
    assert cnt.get("rank_deficient", 0) >= 8 and cnt.get("marginal", 0) == 0
    for c in ("few", "regular", "thin", "point"):
        assert cnt.get(c, 0) >= 3, cnt


def check_leaves_against_model(model, tol, keys, npts, mean, icov, grid=None, pcl_rule=False):
    """everything the model can hold of one library's leaves (the class outcomes of `point` and rank-deficient leaves under PCL's rule apart)"""
    np.testing.assert_array_equal(keys, model.keys)
    np.testing.assert_array_equal(np.where(npts < 0, model.n, npts), model.n)
    assert ((npts >= 0) | (model.n >= M.MIN_POINTS)).all()  # only a leaf that reached the covariance can be rejected
    if grid is not None:
        for a, b in zip(grid, model.grid):
            np.testing.assert_array_equal(a, b)
    dm = M.rel_dev(mean, model.mean)
    print(f"mean: worst deviation {dm.max():.3e}, tolerance {tol['mean']:.3e}")
    assert dm.max() <= tol["mean"]
    acc = npts >= M.MIN_POINTS
    few = model.cls == "few"
    assert not acc[few].any() and (icov[few] == 0).all() and (npts[few] == model.n[few]).all()
    full = np.isin(model.cls, ("regular", "thin"))
    assert acc[full].all()
    assert not acc[model.cls == "point"].any()
    assert (icov[~acc] == 0).all()  # a rejected leaf keeps the zero inverse covariance
    d = M.rel_dev(icov[full], model.icov[full])
    print(f"icov, regular and thin: worst deviation {d.max():.3e}, tolerance {tol['icov']:.3e} (reference alone {tol['measured']['icov']:.3e})")
    assert d.max() <= tol["icov"]
    rd = (model.cls == "rank_deficient") & acc
    if rd.any():
        d = M.rel_dev(icov[rd], model.icov[rd])
        print(f"icov, {rd.sum()} accepted rank-deficient: worst deviation {d.max():.3e}, tolerance {tol['icov_rank_deficient']:.3e}")
        assert d.max() <= tol["icov_rank_deficient"]
    return acc


def check_pcl_rule_outcomes(model, npts):
    acc = npts >= M.MIN_POINTS
    rd, pt = model.cls == "rank_deficient", model.cls == "point"
    print(f"PCL rule: {acc[rd].sum()} of {rd.sum()} rank-deficient leaves accepted, {acc[pt].sum()} of {pt.sum()} point leaves accepted")
    want = np.array(model.accepted_prediction(pcl_rule=True), dtype=object)
    has = np.array([w is not None for w in want])
    np.testing.assert_array_equal(acc[has], want[has].astype(bool))


