"""The first-principles derivative check off the unit grid, shared by tests/test_oracle_ndt.py (the oracle) and tests/test_gpu_ndt.py (the HIP
kernels): a dense cloud (20,000 points of small_cloud in extent (6, 4, 2): at least 300 accepted leaves at every leaf size used, a score far from
underflow), as it is or shifted by (-37.3, 12.9, -2.2), a 400-point source, and tests/ndt_analytic.py evaluated with the library's leaves or with
those tests/ndt_leaves_model.py makes from the raw points."""
import functools

import numpy as np

import ndt_analytic
import ndt_leaves_model as M
from conftest import small_cloud

RESOLUTIONS = [1.0, 0.5, 0.37, 2.0]
SHIFT = (-37.3, 12.9, -2.2)


@functools.lru_cache(maxsize=None)
def dense_case(res, shifted, n_src=400):
    """(target, source, relative pose, model leaves): computed once per (leaf size, origin, source size), shared, never written to"""
    from mrg_slam_amd import synth
    from oracle import oracle as orc

    tgt = small_cloud(20000, 31, extent=(6.0, 4.0, 2.0))
    if shifted:
        tgt[:, :3] += np.array(SHIFT, dtype=np.float32)
    rel = synth.make_pose([0.3, -0.2, 0.05], synth.rot_xyz(0.02, -0.03, 0.06))
    src = orc.transform_points(np.linalg.inv(rel), tgt[:n_src])
    tgt.setflags(write=False)
    src.setflags(write=False)
    return tgt, src, rel, (M.build(tgt, res) if n_src == 400 else dense_case(res, shifted)[3])  # (the leaves are the target's alone)


@functools.lru_cache(maxsize=None)
def leaf_bound(res, shifted):
    tgt, _, _, model = dense_case(res, shifted)
    return M.tolerances(tgt, model)


def check_derivatives(reg, res, search, shifted, model_leaves=False, n_src=400, evaluate=None):
    """`reg`: an oracle Ndt or an NdtHip made with this resolution and search; `n_src`: source points (1300 = six tiles of 256); `evaluate`: one callable
    (reg, T, p, mode) -> (score, gradient, Hessian) or several, each held to the same model values (default: reg.evaluate).  Score within 2e-6, float-path gradient and Hessian within 1e-4 of the
    largest entry, the f64 Hessian pass within 1e-11 of it — with the library's own leaves.  With the MODEL's leaves (made from the raw points) the
    inverse covariances differ from the library's by the single-pass bound of tests/test_ndt_leaves_cpu.py (ndt_leaves_model.tolerances, measured on this
    very cloud, factor 8 included: 8e-11 at 0.5 and 1.8e-10 at 0.37 at the origin, 6.3e-9 and 1.4e-8 shifted), and a pair's exponent d2/2 q^T C q moves by that times ||C|| ||q||^2: the f64 tolerance becomes
    1e-11 + bound * max ||C|| ||q||^2 over the pairs used (computed below from the model: 1.5e-7 ... 7e-5, a worst case over every pair — the
    deviations seen are 3e-13 ... 1e-11; the float-path tolerances stay).  The model runs in longdouble, so its own rounding is out of the comparison."""
    from oracle import oracle as orc

    tgt, src, rel, model = dense_case(res, shifted, n_src)
    resf = float(np.float32(res))  # the library holds the resolution as a float
    assert reg.setInputTarget(tgt) == 0
    reg.setInputSource(src)
    lv = reg.leaves()
    keys, npts, mean, icov = lv[0], lv[1], lv[2], lv[-1]
    np.testing.assert_array_equal(keys, model.keys)
    assert (npts >= M.MIN_POINTS).sum() >= (300 if res == min(RESOLUTIONS) else 30)  # dense at the finest leaf size, never a handful
    f64_tol = 1e-11
    if model_leaves:
        assert np.isin(model.cls, ("few", "regular", "thin")).all()  # nothing whose outcome the model cannot predict
        leaves, grid = model.for_evaluate(), model.grid
    else:
        leaves, grid = (keys, npts, mean, icov), reg.grid()
    rng = np.random.default_rng(5)
    # a pose near the true one: 0.1 m and 0.02 rad off at the origin; 40 m out the same angle would move the points by 0.8 m, two cells of 0.37
    p = np.concatenate([rel[:3, 3] + rng.normal(0, 0.1, 3), np.array([0.02, -0.03, 0.06]) + rng.normal(0, 0.002 if shifted else 0.02, 3)])
    T = orc.pose_to_matrix(p)
    xt = orc.transform_points(T, src)[:, :3]  # the reference's float-transformed cloud
    nb = ndt_analytic.radius_lists(xt, model.centroid, model.n >= M.MIN_POINTS, resf) if search == "KDTREE" else None
    st = {}
    sa, ga, Ha = ndt_analytic.evaluate(src[:, :3], p, search, resf, grid, leaves, transformed=xt, upstream_d1_sign=True, nb_lists=nb, stats=st, dtype=np.longdouble)
    assert abs(sa) > 1e-3 and st["pairs"] >= 200  # far from the underflow of a sparse grid
    if model_leaves:
        f64_tol += leaf_bound(res, shifted)["icov"] * st["max_icov_q2"]
    for ev in ([lambda r, *a: r.evaluate(*a)] if evaluate is None else [evaluate] if callable(evaluate) else list(evaluate)):
        s0, g0, H0 = ev(reg, T, p, 0)
        _, _, H2 = ev(reg, T, p, 2)
        print(f"res {res} {search} shifted={shifted} model_leaves={model_leaves}: pairs {st['pairs']} score {sa:.6g} rel {abs(s0 - sa) / abs(sa):.2e} "
              f"grad {np.abs(g0 - ga).max() / np.abs(ga).max():.2e} H {np.abs(H0 - Ha).max() / np.abs(Ha).max():.2e} "
              f"H64 {np.abs(H2 - Ha).max() / np.abs(Ha).max():.2e} (tolerance {f64_tol:.2e}, max |C| |q|^2 {st['max_icov_q2']:.3g})")
        assert abs(s0 - sa) <= 2e-6 * abs(sa)
        np.testing.assert_allclose(g0, ga, rtol=0, atol=1e-4 * np.abs(ga).max())
        np.testing.assert_allclose(H0, Ha, rtol=0, atol=1e-4 * np.abs(Ha).max())
        np.testing.assert_allclose(H2, Ha, rtol=0, atol=f64_tol * np.abs(Ha).max())


def check_face_lookup(reg, res, search):
    """getNeighborhoodAtPoint's cell, floor(f32(x) / f32(leaf)) in FLOAT, for source points on and next to cell faces of the dense cloud (x or y at
    f32(k leaf) and the floats beside it, identity pose so that the transformed point is the source point): at least 20 of them lie in another cell by
    that rule than by exact arithmetic, and a library that put one elsewhere would add another voxel's Gaussian — score within 2e-6 of the model's,
    gradient and Hessian as everywhere."""
    tgt, _, _, model = dense_case(res, False)
    resf = np.float32(res)
    rng = np.random.default_rng(11)
    src = tgt[rng.choice(len(tgt), 400, replace=False)].copy()
    min_b, max_b, _ = model.grid
    for a in (0, 1):
        ks = rng.integers(min_b[a] + 1, max_b[a], 200)
        face = (ks.astype(np.float32) * resf).astype(np.float32)
        step = rng.choice([-1, 0, 1], 200, p=[0.2, 0.7, 0.1])  # the rule and the exact cell part where f32(k leaf) itself lies just below k leaf
        face = np.where(step > 0, np.nextafter(face, np.float32(np.inf)), np.where(step < 0, np.nextafter(face, np.float32(-np.inf)), face))
        src[a * 200:(a + 1) * 200, a] = face
    fl, ex = M.cell_of(src[:, :3], res, rule="lookup")
    differ = (fl != ex).any(1)
    print(f"leaf {res}: {differ.sum()} of {len(src)} face points change cell under the float lookup rule")
    assert differ.sum() >= 20
    assert reg.setInputTarget(tgt) == 0
    reg.setInputSource(src)
    lv = reg.leaves()
    leaves = (lv[0], lv[1], lv[2], lv[-1])
    p = np.zeros(6)
    sa, ga, Ha = ndt_analytic.evaluate(src[:, :3], p, search, float(resf), reg.grid(), leaves, transformed=src[:, :3], upstream_d1_sign=True, dtype=np.longdouble)
    # the same points by the exact cell: another score, or the case would not tell the rules apart
    shifted_src = src[:, :3] + (ex - fl) * (0.01 * float(resf))
    se = ndt_analytic.evaluate(src[:, :3], p, search, float(resf), reg.grid(), leaves, transformed=shifted_src.astype(np.float32), upstream_d1_sign=True)[0]
    assert abs(sa) > 1e-3 and abs(se - sa) > 1e-5 * abs(sa)
    s0, g0, H0 = reg.evaluate(np.eye(4), p, 0)
    _, _, H2 = reg.evaluate(np.eye(4), p, 2)
    print(f"  score {sa:.6g} rel {abs(s0 - sa) / abs(sa):.2e}; with exact cells the score would be {abs(se - sa) / abs(sa):.2e} off")
    assert abs(s0 - sa) <= 2e-6 * abs(sa)
    np.testing.assert_allclose(g0, ga, rtol=0, atol=1e-4 * np.abs(ga).max())
    np.testing.assert_allclose(H0, Ha, rtol=0, atol=1e-4 * np.abs(Ha).max())
    np.testing.assert_allclose(H2, Ha, rtol=0, atol=1e-11 * np.abs(Ha).max())
