"""Inputs, preconditions and bars that hold the optimisers' steps and trial costs to first principles, shared by
tests/test_optimiser_steps_cpu.py (the oracle against the models) and tests/test_gpu_optimiser_steps.py (the HIP path against them).  The
linearisations, covariances, voxel maps and NDT derivatives are held by tests/gicp_cases.py and tests/ndt_model_cases.py; here it is what
turns those sums into a pose: the frozen-term cost of a Levenberg-Marquardt trial, the joining of many block records, the accepted steps of
the LM loops, ICP's chain of float transformations and NDT's Newton step.

No quantity needs a trace hook: an alignment with maximum_iterations = m is a prefix of the one with m + 1 (the controllers are
deterministic, the sums ordered), so runs with m = 1, 2, 3 ... give the pose after every outer iteration and consecutive poses every step.

DERIVED bars (not from what any code under test gives):
  e            1e-12 max(|e|, 1) up to 800 terms (tests/gicp_cases.py: both sides f64 on f32 inputs, cond(C_B + R C_A R^T) <= 2 / 2e-3,
               n 1e3 2^-53), growing in proportion to n beyond: 1e-12 n / 800 (H and b of a many-block record likewise);
  prefix       exact: one more outer iteration per unit of maximum_iterations, the converged matrix bit for bit afterwards;
  descent      Terms(T_m).cost(T_m+1) <= Terms(T_m).cost(T_m) up to the e bar — the acceptance rule of both LM loops, terms frozen (T_m+1 is
               the float read-out of the accepted pose; on these scenes the cost of the read-out never rises at all);
  NDT length   eps / 2 (1 - 1e-3) <= |delta| <= step_size (1 + 1e-3);  NDT pose arithmetic: 4 ulp_f32 per entry of the rotation block,
               4 ulp_f32 of the largest coordinate on the translation.
MEASURED bars: four quantities pass through float poses and cannot be derived — the residual of the step equation, the floor of the
damping it implies, the ICP chain's max|dT| per m and the angle of the NDT step to the model's Newton direction.  Each is the oracle's
figure against the model, measured by tests/test_optimiser_steps_cpu.py on the CPU and written below beside its constant, times ten (the
margin for a second implementation's rounding, as PCL_F_BAR and ICP_T_BAR of tests/gicp_cases.py).  None comes from the HIP path.

What stays with the oracle comparison: the damping schedule of the LM loops (any damped Gauss-Newton step of the model's (H, b) passes
here), the interior of the More-Thuente line search of NDT — which trial lengths are tried: its upstream form has quirks that belong to
oracle/quirks.h, not to a model — and the BFGS of PCL_GICP_HIP."""
import numpy as np

import gicp_analytic as ga
import gicp_cases as gc
from conftest import small_cloud

SIDE = {"fast": "left", "small": "right", "vgicp": "left"}
VARIANTS = [("fast", 1.0), ("small", 1.0), ("vgicp", 1.0), ("vgicp", 0.37)]
TRIAL_DIRECTION = np.array([0.3, -0.2, 0.5, 1.0, 2.0, -1.0]) / np.linalg.norm([0.3, -0.2, 0.5, 1.0, 2.0, -1.0])
TRIAL_SIZES = (1e-3, 0.05, 0.5)
MANY_BLOCK_SIZES = (14592, 14593, 16385, 33025)  # 57, 58, 65 and 130 workgroups of 256: below, at and past the eight-loads-in-flight loop of the record sum
# noise seeds at which no query of the many-block sources has its two nearest target points within 1e-5 relative (chosen on the CPU by
# many_block_seed(); asserted again wherever a source is drawn)
MANY_BLOCK_SEEDS = {14592: 0, 14593: 0, 16385: 0, 33025: 0}
# rotation_epsilon / transformation_epsilon of the LM trajectories: loose, so that a scene near the origin ends on its second step — the later, shorter
# steps of a tight threshold are of the size of the float poses' rounding (a step of 5e-5 rad / 1e-3 m read from float matrices over points 20 m out
# leaves 3e-3 |b| in the step equation), and a bar measured over them could no longer tell the composition sides apart
ROT_EPS, TRANS_EPS = 1e-2, 0.1

# ---- measured: the oracle against the model (tests/test_optimiser_steps_cpu.py prints them), times ten ---------------------------------
# |(H + lambda I) d + b|_inf / |b|_inf per scene and step, the largest over fast / small / vgicp and 257 / 700 points.  It grows from step to step
# as the steps shrink towards the rounding of the float poses they are read from — 360 m out (far) a rotation entry's last bit moves a point by 2e-5 m.
# None: the oracle's own figure is not well below 1 (far, steps 3 and 4: 0.676 and 0.143 |b| — steps of 1e-5 rad, for which the residual is about |b|
# whatever d is), so the step equation says nothing there and is NOT asserted; prefix, descent and termination still are
STEP_RESIDUAL_ORACLE = {"small": (4.16e-8, 2.05e-6), "large": (7.47e-7, 3.73e-5), "far": (2.53e-6, 2.90e-4, 8.15e-3, None, None, 7.11e-3)}
# -lambda / max diag H, the largest over the steps whose implied damping is negative, per scene
STEP_LAMBDA_ORACLE = {"small": 1.54e-10, "large": 9.85e-9, "far": 2.86e-10}
# max|dT| after m = 1 .. 6 ICP iterations, the largest over plain / reciprocal and both inputs
ICP_CHAIN_ORACLE = (4.77e-7, 2.38e-7, 2.38e-7, 4.77e-7, 2.38e-7, 4.77e-7)  # one and two ulp_f32 of a 3 m translation
# |delta / |delta| - Newton direction| (2-norm) over the steps of every NDT configuration
NDT_DIRECTION_ORACLE = 2.73e-6
STEP_RESIDUAL_BAR = {k: tuple(None if x is None else 10 * x for x in v) for k, v in STEP_RESIDUAL_ORACLE.items()}
STEP_LAMBDA_BAR = {k: 10 * v for k, v in STEP_LAMBDA_ORACLE.items()}
ICP_CHAIN_BAR = tuple(10 * x for x in ICP_CHAIN_ORACLE)
NDT_DIRECTION_BAR = 10 * NDT_DIRECTION_ORACLE


MEASURED = {}  # quantity -> largest discrepancy seen in this process, in units of its bar's scale


def note(quantity, value):
    MEASURED[quantity] = max(MEASURED.get(quantity, 0.0), float(value))


def report(title):
    print(f"\n{title}: largest discrepancy against the first-principles models per quantity")
    for q in sorted(MEASURED):
        print(f"  {q:44s} {MEASURED[q]:.3g}")


def e_bar(n):
    """relative bar of a sum of n terms: 1e-12 up to 800, in proportion to n beyond"""
    return 1e-12 * max(1.0, n / 800.0)


def error_of(reg, T):
    """(cost, terms or None): the oracle returns the sum alone"""
    out = reg.error(np.asarray(T, dtype=np.float64))
    return out if isinstance(out, tuple) else (out, None)


# ---- brute force over blocks of queries -----------------------------------------------------------------------------------------------
def nearest_blocked(target, queries, max_distance, strict=True, block=2048):
    """ga.nearest — float squared distances in the kernels' order, ascending by (distance, index) — over `block` queries at a time"""
    c = np.asarray(target)[:, :3].astype(np.float32)
    ids = np.nonzero(np.isfinite(c).all(1))[0]
    c = c[ids]
    q = np.asarray(queries)[:, :3].astype(np.float32)
    idx, d = np.full(len(q), -1, dtype=np.int64), np.full(len(q), np.inf)
    for s in range(0, len(q), block):
        p = q[s:s + block]
        ok = np.isfinite(p).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = (c[None, :, a] - p[:, None, a] for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
        d2 = np.where(ok[:, None], d2, np.float32(np.inf))
        k = d2.argmin(1)  # the first of equal distances: the lowest index
        idx[s:s + block] = np.where(ok, ids[k], -1)
        d[s:s + block] = np.where(ok, d2[np.arange(len(p)), k].astype(np.float64), np.inf)
    thr = float(max_distance) * float(max_distance)
    idx[(idx >= 0) & (~(d < thr) if strict else (d > thr))] = -1
    return idx, d


def unambiguous(target, source, T, max_distance, block=2048):
    """the precondition of gc.assert_unambiguous as a verdict, over blocks of queries"""
    q = ga.transform_float(T, source).astype(np.float64)
    t = np.asarray(target)[:, :3].astype(np.float64)
    t, q = t[np.isfinite(t).all(1)], q[np.isfinite(q).all(1)]
    for s in range(0, len(q), block):
        d = np.sqrt(((q[s:s + block, None, :] - t[None, :, :]) ** 2).sum(2))
        d = np.partition(d, 1, axis=1)[:, :2]
        if not ((d[:, 1] - d[:, 0] > 1e-5 * d[:, 1]).all() and (np.abs(d[:, 0] - max_distance) > 1e-5 * max_distance).all()):
            return False
    return True


# ---- the frozen terms of a linearisation ----------------------------------------------------------------------------------------------
def frozen_terms(variant, target, source, Ct, Cs, T_corr, T_M, res=1.0, max_distance=2.0):
    """ga.Terms with the correspondences found at T_corr and the Mahalanobis matrices frozen at the rotation of T_M (the linearisation has
    T_corr = T_M; the discriminating-power checks move one of them), and what each source point corresponds to (-1: nothing)"""
    T_corr, R = np.asarray(T_corr, dtype=np.float64), np.asarray(T_M, dtype=np.float64)[:3, :3]
    src = np.asarray(source)[:, :3]
    if variant == "vgicp":
        vox = ga.voxel_map(target, Ct, res)
        cells = list(vox)
        number = {c: k for k, c in enumerate(cells)}
        tA, u = ga.voxel_coords(T_corr, source, res)
        ok = np.isfinite(tA).all(1)
        j = np.full(len(src), -1, dtype=np.int64)
        for i in np.nonzero(ok)[0]:
            j[i] = number.get(tuple(np.floor(u[i]).astype(np.int64)), -1)
        keep = np.nonzero(j >= 0)[0]
        cnt = np.array([vox[c][0] for c in cells], dtype=np.float64)
        mean = np.array([vox[c][1] for c in cells]).reshape(-1, 3)
        cov = np.array([vox[c][2] for c in cells]).reshape(-1, 3, 3)
        mB, CB, w = mean[j[keep]], cov[j[keep]], np.sqrt(cnt[j[keep]])
    else:
        j, _ = nearest_blocked(target, ga.transform_float(T_corr, source), max_distance)
        keep = np.nonzero(j >= 0)[0]
        mB, CB, w = np.asarray(target)[j[keep], :3], np.asarray(Ct)[j[keep]], np.ones(len(keep))
    M = np.linalg.inv(CB + R @ np.asarray(Cs)[keep] @ R.T) if len(keep) else np.zeros((0, 3, 3))
    return ga.Terms(src[keep], mB, M, w), j


def compare_record(got, want, tag, bar):
    """(H, b, e, n) against the model's at the relative bar `bar` (+ 1e-9 absolute on b, as gc.compare_hbe)"""
    (H, b, e, n), (Hm, bm, em, nm) = got, want
    assert n == nm, f"{tag}: {n} correspondences, the model has {nm}"
    sH, sb, se = np.abs(Hm).max(initial=0.0), np.abs(bm).max(initial=0.0), max(abs(em), 1.0)
    dH, db, de = np.abs(H - Hm).max(), np.abs(b - bm).max(), abs(e - em)
    if nm:
        note("record H  |dH| / max|H| / bar", dH / sH / bar)
        note("record b  |db| / max|b| / bar", db / sb / bar)
        note("record e  |de| / |e| / bar", de / se / bar)
    print(f"{tag}: n {n}  dH/max|H| {dH / sH if sH else dH:.2e}  db/max|b| {db / sb if sb else db:.2e}  de/|e| {de / se:.2e}  (bar {bar:.2e})")
    assert dH <= bar * sH, f"{tag}: H differs by {dH / sH if sH else dH:.3g} max|H|"
    assert db <= bar * sb + 1e-9, f"{tag}: b differs by {db:.3g}, max|b| {sb:.3g}"
    assert de <= bar * se, f"{tag}: e differs by {de / se:.3g} |e|"


def linearised(be, variant, target, source, T, tag, res=1.0, max_distance=2.0, check_ambiguity=True):
    """A registration linearised at T and held to the model there: (registration, model terms, (target, source) covariances, selection)"""
    kw = {"resolution": res} if variant == "vgicp" else {"max_correspondence_distance": max_distance}
    reg = gc.load(be.lm(variant, **kw), target, source)
    Ct, Cs = reg.covariances("target"), reg.covariances("source")
    if variant == "vgicp":
        gc.assert_off_the_faces(source, T, res)
    elif check_ambiguity:
        assert unambiguous(target, source, T, max_distance), f"{tag}: an ambiguous correspondence: choose another seed"
    terms, j = frozen_terms(variant, target, source, Ct, Cs, T, T, res, max_distance)
    compare_record(be.linearize(reg, T), terms.linearize(T, SIDE[variant]), f"{be.name} {variant} {tag} linearize", e_bar(len(source)))
    return reg, terms, (Ct, Cs), j


def trial_pose(variant, T_lin, size):
    E = ga.se3_exp(size * TRIAL_DIRECTION)
    return T_lin @ E if SIDE[variant] == "right" else E @ T_lin


# ---- 1 (a), (b): the frozen-term cost at trial poses, and that the case can tell the rules apart ------------------------------------------
def check_trial_costs(be, variant, target, source, T_lin, tag, res=1.0, max_distance=2.0):
    reg, terms, (Ct, Cs), j = linearised(be, variant, target, source, T_lin, tag, res, max_distance)
    n = len(source)
    for size in TRIAL_SIZES:
        T = trial_pose(variant, T_lin, size)
        want = terms.cost(T)
        e, m = error_of(reg, T)
        d = abs(e - want) / max(abs(want), 1.0)
        note("trial cost  |de| / max(|e|, 1) / bar", d / e_bar(n))
        print(f"{be.name} {variant} {tag} |d| = {size}: e {want:.6g}  de/|e| {d:.2e}  terms {len(terms)}")
        assert m is None or m == len(terms), f"{tag}: {m} terms, the model has {len(terms)}"
        assert d <= e_bar(n), f"{tag} |d| = {size}: the trial cost differs by {d:.3g} (bar {e_bar(n):.3g})"
    # a second evaluation at the linearisation pose: the record of the linearisation itself
    e, _ = error_of(reg, T_lin)
    assert abs(e - terms.cost(T_lin)) <= e_bar(n) * max(abs(e), 1.0)
    if len(terms) < 10:
        return  # (a source of one point: nothing to tell apart)
    # (b) from the model alone: at |d| = 0.5 the cost with the correspondences found again, and with M frozen again, is another number
    T = trial_pose(variant, T_lin, TRIAL_SIZES[-1])
    frozen = terms.cost(T)
    refound, j2 = frozen_terms(variant, target, source, Ct, Cs, T, T_lin, res, max_distance)
    refrozen, _ = frozen_terms(variant, target, source, Ct, Cs, T_lin, T, res, max_distance)
    a, b = abs(refound.cost(T) - frozen) / frozen, abs(refrozen.cost(T) - frozen) / frozen
    print(f"  model at |d| = 0.5: correspondences found again {a:.2e}, M frozen again {b:.2e} off the frozen cost; {np.mean(j2 != j):.0%} of the source corresponds elsewhere")
    assert a > 1e-6 and b > 1e-6, f"{tag}: the frozen cost is within 1e-6 of a re-linearised one ({a:.3g}, {b:.3g}): the case tells nothing apart"
    if variant == "vgicp":
        c0, c1 = (np.floor(ga.voxel_coords(P, source, res)[1]) for P in (T_lin, T))
        ok = np.isfinite(c0).all(1) & np.isfinite(c1).all(1)
        assert ((c0 != c1).any(1) & ok).sum() >= 0.1 * len(source), f"{tag}: fewer than 10 % of the source left its voxel"


def pose_case(pose, n):
    """(target, source, linearisation pose) of the three poses the linearisation checks use"""
    T = gc.LARGE_POSE if pose == "large" else gc.SMALL_POSE
    tgt, src = gc.pair(n, T, offset=gc.FAR if pose == "far" else None)
    return tgt, src, gc.nudged(T, gc.FAR if pose == "far" else (0, 0, 0))


# ---- 1 (c): records of 57 .. 130 workgroups --------------------------------------------------------------------------------------------
def many_block_pair(n, seed):
    """The 800-point target and a source of n drawn from it WITH replacement, moved by 5 cm of noise and taken back through SMALL_POSE"""
    tgt = small_cloud(800, 7)
    rng = np.random.default_rng(seed)
    world = tgt[rng.integers(0, len(tgt), n), :3].astype(np.float64) + rng.normal(0, 0.05, (n, 3))
    T = gc.SMALL_POSE
    return tgt, gc.cloud4((world - T[:3, 3]) @ T[:3, :3])


def many_block_seed(n, first=0):
    """the first seed from `first` on at which the source of n points is unambiguous at the linearisation pose"""
    T = gc.nudged(gc.SMALL_POSE)
    for seed in range(first, first + 200):
        tgt, src = many_block_pair(n, seed)
        if unambiguous(tgt, src, T, 2.0):
            return seed
    raise AssertionError("no unambiguous seed")


def check_many_blocks(be, variant, n):
    tgt, src = many_block_pair(n, MANY_BLOCK_SEEDS[n])
    T_lin = gc.nudged(gc.SMALL_POSE)
    reg, terms, _, _ = linearised(be, variant, tgt, src, T_lin, f"n={n} ({(n + 255) // 256} workgroups)")
    assert len(terms) > 0.5 * n
    for size in TRIAL_SIZES:
        T = trial_pose(variant, T_lin, size)
        want = terms.cost(T)
        e, m = error_of(reg, T)
        d = abs(e - want) / max(abs(want), 1.0)
        note("trial cost, many blocks  |de| / |e| / bar", d / e_bar(n))
        print(f"{be.name} {variant} n={n} |d| = {size}: e {want:.6g}  de/|e| {d:.2e} (bar {e_bar(n):.2e})")
        assert m is None or m == len(terms)
        assert d <= e_bar(n), f"n={n} |d| = {size}: the trial cost differs by {d:.3g} (bar {e_bar(n):.3g})"


# ---- 2: the LM trajectories ------------------------------------------------------------------------------------------------------------
def off_guess(T, centre=(0.0, 0.0, 0.0)):
    """T moved by 10 cm / 3 degrees about `centre`: where the trajectories start"""
    C = np.eye(4)
    C[:3, 3] = centre
    w = np.radians(3.0) * np.array([2.0, -1.0, 2.0]) / 3.0
    return C @ ga.se3_exp(np.concatenate([w, [0.06, -0.07, 0.04]])) @ np.linalg.inv(C) @ T


def scene(name, n):
    """(target, source, guess): "small" / "large" — the pair of that pose, the guess 10 cm / 3 degrees off it; "far" — both clouds 360 m out"""
    T = gc.LARGE_POSE if name == "large" else gc.SMALL_POSE
    tgt, src = gc.pair(n, T, offset=gc.FAR if name == "far" else None)
    return tgt, src, off_guess(T, gc.FAR if name == "far" else (0, 0, 0))


def trajectory(be, variant, target, source, guess, res=1.0, m_max=8):
    """The alignments with maximum_iterations = 1 .. m_max (or until one converges, and one more): the records, and the covariances"""
    runs, cov = [], None
    for m in range(1, m_max + 1):
        kw = {"resolution": res} if variant == "vgicp" else {}
        reg = gc.load(be.lm(variant, maximum_iterations=m, transformation_epsilon=TRANS_EPS, rotation_epsilon=ROT_EPS, **kw), target, source)
        reg.align(guess)
        runs.append({"T": reg.getFinalTransformation().copy(), "converged": bool(reg.hasConverged()), "iterations": int(reg.getFinalNumIteration()), "evals": int(reg.evals)})
        cov = cov or (reg.covariances("target"), reg.covariances("source"))
        if len(runs) >= 2 and runs[-2]["converged"]:
            break
    return runs, cov


def step_vector(variant, T0, T1):
    """d with T1 = exp(d) T0 (left) or T0 exp(d) (right)"""
    return ga.se3_log(T1 @ np.linalg.inv(T0)) if SIDE[variant] == "left" else ga.se3_log(np.linalg.inv(T0) @ T1)


def step_equation(H, b, d):
    """(lambda / max diag H, |(H + lambda I) d + b|_inf / |b|_inf) for the damping lambda = -d.(H d + b) / d.d that d implies"""
    lam = -d @ (H @ d + b) / (d @ d)
    return lam / np.abs(np.diag(H)).max(), np.abs((H + lam * np.eye(6)) @ d + b).max() / np.abs(b).max()


def converged_by(variant, d):
    """The termination tests as the step vector shows them: small_gicp |d_rot| <= rotation_epsilon and |d_trans| <= transformation_epsilon; fast_gicp
    (and VGICP) the same bound on the largest entry of exp(d) - I, block by block, strictly.  Returns the verdict and the margins to the thresholds."""
    if SIDE[variant] == "right":
        r, t = np.linalg.norm(d[:3]), np.linalg.norm(d[3:])
        return (r <= ROT_EPS and t <= TRANS_EPS), (r / ROT_EPS, t / TRANS_EPS)
    D = ga.se3_exp(d) - np.eye(4)
    r, t = np.abs(D[:3, :3]).max(), np.abs(D[:3, 3]).max()
    return (r < ROT_EPS and t < TRANS_EPS), (r / ROT_EPS, t / TRANS_EPS)


def check_trajectory(be, variant, name, n, res=1.0):
    target, source, guess = scene(name, n)
    runs, (Ct, Cs) = trajectory(be, variant, target, source, guess, res)
    tag = f"{be.name} {variant} {name} n={n}"
    # -- prefix
    first = next((k for k, r in enumerate(runs) if r["converged"]), None)
    for k, r in enumerate(runs):
        if first is None or k <= first:
            assert r["iterations"] == k, f"{tag}: maximum_iterations = {k + 1} reports iteration {r['iterations']}: the loop gave up (LM not converged)"
            assert k == 0 or r["evals"] > runs[k - 1]["evals"]
        else:
            np.testing.assert_array_equal(r["T"], runs[first]["T"], err_msg=f"{tag}: past convergence")
            assert (r["converged"], r["iterations"], r["evals"]) == (True, runs[first]["iterations"], runs[first]["evals"])
    assert first is not None, f"{tag}: not converged in {len(runs)} iterations: choose another scene"
    poses = [np.asarray(guess).astype(np.float32)] + [r["T"] for r in runs[: first + 1]]
    qualifying = 0
    for k in range(len(poses) - 1):
        T0, T1 = poses[k].astype(np.float64), poses[k + 1].astype(np.float64)
        if variant == "vgicp":
            gc.assert_off_the_faces(source, T0, res)
        else:
            gc.assert_unambiguous(target, source, T0, 2.0)
        terms, _ = frozen_terms(variant, target, source, Ct, Cs, T0, T0, res)
        H, b, e0, m = terms.linearize(T0, SIDE[variant])
        d = step_vector(variant, T0, T1)
        # -- the step equation, where the float poses resolve the step
        qualifies = np.linalg.norm(d[3:]) > 1e3 * float(np.spacing(np.float32(np.abs(T0[:3, 3]).max())))
        assert qualifies or k >= 2, f"{tag}: step {k} is too short to be read from float poses: choose another scene"
        if qualifies:
            qualifying += 1
            lam, res_eq = step_equation(H, b, d)
            note(f"LM step {name} {k}  residual of (H + lambda I) d = -b", res_eq)
            if k < len(STEP_RESIDUAL_BAR[name]) and STEP_RESIDUAL_BAR[name][k] is not None:
                note(f"LM step {name}  -lambda / max diag H", max(-lam, 0.0))
            print(f"{tag} step {k}: |d| rot {np.linalg.norm(d[:3]):.3e} trans {np.linalg.norm(d[3:]):.3e}  lambda / max diag H {lam:.3e}  residual {res_eq:.3e}")
            assert k < len(STEP_RESIDUAL_BAR[name]), f"{tag}: a step {k} the measured trajectories do not have"
            bar = STEP_RESIDUAL_BAR[name][k]
            if bar is not None:  # (None: a step too short for the equation to say anything, see STEP_RESIDUAL_ORACLE)
                assert lam >= -STEP_LAMBDA_BAR[name], f"{tag} step {k}: implied damping {lam:.3g} max diag H (bar {-STEP_LAMBDA_BAR[name]:.3g})"
                assert res_eq <= bar, f"{tag} step {k}: residual of the step equation {res_eq:.3g} |b| (bar {bar:.3g})"
        # -- descent, terms frozen
        e1, slack = terms.cost(T1), e_bar(n) * max(abs(e0), 1.0)
        note("LM descent  (e1 - e0) / max(|e0|, 1) / bar", max(e1 - e0, 0.0) / slack)
        assert e1 <= e0 + slack, f"{tag} step {k}: the frozen-term cost rose from {e0:.12g} to {e1:.12g} (e bar {slack:.3g})"
        # -- termination
        verdict, margins = converged_by(variant, d)
        norms = (np.linalg.norm(d[:3]) / ROT_EPS, np.linalg.norm(d[3:]) / TRANS_EPS)
        assert all(abs(x - 1.0) > 1e-3 for x in margins + norms), f"{tag} step {k}: a step norm on a threshold: choose another scene"
        assert verdict == (norms[0] <= 1 and norms[1] <= 1), f"{tag} step {k}: the entries of exp(d) - I and the norms of d fall on different sides: choose another scene"
        assert runs[k]["converged"] == verdict, f"{tag}: hasConverged {runs[k]['converged']} after step {k} with |d| / eps = {norms}"
    assert qualifying >= 2
    return runs


def check_wrong_side_is_told_apart(variant, n=700):
    """From the model alone, on the large-rotation scene: a damped Gauss-Newton step of the model's (H, b) composed on the variant's side, read on
    the OTHER side, misses the step equation by more than 100 times its bar."""
    target, source, guess = scene("large", n)
    T0 = np.asarray(guess).astype(np.float32).astype(np.float64)
    Ct, Cs = ga.covariances_fast(target)[0], ga.covariances_fast(source)[0]
    terms, _ = frozen_terms(variant, target, source, Ct, Cs, T0, T0)
    H, b, _, _ = terms.linearize(T0, SIDE[variant])
    d = np.linalg.solve(H + 1e-9 * np.abs(np.diag(H)).max() * np.eye(6), -b)
    T1 = ga.se3_exp(d) @ T0 if SIDE[variant] == "left" else T0 @ ga.se3_exp(d)
    own = step_equation(H, b, step_vector(variant, T0, T1))[1]
    other = step_equation(H, b, step_vector("small" if SIDE[variant] == "left" else "fast", T0, T1))[1]
    print(f"model {variant}: residual of the step equation on its own side {own:.2e}, on the other {other:.2e}")
    bar = max(STEP_RESIDUAL_BAR["large"])  # (every step of that scene is held to the equation: no None among them)
    assert own <= 1e-9 and other > 100 * bar, f"{variant}: the wrong side leaves {other:.3g} |b|, 100 x bar is {100 * bar:.3g}"


# ---- 3: ICP chains ---------------------------------------------------------------------------------------------------------------------
ICP_STEPS = 6


def icp_inputs(which):
    """"near": the inputs of gc.check_icp; "changing": a guess 0.4 m / 0.15 rad off, whose correspondence set is another at step 3 than at step 1"""
    tgt, src = gc.pair(513, gc.LARGE_POSE)
    if which == "near":
        return tgt, src, ga.se3_exp([0.01, -0.005, 0.008, 0.05, -0.03, 0.02]) @ gc.LARGE_POSE
    return tgt, src, ga.se3_exp([0.1, -0.08, 0.07, 0.3, -0.2, 0.15]) @ gc.LARGE_POSE


def assert_unambiguous_points(cloud, queries, max_distance):
    """gc.assert_unambiguous for points as they are (float64 distances): no query with its two nearest points of `cloud` within 1e-5 relative, none
    with its nearest on the threshold"""
    c, q = np.asarray(cloud)[:, :3].astype(np.float64), np.asarray(queries)[:, :3].astype(np.float64)
    c, q = c[np.isfinite(c).all(1)], q[np.isfinite(q).all(1)]
    d = np.sort(np.sqrt(((q[:, None, :] - c[None, :, :]) ** 2).sum(2)), axis=1)
    assert (d[:, 1] - d[:, 0] > 1e-5 * d[:, 1]).all(), "a target point with two nearest source points at equal distance: choose another seed"
    assert (np.abs(d[:, 0] - max_distance) > 1e-5 * max_distance).all(), "a reciprocal correspondence on the threshold: choose another seed"


def check_icp_chain(be, which, reciprocal):
    tgt, src, guess = icp_inputs(which)
    poses = ga.icp_chain(tgt, src, guess, ICP_STEPS, 2.0, reciprocal)
    sets = []
    for k in range(ICP_STEPS):
        gc.assert_unambiguous(tgt, src, poses[k], 2.0)
        cur, j = ga.icp_correspondences(tgt, src, poses[k], 2.0, reciprocal)
        if reciprocal:  # the search back — a target point's nearest source point as transformed so far — has ties of its own to rule out
            fwd = ga.nearest(tgt, cur, 2.0, strict=False)[0]
            assert_unambiguous_points(cur, np.asarray(tgt)[np.unique(fwd[fwd >= 0]), :3], 2.0)
        sets.append(j)
        assert (sets[-1] >= 0).sum() >= 3
    if which == "changing":
        changed = int((sets[0] != sets[2]).sum())
        print(f"ICP {which} reciprocal={reciprocal}: {changed} of {len(src)} source points correspond elsewhere at step 3 than at step 1")
        assert changed >= 10
    worst, runs = [], []
    for m in range(1, ICP_STEPS + 1):
        reg = gc.load(be.icp(maximum_iterations=m, transformation_epsilon=1e-12, use_reciprocal_correspondences=reciprocal), tgt, src)
        reg.align(guess)
        it, T = reg.getFinalNumIteration(), reg.getFinalTransformation()
        if it != m:  # pcl's criteria ended the loop earlier (the mean squared distance stopped changing): the earlier run, bit for bit
            assert runs and it == runs[-1][0] < m, f"ICP {which}: maximum_iterations = {m} reports {it} iterations"
            np.testing.assert_array_equal(T, runs[-1][1])
        runs.append((it, T))
        # against the model's pose after m steps, whether or not the loop ended earlier: where it did, the model's chain has to stand still as well
        d = np.abs(T.astype(np.float64) - poses[m].astype(np.float64)).max()
        worst.append(d)
        note(f"ICP chain  max|dT| after {m}", d)
        assert d <= ICP_CHAIN_BAR[m - 1], f"ICP {which} reciprocal={reciprocal}: max|dT| {d:.3g} for maximum_iterations = {m}, {it} run (bar {ICP_CHAIN_BAR[m - 1]:.3g})"
    assert runs[-1][0] >= (ICP_STEPS if which == "changing" else 3)
    print(f"{be.name} ICP chain {which} reciprocal={reciprocal}: max|dT| per m " + " ".join(f"{d:.2e}" for d in worst))
    return worst


# ---- 4: NDT Newton steps ---------------------------------------------------------------------------------------------------------------
NDT_CONFIGS = [("ndt", "DIRECT7", 1.0), ("ndt", "KDTREE", 1.0), ("ndt", "DIRECT7", 0.5), ("ndt", "KDTREE", 0.5), ("pcl", None, 1.0)]
NDT_EPS, NDT_STEP = 0.01, 0.1


def pose_to_matrix(p):
    """T = Translation(p[:3]) Rx(p[3]) Ry(p[4]) Rz(p[5]), in double"""
    import ndt_analytic

    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ndt_analytic.rotation_derivatives(np.asarray(p, dtype=np.float64)[3:])[0], np.asarray(p, dtype=np.float64)[:3]
    return T


def euler_xyz(T):
    """p with pose_to_matrix(p) = T, angles in (-pi / 2, pi / 2): R = Rx(a) Ry(b) Rz(c) has R02 = sin b, R12 = -sin a cos b, R22 = cos a cos b,
    R01 = -cos b sin c, R00 = cos b cos c"""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    return np.concatenate([np.asarray(T, dtype=np.float64)[:3, 3],
                           [np.arctan2(-R[1, 2], R[2, 2]), np.arctan2(R[0, 2], np.hypot(R[0, 0], R[0, 1])), np.arctan2(-R[0, 1], R[0, 0])]])


def ndt_case(res):
    """the dense 20,000-point target and its 400-point source, the guess 0.3 m / 0.03 rad off, the model's leaves (for the centroids of the radius search)"""
    import ndt_model_cases as nm

    tgt, src, rel, model = nm.dense_case(res, False)
    return tgt, src, pose_to_matrix(euler_xyz(rel) + [0.2, -0.2, 0.1, 0.02, -0.02, 0.01]), model


def ndt_registration(be, kind, search, res, m, **kw):
    if be.name == "oracle":
        from oracle import oracle as orc

        if kind == "pcl":
            return orc.PclNdt(resolution=res, transformation_epsilon=NDT_EPS, step_size=NDT_STEP, maximum_iterations=m)
        return orc.Ndt(resolution=res, transformation_epsilon=NDT_EPS, step_size=NDT_STEP, maximum_iterations=m, search=search, num_threads=1)
    import mrg_slam_amd as M

    if kind == "pcl":
        return M.PclNdtHip(resolution=res, transformation_epsilon=NDT_EPS, step_size=NDT_STEP, maximum_iterations=m, **kw)
    return M.NdtHip(resolution=res, transformation_epsilon=NDT_EPS, step_size=NDT_STEP, maximum_iterations=m, search=search, **kw)


def ndt_runs(be, kind, search, res):
    """The alignments with maximum_iterations = 0 .. 5: [(iterations, float matrix, converged)] in the order of m, and the last registration"""
    tgt, src, guess, _ = ndt_case(res)
    out = []
    for m in range(6):
        reg = ndt_registration(be, kind, search, res, m)
        assert reg.setInputTarget(tgt) == 0
        reg.setInputSource(src)
        reg.align(guess)
        out.append((int(reg.getFinalNumIteration()), reg.getFinalTransformation().copy(), bool(reg.hasConverged())))
    return out, reg


def check_ndt_steps(be, kind, search, res):
    import ndt_analytic
    import ndt_leaves_model as M
    from oracle import oracle as orc

    tgt, src, guess, model = ndt_case(res)
    runs, reg = ndt_runs(be, kind, search, res)
    tag = f"{be.name} {kind} {search} res={res}"
    by_count = {}
    for it, T, _ in runs:  # runs that report the same count are the same alignment: the iteration limit was not what ended them
        if it in by_count:
            np.testing.assert_array_equal(T, by_count[it], err_msg=f"{tag}: two alignments of {it} iterations")
        by_count[it] = T
    if 1 in by_count:  # (pcl::NormalDistributionsTransform ends after ONE Newton iteration at these settings — its test is on the SQUARED step, oracle/quirks.h —
        if 0 in by_count:  # whatever the limit: the alignment of no iteration is the float guess it starts from)
            np.testing.assert_array_equal(by_count[0], np.asarray(guess).astype(np.float32), err_msg=f"{tag}: an alignment of no iteration that is not the guess")
        by_count.setdefault(0, np.asarray(guess).astype(np.float32))
    counts = sorted(by_count)
    assert len(counts) >= 2 and all(b - a == 1 for a, b in zip(counts, counts[1:])), f"{tag}: iteration counts {counts}"
    lv = reg.leaves()
    keys, mean, icov = lv[0], lv[-3] if len(lv) == 6 else lv[2], lv[-2] if len(lv) == 6 else lv[-1]
    np.testing.assert_array_equal(keys, model.keys)
    in_search = model.n >= M.MIN_POINTS
    resf = float(np.float32(res))
    if kind == "pcl":  # the model settings of tests/test_oracle_pclndt.py: the radius search over the centroids alone, every leaf it holds
        grid, leaves = ([0, 0, 0], [0, 0, 0], [1, 1, 1]), (keys, np.where(in_search, 6, 0), mean, icov)
    else:
        grid, leaves = reg.grid(), (keys, lv[1], mean, icov)
    for a, b in zip(counts, counts[1:]):
        T0, T1 = by_count[a], by_count[b]
        p0, p1 = euler_xyz(T0), euler_xyz(T1)
        delta = p1 - p0
        xt = orc.transform_points(T0, src)[:, :3]  # the float-transformed cloud the derivatives are taken at
        nb = ndt_analytic.radius_lists(xt, model.centroid, in_search, resf) if kind == "pcl" or search == "KDTREE" else None
        s, g, H = ndt_analytic.evaluate(src[:, :3], p0, search, resf, grid, leaves, transformed=xt, upstream_d1_sign=True, nb_lists=nb)
        assert abs(s) > 1e-3
        # -- direction: Newton's, turned to ascend the score
        newton = np.linalg.solve(H, -g)
        newton = newton / np.linalg.norm(newton) * (1.0 if g @ newton > 0 else -1.0)
        length = np.linalg.norm(delta)
        off = np.linalg.norm(delta / length - newton)
        note("NDT step  |delta / |delta| - Newton direction|", off)
        print(f"{tag} step {a} -> {b}: |delta| {length:.5f}  off the Newton direction by {off:.3e}  (flipped: {g @ np.linalg.solve(H, -g) < 0})")
        assert off <= NDT_DIRECTION_BAR, f"{tag} step {a}: {off:.3g} off the model's Newton direction (bar {NDT_DIRECTION_BAR:.3g})"
        # -- length: the clamp of the line search
        assert NDT_EPS / 2 * (1 - 1e-3) <= length <= NDT_STEP * (1 + 1e-3), f"{tag} step {a}: |delta| = {length:.6g}"
        # -- pose arithmetic: the matrix of p + delta
        want = pose_to_matrix(p0 + delta)
        dR = np.abs(T1[:3, :3].astype(np.float64) - want[:3, :3]).max() / float(np.spacing(np.float32(1.0)))
        dt = np.abs(T1[:3, 3].astype(np.float64) - want[:3, 3]).max() / float(np.spacing(np.float32(np.abs(want[:3, 3]).max())))
        note("NDT pose  rotation block, ulp_f32", dR)
        note("NDT pose  translation, ulp_f32 of the largest", dt)
        assert dR <= 4 and dt <= 4, f"{tag} step {a}: T differs from the matrix of p + delta by {dR:.2f} / {dt:.2f} ulp_f32"
    return runs
