"""CPU: the state machine behind mrgfe_odom_frame (csrc/odom_ctl.h: ScanMatchingOdometryComponent::matching, apps/scan_matching_odometry_component.cpp:195-350)
stepped through mrgfe_dbg_odom_ctl_* with scripted (converged, final) outcomes, no GPU involved.

1. Bit-exact model: the arithmetic the issue fixes — 4 x 4 float products row times column with k ascending and every product and sum rounded, the rigid
   inverse (R^T, -R^T t) of the thresholding delta, float norms, quat_w — restated below in np.float32 SCALAR operations (one rounding each); guess, odom,
   keyframe pose and prev_trans of every frame equal it bit for bit.
2. Decisions against the mirror: outcome, new_keyframe, consecutive_rejections and the keyframe stamp equal mrg_slam_amd.odometry.ScanMatchingOdometry over
   a scripted fake registration, over 240 seeded sequences of 12 frames that reach every branch; no compared quantity of the mirror lies within 1e-3
   relative of its threshold (asserted, nothing is skipped: the mirror multiplies with BLAS and inverts with LAPACK, so it can differ from the float
   restatement in the last bits, never by 1e-3).
3. A failed frame (begun and never ended, or ended without a final transformation) leaves the state byte-equal and the later frames unchanged.
4. tests/sanitize/odom_ctl_san.cpp: the header alone under AddressSanitizer + UndefinedBehaviorSanitizer, NaN / non-rigid finals included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FP = C.POINTER(C.c_float)
N_SEQ, N_FRAMES = 240, 12
# the seeds: picked so that the margin condition of item 2 holds for every sequence (it is asserted below) — these seven of 7000..7246 draw a frame that
# comes within 2e-3 relative of a threshold and are left out
NEAR_A_THRESHOLD = {7015, 7036, 7043, 7133, 7144, 7172, 7243}
SEEDS = [s for s in range(7000, 7000 + N_SEQ + len(NEAR_A_THRESHOLD)) if s not in NEAR_A_THRESHOLD]
assert len(SEEDS) == N_SEQ
MARGIN = 1e-3


# ---- the scripted scenario of one seed ------------------------------------------------------------------------------------------------------------
def rigid(rng, ang, trans):
    """a float32 rigid transform: rotation by `ang` about a random axis, translation of length `trans` in a random direction"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    t = rng.normal(size=3)
    t *= trans / np.linalg.norm(t)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


def scenario(seed):
    rng = np.random.default_rng(seed)
    mode = seed % 4  # 0 drives, 1 turns on the spot, 2 stands still (keyframes by time), 3 mixed
    params = {
        "keyframe_delta_translation": 1.0, "keyframe_delta_angle": 0.3, "keyframe_delta_time": 2.6,
        "enable_transform_thresholding": bool(seed % 3), "max_acceptable_translation": 0.9, "max_acceptable_angle": 0.5,
        "max_consecutive_rejections": 1 + (seed // 4) % 3,
    }
    frames = []
    burst = 0
    for k in range(N_FRAMES):
        step_t = {0: rng.uniform(0.2, 0.4), 1: rng.uniform(0.0, 0.02), 2: rng.uniform(0.0, 0.01), 3: rng.uniform(0.05, 0.3)}[mode]
        step_a = {0: rng.uniform(0.0, 0.03), 1: rng.uniform(0.05, 0.12), 2: rng.uniform(0.0, 0.005), 3: rng.uniform(0.0, 0.09)}[mode]
        if burst == 0 and k > 0 and rng.random() < 0.2:
            burst = int(rng.integers(1, 4))  # 1 to 3 jumping frames in a row
        jump = burst > 0
        burst = max(0, burst - 1)
        frames.append({
            "stamp": 50.0 + 0.45 * k + float(rng.uniform(0, 0.01)),
            "converged": bool(k == 0 or rng.random() > 0.12),
            "step": rigid(rng, step_a, step_t),
            "jump": rigid(rng, rng.uniform(0.7, 1.2), rng.uniform(1.5, 3.0)) if jump else None,
            "msf_delta": rigid(rng, 0.01, 0.05) if rng.random() < 0.5 else None,
        })
    return params, frames


class FakeRegistration:
    """pcl::Registration's call surface with scripted results: the final transformation is the motion since the keyframe (it starts over whenever a target is
    set), a jumping frame adds a large step that is forgotten again when the odometry rejects it."""

    def __init__(self, frames):
        self.frames, self.k = frames, 0
        self.cum = np.eye(4, dtype=np.float32)
        self.guesses, self.finals = [], []

    def setInputTarget(self, cloud):
        self.cum = np.eye(4, dtype=np.float32)

    def setInputSource(self, cloud):
        pass

    def align(self, guess):
        f = self.frames[self.k]
        self.guesses.append(np.array(guess, dtype=np.float32))
        self.cum = (self.cum.astype(np.float64) @ f["step"].astype(np.float64)).astype(np.float32)
        self.final = self.cum if f["jump"] is None else (self.cum.astype(np.float64) @ f["jump"].astype(np.float64)).astype(np.float32)
        self.converged = f["converged"]
        self.finals.append(self.final.copy())

    def hasConverged(self):
        return self.converged

    def getFinalTransformation(self):
        return self.final


def mirror_quantities(m, stamp, trans):
    """What the mirror compares on a converged frame, from its state BEFORE the frame, as odometry.py forms them."""
    from mrg_slam_amd.odometry import rotation_angle

    d = (np.linalg.inv(m.prev_trans).astype(np.float32) @ trans).astype(np.float32)
    return {
        "dx": (float(np.linalg.norm(d[:3, 3].astype(np.float32))), m.p["max_acceptable_translation"]),
        "da": (rotation_angle(d), m.p["max_acceptable_angle"]),
        "d_translation": (float(np.linalg.norm(trans[:3, 3])), m.p["keyframe_delta_translation"]),
        "d_angle": (rotation_angle(trans), m.p["keyframe_delta_angle"]),
        "d_time": (stamp - m.keyframe_stamp, m.p["keyframe_delta_time"]),
    }


def run_mirror(seed):
    """The mirror over the scenario: per frame its decisions, the branch it took, and the margin of every quantity it compared."""
    from mrg_slam_amd.odometry import ScanMatchingOdometry

    params, frames = scenario(seed)
    reg = FakeRegistration(frames)
    m = ScanMatchingOdometry(reg, params)
    rows = []
    for k, f in enumerate(frames):
        reg.k = k
        before = {"keyframes": m.keyframes, "rej": m.consecutive_rejections}
        first = m.keyframe_cloud is None
        prev_state = (m.prev_trans.copy(), m.keyframe_stamp)
        odom = m.matching(f["stamp"], np.zeros((1, 4), np.float32), f["msf_delta"])
        row = {"odom": np.array(odom, dtype=np.float32), "new_keyframe": m.keyframes > before["keyframes"], "rej": m.consecutive_rejections, "keyframe_stamp": m.keyframe_stamp,
               "branches": set(), "margins": []}
        if first:
            row["outcome"] = "first_frame"
        elif not m.last_converged:
            row["outcome"] = "not_converged"
        else:
            trans = reg.finals[-1]
            shadow = type("S", (), {"prev_trans": prev_state[0], "keyframe_stamp": prev_state[1], "p": m.p})
            q = mirror_quantities(shadow, f["stamp"], trans)
            rejected = False
            if m.p["enable_transform_thresholding"]:
                row["margins"] += [q["dx"], q["da"]]
                rejected = q["dx"][0] > q["dx"][1] or q["da"][0] > q["da"][1]
            else:
                row["branches"].add("thresholding_off")
            if rejected:
                row["outcome"] = "rejected_reset" if row["new_keyframe"] else "rejected"
            else:
                row["outcome"] = "accepted"
                row["margins"] += [q["d_translation"], q["d_angle"], q["d_time"]]
                if before["rej"] > 0:
                    row["branches"].add("accepted_after_rejections")
                for name in ("d_translation", "d_angle", "d_time"):
                    if q[name][0] > q[name][1]:
                        row["branches"].add("keyframe_by_" + name[2:])
        row["branches"].add(row["outcome"])
        rows.append(row)
    return params, frames, reg, rows


# ---- the arithmetic of csrc/odom_ctl.h in float32 scalar operations (row-major 4 x 4 arrays of np.float32) -------------------------------------------
def f_mul(A, B):
    out = np.zeros((4, 4), dtype=np.float32)
    for r in range(4):
        for c in range(4):
            s = F(A[r, 0] * B[0, c])
            for k in range(1, 4):
                s = F(s + F(A[r, k] * B[k, c]))
            out[r, c] = s
    return out


def f_rigid_inverse(M):
    out = np.zeros((4, 4), dtype=np.float32)
    for r in range(3):
        for c in range(3):
            out[r, c] = M[c, r]
        s = F(F(F(-M[0, r]) * M[0, 3]) + F(F(-M[1, r]) * M[1, 3]))
        out[r, 3] = F(s + F(F(-M[2, r]) * M[2, 3]))
    out[3, 3] = F(1)
    return out


def f_norm(M):
    s = F(F(M[0, 3] * M[0, 3]) + F(M[1, 3] * M[1, 3]))
    return float(np.sqrt(F(s + F(M[2, 3] * M[2, 3])), dtype=np.float32))


def f_angle(M):
    from mrg_slam_amd.odometry import quat_w

    w = quat_w(M[:3, :3])
    w = w if w > F(-1) else F(-1)
    w = w if w < F(1) else F(1)
    return float(np.arccos(F(w)))


class Model:
    def __init__(self, p):
        self.p = p
        self.has_keyframe = False
        self.keyframe_pose = np.eye(4, dtype=np.float32)
        self.prev_trans = np.eye(4, dtype=np.float32)
        self.keyframe_stamp = 0.0
        self.rej = 0

    def guess(self, msf_delta):
        if not self.has_keyframe:
            return np.eye(4, dtype=np.float32)
        return f_mul(self.prev_trans, np.eye(4, dtype=np.float32) if msf_delta is None else msf_delta)

    def _switch(self, odom, stamp):
        self.keyframe_pose, self.keyframe_stamp, self.prev_trans = odom, stamp, np.eye(4, dtype=np.float32)

    def end(self, stamp, converged, trans):
        """-> (outcome, new_keyframe, odom, keyframe_pose as :323 reads it)"""
        if not self.has_keyframe:
            self.has_keyframe, self.keyframe_stamp = True, stamp
            return "first_frame", True, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
        kp = self.keyframe_pose
        if not converged:
            return "not_converged", False, f_mul(kp, self.prev_trans), kp
        odom = f_mul(kp, trans)
        if self.p["enable_transform_thresholding"]:
            d = f_mul(f_rigid_inverse(self.prev_trans), trans)
            if f_norm(d) > self.p["max_acceptable_translation"] or f_angle(d) > self.p["max_acceptable_angle"]:
                self.rej += 1
                if self.rej >= self.p["max_consecutive_rejections"]:
                    self._switch(odom, stamp)
                    self.rej = 0
                    return "rejected_reset", True, odom, kp
                return "rejected", False, f_mul(kp, self.prev_trans), kp
            self.rej = 0
        self.prev_trans = trans
        new = f_norm(trans) > self.p["keyframe_delta_translation"] or f_angle(trans) > self.p["keyframe_delta_angle"] or stamp - self.keyframe_stamp > self.p["keyframe_delta_time"]
        if new:
            self._switch(odom, stamp)
        return "accepted", new, odom, kp


# ---- the controller through the C ABI ------------------------------------------------------------------------------------------------------------------
class Ctl:
    def __init__(self, params):
        from mrg_slam_amd import _lib

        self.L = _lib.lib()
        p = _lib.OdomParams()
        self.L.mrgfe_odom_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        self.h = C.c_void_p()
        assert self.L.mrgfe_dbg_odom_ctl_create(C.byref(p), C.byref(self.h)) == 0

    def __del__(self):
        self.L.mrgfe_dbg_odom_ctl_destroy(self.h)

    def begin(self, stamp, msf_delta):
        g = np.zeros(16, dtype=np.float32)
        aligns = C.c_int(-1)
        d = None if msf_delta is None else np.ascontiguousarray(msf_delta.T)
        assert self.L.mrgfe_dbg_odom_ctl_begin(self.h, stamp, None if d is None else d.ctypes.data_as(FP), C.byref(aligns), g.ctypes.data_as(FP)) == 0
        return bool(aligns.value), g.reshape(4, 4).T.copy()

    def end(self, converged, final, expect=0):
        from mrg_slam_amd import _lib

        r = _lib.OdomResult()
        f = None if final is None else np.ascontiguousarray(final.T)
        assert self.L.mrgfe_dbg_odom_ctl_end(self.h, int(converged), None if f is None else f.ctypes.data_as(FP), C.byref(r)) == expect
        return r

    def state(self):
        from mrg_slam_amd import _lib

        s = _lib.OdomState()
        assert self.L.mrgfe_dbg_odom_ctl_state(self.h, C.byref(s)) == 0
        return s


def mat(a):
    return np.array(a, dtype=np.float32).reshape(4, 4).T.copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


OUTCOMES = ("first_frame", "accepted", "not_converged", "rejected", "rejected_reset")


@pytest.fixture(scope="module")
def mirrors():
    return {seed: run_mirror(seed) for seed in SEEDS}


def test_sequences_stay_clear_of_every_threshold_and_reach_every_branch(mirrors):
    reached = {}
    for seed, (_, _, _, rows) in mirrors.items():
        for k, row in enumerate(rows):
            for value, threshold in row["margins"]:
                assert abs(value - threshold) > MARGIN * abs(threshold), (seed, k, value, threshold)
            for b in row["branches"]:
                reached[b] = reached.get(b, 0) + 1
    for branch in ("first_frame", "not_converged", "keyframe_by_translation", "keyframe_by_angle", "keyframe_by_time", "rejected", "rejected_reset",
                   "accepted_after_rejections", "thresholding_off", "accepted"):
        assert reached.get(branch, 0) > 0, (branch, reached)


def test_controller_equals_the_float_model_bit_for_bit_and_the_mirror_in_its_decisions(mirrors):
    assert len(SEEDS) >= 200
    for seed, (params, frames, reg, rows) in mirrors.items():
        ctl, model = Ctl(params), Model(params)
        finals = iter(reg.finals)
        for k, (f, row) in enumerate(zip(frames, rows)):
            where = (seed, k)
            aligns, guess = ctl.begin(f["stamp"], f["msf_delta"])
            assert aligns == (k > 0), where
            assert np.array_equal(bits(guess), bits(model.guess(f["msf_delta"]))), where
            final = next(finals) if aligns else None
            r = ctl.end(f["converged"], final)
            outcome, new_kf, odom, kp = model.end(f["stamp"], f["converged"], final)
            s = ctl.state()
            # 1. the model, bit for bit
            assert OUTCOMES[r.outcome] == outcome and bool(r.new_keyframe) == new_kf, where
            assert np.array_equal(bits(mat(r.odom)), bits(odom)), where
            assert np.array_equal(bits(mat(r.keyframe_pose)), bits(kp)), where
            assert np.array_equal(bits(mat(s.keyframe_pose)), bits(model.keyframe_pose)), where
            assert np.array_equal(bits(mat(s.prev_trans)), bits(model.prev_trans)), where
            assert np.array_equal(bits(mat(r.trans)), bits(np.eye(4, dtype=np.float32) if final is None else final)), where
            # 2. the mirror's decisions (its odom is a BLAS product: close, not bit-equal)
            assert OUTCOMES[r.outcome] == row["outcome"], where
            assert bool(r.new_keyframe) == row["new_keyframe"], where
            assert r.consecutive_rejections == row["rej"] == s.consecutive_rejections, where
            assert s.keyframe_stamp == row["keyframe_stamp"], where
            assert r.converged == int(aligns and f["converged"]), where
            np.testing.assert_allclose(mat(r.odom), row["odom"], rtol=0, atol=1e-4, err_msg=str(where))
            if aligns:
                np.testing.assert_allclose(guess, reg.guesses[k - 1], rtol=0, atol=1e-5, err_msg=str(where))


def test_a_failed_frame_leaves_the_state_byte_equal(mirrors):
    from mrg_slam_amd import _lib

    for seed in SEEDS[:40]:
        params, frames, reg, rows = mirrors[seed]
        plain, disturbed = Ctl(params), Ctl(params)
        for k, f in enumerate(frames):
            final = reg.finals[k - 1] if k > 0 else None
            before = bytes(disturbed.state())
            # a frame whose alignment failed: begun, never ended — then one ended without a final transformation (refused), then an end without a begin
            disturbed.begin(f["stamp"] + 0.2, frames[(k + 5) % N_FRAMES]["msf_delta"])
            assert bytes(disturbed.state()) == before
            if k > 0:
                disturbed.end(True, None, expect=_lib.ERR_INVALID)
                assert bytes(disturbed.state()) == before
            results = []
            for c in (plain, disturbed):
                c.begin(f["stamp"], f["msf_delta"])
                results.append(bytes(c.end(f["converged"], final)))
            assert results[0] == results[1], (seed, k)
            assert bytes(plain.state()) == bytes(disturbed.state()), (seed, k)
            plain.end(True, final, expect=_lib.ERR_STATE)  # nothing was begun
            assert bytes(plain.state()) == bytes(disturbed.state())


def test_controller_header_is_clean_under_asan_ubsan(tmp_path):
    """tests/sanitize/odom_ctl_san.cpp: a stand-alone program over csrc/odom_ctl.h, built with g++ -fsanitize=address,undefined (as tests/test_hardening_cpu.py
    builds its programs); nothing is loaded into python under a sanitizer."""
    exe = str(tmp_path / "odom_ctl_san")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "mrg_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "sanitize", "odom_ctl_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert "0 failed checks" in r.stdout
