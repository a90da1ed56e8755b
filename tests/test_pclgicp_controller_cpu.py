"""CPU: tests/sanitize/pclgicp_ctl_san.cpp — a stand-alone program (its own main) over csrc/pclgicp_ctl.h: the loop of a single PCL_GICP_HIP
registration (pclgicp_align_host: BFGS<F> of csrc/bfgs.h calling its functor from inside the line search) against PclGicpController, the resumable
state machine the batch drives, over synthetic evaluators — a coupled bowl whose centre moves with the searched T, a narrow curved valley, kinks
that end the sectioning in round-off, a NaN slope, a slope no step keeps, a zero gradient at the start, fewer than four correspondences at once and
later, none at all, max_inner_iterations 1 and 2, max_iterations 1 and 3, both gradient rules.  Equal byte for byte: the requested (search, T, x)
sequence, evaluations, iterations, the converged flag, the final matrix; and every state of the machine is reached.  Built with
g++ -fsanitize=address,undefined as tests/test_loop_ctl_sanitize_cpu.py builds its program; it is run as a program, nothing is preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_controller_equals_the_bfgs_loop_and_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pclgicp_ctl_san")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "mrg_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "sanitize", "pclgicp_ctl_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert "\n0 failed checks" in r.stdout
