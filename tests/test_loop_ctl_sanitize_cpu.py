"""CPU: tests/sanitize/loop_ctl_san.cpp — a stand-alone program (its own main) over csrc/loop_ctl.h, the host controller behind mrgfe_loop_detect: a scripted
two-robot session in arrival groups against one-keyframe-per-call, and the edge cases (empty lists, key 0, an unknown neighbour, a capacity too small,
NaN / singular records, more SLAM instances than the subset enumeration takes), built with g++ -fsanitize=address,undefined as tests/test_hardening_cpu.py
builds its programs.  It is run as a program: nothing is preloaded and nothing is loaded into python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_controller_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "loop_ctl_san")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "mrg_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "sanitize", "loop_ctl_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert "0 failed checks" in r.stdout
