"""bench.py's plain run and its outputs: a plain `bench.py --steps K --warmup W` prepares only the headline's inputs and times exactly K steps;
`--dump-outputs DIR` writes the records of the timed path's last step as float32 / float64 .npy files, the same on every run of the same
arguments.  The record writer and the input preparation run on the CPU; the timed runs need the GPU."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_dump_outputs_writes_every_record_field_as_float(bench, tmp_path):
    from mrg_slam_amd.registration import RESULT_DTYPE

    rec = np.zeros(5, dtype=RESULT_DTYPE)
    rec["T"] = np.arange(5 * 16, dtype=np.float32).reshape(5, 16) / 7
    rec["H"] = np.arange(5 * 36, dtype=np.float64).reshape(5, 36) / 3
    rec["fitness"] = np.linspace(0.1, 0.5, 5)
    rec["converged"] = [1, 0, 1, 1, 0]
    rec["iterations"] = [3, 64, 2, 5, 7]
    rec["evaluations"] = [6, 130, 4, 9, 12]
    rec["pair_id"] = np.arange(5)
    bench.dump_outputs(str(tmp_path / "out"), rec)
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(f"{n}.npy" for n in RESULT_DTYPE.names)
    for n in RESULT_DTYPE.names:
        a = np.load(tmp_path / "out" / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == rec[n].shape, n
        assert np.array_equal(a, rec[n].astype(a.dtype)), n
    assert np.load(tmp_path / "out" / "T.npy").dtype == np.float32 and np.load(tmp_path / "out" / "H.npy").dtype == np.float64


def test_plain_prepare_only_generates_the_headline_inputs_alone(tmp_path):
    """without --full the config[3] side leg is off, so its 64 ring keyframes are not ray-cast"""
    env = dict(os.environ, BENCH_CACHE=str(tmp_path / "cache"), OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "3", "--prepare-only"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "cache")) == ["street_r0_n4_v2.npz"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    env = dict(os.environ, BENCH_CACHE=str(tmp_path / "cache"), OMP_NUM_THREADS="8")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_DIST_BACKEND"):
        env.pop(k, None)
    lines = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16", "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, out
        lines.append(json.loads(out[0]))
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "alignments/s" and d["higher_is_better"] is True and d["dtype"]
        assert d["ms_per_step"] > 0 and abs(d["value"] - 16 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-4 * d["value"]
        assert d["cpu_baseline"] is None and "value_one_step_at_a_time" not in d and "config3" not in d and d["roofline"]["launches"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "T.npy" in names and "fitness.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and len(a) == 16, n
        assert a.tobytes() == b.tobytes(), n
        total += a.nbytes
    assert total < 64 << 20
    assert np.isfinite(np.load(tmp_path / "a" / "T.npy")).all() and np.load(tmp_path / "a" / "T.npy").shape == (16, 16)
