"""CPU: bench.py fails fast -- one JSON error line, non-zero exit -- when fewer GPUs are visible than --gpus asks for;
--dump-outputs writes the proofs exactly, within its size budget; a plain run refuses the options of --full."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_fails_fast_without_enough_gpus():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 2
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] is None and "64" in d["error"] and d["unit"] == "proofs/s"


def test_dump_outputs_round_trips_every_word_and_samples_within_the_budget(tmp_path):
    bench = _bench_module()
    rng = np.random.default_rng(5)
    P = np.uint64(0xFFFFFFFF00000001)
    small = rng.integers(0, 2**63, size=(6, 100), dtype=np.uint64) * np.uint64(2) % P
    small[0, :3] = [0, P - np.uint64(1), np.uint64(0xFFFFFFFF)]
    bench.dump_outputs(str(tmp_path / "a"), np, small, np.array([0, 0, 3, 0, 0, 0], dtype=np.int32))
    pairs = np.load(tmp_path / "a" / "proofs.npy")
    assert pairs.dtype == np.float64 and pairs.shape == (6, 100, 2)
    back = pairs[..., 0].astype(np.uint64) | (pairs[..., 1].astype(np.uint64) << np.uint64(32))
    assert (back == small).all()
    assert np.load(tmp_path / "a" / "statuses.npy").tolist() == [0, 0, 3, 0, 0, 0]
    assert np.load(tmp_path / "a" / "proof_indices.npy").tolist() == list(range(6))
    # a step larger than the budget: a fixed sample of whole proofs, the same on every call, 64 MB at most in all
    big = np.arange(300 * 40000, dtype=np.uint64).reshape(300, 40000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), np, big, np.zeros(300, dtype=np.int32))
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 64_000_000
    idx = np.load(tmp_path / "b" / "proof_indices.npy").astype(np.int64)
    assert 0 < len(idx) < 300 and (np.diff(idx) > 0).all()
    assert (idx == np.load(tmp_path / "c" / "proof_indices.npy")).all()
    pairs = np.load(tmp_path / "b" / "proofs.npy")
    assert (pairs[..., 0].astype(np.uint64) == big[idx]).all() and not pairs[..., 1].any()


def test_bench_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_bench_options_of_the_full_run_need_full():
    """A plain run refuses what only --full uses instead of ignoring it; with --full the same options are taken (the run
    then stops at the GPU count, before any GPU work)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    for opt in (["--aggregate", "4"], ["--cpu-baseline", "none"], ["--no-cpu-baseline"], ["--extra-configs", "none"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"] + opt, capture_output=True,
                           text=True, timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 2 and f"{opt[0]} only applies with --full" in r.stderr and not r.stdout.strip(), r.stderr
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--full"] + opt,
                           capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 2 and "64" in json.loads(r.stdout.splitlines()[-1])["error"], (r.stdout, r.stderr)
