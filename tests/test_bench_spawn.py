"""bench.py --gpus N starts its N ranks itself when no launcher did; checked without a GPU through the dry-run
switch: the ranks rendezvous over gloo on 127.0.0.1, agree on the world size, rank 0 prints the line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)


def test_gpus_flag_spawns_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"], {"THALLO_BENCH_DRY": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                      # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1


def test_launcher_world_size_must_match_gpus_flag():
    r = _run(["--gpus", "4"], {"THALLO_BENCH_DRY": "1", "WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "--gpus 4" in r.stderr and "WORLD_SIZE=2" in r.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_every_array_under_the_limit(tmp_path):
    """--dump-outputs: DIR/<name>.npy per output; past the size limit every array becomes the same fixed, seeded sample of its elements."""
    import numpy as np
    dump = _bench_module().dump_outputs
    rng = np.random.default_rng(7)
    arrays = {"offset": rng.standard_normal((64, 64, 2)).astype(np.float32), "angle": rng.standard_normal((64, 64)).astype(np.float32),
              "cost": np.array([1.5], np.float64)}
    dump(str(tmp_path / "whole"), arrays)
    for n, a in arrays.items():
        b = np.load(tmp_path / "whole" / f"{n}.npy")
        assert b.dtype == a.dtype and np.array_equal(a, b), n
    limit = 16 << 10                                  # 16 KiB against 48 KiB of outputs
    for run in ("s0", "s1"):
        dump(str(tmp_path / run), arrays, limit=limit)
    total = sum(os.path.getsize(tmp_path / "s0" / f"{n}.npy") for n in arrays)
    assert total <= limit
    for n, a in arrays.items():
        s0, s1 = np.load(tmp_path / "s0" / f"{n}.npy"), np.load(tmp_path / "s1" / f"{n}.npy")
        assert s0.dtype == a.dtype and s0.size >= 1 and np.array_equal(s0, s1), n
        assert np.isin(s0, a.reshape(-1)).all(), n
    with pytest.raises(AssertionError):
        dump(str(tmp_path / "ints"), {"bad": np.zeros(4, np.int32)})


def test_bench_arguments_are_checked_before_any_work():
    r = _run(["--steps", "0"], {"THALLO_BENCH_DRY": "1"})
    assert r.returncode != 0 and "--steps" in r.stderr
    r = _run(["--gpus", "2", "--dump-outputs", "out"], {"THALLO_BENCH_DRY": "1"})
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
