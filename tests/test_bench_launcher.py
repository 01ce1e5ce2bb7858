"""CPU: bench.py's multi-rank plumbing. `python bench.py --gpus 2` with no launcher around it must become two ranks by
itself (`--gpus` used to be parsed and ignored), shard / gather / max-reduce over them, and refuse a world
size that does not match --gpus. Driven with `--stub` (fake engine on CPU tensors, gloo) where there is no GPU."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_gpus2_spawns_two_ranks_itself(lib_built):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub", "--steps", "3", "--warmup", "1", "--batch", "5"],
                       env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 prints exactly one JSON line"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["collective_backend"] == "gloo"
    assert d["config"]["global_batch"] == 10 and d["config"]["parallelism"] == "dp2"
    assert len(d["rank_devices"]) == 2 and len(d["rank_crops_per_s"]) == 2
    assert d["stub_gather_ok"] is True, "records of both ranks must arrive rank-major in the gathered tensor"
    # value is whole-job throughput from the max-over-ranks time
    assert abs(d["value"] - 10 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    assert d["max_rank_ms_per_step"] >= 1e3 * 5 * 3 / max(d["rank_crops_per_s"]) / 3 - 1e-9


def test_records_beyond_the_headline_need_full(lib_built):
    """A plain run times its steps and prints the headline; the passes after them (here the one-step-in-flight run, the
    only one the stub engine takes part in) run with --full alone, on every rank."""
    lines = {}
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub", "--steps", "3", "--warmup", "1", "--batch", "5"] + extra,
                           env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, "rank 0 prints exactly one JSON line"
        lines[bool(extra)] = json.loads(out[0])
    for d in lines.values():
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 1 and d["stub_gather_ok"] is True
    assert "one_step_in_flight" not in lines[False]
    assert lines[True]["one_step_in_flight"]["ms_per_step"] > 0


def test_world_size_mismatch_is_refused(lib_built):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub", "--steps", "1", "--warmup", "0"],
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "refusing" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")], "no JSON line for a job that did not run"


def test_gpus_beyond_the_node_is_refused(lib_built):
    """Without --stub the launcher checks the visible GPU count first (0 in this container, 1 on the gpurun box)."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "64", "--steps", "1", "--warmup", "0"], env=_env(), cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "refusing" in r.stderr


def test_dump_outputs_writes_the_last_timed_step(lib_built, tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float32/float64 .npy, the same from run to run."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, BENCH, "--stub", "--steps", "4", "--warmup", "1", "--batch", "6", "--dump-outputs", str(d)],
                           env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 4 and line["ms_per_step"] > 0
        files = sorted(p.name for p in d.iterdir())
        assert files == ["keypoints.npy", "records.npy", "scalars.npy", "scores.npy"], files
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    a, b = dumps
    assert a["keypoints"].shape == (6, 17, 2) and a["records"].shape == (1, 6, 17, 7)
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), (f, a[f].dtype)
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["keypoints"][:, 0, 0], np.arange(6)), "the stub's keypoints encode the crop index"
    assert sum(p.stat().st_size for p in (tmp_path / "run0").iterdir()) <= 64 << 20
