"""bench.py's own multi-rank launch path on CPU (gloo, stub step): `python bench.py --gpus 2` without a launcher must start two
ranks through torch.distributed.run, report n_gpus from the process group, time with barrier + max over ranks and print ONE JSON line;
a process group smaller than --gpus must fail loudly (VERDICT r01 missing #1: it used to run one rank and print n_gpus 1). And what
--dump-outputs writes, on the stub and (marked gpu) on the HIP step, and (marked gpu) what --full adds to a plain run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra, timeout=600):
    env = dict(os.environ, GSL_BENCH_STUB="1", **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        if k not in env_extra:
            env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_spawns_its_own_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "8"], {})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                       # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 2 * 2 * 8
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True


def test_bench_strong_scaling_splits_the_global_batch():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8", "--scaling", "strong"], {})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["scaling"] == "strong" and out["config"]["global_batch"] == 2 * 8 and out["n_gpus"] == 2


def test_bench_fails_when_the_group_is_smaller_than_requested():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "process group has 1 rank" in (r.stderr + r.stdout)


def test_bench_dumps_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float32 DIR/<name>.npy (the meters are those of the JSON line); two runs with
    the same arguments write the same arrays. --steps below 1 is refused."""
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], {})
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        arrays = {f.name: np.load(f) for f in d.iterdir()}
        assert sorted(arrays) == ["meters.npy", "w.npy"] and all(a.dtype == np.float32 for a in arrays.values())
        assert arrays["meters.npy"][:3].tolist() == list(out["last_step_meters"].values())
        runs.append(arrays)
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "1"], {})
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_what_the_hip_step_computed(tmp_path):
    """--dump-outputs on the GPU (config 5: HIP-graph replay, batch 4 + 4): the meters of the JSON line, and every trainable LoRA tensor
    with its gradient."""
    env = {k: v for k, v in os.environ.items() if k not in ("GSL_BENCH_STUB", "WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "5", "--steps", "2", "--warmup", "2",
                        "--no-eval", "--no-cpu-baseline", "--no-secondary", "--dump-outputs", str(d)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    arrays = {f.name[:-4]: np.load(f) for f in d.iterdir()}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert arrays["meters"].shape == (8,) and all(np.isfinite(a).all() for k, a in arrays.items() if not k.startswith("grad."))
    assert arrays["meters"][:3].tolist() == list(out["last_step_meters"].values())
    params = sorted(k[len("param."):] for k in arrays if k.startswith("param."))
    assert len(params) == 24 and all("lora_" in n for n in params)
    assert params == sorted(k[len("grad."):] for k in arrays if k.startswith("grad."))
    assert all(arrays["param." + n].shape == arrays["grad." + n].shape for n in params)


@pytest.mark.gpu
def test_bench_full_adds_the_legs_after_the_timed_region():
    """A plain run stops at the headline; --full adds what runs after the timed region (config 5, HIP-graph replay: the eval leg, the
    roofline of 3 eager steps, the CPU-baseline note). The headline keys are there in both."""
    env = {k: v for k, v in os.environ.items() if k not in ("GSL_BENCH_STUB", "WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    outs = {}
    for mode in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "5", "--steps", "2", "--warmup", "2"] + mode,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[bool(mode)] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for out in outs.values():
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(out) and out["value"] > 0
    plain, full = outs[False], outs[True]
    assert not {"eval", "roofline", "secondary", "cpu_baseline", "cpu_baseline_note"} & set(plain)
    assert {"fp32", "fp16", "bf16"} <= set(full["eval"]) and "cpu_baseline_note" in full
    assert full["roofline"]["launches_timed"] > 0 and "eager steps" in full["roofline"]["timing_source"]
