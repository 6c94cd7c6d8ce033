"""bench.py driver-contract tests: the round-end driver runs
`python bench.py --gpus N --steps K --warmup W` (N>1 via
torch.distributed.run) and parses ONE JSON line from rank 0 — verify
both launch modes on CPU and the schema of the line."""

import json
import os
import subprocess
import sys

import numpy as np

from conftest import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

REQUIRED_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
                 "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config"}


def _last_json_line(text: str) -> dict:
    for line in reversed(text.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{text[-2000:]}")


def test_bench_single_process(tmp_path):
    out = subprocess.run(
        [sys.executable, BENCH, "--steps", "2", "--warmup", "1"],
        cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _last_json_line(out.stdout)
    assert REQUIRED_KEYS <= set(rec)
    assert rec["n_gpus"] == 1
    assert rec["value"] > 0
    assert rec["config"]["parallelism"] == "dp1"


def _run_dump(out_dir, *extra):
    out = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup",
         "1", "--dump-outputs", str(out_dir), *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _last_json_line(out.stdout)
    assert REQUIRED_KEYS <= set(rec)
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    return {f: np.load(os.path.join(out_dir, f))
            for f in sorted(os.listdir(out_dir))}


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float
    .npy arrays (<= 64 MB in all) and two runs with the same arguments
    agree output for output; --full is accepted and changes neither.
    The dump must also carry the steps' gradients: a run that differs
    only in its dropout rate (other masks and 1/keep scaling in the LoRA
    backward) has to move the AdamW moments by far more than rounding.
    Bound: fp32 rounding is ~1e-7 relative; 1e-3 is 10^4 times that,
    while going from keep 0.9 to keep 0.5 changes every masked
    activation by tens of percent."""
    a = _run_dump(tmp_path / "a")
    b = _run_dump(tmp_path / "b", "--full")
    c = _run_dump(tmp_path / "c", "--lora-dropout", "0.5")
    assert set(a) == set(b) == set(c) == {
        "loss.npy", "trainable_params.npy", "adam_m.npy", "adam_v.npy"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert a[name].size > 0 and np.isfinite(a[name]).all(), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert a["adam_m.npy"].shape == a["adam_v.npy"].shape \
        == a["trainable_params.npy"].shape
    for name in ("adam_m.npy", "adam_v.npy"):
        x, y = a[name].astype(np.float64), c[name].astype(np.float64)
        assert np.linalg.norm(x) > 0, name
        rel = np.linalg.norm(x - y) / np.linalg.norm(x)
        print(f"{name}: dropout 0.1 vs 0.5 relative difference {rel:.3e}")
        assert rel > 1e-3, (name, rel)


def test_dump_outputs_sampling_branch(tmp_path, monkeypatch):
    """Above DUMP_MAX_ELEMS every array is cut to the same fixed sample:
    DUMP_MAX_ELEMS distinct, increasing positions, one per stride,
    identical from call to call."""
    import importlib.util
    import types

    import torch
    spec = importlib.util.spec_from_file_location("_bench_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    n = 1037                       # no multiple of the cap: stride 10, tail
    pos = torch.arange(n, dtype=torch.float32)
    trainer = types.SimpleNamespace(opt=types.SimpleNamespace(
        master=pos, m=-pos, v=pos * 2))
    bench.dump_outputs(str(tmp_path / "a"), 1.5, trainer)
    bench.dump_outputs(str(tmp_path / "b"), 1.5, trainer)
    got = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    p = got["trainable_params.npy"]
    assert p.shape == (100,) and p.dtype == np.float32
    assert (np.diff(p) > 0).all()                  # distinct, increasing
    assert (p // 10 == np.arange(100)).all()       # one per stride of 10
    assert not (p % 10 == p[0] % 10).all()         # seeded, not a comb
    np.testing.assert_array_equal(got["adam_m.npy"], -p)
    np.testing.assert_array_equal(got["adam_v.npy"], 2 * p)
    np.testing.assert_array_equal(got["loss.npy"], [1.5])
    for f in got:
        np.testing.assert_array_equal(got[f], np.load(tmp_path / "b" / f))
    # at or below the cap nothing is sampled
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", n)
    bench.dump_outputs(str(tmp_path / "c"), 1.5, trainer)
    np.testing.assert_array_equal(
        np.load(tmp_path / "c" / "trainable_params.npy"), pos.numpy())


def test_bench_torchrun_two_ranks(tmp_path):
    """The exact multi-GPU launch shape the driver uses, on CPU/gloo."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(free_port()), BENCH, "--gpus", "2", "--steps", "2",
         "--warmup", "1"],
        cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _last_json_line(out.stdout)
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["value"] > 0
