"""bench.py's command line and --dump-outputs writer, on the CPU: a plain run has every side leg
off (--full turns them on), and the verdict dumps are float32 .npy files named per lane, cut to a
fixed seeded sample when an array would pass its share of the 64 MB budget."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_and_full_is_an_option(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"
    # the switches for single legs keep working under --full
    assert not (a.no_cpu_baseline or a.no_latency or a.no_sha or a.no_host_path or a.no_pipelined)


def test_dump_one_lane(tmp_path):
    ok = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path / "d"), [ok], 0, 1)
    assert os.listdir(tmp_path / "d") == ["verdicts.npy"]
    got = np.load(tmp_path / "d" / "verdicts.npy")
    assert got.dtype == np.float32 and got.tolist() == [1.0, 0.0, 1.0, 1.0, 0.0]


def test_dump_lanes_are_named_by_global_index(tmp_path):
    oks = [torch.zeros(3, dtype=torch.uint8), torch.ones(3, dtype=torch.uint8)]
    bench.dump_outputs(str(tmp_path), oks, 2, 4)  # rank 1 of 2, two lanes each
    assert sorted(os.listdir(tmp_path)) == ["verdicts_gpu2.npy", "verdicts_gpu3.npy"]
    assert np.load(tmp_path / "verdicts_gpu3.npy").tolist() == [1.0, 1.0, 1.0]


def test_dump_over_budget_is_a_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4 * (100 + 64))  # 100 elements per lane
    rng = np.random.default_rng(7)
    full = [rng.integers(0, 2, size=1000).astype(np.uint8) for _ in range(2)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [torch.from_numpy(x) for x in full], 0, 2)
    size = 0
    for j, x in enumerate(full):
        a = np.load(tmp_path / "a" / f"verdicts_gpu{j}.npy")
        assert a.dtype == np.float32 and a.shape == (100,)
        assert np.array_equal(a, np.load(tmp_path / "b" / f"verdicts_gpu{j}.npy"))
        idx = np.sort(np.random.default_rng(0).choice(1000, size=100, replace=False))
        assert np.array_equal(a, x[idx].astype(np.float32))
        size += os.path.getsize(tmp_path / "a" / f"verdicts_gpu{j}.npy")
    assert size <= bench.DUMP_BUDGET_BYTES
