"""bench.py's --dump-outputs writer, its step arguments and --full, without a GPU (the GPU runs of these flags are
tests/test_gpu_bench.py::test_dump_outputs_are_the_timed_scores and ::test_plain_run_is_the_headline_only)."""
import numpy as np
import pytest

import bench


def test_dump_writes_every_entry_in_float64(tmp_path):
    scores = np.arange(-5, 995, dtype=np.int32)
    info = bench.dump_outputs(str(tmp_path / "out"), scores)
    s = np.load(tmp_path / "out" / "scores.npy")
    e = np.load(tmp_path / "out" / "entries.npy")
    assert s.dtype == np.float64 and e.dtype == np.float64
    assert np.array_equal(s, scores) and np.array_equal(e, np.arange(1000))
    assert info["entries"] == 1000 and info["sampled"] is False


def test_dump_of_a_large_output_is_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    scores = np.random.default_rng(3).integers(0, 1 << 30, size=300_000).astype(np.int32)
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), scores)
        assert info["sampled"] is True
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= 1 << 20
    e = np.load(tmp_path / "a" / "entries.npy")
    assert np.array_equal(e, np.load(tmp_path / "b" / "entries.npy"))
    assert np.all(np.diff(e) > 0) and e[0] >= 0 and e[-1] < scores.shape[0]
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), scores[e.astype(np.int64)])


def test_steps_and_dump_arguments():
    a = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "d"])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "d"
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--full", "--no-regimes"])
    assert a.full is True and a.no_regimes is True and a.no_cpu_baseline is False
