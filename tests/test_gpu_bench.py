"""bench.py as the driver runs it, on the one-GPU box: the N = 1 line, and the N > 1 flow rehearsed with two
ranks on GPU 0 (gloo carries the gather: RCCL refuses two ranks on one device) - started by bench.py itself,
with no torch.distributed environment, which is how a plain `python bench.py --gpus N` must work."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*argv, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.lstrip().startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_one_gpu_line_carries_the_contract_keys():
    r = _bench("--full", "--steps", "5", "--warmup", "1", "--entries", "20000", "--no-cpu-baseline")
    assert r["n_gpus"] == 1 and r["ranks_seen"] == 1 and r["scaling"] == "weak" and r["steps"] == 5
    assert r["oracle_sample_ok"] is True and len(r["oracle_sample"]) == 16
    assert r["roofline"]["bound"] == "hbm" and 0 < r["roofline"]["frac"] < 1
    assert abs(r["value"] - 20000 * 5 / (r["ms_per_step"] * 5e-3)) < 1e-6 * r["value"]
    assert r["other_regimes"]["all_hit_scorings_per_sec"] > 0 and r["other_regimes"]["planted_query_scorings_per_sec"] > 0
    assert "sat_sa_kernel<32, 1, false, 1, 4, 0>" in r["roofline"]["kernel"]


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_two_ranks_started_by_bench_itself(scaling):
    argv = ["--full", "--gpus", "2", "--backend", "gloo", "--all-ranks-on-device0", "--steps", "5", "--warmup", "1",
            "--scaling", scaling]
    argv += ["--entries", "20000"] if scaling == "weak" else ["--total", "30001"]     # 30001: unequal shards, padded rows
    r = _bench(*argv)
    total = 40000 if scaling == "weak" else 30001
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["scaling"] == scaling
    assert r["gathered_scores"] == total and r["config"]["db_entries"] == total
    assert r["oracle_sample_ok"] is True
    assert len(r["kernel_ms_by_rank"]["all"]) == 2 and r["gather_ms_alone"] > 0
    assert abs(r["value"] - total * 5 / (r["ms_per_step"] * 5e-3)) < 1e-6 * r["value"]


def test_dump_outputs_are_the_timed_scores(tmp_path):
    """--dump-outputs: the per-process path and the sat_multi_* path, at other step counts, dump the same scores
    of the same 20 000-entry database, and sampled entries equal the oracle on the kernel's Philox streams."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cuda_satabsearch_amd as sat
    import oracle_lib
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _bench("--full", "--steps", "3", "--warmup", "1", "--entries", "20000", "--no-cpu-baseline", "--no-regimes",
               "--no-upload-probe", "--dump-outputs", a)
    assert r["steps"] == 3 and r["dump_outputs"]["entries"] == 20000 and r["oracle_sample_ok"] is True
    _bench("--single-process", "--gpus", "2", "--all-ranks-on-device0", "--steps", "1", "--warmup", "0",
           "--entries", "10000", "--dump-outputs", b)
    scores, entries = np.load(os.path.join(a, "scores.npy")), np.load(os.path.join(a, "entries.npy"))
    assert scores.dtype == np.float64 and np.array_equal(entries, np.arange(20000))
    assert np.array_equal(scores, np.load(os.path.join(b, "scores.npy")))
    assert np.array_equal(entries, np.load(os.path.join(b, "entries.npy")))
    q = sat.synth.make_query(32)
    for g in (0, 7777, 19999):
        one = sat.synth.make_db(1, 32, 32, first_index=g, total=20000)
        want, _, _ = oracle_lib.search(one, *q, True, False, 128, db_ordinal=np.array([g]))
        assert scores[g] == want[0]


def test_single_process_multi_gpu_entry_points():
    """--single-process: the product's sat_multi_* calls (two contexts on GPU 0 here: the peer-copy gather)."""
    r = _bench("--full", "--single-process", "--gpus", "2", "--all-ranks-on-device0", "--steps", "3", "--warmup", "1",
               "--entries", "10000")
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["oracle_sample_ok"] is True
    assert r["shards"][0] == 0 and r["shards"][-1] == 20000


def test_plain_run_is_the_headline_only(tmp_path):
    """Without --full the line has the headline and nothing that takes work of its own; the scores it dumps (one
    rank, and two ranks through the gather of the last timed step) are the oracle's on the kernel's Philox streams."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cuda_satabsearch_amd as sat
    import oracle_lib
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _bench("--steps", "3", "--warmup", "1", "--scaling", "strong", "--total", "30001", "--dump-outputs", a)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in r
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["unit"] == "db-structure scorings/sec" and r["dtype"] == "i32"
    assert abs(r["value"] - 30001 * 3 / (r["ms_per_step"] * 3e-3)) < 1e-6 * r["value"]
    for key in ("oracle_sample_ok", "upload_and_search_overlapped_ms", "other_regimes", "cpu_baseline",
                "cpu_baseline_reference", "cpu_baseline_all_cores"):
        assert key not in r
    r2 = _bench("--gpus", "2", "--backend", "gloo", "--all-ranks-on-device0", "--steps", "2", "--warmup", "0",
                "--scaling", "strong", "--total", "30001", "--dump-outputs", b)
    assert r2["ranks_seen"] == 2 and r2["gathered_scores"] == 30001 and r2["gather_ms_alone"] is None
    assert "oracle_sample_ok" not in r2
    scores = np.load(os.path.join(a, "scores.npy"))
    assert np.array_equal(np.load(os.path.join(a, "entries.npy")), np.arange(30001))
    assert np.array_equal(scores, np.load(os.path.join(b, "scores.npy")))
    q = sat.synth.make_query(32)
    for g in (0, 14999, 15000, 30000):                     # both sides of the shard boundary
        one = sat.synth.make_db(1, 32, 32, first_index=g, total=30001)
        want, _, _ = oracle_lib.search(one, *q, True, False, 128, db_ordinal=np.array([g]))
        assert scores[g] == want[0]
