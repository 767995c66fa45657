"""bench.py prints one JSON line with the fields the driver reads (GPU: runs a reduced workload)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                          "--groups", "6", "--cpu-groups", "2", "--full"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]:
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["scaling"] == "strong" and d["data"] == "synthetic" and d["dtype"] == "f32" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert "traffic" in r and r["achieved"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    if "all_cores" in c:                       # present when the process may use more than one core
        assert c["all_cores"]["cores"] >= 2 and c["all_cores"]["value"] > 0
    assert d["sample_check"]["scored_equal"] and d["sample_check"]["entries_equal"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    e = d["e2e"]                               # cold end-to-end build of the same workload (never part of `value`)
    assert "error" not in e, e
    assert e["cold_s"] > 0 and e["gpu_part_s"] <= e["cold_s"] and e["file_bytes"] > 0 and e["scored"] == d["config"]["scored_per_step_per_gpu"]


@pytest.mark.gpu
def test_bench_weak_mode_and_group_output():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--groups", "4",
                          "--cpu-groups", "0", "--scaling", "weak", "--output", "group", "--e2e", "0"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "weak" and d["value"] > 0 and "e2e" not in d


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """Without --full the line carries the headline figure and no side legs; --dump-outputs writes the last timed step's
    database shard, identical from run to run, and (entries beyond the cap) as a seeded sample."""
    import numpy as np
    dumps = []
    for run in range(2):
        d_out = tmp_path / f"run{run}"
        out = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--groups", "4", "--dump-outputs", str(d_out)], timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["metric"] == "scored phylo-k-mers/sec" and d["unit"] == "phylo-k-mers/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        for leg in ("e2e", "cpu_baseline", "sample_check", "e2e_multi"):
            assert leg not in d, leg
        files = {p.name: np.load(p) for p in d_out.glob("*.npy")}
        assert {"keys", "key_offsets", "entry_branches", "entry_scores"} <= {n[:-4] for n in files}
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        n_ent = d["config"]["branch_kmer_entries_per_gpu"]
        assert files["key_offsets.npy"][-1] == n_ent
        if "entry_index.npy" in files:                         # sampled: the scores of the listed entries
            assert len(files["entry_scores.npy"]) == len(files["entry_index.npy"]) and files["entry_index.npy"][-1] < n_ent
        else:
            assert len(files["entry_scores.npy"]) == n_ent
        dumps.append(files)
    assert dumps[0].keys() == dumps[1].keys()
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name


def _run_bench(argv, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout, env=e)


def test_bench_starts_its_own_ranks():
    """`python3 bench.py --gpus N` with no launcher around it (the driver's command form): the parent starts N ranks as
    children, relays rank 0's line and their exit code.  CPU rehearsal of the launcher (--dry-run: gloo, no GPU call)."""
    out = _run_bench(["--gpus", "2", "--dry-run"])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2


def test_bench_watchdog_ends_a_hung_job_with_an_error():
    """A rank that never reaches the collective: its peers' watchdog ends the job non-zero instead of waiting for ever."""
    import time
    t0 = time.time()
    out = _run_bench(["--gpus", "2", "--dry-run"], env={"IPK_BENCH_DRY_HANG": "1", "IPK_BENCH_WATCHDOG_S": "8"}, timeout=200)
    assert out.returncode != 0
    assert time.time() - t0 < 150
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_self_launched():
    """The N > 1 bench path end to end on a one-GPU box: both ranks pinned to GPU 0, gloo transport (RCCL refuses two ranks
    on one device), started by bench.py itself."""
    out = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--groups", "12", "--full"],
                     env={"IPK_BENCH_DEVICE": "0", "IPK_DIST_BACKEND": "gloo"}, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["exchange"] == "torch" and d["value"] > 0
    assert d["scaling"] == "strong" and "roofline" in d
    # the stages behind a step, timed after it: filter, shard files, rank 0's merge -- and the piece rule's arithmetic
    em = d["e2e_multi"]
    assert "error" not in em and em["kmers"] > 0 and em["entries"] > 0 and em["file_bytes"] > 16 * em["kmers"] + 8 * em["entries"]
    assert all(em[x] >= 0 for x in ("build_s", "filter_s", "shard_files_s", "merge_rank0_s"))
    assert d["pieces_used"] >= 1 and len(d["pieces_model"]["by_pieces"]) == 3
    # strong scaling: the two ranks together scored what one rank scores alone
    one = _run_bench(["--gpus", "1", "--steps", "1", "--warmup", "0", "--groups", "12", "--cpu-groups", "0", "--e2e", "0"], timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][0])
    assert d1["n_ranks_seen"] == 1 and d1["exchange"] == "none"
    assert round(d["value"] * d["ms_per_step"]) == round(d1["value"] * d1["ms_per_step"])
