"""bench.py's output contract, single rank and the N > 1 launch path (torch.distributed.run, 127.0.0.1)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _last_json(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_single_rank_line(gpu_required):
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--spectra", "3000", "--proteins", "400",
                        "--cpu-sample", "512", "--traffic-timeout", "90"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "spectra/s" and j["value"] > 0
    assert j["scaling"] == "strong" and j["vs_baseline"] is None and j["higher_is_better"] is True and j["data"] == "synthetic"
    rf = j["roofline"]
    assert rf["bound"] in ("hbm", "valu_issue") and rf["peak"] == 8000.0 and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert "traffic" in rf and rf["traffic_source"]  # measured now (rocprofv3 --pmc passes) or says why not
    if rf["traffic"] is not None:
        assert abs(rf["frac_traffic"] - rf["achieved_traffic"] / rf["peak"]) < 1e-9
    cb = j["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and "identical" in cb["parity"]
    assert cb["threads_table"] and str(cb["cores"]) in cb["threads_table"]
    assert "workload" in j["config"] and j["config"]["spectra_this_rank"] == j["config"]["spectra_total"]
    assert j["sustained"]["seconds"] >= 1.0 and j["sustained"]["value"] > 0
    assert j["concurrent"]["host_threads"] == 2 and j["concurrent"]["value"] > 0  # two scorer handles on the same GPU
    assert set(j["roofline"]["by_kernel"]) == {"prelim", "rescore"}
    assert j["roofline"]["kernel"] in ("prelim", "rescore")
    h2h = j["host_to_host_value"]
    assert h2h["page_locked"] > 0 and h2h["pageable"] > 0 and j["pcie_inclusive_value"] == h2h["page_locked"]


def _torchrun(n, extra, timeout=900, full=True):
    env = dict(os.environ, SAGE_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", "--gpus", str(n), "--steps", "3", "--warmup", "1", "--proteins", "300"] \
        + (["--full", "--no-extras"] if full else []) + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return _last_json(r.stdout)


@pytest.mark.gpu
def test_bench_two_ranks_strong_scaling_through_torchrun(gpu_required):
    """The driver's N > 1 launch line with two ranks.  A 1-GPU box cannot give each rank its own device or run RCCL between
    them, so the rehearsal backend (gloo; ranks share the device) stands in: everything else — env parsing, the one workload cut
    with plan_shards, per-rank scoring, barrier, max-over-ranks, whole-job aggregate, the ordered gather and its check against
    rank 0's single-GPU pass, rank-0-only output — is the code the real run executes."""
    j = _torchrun(2, ["--spectra", "3000"])  # the default: shards contiguous in precursor mass (sharding.plan_mass_shards)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["cpu_baseline"] is None
    sh = j["sharding"]
    total = j["config"]["spectra_total"]
    assert sh["identical_to_single_gpu"] is True and sh["shard_by"] == "mass" and len(sh["spectra_per_rank"]) == 2
    assert 2500 < total <= 3000 and sum(sh["spectra_per_rank"]) == total and 0 < j["config"]["spectra_this_rank"] < total
    assert abs(j["value"] - total * 3 / (j["ms_per_step"] * 3 / 1000.0)) / j["value"] < 0.05
    j = _torchrun(2, ["--spectra", "3000", "--shard-by", "input"])  # round 4's plan: contiguous ranges of the input
    sh = j["sharding"]
    assert sh["identical_to_single_gpu"] is True and len(sh["shards"]) == 2 and sh["shards"][0][1] == sh["shards"][1][0]
    assert sh["shards"][1][1] == j["config"]["spectra_total"] == total


@pytest.mark.gpu
def test_bench_weak_scaling_mode(gpu_required):
    j = _torchrun(2, ["--spectra", "2000", "--scaling", "weak"])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["sharding"] is None
    per_rank = j["config"]["spectra_this_rank"]
    assert 1500 < per_rank <= 2000 and abs(j["config"]["spectra_total"] - 2 * per_rank) < 100


def _dumped(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_same_outputs_every_time(gpu_required, tmp_path):
    """A plain run (no --full) times the steps and prints the headline line only; --dump-outputs writes the last timed step's
    records, the same from run to run, and a 2-rank strong-scaling run gathers the same records in input order."""
    import numpy as np
    args = ["--steps", "4", "--warmup", "1", "--spectra", "3000", "--proteins", "300"]
    lines, dumps = [], []
    for i in range(2):
        d = str(tmp_path / f"run{i}")
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *args, "--dump-outputs", d], cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(_last_json(r.stdout))
        dumps.append(_dumped(d))
    j = lines[0]
    assert j["steps"] == 4 and j["warmup"] == 1 and j["unit"] == "spectra/s" and j["dtype"] == "f32" and j["higher_is_better"] is True
    assert abs(j["value"] - j["config"]["spectra_total"] * 1000.0 / j["ms_per_step"]) / j["value"] < 1e-9
    assert j["cpu_baseline"] is None and j["parity"] is None and j["sustained"] is None and j["concurrent"] is None
    a, b = dumps
    assert sorted(a) == sorted(b) and {"counts", "row_index", "hyperscore", "peptide_idx", "spec_index"} <= set(a)
    assert sum(os.path.getsize(os.path.join(tmp_path, "run0", f)) for f in os.listdir(tmp_path / "run0")) <= 64_000_000
    n = j["config"]["spectra_this_rank"]
    assert np.array_equal(a["row_index"], np.arange(n)) and int(a["counts"].sum()) == j["config"]["psms_per_step_rank0"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and len(a[k]) == n, k
        assert np.array_equal(a[k], b[k]), k
    d = str(tmp_path / "two_ranks")
    j2 = _torchrun(2, ["--spectra", "3000", "--dump-outputs", d], full=False)
    assert j2["n_gpus"] == 2 and j2["config"]["spectra_total"] == n and j2["sharding"] is None
    c = _dumped(d)
    assert sorted(c) == sorted(a)
    for k in a:
        assert np.array_equal(a[k], c[k]), k
