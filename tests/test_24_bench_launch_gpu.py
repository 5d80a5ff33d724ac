"""bench.py's own rank start-up (the reference's data-parallel entry point spawns its workers itself: train_NAR_mp.py:319-326): `python
bench.py --gpus 2` with no WORLD_SIZE in the environment must come back with a line that says n_gpus == 2 -- two real processes, a
verified collective layer between them, per-rank timings and the exchange accounting -- for the headline job and for the BAIR FAR /
KTH128 entry points.  A one-GPU box can run this with both ranks on cuda:0 and gloo as the exchange backend (RCCL refuses two ranks
on one device); the 8-GPU node runs the same code with one GPU per rank over RCCL."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, timeout=900):
    env = dict(os.environ, VPTR_BENCH_SHARE_GPU="1", VPTR_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    # Two ranks and the pytest process time-slice ONE GPU here; a healthy job takes 20 - 90 s, and about one run in ten stalls for minutes
    # (profiles/r06_mp_tests_soak.log; one-process-per-GPU jobs do not share queues).  A job that is still running after `attempt_s` is killed
    # with its whole process group -- the ranks must not linger on the GPU -- and started again; every rank dumps its stacks to stderr first
    # (VPTR_BENCH_HANG_DUMP_S).  Wrong output or a non-zero exit code fails at once.
    import signal
    attempt_s, last = 300, None
    for attempt in range(3):
        p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
                              "--no-cpu-baseline", "--no-other-configs"] + extra, env=dict(env, VPTR_BENCH_HANG_DUMP_S=str(attempt_s - 30)), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            out, err = p.communicate(timeout=min(attempt_s, timeout))
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            out, err = p.communicate()
            last = ("timeout", out[-1000:], err[-3000:])
            print("attempt %d of the 2-rank self-launch did not finish within %d s; stderr tail:\n%s" % (attempt, attempt_s, err[-3000:]))
            continue
        assert p.returncode == 0, (p.returncode, out[-2000:], err[-4000:])
        lines = [l for l in out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out[-2000:]            # rank 0 prints, nobody else does
        return json.loads(lines[0])
    raise AssertionError("three 2-rank self-launches in a row did not finish: %s" % (last,))


def _check(d, per_gpu_batch, frames):
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 2 * per_gpu_batch
    assert d["loss_sane"], d["final_terms"]
    c = d["comm"]
    assert c["backend"] == "gloo" and c["rccl_ranks"] == 2 and d["rccl_ranks"] == 0      # gloo here: no RCCL claim
    assert c["rank_sum_check"] == 3.0 and len(c["devices"]) == 2
    assert c["launched_by"].startswith("bench.py self-launch")
    assert c["allreduce_bytes_per_step"] > 0 and c["allreduce_calls_per_step"] >= 1
    assert c["exposed_comm_ms_per_step"]["max"] >= 0.0
    # round 6: the tuning table of the first real multi-GPU run -- per rank, chunk-end and all-reduce-done times of one untimed step
    tl = c["exchange_timeline"]
    assert "error" not in tl, tl
    assert [t["rank"] for t in tl["per_rank"]] == [0, 1] and c["dp_chunks"] == 4
    for t in tl["per_rank"]:
        assert len(t["chunk_end_ms"]) >= 1 and len(t["allreduce_done_ms"]) == len(t["allreduce_bytes"]) >= 1
        assert sum(t["allreduce_bytes"]) == c["allreduce_bytes_per_step"]
        assert all(b >= a for a, b in zip(t["allreduce_done_ms"], t["allreduce_done_ms"][1:]))
    pr = d["per_rank_ms_per_step"]
    assert 0 < pr["min"] <= pr["max"] <= d["ms_per_step"] * 1.05
    assert abs(d["value"] - 2 * per_gpu_batch * frames / d["ms_per_step"] * 1e3) <= 1e-3 * d["value"] + 0.5
    assert d["roofline"]["frac"] is not None and d["roofline"]["hbm_side"].get("kernel") == "adamw_kernel"


def test_self_launch_two_ranks_k64():
    d = _run(["--batch", "4"])
    _check(d, 4, 10)
    # K64 slab: 118,368,576 fp32 gradients all-reduced every step
    assert d["comm"]["allreduce_bytes_per_step"] == 4 * 118368576
    assert "hipGraph" in d["config"]["launch"], d["config"]["launch"]


def test_self_launch_two_ranks_bair_far():
    d = _run(["--config", "bair_far", "--batch", "2"])
    _check(d, 2, 29)
    assert d["config"]["baseline_config"] == 4 and "FAR" in d["metric"]


def test_self_launch_two_ranks_kth128():
    d = _run(["--config", "kth128", "--batch", "1"])
    _check(d, 1, 40)
    assert d["config"]["baseline_config"] == 5 and "128x128" in d["metric"]


def test_rank_failure_is_loud():
    """a rank that dies takes the job down with a non-zero exit code: no partial line"""
    env = dict(os.environ, VPTR_BENCH_SHARE_GPU="1", VPTR_BENCH_BACKEND="nccl")     # RCCL + shared GPU is refused by every rank
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_plain_run_dumps_outputs(tmp_path):
    """a plain one-GPU run (no --full) prints the headline line only -- the timed path, none of the --full extras -- and
    --dump-outputs writes what its last timed step computed: the loss terms the line reports and a sample of the post-step
    transformer state, float32 / float64, within 64 MB"""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "VPTR_BENCH_SHARE_GPU")}
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["loss_sane"], res
    assert res["ms_per_step"] > 0 and abs(res["value"] - 2 * 10 / res["ms_per_step"] * 1e3) <= 1e-3 * res["value"] + 0.5
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    for k in ("roofline", "other_configs", "cpu_baseline"):
        assert k not in res, k
    assert res["graph_check"] is None and res["config"]["launch"] == "hipGraph"
    files = sorted(os.listdir(d))
    assert set(files) >= {"T_total.npy", "T_GDL.npy", "T_MSE.npy", "T_bpc.npy", "grad_norm.npy", "T_state_sample.npy"}, files
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    for f in files:
        a = np.load(d / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    for k, v in res["final_terms"].items():
        assert abs(float(np.load(d / (k + ".npy"))[0]) - v) <= 1e-6 * abs(v) + 1e-6, k
    assert np.load(d / "T_state_sample.npy").size > 1 << 20
