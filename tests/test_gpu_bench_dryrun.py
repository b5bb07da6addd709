"""`python bench.py --gpus 2` typed by itself must work: bench.py starts its own ranks under
torch.distributed.run; on a box with fewer devices than ranks the ranks share a device (gloo control plane, the RCCL exchange
reported as skipped) -- a dry run of the N > 1 path: sharded S with the shared-memory exchange, the batched configuration over
two shards, and the one-process sharded engine whose batched call has every shard in flight."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_2_self_spawns():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "50", "--warmup", "20", "--full", "--no-quiz-loop",
                        "--sharded-configs", "S,L1", "--l1-config", "LS", "--batch", "0"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    if r.returncode != 0:   # (the ranks' own tracebacks stand far above the launcher's summary)
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        open(os.path.join(ROOT, "gpurun_out", "dryrun_stderr.txt"), "w").write(r.stderr)
    assert r.returncode == 0, r.stderr[-12000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["scaling"] == "strong"
    assert out["config"]["questions_per_gpu"] == 500
    ex = out["exchange_1000x5x1000"]
    assert ex["shm"]["selections_per_sec"] > 0 and ("selections_per_sec" in ex["rccl"] or "skipped" in ex["rccl"])
    b = out["sharded_12500x5x100000_per_gpu"]
    assert b["n_gpus"] == 2 and b["exchange"]["shm"]["selections_per_sec"] > 0
    one = out["one_process_sharded_engine"]
    assert one["1000x5x1000"]["shards"] == 2
    l1 = [v for k, v in one.items() if k.endswith("_per_shard")][0]
    assert l1["shards"] == 2 and l1["shards_in_flight_max"] == 2


def _bench(extra):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "300", "--full", "--no-quiz-loop",
                        "--no-points", "--no-cpu-baseline", "--batch", "0", "--no-server"] + extra,
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_force_collective_agrees_with_plain_run():
    """N = 1 through the sharded selector (--force-collective: a world of one, both exchanges -- the RCCL all-gather really runs)
    against the plain run: the same question, and a rate within 10 % (a SCALE file's N = 1 point must agree with the BENCH file's).
    Both launch one kernel per selection (--no-server: the sharded path has no resident form)."""
    plain = _bench([])
    forced = _bench(["--force-collective", "--sharded-configs", "S"])
    if not 0.9 < forced["value"] / plain["value"] < 1.1:   # (two processes a few seconds apart on a shared box: measured once more before it counts)
        plain = _bench([])
        forced = _bench(["--force-collective", "--sharded-configs", "S"])
    assert forced["config"]["selected_question"] == plain["config"]["selected_question"]
    mg = forced["multi_gpu"]
    assert mg["n_gpus"] == 1 and mg["rccl_ranks_seen"] == 1 and mg["peer_access_matrix"][0][0] == 1
    assert mg["exchange"] == "shm" and mg["selections_per_sec"]["shm"] > 0 and mg["selections_per_sec"]["rccl"] > 0
    assert plain["multi_gpu"]["exchange"] is None and plain["multi_gpu"]["rccl_ranks_seen"] is None
    ratio = forced["value"] / plain["value"]
    assert 0.9 < ratio < 1.1, (forced["value"], plain["value"])


def _plain(args, tmp):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(tmp)] + args,
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_what_the_last_step_returned(tmp_path):
    """Without --full: the timed steps and the line, none of the extras; --steps is the number of timed steps; --dump-outputs
    holds the question the last timed step returned (batched config: one per quiz)."""
    import numpy as np

    out = _plain(["--steps", "37", "--warmup", "5"], tmp_path / "s")
    assert out["metric"] == "next_question_selections_per_sec" and out["unit"] == "selections/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64" and out["steps"] == 37 and out["value"] > 0
    assert abs(out["ms_per_step"] - 1e3 / out["value"]) < 1e-6 * out["ms_per_step"]
    for extra in ("roofline", "cpu_baseline", "step_latency_us", "resident_sweep", "quiz_loop", "hbm_point_M", "valu_point_L1"):
        assert extra not in out, extra
    sel = np.load(tmp_path / "s" / "selected_question.npy")
    assert sel.dtype == np.float64 and sel.shape == (1,) and int(sel[0]) == out["config"]["selected_question"]

    out = _plain(["--config", "LS", "--steps", "7", "--warmup", "1"], tmp_path / "b")
    assert out["steps"] == 7 and out["warmup"] == 1 and out["dtype"] == "f32" and "cpu_baseline" not in out
    picks = np.load(tmp_path / "b" / "selected_questions.npy")
    assert picks.dtype == np.float64 and picks.shape == (256,) and int(picks[0]) == out["config"]["selected_question_of_quiz_0"]
    assert ((picks >= 0) & (picks < 1000)).all()
