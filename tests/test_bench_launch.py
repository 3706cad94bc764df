"""bench.py --gpus N starts its own N ranks (python/sglang/bench_one_batch.py:527-546 spawns one process per tp_rank):
the parent relays rank 0's JSON line, carries --gpus and the observed world size on it, and fails when any rank fails."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return env


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def test_world_size_must_agree_with_gpus_flag():
    """Under a launcher (WORLD_SIZE set) --gpus has to say the same: a flat 8-GPU scaling run must not be possible."""
    env = dict(_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--model", "tiny"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "must agree" in r.stderr


def _run_line(args, timeout=600):
    r = subprocess.run([sys.executable, BENCH] + args, env=_env(), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load_dump(d):
    import numpy as np

    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(f.endswith(".npy") for f in os.listdir(d))
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_steps_sets_the_timed_steps_and_dump_outputs_writes_the_last_step(tmp_path):
    """--steps K times K steps (17: the CPU configuration once stopped at 16), ms_per_step is on the line, and --dump-outputs
    writes what the last step returned as float32 / float64 .npy files (the CPU plumbing configuration: no GPU needed)."""
    import numpy as np

    out = _run_line(["--config", "1", "--steps", "17", "--dump-outputs", str(tmp_path / "dump")])
    assert out["steps"] == 17 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]   # batch 1: tokens/s = steps/s
    dump = _load_dump(str(tmp_path / "dump"))
    assert dump["logits"].dtype == np.float32 and dump["logits"].shape == (1, 50272) and np.isfinite(dump["logits"]).all()
    assert dump["next_token_ids"].tolist() == [float(dump["logits"][0].argmax())]


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_the_rest_with_identical_outputs(tmp_path):
    """A plain run carries the headline fields and none of the measurements that take runs of their own; --full adds them; both
    compute the same last step from the same seeded inputs, so their dumped outputs are equal."""
    import numpy as np

    small = ["--gpus", "1", "--model", "tiny", "--batch", "4", "--seq-len", "64", "--steps", "3", "--warmup", "1"]
    plain = _run_line(small + ["--dump-outputs", str(tmp_path / "plain")])
    full = _run_line(small + ["--full", "--dump-outputs", str(tmp_path / "full")])
    for out in (plain, full):
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["unit"] == "tokens/s"
        assert abs(out["value"] - 4 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
        assert out["higher_is_better"] is True and out["config"]["hip_graph"] is True
    assert plain["roofline"] is None and "cpu_baseline" not in plain and plain["prefill"]["warm"] is False
    assert "roofline_probe" not in plain["phases_s"] and "cpu_baseline" not in plain["phases_s"]
    assert full["roofline"]["launch_us"] > 0 and full["prefill"]["warm"] is True
    a, b = _load_dump(str(tmp_path / "plain")), _load_dump(str(tmp_path / "full"))
    assert a["logits"].shape == (4, 2048) and a["next_token_ids"].shape == (4,) and np.isfinite(a["logits"]).all()
    assert a["next_token_ids"].tolist() == a["logits"].argmax(-1).astype(np.float64).tolist()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.skipif(_has_gpu(), reason="needs a box WITHOUT a GPU: the ranks then fail at start-up, which is the case under test")
def test_parent_fails_when_a_rank_fails():
    """Without a GPU every rank exits non-zero at once ('bench.py needs an MI355X'): the parent must report that, not hang."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dist-backend", "gloo", "--model", "tiny", "--no-cpu-baseline"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "a rank exited with code" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
@pytest.mark.parametrize("all_reduce", ["auto", "p2p"])
def test_bench_gpus_2_spawns_two_ranks(all_reduce):
    """Two ranks on ONE GPU over gloo (the rehearsal transport); p2p = the P2P communicator with both collectives inside the
    captured graph, auto = host-staged collectives, eager by design and marked so in the metric name."""
    cmd = [sys.executable, BENCH, "--gpus", "2", "--dist-backend", "gloo", "--model", "tiny", "--no-cpu-baseline", "--batch", "4",
           "--seq-len", "64", "--steps", "3", "--warmup", "1", "--all-reduce", all_reduce]
    r = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2
    assert out["config"]["parallelism"].startswith("tp2")
    if all_reduce == "p2p":
        assert out["config"]["hip_graph"] is True and out["config"]["all_reduce"].startswith("p2p")
        assert "EAGER" not in out["metric"]
    else:
        assert out["config"]["hip_graph"] is False and "EAGER" in out["metric"]
