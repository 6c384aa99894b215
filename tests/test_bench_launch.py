"""bench.py's multi-GPU launch contract on CPU (gloo, two processes, train step stubbed): `python bench.py --gpus N` launches N
ranks itself when no launcher environment is present, reports n_gpus == N, and refuses to print a line for a world size that is
not the one asked for (reference: MirroredStrategy over every visible GPU, tensorflow_asr/utils/env_util.py:57-70); a plain run times
exactly --steps steps and writes its outputs with --dump-outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(TFASR_BENCH_STUB="1", **kw)
    return env


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_relaunch_cmd_shapes():
    b = _bench_module()
    assert b.relaunch_cmd(1, ["--gpus", "1"], {}) is None
    assert b.relaunch_cmd(4, ["--gpus", "4"], {"WORLD_SIZE": "4"}) is None  # already a rank of a launcher
    cmd = b.relaunch_cmd(4, ["--gpus", "4", "--steps", "3"], {})
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5] == BENCH


def test_self_launch_two_ranks_gloo(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--dump-outputs", str(tmp_path)], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 2 * 32 and out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0
    # three timed regions with --full, the line reports the median one; per-rank wire accounting of the data-parallel route
    reg = out["regions"]
    assert len(reg["ms_per_step"]) == 3 and reg["min"] <= reg["median"] <= reg["max"] and out["ms_per_step"] == reg["median"]
    assert len(reg["host_enqueue_ms_per_step"]) == 3
    dpr = out["dp"]
    assert dpr["rank0"]["syncbn_wait_calls_per_step"] == 1.0 and dpr["rank_step_ms_min"] <= dpr["rank_step_ms_max"]
    assert set(dpr["max_over_ranks"]) == {"syncbn_wait_ms", "grad_allreduce_exposed_ms"} and dpr["stats_communicator"] == "own"
    # the stub's loss = its number of train steps: the dump is rank 0's last timed step (1 warm-up + 3 regions x 3), not a later leg's
    assert np.load(tmp_path / "loss.npy").tolist() == [10.0, 10.0]


def test_plain_two_ranks_gloo(tmp_path):
    # the plain multi-rank run: one timed region of exactly --steps steps, no --full figures, per-rank accounting still reported
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["config"]["parallelism"] == "dp2"
    assert out["regions"]["ms_per_step"] == [out["ms_per_step"]] and out["dp"]["rank0"]["syncbn_wait_calls_per_step"] == 1.0
    assert not {"roofline", "roofline_rnnt", "box", "cpu_baseline"} & set(out)
    assert np.load(tmp_path / "loss.npy").tolist() == [5.0, 5.0]  # 2 warm-up + 3 timed steps


def test_plain_run_times_exactly_steps_and_dumps_outputs(tmp_path):
    # a plain run: ONE timed region of exactly --steps steps, no --full figures; --dump-outputs writes the last step's outputs as float32 .npy
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs", str(d)], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["ms_per_step"] > 0
    assert out["regions"]["ms_per_step"] == [out["ms_per_step"]]
    assert not {"roofline", "roofline_rnnt", "box", "cpu_baseline", "decode", "dp_route_ms"} & set(out)
    loss = np.load(d / "loss.npy")
    # the stub's loss = its number of train steps: the last of 1 warm-up + exactly 4 timed steps
    assert loss.dtype == np.float32 and loss.tolist() == [5.0, 5.0]


@pytest.mark.gpu
def test_dump_outputs_of_the_real_step(dev, tmp_path):
    """--dump-outputs on the real Conformer-S train step: per-utterance losses and the layout-independent samples of the parameters and
    gradients after the last timed step."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--model", "S", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["grads_sample.npy", "loss.npy", "params_sample.npy"]
    loss, p, g = (np.load(tmp_path / f"{n}.npy") for n in ("loss", "params_sample", "grads_sample"))
    assert loss.dtype == p.dtype == g.dtype == np.float32
    assert loss.shape == (32,) and np.isfinite(loss).all() and (loss > 0).all()
    assert p.shape == g.shape == (1 << 20,) and np.isfinite(p).all() and np.isfinite(g).all()
    assert np.count_nonzero(p) > 0.9 * p.size and np.count_nonzero(g) > 0.5 * g.size


def test_refuses_world_mismatch():
    # a launcher environment of ONE rank with --gpus 2: no line, non-zero exit
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=_env(WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "refusing" in (r.stderr + r.stdout)
