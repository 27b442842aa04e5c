"""`python bench.py --gpus N` as the driver's SCALE tier gives it: without a launcher around it the script must start
its own ranks (one process per GPU, torch.distributed.run on 127.0.0.1) before making any GPU call, relay rank 0's
single JSON line and the children's exit code.  On CPU the hot path cannot run (no fallback), so the launcher, the
rendezvous and the gradient all-reduce are covered with --plumbing-only over gloo; the real two-rank step is the gpu test."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra, timeout=300):
    env = dict(os.environ, PSVO_DIST_BACKEND="gloo", **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]      # (gloo prints connection chatter on stdout)
    return p, lines


@pytest.mark.timeout(400)
def test_bench_gpus2_launches_its_own_ranks_cpu():
    p, lines = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--plumbing-only"], {})
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, lines                      # exactly one JSON line on stdout: rank 0's
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["allreduce_ok"] is True


@pytest.mark.timeout(400)
def test_bench_relays_a_failing_rank_cpu():
    p, _ = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "C*"], {})
    # no --plumbing-only: on a CPU-only host every rank refuses (no CPU fallback); on a GPU host this is a real run
    import torch
    if not torch.cuda.is_available():
        assert p.returncode != 0 and "no CPU fallback" in (p.stderr + p.stdout)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_gpus2_real_step_on_one_card():
    """two ranks sharing the one card of the test box (gloo for the collective: RCCL refuses two ranks on one device):
    the whole bench path -- sharded batch, flat-gradient all-reduce, Adam, max-over-ranks timing -- prints n_gpus = 2"""
    p, lines = _run(["--gpus", "2", "--steps", "3", "--warmup", "2", "--workload", "tiny", "--no-cpu-baseline"], {})
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(lines[-1])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 8 and out["value"] > 0


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_of_large_ones_cpu(tmp_path):
    import numpy as np
    import torch
    dump = _bench_module().dump_outputs
    big = torch.arange(50, dtype=torch.int32)
    arrays = {"elbo": torch.tensor(-1.5, dtype=torch.float64), "small": torch.ones(3, 4), "big": big}
    for d in ("a", "b"):
        dump(str(tmp_path / d), arrays, cap=20)
    elbo, small, sample = (np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("elbo", "small", "big"))
    assert elbo.dtype == np.float64 and elbo.shape == () and float(elbo) == -1.5
    assert small.dtype == np.float32 and small.shape == (3, 4)
    assert sample.dtype == np.float32 and sample.shape == (20,) and len(set(sample.tolist())) == 20
    assert (np.diff(sample) > 0).all() and set(sample.tolist()) <= set(range(50))      # sorted indices into the original
    assert (np.load(str(tmp_path / "b" / "big.npy")) == sample).all()                    # the same sample on every run


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["train", "forward"])
def test_bench_dump_outputs_holds_the_last_timed_step(tmp_path, mode):
    """--dump-outputs: the ELBO of the last timed step (the one the JSON line reports) and, training, the updated flat
    parameters and their gradient, forward-only, the smoothed trajectories"""
    import numpy as np
    p, lines = _run(["--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "tiny", "--no-cpu-baseline",
                     "--mode", mode, "--dump-outputs", str(tmp_path)], {})
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(lines[-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    elbo = np.load(str(tmp_path / "elbo.npy"))
    assert elbo.dtype == np.float64 and float(elbo) == out["config"]["elbo"]
    if mode == "train":
        params, grad = np.load(str(tmp_path / "params.npy")), np.load(str(tmp_path / "grad.npy"))
        assert params.dtype == grad.dtype == np.float32 and params.shape == grad.shape and params.ndim == 1
        assert np.isfinite(params).all() and np.isfinite(grad).all() and np.abs(grad).max() > 0
    else:
        Xs = np.load(str(tmp_path / "Xs.npy"))
        assert Xs.dtype == np.float32 and Xs.shape == (4, 12, 32, 2) and np.isfinite(Xs).all()
