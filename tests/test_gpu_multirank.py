"""bench.py's N > 1 code paths on a 1-GPU box: two ranks sharing the device over gloo (HESIC_DIST_BACKEND / HESIC_SINGLE_DEVICE;
RCCL refuses two ranks on one GPU).  Regression for a deadlock found in round 2: the training leg ran its metering steps --
which contain the gradient collectives -- on rank 0 only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(port, *flags, env_extra=None):
    env = dict(os.environ, HESIC_DIST_BACKEND="gloo", HESIC_SINGLE_DEVICE="1", **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", *flags]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]                      # exactly ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_two_rank_inference_and_training_bench_lines():
    d = _run(29541, "--batch", "2", "--size", "256")
    assert d["n_gpus"] == 2 and d["config"]["pairs_per_step"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    t = _run(29542, "--mode", "train", "--batch", "2", "--size", "256", "--full")         # the roofline is measured with --full
    assert t["n_gpus"] == 2 and t["config"]["global_batch"] == 4 and t["value"] > 0 and t["roofline"]["kernel"].startswith("wgrad_")
    assert all(v == v for v in t["losses_last_step"].values())    # finite


def test_two_rank_training_with_reduce_scatter_all_gather_matches_the_all_reduce():
    """The same two-rank training run with the gradient buckets summed as reduce-scatter + all-gather (``HESIC_DP_COLLECTIVE=rsag``, round 5):
    the step's losses equal the all-reduce run's (the first steps see identical parameters; the averaged gradients differ in summation
    order only)."""
    a = _run(29543, "--mode", "train", "--batch", "2", "--size", "256", "--eager")
    b = _run(29544, "--mode", "train", "--batch", "2", "--size", "256", "--eager", env_extra={"HESIC_DP_COLLECTIVE": "rsag"})
    for k in ("bpp_loss", "mse_loss", "aux_loss"):
        va, vb = a["losses_last_step"][k], b["losses_last_step"][k]
        # two separate runs: the scatter-adds of the warp's backward (atomics) already make a step's gradients differ by ~1e-5 relative from
        # run to run (profiles/scripts/train_determinism.py), and three Adam steps at random-init weights amplify that to a few 1e-3 of the
        # rate term -- the exact value equality of the two collectives is the gloo test's job (tests/test_dp_gloo.py); here: same trajectory
        assert va == va and vb == vb and abs(va - vb) <= 1e-2 * abs(va) + 1e-6, (k, va, vb)


def _run_self(*flags, env_extra=None):
    """``python bench.py --gpus 2 ...`` with NO launcher around it (the driver's command shape): bench.py starts its own ranks."""
    env = dict(os.environ, HESIC_DIST_BACKEND="gloo", HESIC_SINGLE_DEVICE="1", **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", *flags]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks_when_no_launcher_is_around():
    d = _run_self("--batch", "2", "--size", "256")
    assert d["n_gpus"] == 2 and d["config"]["pairs_per_step"] == 4 and d["value"] > 0
    assert d["ranks"]["nranks"] == 2 and len(d["ranks"]["per_rank_pairs_per_s"]) == 2 and d["ranks"]["backend"] == "gloo"
    t = _run_self("--mode", "train", "--batch", "2", "--size", "256", "--full")
    assert t["n_gpus"] == 2 and t["config"]["global_batch"] == 4 and t["ranks"]["nranks"] == 2 and "comm" in t          # the comm block itself is measured on RCCL only (gloo has no AVG op)
    s = _run_self("--sweep", "--batch", "1", "--height", "128", "--width", "192")
    assert s["n_gpus"] == 2 and s["ranks"]["nranks"] == 2 and len(s["per_lambda"]) >= 2           # two steps x two ranks touch three of the four lambda-models
