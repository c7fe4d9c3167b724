"""bench.py's multi-rank path, rehearsed on one GPU: the launcher
the driver's N-GPU runs use (`--gpus N` starting N rank processes with the torchrun
environment), the process group, the barrier-bracketed max-over-ranks timing and the
fast_st leg's all-reduce of the flat gradient.  Two ranks share cuda:0 and exchange over
gloo (RCCL refuses two ranks on one device); on the 8-GPU node the same code runs one
rank per GPU over RCCL.  Reference: the static_train loop being sharded,
stransfer/network.py:651-770."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_bench_plain_run_and_dump(tmp_path):
    """A plain run: the headline Gatys window alone (none of --full's legs in the line),
    `steps` timed steps with ms_per_step = 1000 / value at one GPU, and --dump-outputs
    leaves the last timed step's image, gradient, total and losses as float32 .npy: the
    image is 3 Adam steps of lr 1e-3 away from the content image (each moves an element by
    about lr at most), the total is the folded weights' sum of
    the seven losses."""
    import numpy as np
    from styletransfer_amd import weights as W
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--size", "64", "--dump-outputs", str(out)]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["full"] is False and res["unit"] == "iters/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["value"] > 0
    assert abs(res["ms_per_step"] * res["value"] / 1e3 - 1) < 1e-3
    for leg in ("roofline", "gram_roofline", "cpu_baseline", "box", "gatys_config2_run",
                "gatys_lbfgs", "fast_st", "fast_st_b64", "coco_loader", "video_st",
                "fast_st_convert"):
        assert leg not in res, leg
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["grad.npy", "image.npy", "losses.npy", "total.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["image.npy"].shape == got["grad.npy"].shape == (1, 3, 64, 64)
    assert got["total.npy"].shape == (1,) and got["losses.npy"].shape == (7,)
    x0 = W.synthetic_image(2000, (1, 3, 64, 64))
    d = np.abs(got["image.npy"] - x0)
    # |m_hat| / sqrt(v_hat) <= sqrt(sum a_i^2 / b_i) (Cauchy-Schwarz over the bias-corrected
    # weights a of m and b of v): 1, 1.0014, 1.0037 at steps 1, 2, 3 for betas (0.9, 0.999)
    assert 0 < d.max() <= 1e-3 * (1 + 1.0014 + 1.0037) + 1e-6
    assert np.abs(got["grad.npy"]).max() > 0
    lo = got["losses.npy"].astype(np.float64)
    tot = 100_000 * lo[:5].sum() + lo[5]
    assert abs(float(got["total.npy"][0]) - tot) <= 1e-5 * abs(tot)


@pytest.mark.timeout(600)
def test_bench_two_ranks_same_device():
    env = dict(os.environ, STX_BENCH_SAME_DEVICE="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--full", "--fast-steps", "2", "--gatys-run-iters", "10",
           "--skip-cpu", "--skip-infer"]
    # (the ranks' stderr goes to this test's own output: a hang or crash shows where)
    r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, text=True, timeout=540)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 alone prints the line
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["devices"] == 1
    assert res["value"] > 0 and res["config"]["parallelism"] == "replicas2"
    fs = res["fast_st"]
    assert fs["parallelism"] == "dp2" and fs["global_batch"] == 2 * fs["per_gpu_batch"]
    assert fs["collective"] and "all_reduce" in fs["collective"]
    assert fs["value"] > 0
