"""GPU: the HIP TrainStep with world_size > 1 (train.py:21-25,53-55, rendering/renderer.py:757-765).
The lease has ONE GPU: the ranks share cuda:0 and gloo carries the collectives -- the data path (shard -> render -> loss
-> backward -> ONE flat all-reduce -> clip + Adam) is the one `bench.py --gpus N` runs over RCCL."""
import json
import os
import socket
import subprocess
import sys

import pytest

from tests._util import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(script_args, env_extra, nproc=2, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port())] + script_args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_two_ranks_stay_identical_and_match_the_per_shard_oracle():
    """Config 4 in miniature: 2 ranks x 48 rays.  fp32 mode: averaged gradient == mean of the per-shard oracle gradients
    within 2e-3 of the network's largest gradient (the single-rank tolerance of tests/test_gpu_fullsize.py); fp16 mode
    (the timed default, f32 atomics -> order-dependent local gradients): within the single-rank fp16 tolerance.  In both,
    the replicas are bit-identical after every one of 3 steps although they were initialised differently."""
    out = _torchrun([os.path.join(ROOT, "tests", "_ddp_worker.py")], {"NCW_DDP_PRECS": "f32,f16"})
    assert out["world"] == 2
    r32, r16 = out["results"]["f32"], out["results"]["f16"]
    print(json.dumps(out["results"], indent=1))
    for r in (r32, r16):
        assert r["replicas_identical"] and r["finite"] and r["applied_steps"] == 3 and r["skipped"] == 0
        assert r["param_abs_sums"][0] != r["param_abs_sums"][-1]  # the parameters did move
    assert r32["grad_err_vs_shard_oracle_mean"] < 2e-3, r32
    # W = 64, 16 + 16 samples is fp16's worst case (few samples, sharp sigmoid; single-rank smoke(): 2.4e-2 on lin4.weight_v,
    # tests/test_gpu_f16.py: 7.6e-2): measured here 0.19 on embedding_a.weight
    assert r16["grad_err_vs_shard_oracle_mean"] < 0.4, r16


def test_two_ranks_at_the_bench_width():
    """The same at W = 256 / colour 256 / NeRF 256 (the headline networks) in the timed fp16 mode, 2 x 32 rays."""
    out = _torchrun([os.path.join(ROOT, "tests", "_ddp_worker.py")], {"NCW_DDP_PRECS": "f16", "NCW_DDP_W": "256", "NCW_DDP_R": "32"})
    r = out["results"]["f16"]
    print(json.dumps(r, indent=1))
    assert r["replicas_identical"] and r["finite"] and r["applied_steps"] == 3
    assert r["grad_err_vs_shard_oracle_mean"] < 0.05, r


def test_bench_gpus_2_prints_one_line_with_world_2():
    """`python bench.py --gpus 2` end to end (self-launch, 2 ranks sharing GPU 0 over gloo through the
    NCW_BENCH_ONE_GPU_TEST hook): ONE JSON line, world_size 2, value = both ranks' ray-samples / max-over-ranks time."""
    env = dict(os.environ, NCW_DIST_BACKEND="gloo", NCW_BENCH_ONE_GPU_TEST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--rays", "256",
                        "--no-cpu-baseline", "--no-pmc", "--no-parity-mode"], capture_output=True, text=True, env=env,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["world_size"] == 2 and out["config"]["global_rays"] == 512
    assert out["scaling"] == "weak" and out["value"] > 0 and len(out["config"]["ranks"]) == 2
    assert abs(out["value"] - 2 * 256 * 128 / (out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]


def test_inference_collectives_with_two_ranks():
    """The two inference-side exchange steps at world 2 (ranks sharing GPU 0, gloo): grid.sdf_grid's all_gather over padded
    contiguous slices (config 5, utils/visualization.py:27-35,81-83) and voxel.surface_selection's sharded sweep + all_gather
    (N1, neuconw_system.py:236-258) reproduce the single-process results exactly."""
    out = _torchrun([os.path.join(ROOT, "tests", "_ddp_infer_worker.py")], {})
    print(out)
    assert out["world"] == 2 and out["all_ranks_ok"]
    assert out["grid_equal"] and out["selection_equal"]
    assert 0 < out["selection_points"] < out["candidates"]


def test_bench_gpus_2_line_is_complete():
    """An N > 1 bench line carries what the N = 1 line carries (a SCALE record must not be "unmeasured" by construction):
    `cpu_baseline`, `parity` (rank 0), the secondary modes, `allreduce_ms`, `roofline` with per-kernel HIP-event times, and
    `skipped_steps` 0.  (PMC passes are exercised at N = 1 by the driver; here --no-pmc keeps the test short.)"""
    env = dict(os.environ, NCW_DIST_BACKEND="gloo", NCW_BENCH_ONE_GPU_TEST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "2", "--no-pmc"],
                       capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["config"]["skipped_steps"] == 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["repeats"] >= 3
    assert out["parity"]["colour"] < 1.2e-4 and "weights" in out["parity"] and "sdf_abs" in out["parity"]
    assert "trained_40_steps_inv_s_403" in out["parity"]
    assert out["parity_mode"]["ms_per_step"] > 0 and out["bg_elimination"]["ms_per_step"] > 0
    assert out["allreduce_ms"] is not None and out["allreduce"]["world"] == 2
    assert out["roofline"]["bound"] == "mfma" and 0 < out["roofline"]["frac"] < 1
    if out["roofline"]["kernel"].startswith("ncw_wgrad"):  # (two ranks time-share the GPU here: another kernel may lead)
        assert out["roofline"]["frac_hbm_design"] > 0
