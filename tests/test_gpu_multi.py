"""GPU tests of the N > 1 code path with the REAL HIP generator on one GPU: a 1-rank RCCL process group
(FV_BENCH_FORCE_DIST=1) drives bench.py's broadcast / gather / scatter legs, parallel.synthesize_sharded runs the real
forward, and TWO ranks share cuda:0 under torch.distributed.run (gloo with host-staged device tensors: RCCL wants one
GPU per rank) so that world_size > 1 has met the real generator before the driver's 8-GPU run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu


def _bench(*args, **env):
    e = dict(os.environ, FV_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533",
             RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", **env)
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bench.py"), *args], env=e, cwd=cases.ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1])


def test_bench_light_through_the_distributed_path():
    """Default workload through RCCL init, weight broadcast, per-step gather inside the timed region,
    barrier bracket and MAX all-reduce; the timed output is checked against the reference golden."""
    out = _bench("--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-job", "--no-exact")
    assert out["n_gpus"] == 1 and out["scaling"] == "weak" and out["unit"] == "samples/s"
    assert "gathered to rank 0 inside the timed steps" in out["config"]["workload"]
    assert out["parity"]["max_abs_vs_reference_golden"] <= 1e-4
    assert out["without_gather"]["ms_per_step"] > 0
    assert abs(out["value"] - 240000 * 3 / (out["ms_per_step"] * 3e-3)) / out["value"] < 1e-6
    r = out["roofline"]
    assert r["bound"] == "mfma" and 0 < r["frac"] < 1 and r["kernel_ms_per_step"] <= out["ms_per_step"] * 1.05
    h = out["roofline_hbm_stage"]
    assert 1.5e7 < h["bytes"] < 2.0e7 and "effective" not in h                                   # external tensors only
    assert h["launches_per_step"] == 1 and 0 < h["bound_now"]["frac"] < 1                       # the stage is ONE launch
    assert out["range_guard"]["timed_steps_clean"] is True
    assert out["summary"]["ms_per_step"] == out["ms_per_step"] and out["summary"]["ms_per_step_default_policy"] > 0


def test_bench_large512_job_shape_on_one_rank():
    """BASELINE configs[4] harness (scatter of mels, sub-batched forward, int16 sink, gather), shrunk to
    6 utterances: rows equal solo runs bit for bit (asserted inside bench.py)."""
    out = _bench("--full", "--config", "large512", "--steps", "1", "--warmup", "0", "--sub", "4", FV_BENCH_JOB="6")
    assert out["scaling"] == "strong" and out["config"]["global_batch"] == 6
    assert "int16 wav sink" in out["config"]["workload"]
    assert abs(out["value"] - 6 * 240000 / (out["ms_per_step"] * 1e-3)) / out["value"] < 1e-6


def _torchrun2(*args, **env):
    """bench.py as two ranks on ONE GPU: `python -m torch.distributed.run --nproc-per-node 2`, both ranks on cuda:0."""
    e = dict(os.environ, FV_BENCH_ONE_GPU="1", FV_BENCH_BACKEND="gloo", **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "FV_BENCH_FORCE_DIST"):
        e.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29541", os.path.join(cases.ROOT, "bench.py"), "--gpus", "2", *args]
    r = subprocess.run(cmd, env=e, cwd=cases.ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_gpus_2_started_directly_launches_its_ranks():
    """`python bench.py --gpus 2` started as ONE process, the way the driver starts the bench: it runs itself
    under torch.distributed.run as a child (two ranks, here both on cuda:0 over gloo) and prints ONE line with both curves -- the
    weak-scaling headline, golden-checked, and the appended strong-scaling job through parallel.synthesize_pipelined
    (rows bit-identical to solo runs, asserted inside bench.py)."""
    e = dict(os.environ, FV_BENCH_ONE_GPU="1", FV_BENCH_BACKEND="gloo", FV_BENCH_JOB="10")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "FV_BENCH_FORCE_DIST", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-exact", "--sub", "2"], env=e, cwd=cases.ROOT, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["global_batch"] == 2
    assert out["parity"]["max_abs_vs_reference_golden"] <= 1e-4 and out["without_gather"]["ms_per_step"] > 0
    job = out["strong_scaling_job"]
    assert job["scaling"] == "strong" and job["n_gpus"] == 2 and "10 utterances" in job["workload"]
    assert "synthesize_pipelined" in job["workload"] and job["without_gather"]["ms_per_step"] > 0


def test_two_ranks_share_the_gpu_strong_scaling_job():
    """BASELINE configs[4] with world_size 2 and the real generator: root scatter of 8 mels, two HIP forwards (one
    per rank, sub-batches of 2), int16 sink, root gather -- rows bit-identical to the root's own solo runs (asserted
    inside bench.py), and the job without scatter / gather timed beside it."""
    out = _torchrun2("--full", "--config", "large512", "--steps", "1", "--warmup", "0", "--sub", "2", FV_BENCH_JOB="8")
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["global_batch"] == 8
    assert out["without_gather"]["ms_per_step"] > 0
    assert abs(out["value"] - 8 * 240000 / (out["ms_per_step"] * 1e-3)) / out["value"] < 1e-6


def test_two_ranks_share_the_gpu_default_line_has_both_curves():
    """The default invocation at N = 2: the weak-scaling headline (each rank its own utterance, gathered inside the
    steps, golden-checked on rank 0) AND the appended strong-scaling job, each with its no-gather figure."""
    out = _torchrun2("--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-exact", FV_BENCH_JOB="6")
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["global_batch"] == 2
    assert out["parity"]["max_abs_vs_reference_golden"] <= 1e-4
    assert out["without_gather"]["ms_per_step"] > 0
    job = out["strong_scaling_job"]
    assert job["scaling"] == "strong" and job["n_gpus"] == 2 and job["without_gather"]["ms_per_step"] > 0
    assert "6 utterances" in job["workload"]


def test_synthesize_sharded_with_the_hip_generator():
    """parallel.synthesize_sharded (scatter from the root + gather) around the real generator forward in a
    1-rank RCCL group: identical bits to the direct forward, fp32 and through the int16 sink."""
    import torch.distributed as dist
    from fastvocoder_amd import audio, parallel
    from fastvocoder_amd.bin.synthesize import build_generator
    from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
    dev = torch.device("cuda:0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        cfg = cases.load_conf("conf/hifigan/light.yaml")
        m = build_generator("hifigan", cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=0).items()})
        m = m.to(dev).eval()
        parallel.broadcast_weights(m, src=0)
        mels = torch.from_numpy(seeded_mel(64, seed=9, batch=3)).to(dev)
        with torch.no_grad():
            direct = m(mels)
            got = parallel.synthesize_sharded(lambda b: m(b), mels, scatter=True, device=dev)
            assert torch.equal(got, direct)
            pcm = parallel.synthesize_sharded(lambda b: audio.encode_16bits(m(b), 0.4), mels, scatter=True, device=dev)
        assert pcm.dtype == torch.int16 and pcm.shape == direct.shape
        want = direct.cpu().numpy().copy()
        for r in range(3):
            row = want[r]
            row *= 32767 / max(0.01, np.max(np.abs(row))) * 0.4
            assert np.array_equal(pcm[r].cpu().numpy(), row.astype(np.int16))
    finally:
        dist.destroy_process_group()


def test_rccl_collectives_of_a_job_are_root_directed():
    """What RCCL is asked to do for a job: under NCCL_DEBUG=INFO / NCCL_DEBUG_SUBSYS=COLL a 1-rank RCCL group runs the
    weight broadcast, a scatter + gather job and a ragged-length job (parallel.synthesize_ragged) around the real
    generator.  The log must show ONE broadcast for the whole checkpoint (round 3: one per tensor, 234), and no ring
    collective (all-gather / reduce-scatter) anywhere: torch's gather / scatter on the nccl backend are grouped
    ncclSend / ncclRecv to / from the root -- each peer's own xGMI link.  (The only all-reduce is the one-word maximum
    of synthesize_ragged.)  The 8-GPU run is the driver's; this pins the call pattern it will see."""
    code = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.getcwd())
from fastvocoder_amd import parallel
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
from tests import cases
dev = torch.device("cuda:0")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
cfg = cases.load_conf("conf/hifigan/light.yaml")
m = build_generator("hifigan", cfg)
m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=0).items()})
m = m.to(dev).eval()
print("MARK broadcast", flush=True)
parallel.broadcast_weights(m, src=0)
torch.cuda.synchronize()
print("MARK job", flush=True)
mels = torch.from_numpy(seeded_mel(32, seed=9, batch=3)).to(dev)
with torch.no_grad():
    got = parallel.synthesize_sharded(lambda b: m(b), mels, scatter=True, device=dev)
    assert torch.equal(got, m(mels))
    torch.cuda.synchronize()
    print("MARK ragged", flush=True)
    rag = [torch.from_numpy(seeded_mel(t, seed=20 + t).T.copy()).to(dev) for t in (24, 40, 16)]
    res = parallel.synthesize_ragged(lambda b: m(b), rag)
    for r, x in zip(res, rag):
        assert torch.equal(r, m(x[None])[0])
torch.cuda.synchronize()
print("MARK end", flush=True)
dist.destroy_process_group()
'''
    e = dict(os.environ, NCCL_DEBUG="INFO", NCCL_DEBUG_SUBSYS="COLL", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    r = subprocess.run([sys.executable, "-c", code], env=e, cwd=cases.ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    low = log.lower()
    assert "mark end" in low
    for ring in ("allgather", "reducescatter", "alltoall"):
        assert ring not in low, ring
    n_bcast = sum(1 for ln in log.splitlines() if "NCCL INFO" in ln and "Broadcast" in ln and "opCount" in ln)
    # (RCCL logs one "Broadcast: opCount ..." line per call under the COLL subsystem; a build that logs nothing at all
    # for a 1-rank communicator leaves the count at zero -- the structural claim then rests on parallel.py alone)
    assert n_bcast <= 3, n_bcast                     # weights once (+ the job's shape words): not one per tensor
