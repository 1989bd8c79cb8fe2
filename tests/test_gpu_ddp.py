"""GPU tests of data-parallel training: the gradient bucket kernel (fv_grad_bucket_pack), ``optim.Adam.step`` and
``Trainer`` with a process group, and ``MODE=train --gpus 2``.

Everything here is an equality.  The pack multiplies once per element, as torch does; a one-rank group adds nothing
to the bucket, so the step over it must leave the bits of the step without a group; at world 2 the collective is one
commutative fp32 add per word and halving is exact, so two ranks over two shards must leave the bits of the two shards'
gradients averaged by hand.  (A wider world would add the collective's summation order: not tested on the GPU.)  The
distributed cases run in child processes (tests/ddp_worker.py), each with a timeout, each on a port of its own in
29562-29569, every process group with a timeout of 120 s.
"""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastvocoder_amd import _native, optim
from tests import cases
from tests import ddp_worker as case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORKER = os.path.join(cases.ROOT, "tests", "ddp_worker.py")


# ---- 1. the pack kernel alone ------------------------------------------------------------------------------------------

def _pack(grads, scale, prefill):
    """The launch over a fresh table -> (the whole bucket, the offsets)."""
    params = [torch.nn.Parameter(torch.empty(case.NO_GRAD_SHAPE if g is None else tuple(g.shape))) for g in grads]
    offsets, total = optim.bucket_layout(params)
    flat = torch.full((total,), prefill, dtype=torch.float32, device=DEV)
    rows = [(0, flat.data_ptr() + 4 * off, 0, 0, p.numel(), 1.0, 1.0) for p, off in zip(params, offsets)]
    host, first = optim.adam_table(rows, [0 if g is None else g.data_ptr() for g in grads])
    table = torch.from_numpy(host).to(DEV)
    _native.grad_bucket_pack(table, len(rows), int(first[-1]), scale)
    torch.cuda.synchronize()
    return flat, offsets


@pytest.fixture(scope="module")
def pack_gradients():
    grads = case.case_gradients(0)
    assert grads[-1] is None and grads[-2].data_ptr() % 16 == 4 and grads[-2].numel() == 1030
    assert [tuple(g.shape) for g in grads[:-2]] == [(1,), (7,), (4096,), (4097,), (3, 5, 1031), (256, 128, 16)]
    return grads


@pytest.mark.parametrize("scale", [1.0, 0.5, float(np.float32(1.0) / np.float32(3.0))])
def test_pack_writes_every_word_of_the_bucket(pack_gradients, scale):
    grads = pack_gradients
    flat, offsets = _pack(grads, scale, 0.0)
    want = torch.zeros_like(flat)                       # pad words and the missing gradient's span: zeros
    for g, off in zip(grads, offsets):
        if g is not None:
            want[off:off + g.numel()] = (g * scale).reshape(-1)             # torch's fp32 product: one rounding
    assert offsets[-1] + 8 == flat.numel() and flat.numel() % 4 == 0
    for k, (g, off) in enumerate(zip(grads, offsets)):
        n = int(np.prod(case.NO_GRAD_SHAPE)) if g is None else g.numel()
        end = flat.numel() if k + 1 == len(offsets) else offsets[k + 1]
        assert case.same_bits(flat[off:off + n], want[off:off + n]), (k, scale)
        assert end - off == (n + 3) // 4 * 4 and not bool(case.bits(flat[off + n:end]).any()), (k, "pad")
    assert case.same_bits(flat, want)
    # whatever the bucket held before, and again: the same bits
    assert case.same_bits(_pack(grads, scale, float("nan"))[0], flat)
    assert case.same_bits(_pack(grads, scale, 0.0)[0], flat)
    if scale == 1.0:
        assert not bool(torch.equal(want, torch.zeros_like(want)))


def test_pack_refuses_a_table_without_its_source_pointers():
    flat = torch.zeros(8, dtype=torch.float32, device=DEV)
    host, first = optim.adam_table([(0, flat.data_ptr(), 0, 0, 5, 1.0, 1.0)])
    with pytest.raises(_native.NativeError, match="source"):
        _native.grad_bucket_pack(torch.from_numpy(host).to(DEV), 1, 1, 1.0)


# ---- 2-4. the child processes ------------------------------------------------------------------------------------------

def _env(port, **extra):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    return dict(e, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **extra)


def _one_rank(mode, port):
    r = subprocess.run([sys.executable, WORKER, mode], env=_env(port), cwd=cases.ROOT, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert f"DDP_OK {mode}" in r.stdout


def test_adam_over_the_bucket_equals_adam_without_a_group():
    """Three steps, max_norm 1, a one-rank RCCL group: p, m, v, the norm and the clipped gradients bit for bit; p.grad
    aliases the bucket."""
    _one_rank("adam", 29562)


def test_two_ranks_equal_the_two_shards_averaged_by_hand():
    """Two ranks on one GPU over gloo, 2 x 140 frames each: one STFT-only and one adversarial step against the oracle
    composed from the public pieces, bit for bit, and rank against rank."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29563", WORKER, "two_ranks"]
    r = subprocess.run(cmd, env=_env(29563), cwd=cases.ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-8000:]
    assert r.stdout.count("DDP_OK two_ranks") == 2


def test_trainer_with_a_one_rank_group_equals_trainer_without():
    _one_rank("trainer", 29564)


# ---- 5. MODE=train --gpus 2 --------------------------------------------------------------------------------------------

CLI_CFG = dict(cases._H, upsample_rates=[8, 5, 3, 2], upsample_kernel_sizes=[16, 10, 6, 4], upsample_initial_channel=32,
               lamda_stft=5.0, multiband=False, use_feature_map_loss=True)


def _dataset(tmp_path, split, count, seed):
    rs = np.random.RandomState(seed)
    audio, mel = [], []
    for i in range(count):
        frames = int(rs.randint(150, 171))
        t = np.arange(frames * 240) / 24000.0
        wav = (0.3 * np.sin(2 * np.pi * (150.0 + 40 * i) * t) + 0.02 * rs.randn(t.size)).astype(np.float32)
        np.save(tmp_path / f"{split}{i}.npy", wav)
        np.save(tmp_path / f"{split}{i}.mel.npy", rs.uniform(0.0, 1.0, (80, frames)).astype(np.float32))
        audio.append(str(tmp_path / f"{split}{i}.npy"))
        mel.append(str(tmp_path / f"{split}{i}.mel.npy"))
    for kind, paths in (("audio", audio), ("mel", mel)):
        (tmp_path / f"{kind}_{split}.txt").write_text("".join(p + "\n" for p in paths))


def _train(tmp_path, env, *extra):
    args = ["--model_name", "hifigan", "--config", str(tmp_path / "cfg.yaml"),
            "--audio_index_path", str(tmp_path / "audio_train.txt"), "--mel_index_path", str(tmp_path / "mel_train.txt"),
            "--audio_index_valid_path", str(tmp_path / "audio_valid.txt"),
            "--mel_index_valid_path", str(tmp_path / "mel_valid.txt"), *extra]
    return subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), *args],
                          env=dict(env, MODE="train"), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)


@pytest.fixture(scope="module")
def train_dir(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("ddp_train")
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(CLI_CFG))
    _dataset(tmp_path, "train", 8, seed=0)
    _dataset(tmp_path, "valid", 2, seed=1)
    return tmp_path


def test_mode_train_gpus_2(train_dir):
    from fastvocoder_amd.bin.synthesize import load_checkpoint
    r = _train(train_dir, _env(29566, FV_TRAIN_ONE_GPU="1", FV_TRAIN_BACKEND="gloo"), "--gpus", "2", "--batch_size", "2",
               "--max_steps", "3", "--log_step", "1", "--save_step", "3", "--valid_step", "3",
               "--discriminator_train_start_steps", "1")
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-8000:]
    out = r.stdout
    for step in (1, 2, 3):                                   # rank 0 alone prints
        assert len(re.findall(r"Step \[%d/\d+\]:" % step, out)) == 1, step
    assert out.count("STFT Loss: ") == 3 and out.count("Time Used: ") == 3
    assert out.count("---Start New Training---") == 1
    assert out.count("Length of training loader is 2") == 1
    assert len(re.findall(r"^valid 3 stft=\d\.\d{8}e[+-]\d\d$", out, flags=re.M)) == 1
    assert out.count("save model at step 3 ...") == 1
    checkpoints = glob.glob(str(train_dir / "checkpoint" / "*" / "*.pth.tar"))
    assert [os.path.basename(c) for c in checkpoints] == ["checkpoint_3.pth.tar"]
    ckpt = load_checkpoint(checkpoints[0], "cpu")
    assert sorted(ckpt) == ["discriminator", "discriminator_optimizer", "model", "optimizer"]
    assert {float(s["step"]) for s in ckpt["optimizer"]["state"].values()} == {3.0}
    assert {float(s["step"]) for s in ckpt["discriminator_optimizer"]["state"].values()} == {2.0}
    (log_dir,) = glob.glob(str(train_dir / "logger" / "*"))
    assert len(open(os.path.join(log_dir, "total_loss.txt")).read().split()) == 3


def test_mode_train_refuses_more_ranks_than_visible_devices(train_dir):
    env = _env(29567, HIP_VISIBLE_DEVICES="0")
    env.pop("FV_TRAIN_ONE_GPU", None)
    r = _train(train_dir, env, "--gpus", "3", "--batch_size", "2", "--max_steps", "1")
    assert r.returncode != 0
    assert "--gpus 3 needs 3 visible devices, this node shows 1" in r.stderr, r.stderr[-3000:]
    assert "Start New Training" not in r.stdout and "Loading Model" not in r.stdout
