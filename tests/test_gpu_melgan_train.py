"""GPU test of ``MODE=train --model_name melgan --stack_grad 1`` through bin/launcher.py: six steps on a tiny MelGAN and
a synthetic index, the discriminator from step 4 on, a checkpoint and a validation every three steps; the log lines,
the checkpoints' keys, a resumed run and MODE=synthesize's loader on the written ``model`` entry.

Both utterances are one frame longer than the crop and the batch holds both, so every step sees the same batch (the
crop's first frame is drawn from [0, frames - fixed_length - 1] = {0}) and a run resumed from step 3 repeats steps
4 .. 6 of the first one up to the order of the two rows.  Each subprocess runs under a time limit; the module-scoped
fixtures make the first failure the last launch."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastvocoder_amd.bin.synthesize import build_generator
from tests import cases
from tests import melgan_grad_reference as mref
from tests.test_gpu_melgan_grad import GRAD_RTOL, WAVE_TOL

pytestmark = pytest.mark.gpu

CLI_CFG = dict(mref.GOLDEN_CFG, lamda_stft=1.0, multiband=False, use_feature_map_loss=True)
SPF, FIXED = 12, 140                     # 140 frames x 12 = 1680 samples: what the 2048-point STFT's reflect pad takes
LIMIT = 300                              # seconds per subprocess
LINES = [r"Epoch \[\d+/100000\], Step \[{step}/\d+\]:",
         r"STFT Loss: (\d+\.\d{{6}}), Weight Loss: 0\.000000, Total Loss: (\d+\.\d{{6}});",
         r"Adversarial Loss: (\d+\.\d{{6}}), Discriminator Loss: (\d+\.\d{{6}}), Feature Map Loss: (\d+\.\d{{6}});",
         r"Current Learning Rate is 0\.000100, discriminator Learning Rate is 0\.000050;",
         r"Time Used: \d+\.\d{{3}}s, Estimated Time Remaining: \d+\.\d{{3}}s\."]


def _dataset(tmp_path, split, count, seed):
    rs = np.random.RandomState(seed)
    audio, mel = [], []
    for i in range(count):
        t = np.arange((FIXED + 1) * SPF) / 24000.0
        wav = (0.3 * np.sin(2 * np.pi * (150.0 + 40 * i) * t) + 0.02 * rs.randn(t.size)).astype(np.float32)
        np.save(tmp_path / f"{split}{i}.npy", wav)
        np.save(tmp_path / f"{split}{i}.mel.npy", rs.uniform(-4.0, 1.0, (80, FIXED + 1)).astype(np.float32))
        audio.append(str(tmp_path / f"{split}{i}.npy"))
        mel.append(str(tmp_path / f"{split}{i}.mel.npy"))
    for kind, paths in (("audio", audio), ("mel", mel)):
        (tmp_path / f"{kind}_{split}.txt").write_text("".join(p + "\n" for p in paths))


def _launch(tmp_path, *extra):
    args = ["--model_name", "melgan", "--config", str(tmp_path / "cfg.yaml"),
            "--audio_index_path", str(tmp_path / "audio_train.txt"), "--mel_index_path", str(tmp_path / "mel_train.txt"),
            "--audio_index_valid_path", str(tmp_path / "audio_valid.txt"),
            "--mel_index_valid_path", str(tmp_path / "mel_valid.txt"),
            "--discriminator_train_start_steps", "3", "--batch_size", "2", "--fixed_length", str(FIXED),
            "--log_step", "1", "--save_step", "3", "--valid_step", "3", *extra]
    return subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), *args],
                          env=dict(os.environ, MODE="train"), cwd=str(tmp_path), capture_output=True, text=True,
                          timeout=LIMIT)


def _logged(out, step):
    """The figures of the log lines of ``step``: (stft, total, adversarial, discriminator, feature map)."""
    m = re.search("\n".join(line.format(step=step) for line in LINES), out)
    assert m, f"the log lines of step {step} are missing or malformed:\n{out}"
    return [float(v) for v in m.groups()]


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("melgan_train")
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(CLI_CFG))
    _dataset(tmp_path, "train", 2, seed=0)
    _dataset(tmp_path, "valid", 2, seed=1)
    r = _launch(tmp_path, "--stack_grad", "1", "--max_steps", "6")
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp_path, r.stdout


def _checkpoint(tmp_path, step, which=0):
    found = sorted(glob.glob(str(tmp_path / "checkpoint" / "*" / f"checkpoint_{step}.pth.tar")), key=os.path.getmtime)
    assert len(found) > which, (step, found)
    return found[which]


def test_the_run_logs_validates_and_saves(first_run):
    tmp_path, out = first_run
    assert "Loading Model of melgan..." in out and "---Start New Training---" in out
    for step in range(1, 7):
        stft, total, adv, dis, fm = _logged(out, step)
        assert stft > 0.0 and total > 0.0
        if step <= 3:
            assert adv == dis == fm == 0.0 and abs(total - stft) <= 2e-6          # lamda_stft: 1.0, two roundings
        else:
            assert adv > 0.0 and dis > 0.0 and fm > 0.0
    assert len(re.findall(r"^valid [36] stft=\d\.\d{8}e[+-]\d\d$", out, flags=re.M)) == 2
    assert "save model at step 3 ..." in out and "save model at step 6 ..." in out


def test_the_checkpoints_have_the_four_keys_and_the_model_loads_into_synthesize(first_run):
    from fastvocoder_amd.bin.synthesize import Synthesizer, load_checkpoint
    tmp_path, _ = first_run
    for step, d_steps in ((3, set()), (6, {3.0})):
        ckpt = load_checkpoint(_checkpoint(tmp_path, step), "cpu")
        assert sorted(ckpt) == ["discriminator", "discriminator_optimizer", "model", "optimizer"]
        assert {float(s["step"]) for s in ckpt["optimizer"]["state"].values()} == {float(step)}
        assert {float(s["step"]) for s in ckpt["discriminator_optimizer"]["state"].values()} == d_steps
    reference_keys = sorted(build_generator("melgan", CLI_CFG).state_dict())
    assert sorted(ckpt["model"]) == reference_keys
    syn = Synthesizer(_checkpoint(tmp_path, 6), str(tmp_path / "cfg.yaml"), "melgan")
    mel = np.random.RandomState(0).uniform(-4.0, 1.0, (30, 80)).astype(np.float32)
    est = syn.synthesize(mel)[0]
    gen = build_generator("melgan", CLI_CFG)
    gen.load_state_dict(ckpt["model"])
    mine = gen.to(est.device).eval().inference(torch.from_numpy(mel))
    diff = float((est - mine).abs().max())
    print(f"synthesize on the trained model against the in-process generator: {diff:.2e}")
    assert est.shape == (30 * SPF,) and bool(torch.isfinite(est).all()) and diff <= WAVE_TOL
    fresh = build_generator("melgan", CLI_CFG).state_dict()
    assert all(v.shape == fresh[k].shape for k, v in ckpt["model"].items())


def test_a_run_resumed_from_the_first_checkpoint_reaches_the_second(first_run):
    from fastvocoder_amd.bin.synthesize import load_checkpoint
    tmp_path, _ = first_run
    want = load_checkpoint(_checkpoint(tmp_path, 6), "cpu")["model"]
    r = _launch(tmp_path, "--stack_grad", "1", "--checkpoint_path", _checkpoint(tmp_path, 3), "--restore_step", "3",
                "--max_steps", "3")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "---Model Restored at Step 3---" in r.stdout and "optimizer state at step count 3" in r.stdout
    for step in (4, 5, 6):
        assert all(v > 0.0 for v in _logged(r.stdout, step))
    assert not re.search(r"Step \[[1-3]/", r.stdout)
    got = load_checkpoint(_checkpoint(tmp_path, 6, which=1), "cpu")["model"]
    start = load_checkpoint(_checkpoint(tmp_path, 3), "cpu")["model"]
    worst = max(mref.rel_err(got[k].numpy(), want[k].numpy()) for k in want)
    moved = max(mref.rel_err(start[k].numpy(), want[k].numpy()) for k in want)
    print(f"resumed run against the first: parameters {worst:.2e} (steps 4 .. 6 moved them by {moved:.2e})")
    assert worst <= GRAD_RTOL < moved, (worst, moved)


def test_without_the_flag_the_run_exits_before_it_loads_anything(first_run):
    tmp_path, _ = first_run
    r = _launch(tmp_path, "--max_steps", "1")
    assert r.returncode != 0 and "Loading Model" not in r.stdout
    assert "melgan" in r.stderr and "no parameter gradient" in r.stderr and "--stack_grad 1" in r.stderr
