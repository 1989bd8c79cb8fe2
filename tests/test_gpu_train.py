"""GPU tests of the training step (fastvocoder_amd/train.py), of what it is for (a loss that goes down) and of
MODE=train through bin/launcher.py.

Step equivalence: ``Trainer.step`` against the same public pieces composed by hand with ``clip_grad_norm_`` +
``torch.optim.Adam``, one step at ``current_step <= start`` and one past it, each from the same fresh state (so the
gradients of both sides are the same launches on the same bits), on the 16-channel HiFi-GAN of
tests/generator_grad_reference.py (12 samples per frame, 2 x 140 frames = 1680 samples, the shortest the 2048-point
STFT's reflect padding takes) and on a 16-channel Multiband-HiFi-GAN with PQMF.  The generator's parameters of the two
sides agree within the optimizer's constants (tests/test_gpu_optim.py); the discriminator's half is composed on the
generator the trainer left, so its loss is the same number and its parameters agree within the same constants.

Overfit: 30 STFT-only steps on one batch must halve ``sc + mag``.  The reference's own modules on the CPU reach 0.31 of
the first value for two input seeds (6.29 -> 1.97, 6.25 -> 1.95); 0.5 leaves room and still fails when the weights do
not move or a packed-weight cache goes stale.
"""
import copy
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastvocoder_amd import optim
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import Discriminator
from fastvocoder_amd.generator import PQMF
from fastvocoder_amd.loss import (Loss, discriminator_step_terms, generator_adversarial_terms, pqmf_synthesis)
from fastvocoder_amd.synthetic import seeded_state_dict
from fastvocoder_amd.train import KEYS, Trainer, fit_estimate, samples_per_frame
from tests import cases
from tests import generator_grad_reference as gref
from tests import optim_reference as oref
from tests.test_gpu_optim import TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRAMES, BATCH = 140, 2
MB_CFG = dict(next(c for t, _, c in cases.SMALL if t == "mb_s"), upsample_initial_channel=16)
CONFIGS = {"hifigan": ("hifigan", gref.GOLDEN_CFG), "multiband": ("multiband-hifigan", MB_CFG)}
LR, LR_D, CLIP, LAMBDA_STFT = 1e-4, 5e-5, 1.0, 5.0
P_TOL, NORM_TOL = TOL["p"][1], TOL["norm"][1]
# torch's own float32 norm errs by 2.9e-6 on the optimizer's case (tests/test_optim_host.py prints it): ours against
# torch's is bounded by the sum of the two, with the margin of ten the other constants have
NORM_VS_TORCH = 10 * 2.9e-6 + NORM_TOL


def _generator(name, cfg, weight_seed=3):
    g = build_generator(name, cfg)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(name, cfg, seed=weight_seed).items()})
    return g.to(DEV).train()


def _batch(spf, seed):
    """mel uniform in [-4, 1]; the target two sinusoids per row plus 0.02 noise."""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(-4.0, 1.0, (BATCH, 80, FRAMES)).astype(np.float32)
    t = np.arange(FRAMES * spf) / 24000.0
    wav = np.stack([0.4 * np.sin(2 * np.pi * (180.0 + 70 * b) * t) + 0.2 * np.sin(2 * np.pi * (1900.0 + 300 * b) * t + 1.0)
                    for b in range(BATCH)]) + 0.02 * rs.randn(BATCH, FRAMES * spf)
    return torch.from_numpy(mel).to(DEV), torch.from_numpy(wav.astype(np.float32)).to(DEV)


@pytest.fixture(scope="module")
def discriminator_state():
    torch.manual_seed(5)
    return copy.deepcopy(Discriminator().state_dict())


def _discriminator(state):
    d = Discriminator()
    d.load_state_dict(state)
    return d.to(DEV)


def _worst(named_a, named_b):
    worst, where = 0.0, None
    for (ka, a), (kb, b) in zip(named_a, named_b):
        assert ka == kb
        e = oref.rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())
        if e > worst:
            worst, where = e, ka
    return worst, where


@pytest.mark.parametrize("phase", ["stft_only", "adversarial"])
@pytest.mark.parametrize("family", sorted(CONFIGS))
def test_a_step_equals_the_pieces_composed_by_hand(family, phase, discriminator_state):
    name, cfg = CONFIGS[family]
    start = 1 if phase == "stft_only" else 0           # current_step = 1 on both sides
    pqmf = PQMF().to(DEV) if family == "multiband" else None

    # ---- the trainer
    g, d = _generator(name, cfg), _discriminator(discriminator_state)
    trainer = Trainer(g, d, optim.Adam(g.parameters(), lr=LR, eps=1e-6), optim.Adam(d.parameters(), lr=LR_D, eps=1e-6),
                      pqmf=pqmf, lambda_stft=LAMBDA_STFT, use_feature_map_loss=True,
                      discriminator_train_start_steps=start, grad_clip_thresh=CLIP)
    spf = samples_per_frame(g, pqmf)
    assert spf == (12 if family == "hifigan" else 240)
    mel, wav = _batch(spf, seed=1)
    d_before = copy.deepcopy(d.state_dict())
    out = trainer.step(mel, wav, 1)
    assert tuple(out) == KEYS and all(isinstance(v, float) and np.isfinite(v) for v in out.values())

    # ---- the generator's half by hand: clip_grad_norm_ + torch.optim.Adam
    g2, d2 = _generator(name, cfg), _discriminator(discriminator_state)
    g2.parameter_grad = True
    opt2 = torch.optim.Adam(g2.parameters(), lr=LR, eps=1e-6)
    loss = Loss().to(DEV)
    loss.differentiable = True
    opt2.zero_grad()
    est = fit_estimate(g2(mel), wav.shape[1], pqmf)       # GOLDEN_CFG makes 1681 samples of 140 frames
    stft, _ = loss(est, wav, pqmf=pqmf)
    total = LAMBDA_STFT * stft
    adv = fm = torch.zeros((), device=DEV)
    if phase == "adversarial":
        wave = est if pqmf is None else pqmf_synthesis(est, pqmf)[:, 0, :]
        t = generator_adversarial_terms(d2, wave.unsqueeze(1), wav.unsqueeze(1))
        adv, fm = t["adversarial"], t["feature_map"]
        total = total + 1.0 * adv + 1.0 * fm
    total.backward()
    assert all(p.grad is None for p in d2.parameters())
    norm2 = torch.nn.utils.clip_grad_norm_(g2.parameters(), CLIP)
    opt2.step()

    assert out["stft"] == float(stft.detach()) and out["total"] == float(total.detach())
    assert out["adversarial"] == float(adv.detach()) and out["feature_map"] == float(fm.detach())
    assert abs(out["grad_norm"] - float(norm2)) <= NORM_VS_TORCH * float(norm2)
    worst, where = _worst(g.named_parameters(), g2.named_parameters())
    gworst, gwhere = _worst([(k, p.grad) for k, p in g.named_parameters()],
                            [(k, p.grad) for k, p in g2.named_parameters()])
    print(f"{family} {phase}: generator p {worst:.2e} ({where}), clipped grad {gworst:.2e} ({gwhere}), "
          f"norm {out['grad_norm']:.6e} / {float(norm2):.6e}")
    assert worst <= P_TOL, (worst, where)
    assert gworst <= NORM_VS_TORCH, (gworst, gwhere)          # the two clip factors differ by the norms' difference
    assert any(not torch.equal(p, q) for p, q in zip(g.parameters(), _generator(name, cfg).parameters()))

    if phase == "stft_only":
        assert out["adversarial"] == out["feature_map"] == out["discriminator"] == 0.0
        assert out["discriminator_grad_norm"] == 0.0
        for k, v in d.state_dict().items():
            assert torch.equal(v, d_before[k]), k              # the discriminator has not moved
        assert len(trainer.discriminator_optimizer.state) == 0
        return

    # ---- the discriminator's half by hand, on the generator the trainer left
    assert out["adversarial"] > 0.0 and out["feature_map"] > 0.0 and out["discriminator"] > 0.0
    opt_d2 = torch.optim.Adam(d2.parameters(), lr=LR_D, eps=1e-6)
    opt_d2.zero_grad()
    with torch.no_grad():
        est_d = fit_estimate(g(mel), wav.shape[1], pqmf)
        if pqmf is not None:
            est_d = pqmf.synthesis(est_d)[:, 0, :]
    d_loss = discriminator_step_terms(d2, est_d.unsqueeze(1), wav.unsqueeze(1), stft_grad=True)["discriminator"]
    d_loss.backward()
    dnorm2 = torch.nn.utils.clip_grad_norm_(d2.parameters(), CLIP)
    opt_d2.step()
    assert out["discriminator"] == float(d_loss.detach())
    assert abs(out["discriminator_grad_norm"] - float(dnorm2)) <= NORM_VS_TORCH * float(dnorm2)
    worst, where = _worst(d.named_parameters(), d2.named_parameters())
    print(f"{family} {phase}: discriminator p {worst:.2e} ({where}), norm {out['discriminator_grad_norm']:.6e} / "
          f"{float(dnorm2):.6e}")
    assert worst <= P_TOL, (worst, where)
    assert any(not torch.equal(v, d_before[k]) for k, v in d.state_dict().items())


def test_thirty_stft_steps_halve_the_loss_on_one_batch():
    name, cfg = CONFIGS["hifigan"]
    g, d = _generator(name, cfg, weight_seed=3), Discriminator().to(DEV)
    trainer = Trainer(g, d, optim.Adam(g.parameters(), lr=1e-3, eps=1e-6), optim.Adam(d.parameters(), lr=LR_D, eps=1e-6),
                      lambda_stft=LAMBDA_STFT, use_feature_map_loss=True, discriminator_train_start_steps=10 ** 9,
                      grad_clip_thresh=1.0)
    mel, wav = _batch(samples_per_frame(g), seed=2)
    losses = [trainer.step(mel, wav, s + 1)["stft"] for s in range(30)]
    print("overfit: sc + mag " + " ".join(f"{v:.3f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])


# ---- MODE=train through the launcher ----------------------------------------------------------------------------------

CLI_CFG = dict(cases._H, upsample_rates=[8, 5, 3, 2], upsample_kernel_sizes=[16, 10, 6, 4], upsample_initial_channel=32,
               lamda_stft=5.0, multiband=False, use_feature_map_loss=True)
LINES = [r"Epoch \[\d+/100000\], Step \[{step}/\d+\]:",
         r"STFT Loss: (\d+\.\d{{6}}), Weight Loss: 0\.000000, Total Loss: (\d+\.\d{{6}});",
         r"Adversarial Loss: (\d+\.\d{{6}}), Discriminator Loss: (\d+\.\d{{6}}), Feature Map Loss: (\d+\.\d{{6}});",
         r"Current Learning Rate is 0\.000100, discriminator Learning Rate is 0\.000050;"]


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


def _train(tmp_path, *extra):
    args = ["--model_name", "hifigan", "--config", str(tmp_path / "cfg.yaml"),
            "--audio_index_path", str(tmp_path / "audio_train.txt"), "--mel_index_path", str(tmp_path / "mel_train.txt"),
            "--audio_index_valid_path", str(tmp_path / "audio_valid.txt"),
            "--mel_index_valid_path", str(tmp_path / "mel_valid.txt"),
            "--discriminator_train_start_steps", "2", "--batch_size", "2", "--log_step", "1", *extra]
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), *args],
                       env=dict(os.environ, MODE="train"), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _logged(out, step):
    """The figures of the four log lines of ``step``: (stft, total, adversarial, discriminator, feature map)."""
    pattern = "\n".join(line.format(step=step) for line in LINES)
    m = re.search(pattern, out)
    assert m, f"the log lines of step {step} are missing or malformed:\n{out}"
    return [float(v) for v in m.groups()]


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    """Four steps of MODE=train on five utterances, the discriminator from step 3 on -> (directory, stdout)."""
    tmp_path = tmp_path_factory.mktemp("train")
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(CLI_CFG))
    _dataset(tmp_path, "train", 5, seed=0)
    _dataset(tmp_path, "valid", 2, seed=1)
    return tmp_path, _train(tmp_path, "--max_steps", "4", "--save_step", "4", "--valid_step", "4")


def test_mode_train_logs_validates_and_writes_its_files(first_run):
    tmp_path, out = first_run
    assert "---Start New Training---" in out
    for step in (1, 2, 3, 4):
        stft, total, adv, dis, fm = _logged(out, step)
        assert stft > 0.0 and total > 0.0
        if step <= 2:
            assert adv == dis == fm == 0.0
        else:
            assert adv > 0.0 and dis > 0.0 and fm > 0.0
    assert re.search(r"^valid 4 stft=\d\.\d{8}e[+-]\d\d$", out, flags=re.M)
    assert "save model at step 4 ..." in out
    (log_dir,) = glob.glob(str(tmp_path / "logger" / "*"))
    assert sorted(os.listdir(log_dir)) == ["logger.txt", "stft_loss.txt", "total_loss.txt"]
    assert len(open(os.path.join(log_dir, "total_loss.txt")).read().split()) == 4
    assert open(os.path.join(log_dir, "logger.txt")).read().count("Time Used: ") == 4


def test_the_checkpoint_has_the_four_keys_and_loads(first_run):
    from fastvocoder_amd.bin.synthesize import Synthesizer, load_checkpoint
    tmp_path, _ = first_run
    (ck,) = glob.glob(str(tmp_path / "checkpoint" / "*" / "checkpoint_4.pth.tar"))
    ckpt = load_checkpoint(ck, "cpu")
    assert sorted(ckpt) == ["discriminator", "discriminator_optimizer", "model", "optimizer"]
    assert {float(s["step"]) for s in ckpt["optimizer"]["state"].values()} == {4.0}
    assert {float(s["step"]) for s in ckpt["discriminator_optimizer"]["state"].values()} == {2.0}
    topt = torch.optim.Adam(build_generator("hifigan", CLI_CFG).parameters())       # torch's own Adam takes the entry
    topt.load_state_dict(ckpt["optimizer"])
    syn = Synthesizer(ck, str(tmp_path / "cfg.yaml"), "hifigan")
    est = syn.synthesize(np.random.RandomState(0).rand(30, 80).astype(np.float32))[0]
    assert est.shape == (30 * 240,) and bool(torch.isfinite(est).all())


def test_mode_train_resumes_from_its_checkpoint(first_run):
    from fastvocoder_amd.bin.synthesize import load_checkpoint
    tmp_path, _ = first_run
    (ck,) = glob.glob(str(tmp_path / "checkpoint" / "*" / "checkpoint_4.pth.tar"))
    out = _train(tmp_path, "--checkpoint_path", ck, "--restore_step", "4", "--max_steps", "2", "--save_step", "2",
                 "--valid_step", "100")
    assert "---Model Restored at Step 4---" in out and "optimizer state at step count 4" in out
    for step in (5, 6):
        stft, total, adv, dis, fm = _logged(out, step)
        assert adv > 0.0 and dis > 0.0 and fm > 0.0
    assert not re.search(r"Step \[[1-4]/", out)
    (ck6,) = glob.glob(str(tmp_path / "checkpoint" / "*" / "checkpoint_6.pth.tar"))
    ckpt6 = load_checkpoint(ck6, "cpu")
    assert {float(s["step"]) for s in ckpt6["optimizer"]["state"].values()} == {6.0}
    assert {float(s["step"]) for s in ckpt6["discriminator_optimizer"]["state"].values()} == {4.0}


def test_a_checkpoint_that_does_not_load_ends_the_run(first_run):
    tmp_path, _ = first_run
    (tmp_path / "broken.pth.tar").write_bytes(b"not a checkpoint")
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), "--model_name", "hifigan",
                        "--config", str(tmp_path / "cfg.yaml"), "--checkpoint_path", str(tmp_path / "broken.pth.tar")],
                       env=dict(os.environ, MODE="train"), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "MODE=train: cannot load --checkpoint_path" in r.stderr
    assert "Start New Training" not in r.stdout
