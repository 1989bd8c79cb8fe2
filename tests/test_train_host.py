"""CPU tests of the training path's host side: the buffer dataset and its seeded crops (fastvocoder_amd/data.py), the
arguments, refusals and log lines of MODE=train (fastvocoder_amd/bin/train.py), the launcher's dispatch, the training
constants of hparams.py and what ``Trainer`` checks before it touches the GPU."""
import numpy as np
import pytest
import torch

from fastvocoder_amd import data, hparams, optim
from fastvocoder_amd.bin import launcher
from fastvocoder_amd.bin import train as train_cli
from fastvocoder_amd.discriminator import Discriminator
from fastvocoder_amd.generator import HiFiGANGenerator, MelGANGenerator, MultiBandHiFiGANGenerator, PQMF
from fastvocoder_amd.loss import PqmfSynthesis, pqmf_synthesis  # noqa: F401 -- the public names
from fastvocoder_amd.train import KEYS, Trainer, samples_per_frame

HOP = 12


def _write(tmp_path, frames_list, hop=HOP):
    audio, mel = [], []
    for i, frames in enumerate(frames_list):
        wav = (np.arange(frames * hop) + 100000 * i).astype(np.float32)          # a sample names its utterance and position
        m = np.tile((np.arange(frames) + 1000 * i).astype(np.float32), (80, 1))   # [80, T]: column t holds t (+ 1000 i)
        np.save(tmp_path / f"u{i}.npy", wav)
        np.save(tmp_path / f"u{i}.mel.npy", m)
        audio.append(str(tmp_path / f"u{i}.npy"))
        mel.append(str(tmp_path / f"u{i}.mel.npy"))
    (tmp_path / "audio.txt").write_text("".join(p + "\n" for p in audio))
    (tmp_path / "mel.txt").write_text("".join(p + "\n" for p in mel))
    return str(tmp_path / "audio.txt"), str(tmp_path / "mel.txt")


def test_the_buffer_holds_transposed_mels(tmp_path):
    buffer = data.load_data_to_buffer(*_write(tmp_path, [9, 12]))
    assert [tuple(b["mel"].shape) for b in buffer] == [(9, 80), (12, 80)]              # [T, 80], dataset.py:38
    assert [tuple(b["wav"].shape) for b in buffer] == [(9 * HOP,), (12 * HOP,)]
    assert buffer[1]["mel"].dtype == buffer[1]["wav"].dtype == torch.float32
    assert buffer[1]["mel"][5, 0] == 1005.0 and buffer[1]["mel"][5, 79] == 1005.0
    assert len(data.load_data_to_buffer(*_write(tmp_path, [9, 12]), size=1)) == 1       # hparams.test_size's role
    (tmp_path / "short.txt").write_text(str(tmp_path / "u0.npy") + "\n")
    with pytest.raises(ValueError, match="lists 1 waveforms"):
        data.load_data_to_buffer(str(tmp_path / "short.txt"), str(tmp_path / "mel.txt"))


def test_the_crops_have_the_reference_ranges_and_are_seeded(tmp_path, capsys):
    fixed = 6
    frames = [7, 10, 6, 5, 15, 8, 7]               # 6 and 5 are too short: randint(0, len - fixed - 1) needs len > fixed
    buffer = data.load_data_to_buffer(*_write(tmp_path, frames))
    it = data.BatchIterator(buffer, batch_size=2, fixed_length=fixed, hop=HOP, seed=3)
    assert "data: 2 of 7 train utterances are too short for a crop of 6 frames and are left out" in capsys.readouterr().out
    assert it.skipped == 2 and len(it.items) == 5 and len(it) == 2                      # drop_last: 5 // 2
    starts = {i: set() for i in range(len(frames))}
    for _ in range(200):
        seen = []
        for mel, wav in it.epoch():
            assert mel.shape == (2, fixed, 80) and wav.shape == (2, fixed * HOP)
            for m, w in zip(mel, wav):
                utt, start = int(m[0, 0]) // 1000, int(m[0, 0]) % 1000
                assert torch.equal(m[:, 0], torch.arange(start, start + fixed).float() + 1000 * utt)
                assert torch.equal(w, torch.arange(start * HOP, (start + fixed) * HOP).float() + 100000 * utt)
                starts[utt].add(start)
                seen.append(utt)
        assert len(seen) == 4 and len(set(seen)) == 4                                   # an epoch visits no utterance twice
    # the first frame is uniform in [0, frames - fixed - 1], both ends reached, never beyond
    assert starts == {0: {0}, 1: {0, 1, 2, 3}, 2: set(), 3: set(), 4: set(range(9)), 5: {0, 1}, 6: {0}}

    def run(seed):
        it = data.BatchIterator(buffer, batch_size=2, fixed_length=fixed, hop=HOP, seed=seed)
        return [(m.clone(), w.clone()) for _ in range(3) for m, w in it.epoch()]
    a, b, c = run(5), run(5), run(6)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(a, c))
    orders = {tuple(int(m[0, 0, 0]) // 1000 for m, _ in run(s)[:2]) for s in range(12)}
    assert len(orders) > 1                                                              # shuffled per seed


def test_nothing_is_printed_when_every_utterance_fits(tmp_path, capsys):
    buffer = data.load_data_to_buffer(*_write(tmp_path, [9, 12]))
    it = data.BatchIterator(buffer, batch_size=1, fixed_length=6, hop=HOP)
    assert it.skipped == 0 and capsys.readouterr().out == ""


def test_the_arguments_are_the_references_plus_the_overrides():
    args = train_cli.build_parser().parse_args([])
    want = dict(audio_index_path="dataset/audio/train", mel_index_path="dataset/mel/train",
                audio_index_valid_path="dataset/audio/valid", mel_index_valid_path="dataset/mel/valid",
                checkpoint_path="", restore_step=0, learning_rate=1e-4, learning_rate_discriminator=5e-5,
                model_name=None, config=None, use_scheduler=0, mixprecision=0,
                max_steps=0, seed=0, batch_size=32, fixed_length=140, discriminator_train_start_steps=100000,
                log_step=5, save_step=5000, valid_step=500, valid_num=100, use_mpd=0)
    assert vars(args) == want


@pytest.mark.parametrize("argv, words", [
    (["--model_name", "melgan", "--config", "c.yaml"], ("melgan", "no parameter gradient")),
    (["--model_name", "basis-melgan", "--config", "c.yaml"], ("basis-melgan", "no parameter gradient")),
    (["--model_name", "hifigan", "--config", "c.yaml", "--mixprecision", "1"], ("mixprecision", "mixed-precision")),
    (["--model_name", "wavenet", "--config", "c.yaml"], ("model_name", "hifigan, multiband-hifigan")),
    (["--model_name", "hifigan"], ("--config",)),
    (["--model_name", "hifigan", "--config", "c.yaml", "--batch_size", "0"], ("batch_size",)),
])
def test_what_cannot_be_trained_exits_with_one_sentence(argv, words):
    with pytest.raises(SystemExit) as e:
        train_cli.run_train(argv)
    message = str(e.value)
    assert message.startswith("MODE=train: ") and "\n" not in message
    assert all(w in message for w in words), message


def test_mode_train_reaches_run_train(monkeypatch):
    called = []
    monkeypatch.setattr(train_cli, "run_train", lambda: called.append(True))
    monkeypatch.setenv("MODE", "train")
    launcher.main()
    assert called == [True]
    monkeypatch.setenv("MODE", "nonsense")
    with pytest.raises(SystemExit, match="MODE=train"):
        launcher.main()


def test_the_log_lines_have_the_reference_format():
    # the reference's format strings, bin/train.py:201-208
    epoch, epochs, current_step, total_step = 2, 100000, 17, 2800000
    s_l, w_l, t_l, a_l, d_l, f_l, lr, lr_d = 1.23456789, 0., 6.5, 0.25, 0.5000004, 3.0, 1e-4, 5e-5
    want = [f"Epoch [{epoch + 1}/{epochs}], Step [{current_step}/{total_step}]:",
            "STFT Loss: {:.6f}, Weight Loss: {:.6f}, Total Loss: {:.6f};".format(s_l, w_l, t_l),
            "Adversarial Loss: {:.6f}, Discriminator Loss: {:.6f}, Feature Map Loss: {:.6f};".format(a_l, d_l, f_l),
            "Current Learning Rate is {:.6f}, discriminator Learning Rate is {:.6f};".format(lr, lr_d)]
    got = train_cli.format_log_lines(epoch, epochs, current_step, total_step, s_l, w_l, t_l, a_l, d_l, f_l, lr, lr_d)
    assert got == want
    assert got == ["Epoch [3/100000], Step [17/2800000]:",
                   "STFT Loss: 1.234568, Weight Loss: 0.000000, Total Loss: 6.500000;",
                   "Adversarial Loss: 0.250000, Discriminator Loss: 0.500000, Feature Map Loss: 3.000000;",
                   "Current Learning Rate is 0.000100, discriminator Learning Rate is 0.000050;"]
    assert train_cli.format_time_line(12.3456, 7.0) == "Time Used: 12.346s, Estimated Time Remaining: 7.000s."


def test_hparams_carry_the_reference_training_constants():
    want = dict(test_size=0, train_size=9000, valid_size=500, eval_size=100, epochs=100000, batch_size=32,
                batch_expand_size=8, discriminator_train_start_steps=100000, n_warm_up_step=0,
                use_feature_map_loss=True, learning_rate=1e-4, learning_rate_discriminator=5e-5, grad_clip_thresh=1.0,
                log_step=5, clear_time=20, save_step=5000, valid_step=500, valid_num=100, checkpoint_path="checkpoint",
                logger_path="logger", tensorboard_path="tensorboard", fixed_length=140, lambda_adv=1.0, lambda_fm=1.0,
                lambda_stft=5.0, hop_size=240, sample_rate=24000)
    assert {k: getattr(hparams, k) for k in want} == want


def test_the_samples_per_frame_come_from_the_generator():
    assert samples_per_frame(HiFiGANGenerator()) == 240 == hparams.hop_size
    assert samples_per_frame(HiFiGANGenerator(upsample_rates=[4, 3], upsample_kernel_sizes=[8, 7],
                                              upsample_initial_channel=16)) == 12
    mb = MultiBandHiFiGANGenerator(upsample_initial_channel=16)
    assert samples_per_frame(mb) == 60 and samples_per_frame(mb, PQMF()) == 240


def test_the_trainer_checks_its_parts_before_any_launch():
    small = dict(upsample_rates=[4, 3], upsample_kernel_sizes=[8, 7], upsample_initial_channel=16)
    g, d = HiFiGANGenerator(**small), Discriminator()
    kw = dict(lambda_stft=5.0, use_feature_map_loss=True, discriminator_train_start_steps=10, grad_clip_thresh=1.0)
    ours = optim.Adam(g.parameters(), lr=1e-4), optim.Adam(d.parameters(), lr=5e-5)
    with pytest.raises(TypeError, match="fastvocoder_amd.optim.Adam"):
        Trainer(g, d, torch.optim.Adam(g.parameters()), ours[1], **kw)
    with pytest.raises(TypeError, match="discriminator_optimizer"):
        Trainer(g, d, ours[0], torch.optim.Adam(d.parameters()), **kw)
    assert g.parameter_grad is False
    t = Trainer(g, d, *ours, **kw)
    assert g.parameter_grad is True and t.samples_per_frame == 12 and t.vocoder_loss.differentiable is True
    assert t.period_grad is False and Trainer(g, Discriminator(use_mpd=True), *ours, **kw).period_grad is True
    with pytest.raises(ValueError, match=r"wav \(B, T \* 12\)"):
        t.step(torch.zeros(2, 80, 140), torch.zeros(2, 140 * 240), 1)
    up = HiFiGANGenerator(transposedconv=False, **small)
    with pytest.raises(NotImplementedError, match="UpsampleLayer"):
        Trainer(up, d, optim.Adam(up.parameters()), ours[1], **kw)
    from tests import cases
    mel = MelGANGenerator(**next(c for t_, _, c in cases.SMALL if t_ == "melgan_s"))
    with pytest.raises(NotImplementedError, match="ResidualStack"):
        Trainer(mel, d, optim.Adam(mel.parameters()), ours[1], **kw)
    assert KEYS == ("stft", "total", "adversarial", "feature_map", "discriminator", "grad_norm",
                    "discriminator_grad_norm")
