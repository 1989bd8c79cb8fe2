"""GPU tests of the mel front end (csrc/mel.hip, fv_melspectrogram; audio.melspectrogram) against the
float64 oracle tests/mel_reference.py, its copy-synthesis chain into a generator, and MODE=preprocess."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from fastvocoder_amd import _native, audio, hparams
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.synthetic import seeded_state_dict
from tests import cases
from tests import mel_reference
from tests import stream_tools

pytestmark = pytest.mark.gpu

TOL, TOL_HI = 1e-4, 5e-6          # normalised units (1e-4 = 0.01 dB); the tighter bound where the mel is >= 0.3


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _demo(golden_dir):
    d = np.load(os.path.join(golden_dir, "mel_demo.npz"))
    return d["wav"], d["mel"].astype(np.float64)


def _signals(golden_dir):
    wav, _ = _demo(golden_dir)
    demo = wav / 32768.0
    rs = np.random.RandomState(11)
    t = np.arange(48000) / 24000.0
    return {
        "demo": demo,
        "noise": rs.uniform(-1, 1, 30000),
        "sine440": np.sin(2 * np.pi * 440 * t),
        "demo_1e-3": demo * 1e-3,
        "silence": np.zeros(24000),
        "int16_extremes": rs.choice([-32768.0, 32767.0], 12000),
    }


def _check(got, y):
    ref = mel_reference.melspectrogram(y)
    assert got.shape == ref.shape == (80, 1 + len(y) // 240), (got.shape, ref.shape)
    d = np.abs(got.astype(np.float64) - ref)
    hi = ref >= 0.3
    return float(d.max()), float(d[hi].max()) if hi.any() else 0.0


def test_signals_against_the_oracle(golden_dir):
    for name, y in _signals(golden_dir).items():
        got = audio.melspectrogram(y.astype(np.float32))
        err, err_hi = _check(got, y.astype(np.float32).astype(np.float64))
        print(f"{name}: max {err:.2e}, where ref >= 0.3: {err_hi:.2e}")
        assert err <= TOL and err_hi <= TOL_HI, (name, err, err_hi)
        if name == "silence":
            assert not got.any()


def test_lengths_against_the_oracle():
    rs = np.random.RandomState(5)
    for n in (1025, 1026, 1200, 2047, 2048, 2401, 24000, 24119, 37777, 240000):
        y = (rs.uniform(-1, 1, n) * np.sin(np.arange(n) / 300.0)).astype(np.float32)
        got = audio.melspectrogram(y)
        err, err_hi = _check(got, y.astype(np.float64))
        assert got.shape[1] == 1 + n // 240
        assert err <= TOL and err_hi <= TOL_HI, (n, err, err_hi)


def test_demo_meets_the_reference_mel(golden_dir):
    wav, ref = _demo(golden_dir)
    got = audio.melspectrogram((wav / 32768.0).astype(np.float32)).astype(np.float64)
    mae, corr = mel_reference.offset_free_agreement(got[:, :ref.shape[1]], ref)
    assert mae <= 0.03 and corr >= 0.98, (mae, corr)


def test_batch_rows_equal_single_calls_and_numpy_route():
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.uniform(-1, 1, (5, 9000)).astype(np.float32)).to(_dev())
    x[2] *= 1e-3
    x[4].zero_()
    batch = audio.melspectrogram(x)
    assert batch.shape == (5, 80, 1 + 9000 // 240) and batch.is_cuda and batch.dtype == torch.float32
    for b in range(5):
        single = audio.melspectrogram(x[b])
        assert single.shape == (1, 80, batch.shape[2])
        assert torch.equal(single[0], batch[b]), b
        assert np.array_equal(audio.melspectrogram(x[b].cpu().numpy()), batch[b].cpu().numpy()), b


def test_non_default_stream_gives_identical_results():
    """On a side stream that is still busy (tests/stream_tools.py): the input arrives behind a delay and holds NaN until
    then, so a launch on any other stream than the caller's reads NaN."""
    x = np.random.RandomState(9).uniform(-1, 1, (3, 50000)).astype(np.float32)
    want, wall = stream_tools.timed(lambda: audio.melspectrogram(torch.from_numpy(x).to(_dev())))
    torch.cuda.synchronize()
    s = stream_tools.side_stream()
    with stream_tools.delayed(s, stream_tools.delay_ms(wall)) as put:
        got = audio.melspectrogram(put(x))
        stream_tools.assert_busy(put, "melspectrogram")
    s.synchronize()
    assert torch.equal(got, want)


def test_bad_input_raises():
    x = torch.zeros((2, 1024), device=_dev())
    with pytest.raises(_native.NativeError, match="reflect"):
        audio.melspectrogram(x)
    x = torch.zeros((2, 4000), device=_dev())
    tab = audio.mel_tables(x.device)
    for kw in (dict(n_fft=1024), dict(hop=256), dict(win_length=1024), dict(n_mels=128), dict(fmin=0.0),
               dict(sample_rate=22050)):
        with pytest.raises(_native.NativeError, match="only sr=24000"):
            _native.melspectrogram(x, tab, **kw)
    with pytest.raises(_native.NativeError):
        audio.melspectrogram(torch.zeros(4000))                      # a CPU tensor: no host path


def test_copy_synthesis_through_hifigan_light(golden_dir):
    """wav -> melspectrogram -> HiFi-GAN light forward, all on the device, against the generator on the oracle's mel."""
    wav, _ = _demo(golden_dir)
    y = (wav[24000:72000] / 32768.0).astype(np.float32)
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    model = build_generator("hifigan", cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=3).items()})
    model = model.to(_dev()).eval()
    with torch.no_grad():
        got = model(audio.melspectrogram(torch.from_numpy(y).to(_dev())))
        ref = model(torch.from_numpy(mel_reference.melspectrogram(y.astype(np.float64))[None].astype(np.float32)).to(_dev()))
    assert got.shape == ref.shape and got.shape[-1] == (1 + len(y) // 240) * 240
    err = float((got - ref).abs().max())
    print(f"copy-synthesis: max |forward(kernel mel) - forward(oracle mel)| = {err:.2e}")
    assert err <= 1e-4, err


def _write_wavs(tmp_path, n_files):
    rs = np.random.RandomState(21)
    paths = []
    for i in range(n_files):
        n = 3000 + 977 * i
        s = (rs.uniform(-0.6, 0.6, n) * 32767).astype(np.int16)
        p = str(tmp_path / f"utt{i}.wav")
        scipy.io.wavfile.write(p, 24000, s)
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(p + "\n" for p in paths))
    return paths, str(lst)


def _check_outputs(paths, save):
    for p in paths:
        name = os.path.basename(p)
        mel = np.load(os.path.join(save, f"{name}.mel.npy"))
        y = np.load(os.path.join(save, f"{name}.npy"))
        want_y = audio.load_wav(p, encode=False)
        assert y.dtype == np.float32 and np.array_equal(y, want_y)
        assert mel.dtype == np.float64 and mel.shape == (80, 1 + len(y) // 240)
        assert np.array_equal(mel, audio.melspectrogram(want_y).astype(np.float64))


def _read_index(path):
    with open(path) as f:
        return [line.rstrip("\n") for line in f]


def test_run_preprocess_in_process_partitions_the_list(tmp_path, monkeypatch, capsys):
    from fastvocoder_amd.bin import preprocess
    paths, lst = _write_wavs(tmp_path, 6)
    monkeypatch.setattr(hparams, "train_size", 3)
    monkeypatch.setattr(hparams, "valid_size", 2)
    monkeypatch.setattr(hparams, "eval_size", 1)
    save, ai, mi = str(tmp_path / "out"), str(tmp_path / "audio"), str(tmp_path / "mel")
    preprocess.run_preprocess(["--data_path", lst, "--save_path", save, "--audio_index_path", ai,
                               "--mel_index_path", mi])
    out = capsys.readouterr().out
    assert f"min length of mel spectrogram is {1 + 3000 // 240}." in out
    _check_outputs(paths, save)
    parts = {k: _read_index(os.path.join(ai, k)) for k in ("train", "valid", "eval")}
    assert [len(parts[k]) for k in ("train", "valid", "eval")] == [3, 2, 1]
    names = sorted(sum(parts.values(), []))
    assert names == sorted(os.path.join(save, os.path.basename(p) + ".npy") for p in paths)
    for k in parts:
        assert _read_index(os.path.join(mi, k)) == [p[:-len(".npy")] + ".mel.npy" for p in parts[k]]


def test_mode_preprocess_through_the_launcher(tmp_path):
    """The command line of the reference: MODE=preprocess bin/launcher.py with its four flags.  With the default
    split sizes (9600 utterances) a small list trips the reference's assert, after the files are written."""
    paths, lst = _write_wavs(tmp_path, 2)
    save, ai, mi = str(tmp_path / "out"), str(tmp_path / "audio"), str(tmp_path / "mel")
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), "--data_path", lst,
                        "--save_path", save, "--audio_index_path", ai, "--mel_index_path", mi],
                       env=dict(os.environ, MODE="preprocess"), cwd=cases.ROOT, capture_output=True, text=True,
                       timeout=600)
    assert f"min length of mel spectrogram is {1 + 3000 // 240}." in r.stdout, r.stdout + r.stderr
    assert r.returncode != 0 and "train + valid + eval = 9600" in r.stderr, r.stdout + r.stderr
    _check_outputs(paths, save)
