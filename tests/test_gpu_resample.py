"""GPU tests of the resampler (csrc/resample.hip, fv_resample; audio.resample, load_wav(resample=True), MODE=preprocess
--resample) against the float64 oracle tests/resample_reference.py.

The accuracy bound is derived, not tuned (resample_reference.error_bound): the table's coefficients are rounded once to fp32
and an output is a chain of `taps` fp32 FMAs whose partial sums stay below ||h_r||_1 max|x|, so
    |kernel - oracle| <= (taps + 2) 2^-24 max_r ||h_r||_1 max|x|
(4.7e-5 at full scale for the longest filter, 96000 -> 24000).  The bit identities hold because an output is one thread's
FMA chain over its taps in a fixed order: its bits depend on its input neighbourhood and its phase alone."""
import os

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from fastvocoder_amd import _native, audio, hparams
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.synthetic import seeded_state_dict
from tests import cases
from tests import resample_reference as rr

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _err(got, x32, sr_in, sr_out, start=0, stop=None):
    """(max |got - oracle|, bound) for float32 samples x32; got: the kernel's outputs [start, stop)."""
    ref = rr.resample(x32.astype(np.float64), sr_in, sr_out, start, stop)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = rr.error_bound(sr_in, sr_out, float(np.abs(x32).max()) if len(x32) else 0.0)
    return (float(np.abs(got.astype(np.float64) - ref).max()) if len(ref) else 0.0), bound


def _signals():
    rs = np.random.RandomState(17)
    noise = rs.uniform(-1, 1, 4000).astype(np.float32)
    return {
        "noise": noise,
        "sine440": np.sin(2 * np.pi * 440 * np.arange(4000) / 24000.0).astype(np.float32),
        "noise_1e-3": (noise * np.float32(1e-3)).astype(np.float32),
        "zeros": np.zeros(4000, dtype=np.float32),
        "int16_extremes": rs.choice(np.array([-32768, 32767], dtype=np.int16), 4000),
    }


@pytest.mark.parametrize("sr_in,sr_out", rr.PAIRS)
def test_signals_against_the_oracle(sr_in, sr_out):
    worst = 0.0
    for name, x in _signals().items():
        if x.dtype == np.int16:                                   # the PCM route: converted on the device
            got = audio.resample(_to_dev(x), sr_in, sr_out).cpu().numpy()
            x = x.astype(np.float32) / np.float32(32768)
        else:
            got = audio.resample(x, sr_in, sr_out)
        assert got.dtype == np.float32
        err, bound = _err(got, x, sr_in, sr_out)
        worst = max(worst, err / bound if bound else 0.0)
        print(f"{sr_in} -> {sr_out} {name}: max |kernel - oracle| = {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (name, err, bound)
        if name == "zeros":
            assert not got.any()
    print(f"{sr_in} -> {sr_out}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 24000), (22050, 24000), (48000, 22050)])
def test_lengths_against_the_oracle(sr_in, sr_out):
    """Inputs shorter than the filter, and the ragged last block."""
    L, M, _, half = rr.geometry(sr_in, sr_out)
    taps = 2 * half + 2
    rs = np.random.RandomState(23)
    for n in (1, 2, half - 1, taps, taps + 1, 1000, 4097, 24001):
        x = rs.uniform(-1, 1, n).astype(np.float32)
        got = audio.resample(x, sr_in, sr_out)
        assert got.shape == (int(np.ceil(n * L / M)),)
        err, bound = _err(got, x, sr_in, sr_out)
        assert err <= bound, (n, err, bound)


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 24000), (48000, 22050), (16000, 24000)])
def test_batch_rows_numpy_route_and_int16_are_bit_identical(sr_in, sr_out):
    rs = np.random.RandomState(29)
    pcm = rs.randint(-32768, 32768, (5, 9000)).astype(np.int16)
    pcm[2] //= 1000
    pcm[4] = 0
    x16 = _to_dev(pcm)
    x = _to_dev(pcm.astype(np.float32) / np.float32(32768))
    batch = audio.resample(x, sr_in, sr_out)
    L, M, _, _ = rr.geometry(sr_in, sr_out)
    assert batch.shape == (5, rr.out_len(9000, L, M)) and batch.is_cuda and batch.dtype == torch.float32
    assert torch.equal(audio.resample(x16, sr_in, sr_out), batch)            # int16 against the same samples as float32
    for b in range(5):
        single = audio.resample(x[b], sr_in, sr_out)
        assert single.shape == (batch.shape[1],)
        assert torch.equal(single, batch[b]), b
        assert torch.equal(audio.resample(x16[b], sr_in, sr_out), batch[b]), b
        assert np.array_equal(audio.resample(x[b].cpu().numpy(), sr_in, sr_out), batch[b].cpu().numpy()), b


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 24000), (48000, 22050)])
@pytest.mark.parametrize("k", [1, 7])
def test_outputs_do_not_depend_on_their_position_in_a_block(sr_in, sr_out, k):
    """k M zeros in front move every output by k L -- to another thread, another block -- and leave its phase alone."""
    L, M, _, half = rr.geometry(sr_in, sr_out)
    x = _to_dev(np.random.RandomState(31).uniform(-1, 1, 6000).astype(np.float32))
    plain = audio.resample(x, sr_in, sr_out)
    moved = audio.resample(torch.cat([torch.zeros(k * M, device=x.device), x]), sr_in, sr_out)
    assert moved.shape[0] == plain.shape[0] + k * L
    first = -((-half * L) // M)                 # the first output whose window starts at x[0] or later: c >= half
    assert first < plain.shape[0]
    assert torch.equal(moved[k * L + first:], plain[first:])


def test_equal_rates_and_refusals_on_the_device():
    x = torch.arange(-5, 5, dtype=torch.int16, device=_dev())
    same = audio.resample(x, 24000, 24000)
    assert same.dtype == torch.float32 and torch.equal(same, x.float() / 32768)
    xf = torch.rand(10, device=_dev())
    assert audio.resample(xf, 16000, 16000) is xf
    with pytest.raises(_native.NativeError, match="ROCm device"):
        audio.resample(torch.zeros(4000), 48000, 24000)                 # a CPU tensor: no host path
    with pytest.raises(_native.NativeError):
        audio.resample(torch.zeros(4000, dtype=torch.float64, device=_dev()), 48000, 24000)
    with pytest.raises(ValueError, match="empty"):
        audio.resample(torch.zeros((2, 0), device=_dev()), 48000, 24000)
    tab = audio.resample_tables(_dev(), 48000, 24000)
    with pytest.raises(_native.NativeError, match="table"):
        _native.resample(torch.zeros((1, 100), device=_dev()), tab, 1, 2, 135)   # half is 136: another table size


def test_indices_beyond_32_bits():
    """48000 -> 22050 (M = 320): j M passes 2^31 at j = 6 710 887.  Outputs around it and the last ones."""
    sr_in, sr_out, n = 48000, 22050, 14_700_000
    x = np.random.RandomState(37).uniform(-1, 1, n).astype(np.float32)
    y = audio.resample(_to_dev(x), sr_in, sr_out)
    n_out = rr.out_len(n, 147, 320)
    assert y.shape == (n_out,) and n_out > 6_710_887 + 1024
    for start, stop in ((6_710_887 - 1024, 6_710_887 + 1024), (n_out - 2048, n_out)):
        err, bound = _err(y[start:stop].cpu().numpy(), x, sr_in, sr_out, start, stop)
        print(f"outputs [{start}, {stop}): max |kernel - oracle| = {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (start, err, bound)


def _write_off_rate_wavs(tmp_path):
    rs = np.random.RandomState(41)
    files = {
        "mono48k.wav": (48000, (rs.uniform(-0.6, 0.6, 9000) * 32767).astype(np.int16)),
        "stereo44k.wav": (44100, (rs.uniform(-0.6, 0.6, (8000, 2)) * 32767).astype(np.int16)),
        "float22k.wav": (22050, rs.uniform(-0.6, 0.6, 5000).astype(np.float32)),
    }
    paths = {}
    for name, (sr, s) in files.items():
        paths[name] = str(tmp_path / name)
        scipy.io.wavfile.write(paths[name], sr, s)
    return files, paths


def _host_samples(s):
    """load_wav's host conversion: mono float32."""
    s = s.astype(np.float32) / 32768.0 if s.dtype == np.int16 else s.astype(np.float32)
    return np.ascontiguousarray(s.mean(axis=1, dtype=np.float32) if s.ndim == 2 else s, dtype=np.float32)


def test_load_wav_resamples_files_at_another_rate(tmp_path):
    files, paths = _write_off_rate_wavs(tmp_path)
    for name, (sr, s) in files.items():
        with pytest.raises(ValueError, match="does not resample"):
            audio.load_wav(paths[name], encode=False)
        want = audio.resample(_host_samples(s), sr, 24000)
        got = audio.load_wav(paths[name], encode=False, resample=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want), name
        kept = audio.load_wav(paths[name], encode=False, resample=True, keep_on_device=True)
        assert torch.is_tensor(kept) and kept.is_cuda and np.array_equal(kept.cpu().numpy(), want), name
        enc = audio.load_wav(paths[name], resample=True)
        assert enc.dtype == np.int16 and np.array_equal(enc, audio.encode_16bits(want.copy())), name


def _write_mixed_list(tmp_path):
    rs = np.random.RandomState(43)
    paths = []
    for i, (sr, n) in enumerate(((48000, 9000), (44100, 8000), (24000, 3000))):
        p = str(tmp_path / f"utt{i}_{sr}.wav")
        scipy.io.wavfile.write(p, sr, (rs.uniform(-0.6, 0.6, n) * 32767).astype(np.int16))
        paths.append((p, sr))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(p + "\n" for p, _ in paths))
    return paths, str(lst)


def _read_index(path):
    with open(path) as f:
        return [line.rstrip("\n") for line in f]


def _split(monkeypatch, train, valid, evals):
    monkeypatch.setattr(hparams, "train_size", train)
    monkeypatch.setattr(hparams, "valid_size", valid)
    monkeypatch.setattr(hparams, "eval_size", evals)


def test_run_preprocess_with_resample_takes_every_file(tmp_path, monkeypatch, capsys):
    from fastvocoder_amd.bin import preprocess
    paths, lst = _write_mixed_list(tmp_path)
    _split(monkeypatch, 1, 1, 1)
    save, ai, mi = str(tmp_path / "out"), str(tmp_path / "audio"), str(tmp_path / "mel")
    preprocess.run_preprocess(["--data_path", lst, "--save_path", save, "--audio_index_path", ai,
                               "--mel_index_path", mi, "--resample"])
    out = capsys.readouterr().out
    assert "ERROR" not in out and f"min length of mel spectrogram is {1 + 3000 // 240}." in out
    for p, sr in paths:
        name = os.path.basename(p)
        y, mel = np.load(os.path.join(save, f"{name}.npy")), np.load(os.path.join(save, f"{name}.mel.npy"))
        pcm = scipy.io.wavfile.read(p)[1]
        want = audio.resample(pcm.astype(np.float32) / 32768.0, sr, 24000)
        assert y.dtype == np.float32 and np.array_equal(y, want), name
        assert mel.dtype == np.float64 and mel.shape == (80, 1 + len(want) // 240)
        assert np.array_equal(mel, audio.melspectrogram(want).astype(np.float64)), name
    parts = {k: _read_index(os.path.join(ai, k)) for k in ("train", "valid", "eval")}
    assert [len(parts[k]) for k in ("train", "valid", "eval")] == [1, 1, 1]
    assert sorted(sum(parts.values(), [])) == sorted(os.path.join(save, os.path.basename(p) + ".npy") for p, _ in paths)
    for k in parts:
        assert _read_index(os.path.join(mi, k)) == [p[:-len(".npy")] + ".mel.npy" for p in parts[k]]


def test_run_preprocess_without_the_flag_reports_off_rate_files(tmp_path, monkeypatch, capsys):
    """Today's behaviour, pinned: one ERROR line per file at another rate, only the 24 kHz file indexed."""
    from fastvocoder_amd.bin import preprocess
    paths, lst = _write_mixed_list(tmp_path)
    _split(monkeypatch, 1, 0, 0)
    save, ai, mi = str(tmp_path / "out"), str(tmp_path / "audio"), str(tmp_path / "mel")
    preprocess.run_preprocess(["--data_path", lst, "--save_path", save, "--audio_index_path", ai,
                               "--mel_index_path", mi])
    out = capsys.readouterr().out
    errors = [line for line in out.splitlines() if line.startswith("ERROR:")]
    assert len(errors) == 2 and all("does not resample" in line for line in errors), out
    for (p, sr), line in zip(paths[:2], errors):
        assert p in line and f"{sr} Hz" in line
    at_rate = os.path.join(save, os.path.basename(paths[2][0]))
    assert _read_index(os.path.join(ai, "train")) == [at_rate + ".npy"]
    assert _read_index(os.path.join(mi, "train")) == [at_rate + ".mel.npy"]
    assert sorted(os.listdir(save)) == sorted(os.path.basename(at_rate) + e for e in (".npy", ".mel.npy"))


def test_resample_chains_into_mel_and_generator_on_the_device():
    """48 kHz PCM -> resample -> melspectrogram -> HiFi-GAN light forward: every intermediate is a device tensor."""
    pcm = (np.random.RandomState(47).uniform(-0.5, 0.5, 48000) * 32767).astype(np.int16)
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    model = build_generator("hifigan", cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=3).items()})
    model = model.to(_dev()).eval()
    with torch.no_grad():
        y = audio.resample(_to_dev(pcm), 48000, 24000)
        mel = audio.melspectrogram(y)
        out = model(mel)
        host = audio.resample(pcm.astype(np.float32) / 32768.0, 48000, 24000)      # the same chain from the host route
        ref = model(_to_dev(audio.melspectrogram(host)[None]))
    assert y.is_cuda and y.shape == (24000,) and mel.is_cuda and mel.shape == (1, 80, 101) and out.is_cuda
    assert out.shape[-1] == 101 * 240 and bool(torch.isfinite(out).all())
    assert torch.equal(out, ref)
