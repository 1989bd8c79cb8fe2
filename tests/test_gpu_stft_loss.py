"""GPU tests of the multi-resolution STFT distance (csrc/stft_loss.hip, fv_stft_magnitude / fv_stft_distance;
fastvocoder_amd.loss) against the float64 oracle tests/stft_loss_reference.py and the reference's values
(tests/golden/stft_loss.npz), and of MODE=evaluation."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.generator.pqmf import PQMF
from fastvocoder_amd.loss import Loss, MultiResolutionSTFTLoss, STFTLoss, stft
from fastvocoder_amd.synthetic import seeded_state_dict
from tests import cases
from tests import stft_loss_reference as ref
from tests import stream_tools

pytestmark = pytest.mark.gpu

# against the float64 oracle: the worst errors measured on MI355X times a margin of about 10
MAG_RTOL = 2e-5          # magnitudes, relative to the frame's largest bin (fp32 FFT round-off)
SC_RTOL = 1e-6           # spectral convergence, relative (worst 4.3e-8)
MAG_ATOL = 2e-6          # log-magnitude L1, absolute, broadband signals (worst 2.3e-7)
MAG_ATOL_CLAMP = 2e-5    # the same where many bins sit near the 1e-7 power clamp: sine, silent target (worst 2.5e-6)
# against the reference's own values, computed in float32 torch (the oracle meets them within 2e-6)
GOLDEN_RTOL = 1e-5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _demo(golden_dir):
    return np.load(os.path.join(golden_dir, "mel_demo.npz"))["wav"] / 32768.0


def _pairs(golden_dir):
    """name -> (x estimate, y target, clamp-sensitive) float32 [B, n]"""
    rs = np.random.RandomState(17)
    demo = _demo(golden_dir)[:60000]
    n = demo.shape[0]
    t = np.arange(n) / 24000.0
    sine = 0.5 * np.sin(2 * np.pi * 440 * t)
    return {
        "noise": (rs.uniform(-1, 1, (2, 30000)), rs.uniform(-1, 1, (2, 30000)), False),
        "demo": (np.stack([demo + 0.01 * rs.randn(n), 0.8 * demo]), np.stack([demo, demo]), False),
        "sine": (np.stack([sine + 1e-3 * rs.randn(n)]), np.stack([np.sin(2 * np.pi * 440 * t + 0.3)]), True),
        "silent_target": (np.stack([0.1 * rs.randn(n)]), np.zeros((1, n)), True),
        "quiet": (np.stack([1e-3 * demo]), np.stack([1e-3 * (demo + 0.01 * rs.randn(n))]), True),
    }


def test_magnitudes_against_the_oracle():
    rs = np.random.RandomState(5)
    worst = 0.0
    for nf, hop, wl in ref.RESOLUTIONS + ((1024, 77, 1024), (2048, 333, 601), (512, 1, 7)):
        lengths = {nf // 2 + 1, nf // 2 + 2, max(nf // 2 + 1, 3 * hop + 1), 5003, 24119}   # + non-multiples of hop
        for n in sorted(lengths) + ([240000] if hop >= 50 else []):
            x = (rs.uniform(-1, 1, (2, n)) * np.sin(np.arange(n) / 300.0)).astype(np.float32)
            got = stft(_t(x), nf, hop, wl, "hann_window").cpu().numpy()
            want = ref.stft_magnitude(x.astype(np.float64), nf, hop, wl)
            assert got.shape == want.shape == (2, 1 + n // hop, nf // 2 + 1), (nf, hop, n, got.shape)
            err = float((np.abs(got - want) / want.max(axis=2, keepdims=True)).max())
            worst = max(worst, err)
            assert err <= MAG_RTOL, (nf, hop, wl, n, err)
    print(f"magnitudes: worst error relative to the frame's peak {worst:.2e}")


def test_stft_takes_a_window_tensor_and_other_windows():
    x = np.random.RandomState(6).randn(1, 7000).astype(np.float32)
    w = torch.hamming_window(600)
    got = stft(_t(x), 1024, 120, 600, w.to(_dev())).cpu().numpy()
    want = ref.stft_magnitude(x.astype(np.float64), 1024, 120, 600, window=w.double().numpy())
    assert float(np.abs(got - want).max() / want.max()) <= MAG_RTOL
    got2 = stft(_t(x), 1024, 120, 600, "hamming_window").cpu().numpy()
    assert float(np.abs(got2 - want).max() / want.max()) <= MAG_RTOL


def test_losses_against_the_oracle(golden_dir):
    mr = MultiResolutionSTFTLoss().to(_dev())
    report = []
    for name, (x, y, clamp) in _pairs(golden_dir).items():
        x32, y32 = x.astype(np.float32), y.astype(np.float32)
        x64, y64 = x32.astype(np.float64), y32.astype(np.float64)
        with torch.no_grad():
            sc, mag = (float(v) for v in mr(_t(x32), _t(y32)))
            per = mr.per_utterance(_t(x32), _t(y32)).cpu().numpy()
        want_sc, want_mag = ref.multi_resolution_stft_loss(x64, y64)
        want_per = ref.per_utterance(x64, y64)
        atol = MAG_ATOL_CLAMP if clamp else MAG_ATOL
        e_sc = max(abs(sc - want_sc) / want_sc, float(np.max(np.abs(per[:, 0] - want_per[:, 0]) / want_per[:, 0])))
        e_mag = max(abs(mag - want_mag), float(np.max(np.abs(per[:, 1] - want_per[:, 1]))))
        report.append(f"{name}: sc rel {e_sc:.2e}, mag abs {e_mag:.2e}")
        assert e_sc <= SC_RTOL and e_mag <= atol, (name, sc, want_sc, mag, want_mag, per, want_per)
        for nf, hop, wl in ref.RESOLUTIONS:
            with torch.no_grad():
                s_sc, s_mag = (float(v) for v in STFTLoss(nf, hop, wl).to(_dev())(_t(x32), _t(y32)))
            w_sc, w_mag = ref.stft_loss(x64, y64, nf, hop, wl)
            assert abs(s_sc - w_sc) <= SC_RTOL * w_sc and abs(s_mag - w_mag) <= atol, (name, nf)
    print("; ".join(report))


def test_losses_meet_the_reference_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "stft_loss.npz"))
    x, y = _t(d["x"]), _t(d["y"])
    with torch.no_grad():
        for (nf, hop, wl), want in zip(ref.RESOLUTIONS, d["stft_terms"]):
            got = np.array([float(v) for v in STFTLoss(nf, hop, wl)(x, y)])
            assert np.allclose(got, want, rtol=GOLDEN_RTOL, atol=0), (nf, got, want)
        got = np.array([float(v) for v in MultiResolutionSTFTLoss()(x, y)])
        assert np.allclose(got, d["mr_terms"], rtol=GOLDEN_RTOL, atol=0), (got, d["mr_terms"])
        single, wl_ = Loss()(x, y)
        assert wl_ is None and abs(float(single) - float(d["loss_single"])) <= GOLDEN_RTOL * float(d["loss_single"])
        multi, _ = Loss()(_t(d["est_sub"]), y, pqmf=PQMF().to(_dev()))
        assert abs(float(multi) - float(d["loss_multi"])) <= GOLDEN_RTOL * float(d["loss_multi"]), \
            (float(multi), float(d["loss_multi"]))


def test_basis_weight_term():
    x = _t(np.random.RandomState(1).randn(2, 4000))
    ew, w = torch.randn(3, 5, device=_dev()), torch.randn(3, 5, device=_dev())
    with torch.no_grad():
        _, wl = Loss()(x, x, est_weight=ew, weight=w)
    assert torch.allclose(wl, (ew - w).abs().mean())


def test_identical_signals_give_exactly_zero():
    x = _t(np.random.RandomState(2).uniform(-1, 1, (3, 20011)))
    mr = MultiResolutionSTFTLoss()
    with torch.no_grad():
        sc, mag = mr(x, x.clone())
        sums = mr.partial_sums(x, x)
    assert float(sc) == 0.0 and float(mag) == 0.0
    assert torch.all(sums[:, :, 0] == 0) and torch.all(sums[:, :, 2] == 0) and torch.all(sums[:, :, 1] > 0)


def test_batch_terms_are_the_combination_of_the_partials():
    rs = np.random.RandomState(3)
    x, y = _t(rs.randn(4, 9000)), _t(rs.randn(4, 9000))
    x[2] *= 1e-2
    mr = MultiResolutionSTFTLoss()
    with torch.no_grad():
        sc, mag = mr(x, y)
        sums = mr.partial_sums(x, y).cpu().numpy()
        per = mr.per_utterance(x, y).cpu().numpy()
    counts = np.array([(1 + 9000 // hop) * (nf // 2 + 1) for nf, hop, _ in ref.RESOLUTIONS], np.float64)
    tot = sums.sum(axis=1)
    assert np.isclose(float(sc), np.mean(np.sqrt(tot[:, 0]) / np.sqrt(tot[:, 1])), rtol=1e-6)
    assert np.isclose(float(mag), np.mean(tot[:, 2] / (4 * counts)), rtol=1e-6)
    assert np.allclose(per[:, 0], np.mean(np.sqrt(sums[:, :, 0]) / np.sqrt(sums[:, :, 1]), axis=0), rtol=1e-6)
    assert np.allclose(per[:, 1], np.mean(sums[:, :, 2] / counts[:, None], axis=0), rtol=1e-6)
    for b in range(4):                                   # a row alone gives its row's sums, bit for bit
        with torch.no_grad():
            alone = mr.partial_sums(x[b:b + 1], y[b:b + 1]).cpu().numpy()
        assert np.array_equal(alone[:, 0], sums[:, b]), b


def test_two_calls_are_bit_identical():
    rs = np.random.RandomState(4)
    x, y = _t(rs.randn(8, 50000)), _t(rs.randn(8, 50000))
    mr = MultiResolutionSTFTLoss()
    with torch.no_grad():
        a = mr.partial_sums(x, y)
        b = mr.partial_sums(x, y)
    assert torch.equal(a, b)


def test_non_default_stream_and_non_contiguous_input():
    rs = np.random.RandomState(5)
    xh, yh = rs.randn(3, 30000).astype(np.float32), rs.randn(3, 30000).astype(np.float32)
    x, y = _t(xh), _t(yh)
    mr = MultiResolutionSTFTLoss()
    with torch.no_grad():
        want, wall = stream_tools.timed(mr.partial_sums, x, y)
        torch.cuda.synchronize()
        # on a side stream that is still busy (tests/stream_tools.py): the inputs arrive behind a delay and hold NaN until
        # then, so a launch on any other stream than the caller's reads NaN
        s = stream_tools.side_stream()
        with stream_tools.delayed(s, stream_tools.delay_ms(wall)) as put:
            got = mr.partial_sums(put(xh), put(yh))
            stream_tools.assert_busy(put, "partial_sums")
        s.synchronize()
        assert torch.equal(got, want)
        xt = torch.empty((30000, 3), device=_dev()).copy_(x.t()).t()      # a transposed view
        assert not xt.is_contiguous()
        assert torch.equal(mr.partial_sums(xt, y[:, :]), want)
        xs = torch.empty((3, 60000), device=_dev())[:, ::2]
        xs.copy_(x)
        assert torch.equal(mr.partial_sums(xs, y), want)
        mag_nc = stft(xt, 1024, 120, 600, "hann_window")
        assert torch.equal(mag_nc, stft(x, 1024, 120, 600, "hann_window"))


def test_bad_input_raises():
    mr = MultiResolutionSTFTLoss()
    x = torch.zeros((2, 5000), device=_dev())
    with pytest.raises(_native.NativeError, match="n_fft"):
        tab = torch.zeros(2 * 256 + 200, device=_dev())
        _native.stft_distance(x, x, [tab], [256], [50], [200])
    with pytest.raises(_native.NativeError, match="n_fft"):
        _native.stft_magnitude(x, torch.zeros(3000, device=_dev()), 1000, 50, 200)
    short = torch.zeros((2, 1024), device=_dev())                       # 2048-point needs n >= 1025
    with pytest.raises(_native.NativeError, match="reflect"):
        mr(short, short)
    with pytest.raises(_native.NativeError, match="reflect"):
        stft(short[:, :256], 512, 50, 240, "hann_window")
    with torch.no_grad():
        mr(torch.zeros((1, 1025), device=_dev()), torch.zeros((1, 1025), device=_dev()))   # the shortest allowed
    with pytest.raises(ValueError, match="same shape"):
        mr(x, torch.zeros((2, 5001), device=_dev()))
    with pytest.raises(ValueError, match="same shape"):
        mr(x, torch.zeros((3, 5000), device=_dev()))
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        mr(x[0], x[0])
    with pytest.raises(ValueError):
        Loss()(x, torch.zeros((2, 4999), device=_dev()))
    with pytest.raises(TypeError):
        mr(x.int(), x.int())
    g = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        mr(g, x)
    with pytest.raises(RuntimeError, match="inference-only"):
        Loss()(g, x)
    with torch.no_grad():
        mr(g, x)                                                         # no grad mode: fine
    with pytest.raises(_native.NativeError):
        mr(x.cpu(), x.cpu())
    too_many = [torch.zeros(2 * 512 + 240, device=_dev())] * 9
    with pytest.raises(_native.NativeError, match="resolutions"):
        _native.stft_distance(x, x, too_many, [512] * 9, [50] * 9, [240] * 9)


def test_mode_evaluation_end_to_end(tmp_path):
    """MODE=preprocess on three wavs, a seeded HiFi-GAN light checkpoint, then MODE=evaluation through the
    launcher: every printed number equals the library call on the same data."""
    from fastvocoder_amd.bin.synthesize import Synthesizer
    rs = np.random.RandomState(23)
    paths = []
    for i in range(3):
        n = 9000 + 2411 * i
        s = (0.5 * np.sin(2 * np.pi * (180 + 60 * i) * np.arange(n) / 24000) * 32767
             + rs.uniform(-2000, 2000, n)).astype(np.int16)
        p = str(tmp_path / f"utt{i}.wav")
        scipy.io.wavfile.write(p, 24000, s)
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(p + "\n" for p in paths))
    save, ai, mi = str(tmp_path / "out"), str(tmp_path / "audio"), str(tmp_path / "mel")
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), "--data_path", str(lst),
                        "--save_path", save, "--audio_index_path", ai, "--mel_index_path", mi],
                       env=dict(env, MODE="preprocess"), cwd=cases.ROOT, capture_output=True, text=True, timeout=600)
    assert "min length of mel spectrogram" in r.stdout, r.stdout + r.stderr
    # the default split sizes trip the reference's assert after the files are written: list them ourselves
    audio_idx, mel_idx = tmp_path / "eval_audio", tmp_path / "eval_mel"
    audio_idx.write_text("".join(os.path.join(save, os.path.basename(p) + ".npy\n") for p in paths))
    mel_idx.write_text("".join(os.path.join(save, os.path.basename(p) + ".mel.npy\n") for p in paths))

    conf = os.path.join(cases.ROOT, "conf", "hifigan", "light.yaml")
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    ck = str(tmp_path / "ck.pth.tar")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=3).items()}}, ck)
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), "--checkpoint_path", ck,
                        "--audio_index_path", str(audio_idx), "--mel_index_path", str(mel_idx), "--config", conf,
                        "--model_name", "hifigan", "--num", "3"],
                       env=dict(env, MODE="evaluation"), cwd=cases.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^eval (\d+) (\S+) samples=(\d+) sc=(\S+) mag=(\S+)$", r.stdout, re.M)
    mean = re.findall(r"^eval mean utterances=3 sc=(\S+) mag=(\S+)$", r.stdout, re.M)
    assert len(lines) == 3 and len(mean) == 1, r.stdout

    synth = Synthesizer(ck, conf, "hifigan")
    mr = MultiResolutionSTFTLoss()
    rows = []
    for i, (idx, name, n, sc, mag) in enumerate(lines):
        assert int(idx) == i and name == os.path.join(save, os.path.basename(paths[i]) + ".npy")
        wav = np.load(name)
        mel = np.load(os.path.join(save, os.path.basename(paths[i]) + ".mel.npy"))
        est = synth.synthesize(mel.T)[0]
        m = min(est.shape[0], wav.shape[0])
        assert int(n) == m and m == wav.shape[0]          # HiFi-GAN gives 240 T >= len(wav) samples
        with torch.no_grad():
            want = mr.per_utterance(est[None, :m], _t(wav[None, :m]))[0].tolist()
        assert (sc, mag) == (f"{want[0]:.8e}", f"{want[1]:.8e}"), (i, sc, mag, want)
        rows.append(want)
    rows = np.array(rows)
    assert mean[0] == (f"{rows[:, 0].mean():.8e}", f"{rows[:, 1].mean():.8e}")
