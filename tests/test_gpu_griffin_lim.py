"""GPU tests of the Griffin-Lim path (csrc/griffin_lim.hip, fastvocoder_amd.audio.inv_mel_spectrogram and its parts)
against tests/griffin_lim_reference.py, the float64 numpy oracle (cross-checked on the CPU in
tests/test_griffin_lim_host.py).

Tolerances.  Griffin-Lim divides by the magnitude in its phase step, so a float32 and a float64 run drift apart over
the iterations; no tolerance here is guessed.  Every bound is computed by this module, on the test's own input, as

    MARGIN x max |oracle cast to float32 - float64 oracle| / peak of the float64 output,

the float32 cast being the SAME numpy arithmetic with every array and transform (pocketfft) in single precision, and
MARGIN = 4 for the GPU's different summation order (radix-4 Stockham against pocketfft, the overlap-add's frame order,
fused multiply-adds).  The float32-cast errors measured on the CPU are recorded beside each test (``cast:``), the
bound is 4 times that figure; each test prints cast error, bound and the GPU's error before it asserts.
The layers (primitives, one projection, short runs, full runs, round trip, structure, flows) are ordered so that a
failure says where."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from fastvocoder_amd import _native, audio, hparams
from tests import cases
from tests import griffin_lim_reference as gr
from tests import mel_reference as mr
from tests import stream_tools

pytestmark = pytest.mark.gpu

MARGIN = 4.0
F32 = np.float32
DRAWS = 5                      # rand01 draws of the oracle's seed-to-seed spread


def _peak_err(a, ref):
    wide = np.complex128 if np.iscomplexobj(ref) else np.float64
    ref = np.asarray(ref, dtype=wide)
    return float(np.abs(np.asarray(a, dtype=wide) - ref).max() / np.abs(ref).max())


def _check(name, got, ref, cast):
    """got (GPU) against ref (float64 oracle) within MARGIN x the float32-cast oracle's error."""
    cast_err, err = _peak_err(cast, ref), _peak_err(got, ref)
    print(f"{name}: cast {cast_err:.3e} bound {MARGIN * cast_err:.3e} gpu {err:.3e}")
    assert np.all(np.isfinite(got))
    assert err <= MARGIN * cast_err, (name, err, MARGIN * cast_err)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


@functools.lru_cache(None)
def _demo_mel():
    return np.load(os.path.join(cases.ROOT, "tests", "golden", "mel_demo.npz"))["mel"].astype(np.float64)   # [80, 585]


@functools.lru_cache(None)
def _synthetic_mel():
    """Seeded, smooth in time and frequency, spanning [0, 1] (clipped at both ends): [80, 96]."""
    rs = np.random.RandomState(11)
    g = rs.randn(80 + 8, 96 + 8)
    k = np.ones((9, 9)) / 81.0
    sm = np.array([[np.sum(g[i:i + 9, j:j + 9] * k) for j in range(96)] for i in range(80)])
    return np.clip(0.5 + 2.5 * sm, 0, 1)


def _mel(name):
    return {"demo": _demo_mel(), "excerpt": _demo_mel()[:, :200], "synthetic": _synthetic_mel(),
            "zero": np.zeros((80, 40))}[name]


def _rand01(name, draw=0):
    T = _mel(name).shape[1]
    return np.random.RandomState(1000 + draw).rand(gr.N_FREQ, T)


@functools.lru_cache(None)
def _S(name):
    """The oracle's S on the fp32 mel the GPU sees (the input cast is not the code under test)."""
    return gr.mel_to_linear(_mel(name).astype(F32).astype(np.float64))


@functools.lru_cache(None)
def _oracle_run(name, draw=0, iters=gr.ITERS, dtype=np.float64):
    """(final iterate, {count: iterate}) of the oracle's Griffin-Lim on S(name); the float32 run starts from the float64
    S rounded once, as the GPU's does."""
    return gr.griffin_lim(_S(name).astype(dtype), _rand01(name, draw), iters, dtype, keep=(0, 1, 2, 5, 6, 59, 60))


# ---------------------------------------------------------------------------
# 1. primitives
# ---------------------------------------------------------------------------

def _signal(n, seed):
    return (0.1 * np.random.RandomState(seed).randn(n)).astype(F32)


# cast: 1.16e-7 / 1.38e-7 / 1.59e-7 (n = 1025, 7277, 48000); bounds 4.6e-7 / 5.5e-7 / 6.3e-7
@pytest.mark.parametrize("n", [1025, 240 * 30 + 77, 48000])
def test_stft_against_the_oracle(n):
    y = _signal(n, n)
    got = audio._stft(y)
    assert got.dtype == np.complex64 and got.shape == (gr.N_FREQ, 1 + n // gr.HOP)
    _check(f"stft n={n}", got, gr.stft(y.astype(np.float64)), gr.stft(y, F32))


# cast: 1.67e-7 / 1.94e-7 / 1.73e-7 (seeded complex spectra, T = 2, 7, 64); bounds 6.7e-7 / 7.8e-7 / 6.9e-7
@pytest.mark.parametrize("T", [2, 7, 64])
def test_istft_of_seeded_spectra(T):
    rs = np.random.RandomState(T)
    D = (rs.randn(gr.N_FREQ, T) + 1j * rs.randn(gr.N_FREQ, T)).astype(np.complex64)
    got = audio._istft(D)
    assert got.dtype == np.float32 and got.shape == (gr.HOP * (T - 1),)
    _check(f"istft T={T}", got, gr.istft(D.astype(np.complex128)), gr.istft(D, F32))


def test_istft_of_a_signals_stft_returns_the_signal():
    y = _signal(240 * 50, 3)
    D = gr.stft(y.astype(np.float64)).astype(np.complex64)
    got = audio._istft(D)
    _check("istft(stft(y))", got, gr.istft(D.astype(np.complex128)), gr.istft(D, F32))
    assert _peak_err(got, y[:len(got)]) <= 2e-6           # and so the signal itself, to fp32


# cast, relative above the floor: demo 8.4e-2 (smallest value above the floor 5e-12), synthetic 6.6e-3, zero 5.1e-7;
# absolute at the floor: 3.6e-24 each (the rounding of 1e-15 to fp32; demo 14035 values, synthetic 16396, zero 200)
@pytest.mark.parametrize("name", ["demo", "synthetic", "zero"])
def test_mel_to_linear_against_the_oracle(name):
    """S spans many decades: relative error where the oracle's value is above the floor (1e-10 ** 1.5), absolute at
    the floor.  (The pseudo-inverse's rows have mixed signs: values a little above the floor are the difference of
    terms 1e6 times larger, in the float32 cast and on the GPU alike.)"""
    mel = _mel(name).astype(F32)
    ref = gr.mel_to_linear(mel.astype(np.float64))
    cast = gr.mel_to_linear(mel, F32)
    got = audio._mel_to_linear_device(_dev(mel[None]), hparams.power)[0].cpu().numpy().T
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and got.min() > 0
    floor = gr.FLOOR ** gr.POWER
    above = ref > floor

    def errs(a):
        a = a.astype(np.float64)
        rel = float(np.abs(a[above] / ref[above] - 1).max()) if above.any() else 0.0
        ab = float(np.abs(a[~above] - floor).max()) if (~above).any() else 0.0
        return rel, ab
    (crel, cabs), (grel, gabs) = errs(cast), errs(got)
    print(f"S {name}: relative cast {crel:.3e} gpu {grel:.3e}; at the floor ({(~above).sum()} values) cast {cabs:.3e} "
          f"gpu {gabs:.3e}")
    assert grel <= MARGIN * crel and gabs <= MARGIN * cabs


def _preemph_inputs():
    rs = np.random.RandomState(21)
    return {"noise": rs.randn(5000).astype(F32), "step": np.ones(3000, F32), "silence": np.zeros(2000, F32),
            "long": (0.3 * rs.randn(240000)).astype(F32), "short": rs.randn(5).astype(F32)}


# cast: noise 9.5e-7, step 1.20e-6, long 7.1e-7, short 1.4e-7 (bounds 3.8e-6, 4.8e-6, 2.8e-6, 5.7e-7); silence: exact zeros
@pytest.mark.parametrize("name", ["noise", "step", "silence", "long", "short"])
def test_inv_preemphasis_against_the_oracle(name):
    x = _preemph_inputs()[name]
    got = audio.inv_preemphasis(x)
    ref = gr.inv_preemphasis(x.astype(np.float64))
    assert got.dtype == np.float32 and got.shape == x.shape
    if name == "silence":
        assert not got.any()
        return
    _check(f"inv_preemphasis {name}", got, ref, gr.inv_preemphasis(x, F32))


# ---------------------------------------------------------------------------
# 2. one projection from a given iterate
# ---------------------------------------------------------------------------

# cast: 1.27e-7 (k = 0) / 1.68e-7 (k = 5) / 1.37e-7 (k = 59) on the 200-frame excerpt; bounds 5.1e-7 / 6.7e-7 / 5.5e-7
@pytest.mark.parametrize("k", [0, 5, 59])
def test_one_projection_from_the_oracles_iterate(k):
    """From the oracle's iterate after k iterations (uploaded as fp32), one GPU projection against one oracle
    projection: the fused kernel's every stage with no accumulated drift.  Ill-conditioned bins (small magnitudes, whose
    phase is noise in both implementations) carry almost no energy of the output waveform, which is what is compared."""
    S = _S("excerpt")
    y = _oracle_run("excerpt")[1][k].astype(F32)
    ref = gr.project(S, y.astype(np.float64))
    cast = gr.project(S.astype(F32), y, F32)
    got = _native.griffin_lim(_dev(S.T[None]), None, audio.griffin_lim_tables("cuda"), 1, y=_dev(y[None]))[0]
    _check(f"projection k={k}", got.cpu().numpy(), ref, cast)


# ---------------------------------------------------------------------------
# 3. short runs
# ---------------------------------------------------------------------------

# cast: 2.48e-7 / 2.18e-7 / 2.63e-7 (0, 1, 2 iterations, 200-frame excerpt); bounds 9.9e-7 / 8.7e-7 / 1.05e-6
# (after 60 iterations the same cast is at 2.4e-5: the drift the full runs below carry)
@pytest.mark.parametrize("iters", [0, 1, 2])
def test_short_runs_against_the_oracle(iters):
    S = _S("excerpt")
    got = audio._griffin_lim(S, angles=_rand01("excerpt"), iters=iters)
    assert got.dtype == np.float32 and got.shape == (gr.HOP * (S.shape[1] - 1),)
    _check(f"griffin_lim iters={iters}", got, _oracle_run("excerpt")[1][iters],
           _oracle_run("excerpt", dtype=F32)[1][iters])


# ---------------------------------------------------------------------------
# 4. full runs
# ---------------------------------------------------------------------------

@functools.lru_cache(None)
def _full(name, draw=0, dtype=np.float64):
    """The oracle's inv_mel_spectrogram(name) with its Griffin-Lim output and S, on the fp32 mel."""
    mel = _mel(name).astype(F32).astype(dtype)
    S = gr.mel_to_linear(mel, dtype)
    y, kept = gr.griffin_lim(S, _rand01(name, draw), gr.ITERS, dtype, keep=(5, 60))
    return gr.inv_preemphasis(y, dtype), y, kept[5], S


@functools.lru_cache(None)
def _oracle_spread(name):
    """Spectral-convergence error after 60 iterations of the float64 oracle over DRAWS rand01 draws."""
    return [gr.spectral_convergence(_full(name, d)[1], _full(name, d)[3]) for d in range(DRAWS)]


# cast (waveform after 60 iterations and the inverse preemphasis): demo 3.9e-6, synthetic 8.9e-6, zero 7.6e-6;
# bounds 1.5e-5 / 3.6e-5 / 3.0e-5
# oracle's spectral convergence over 5 draws at 60 iterations (after 5 iterations, draw 0): demo 0.18602-0.19064 (0.2640),
# synthetic 0.35509-0.36117 (0.4153), zero 0.24908-0.25064 (0.2912); bound on |gpu - oracle| for the same draw = a tenth of
# the spread: demo 4.6e-4, synthetic 6.1e-4, zero 1.6e-4
@pytest.mark.parametrize("name", ["demo", "synthetic", "zero"])
def test_full_run_waveform_and_quality(name):
    mel = _mel(name).astype(F32)
    ref, ref_gl, _, S = _full(name)
    cast = _full(name, dtype=F32)[0]
    r = _rand01(name)
    got = audio.inv_mel_spectrogram(mel, angles=r)
    assert got.dtype == np.float32 and got.shape == ref.shape
    # (b) quality first (it does not depend on the drift), evaluated by the float64 oracle on the Griffin-Lim outputs
    Sg = _dev(S.T[None])
    g60 = audio._griffin_lim(Sg, angles=r, iters=gr.ITERS)[0].cpu().numpy()
    g5 = audio._griffin_lim(Sg, angles=r, iters=5)[0].cpu().numpy()
    spread = _oracle_spread(name)
    e_ref, e60, e5 = spread[0], gr.spectral_convergence(g60, S), gr.spectral_convergence(g5, S)
    bound = (max(spread) - min(spread)) / 10
    print(f"quality {name}: oracle {e_ref:.6f} (draws {min(spread):.6f}-{max(spread):.6f}, bound {bound:.2e}) "
          f"gpu 60 it {e60:.6f}, 5 it {e5:.6f}")
    assert abs(e60 - e_ref) <= bound and e60 < e5
    # (a) waveform
    _check(f"inv_mel_spectrogram {name}", got, ref, cast)


# ---------------------------------------------------------------------------
# 5. round trip
# ---------------------------------------------------------------------------

# oracle chain, demo mel (585 frames), 5 draws: MAE 0.05546-0.05558, correlation 0.94958-0.94971: the bounds on the
# distance to the oracle's figures of the same draw are 1.2e-4 and 1.3e-4
def test_round_trip_through_melspectrogram():
    """melspectrogram(inv_mel_spectrogram(mel)) against mel, up to a constant offset: Griffin-Lim from an 80-band mel is
    a lossy inverse, so the figures are the oracle chain's (float64 throughout), and the GPU chain must reach them, for
    the same draw, within the oracle's own seed-to-seed spread."""
    mel = _mel("demo")
    figs = [mr.offset_free_agreement(mr.melspectrogram(_full("demo", d)[0]), mel) for d in range(DRAWS)]
    maes, corrs = zip(*figs)
    wav = audio.inv_mel_spectrogram(_dev(mel), angles=_rand01("demo"))
    back = audio.melspectrogram(wav)[0].cpu().numpy().astype(np.float64)
    assert back.shape == (80, mel.shape[1])                  # 1 + 240 (T - 1) // 240 frames
    mae, corr = mr.offset_free_agreement(back, mel)
    print(f"round trip: oracle MAE {min(maes):.4f}-{max(maes):.4f} corr {min(corrs):.4f}-{max(corrs):.4f}; "
          f"gpu MAE {mae:.4f} corr {corr:.4f} (oracle, same draw: {maes[0]:.4f} / {corrs[0]:.4f})")
    assert abs(mae - maes[0]) <= max(maes) - min(maes)
    assert abs(corr - corrs[0]) <= max(corrs) - min(corrs)


# ---------------------------------------------------------------------------
# 6. structure
# ---------------------------------------------------------------------------

def test_batched_rows_equal_single_calls_bit_for_bit():
    rs = np.random.RandomState(31)
    mels = rs.rand(3, 80, 37).astype(F32)
    r = rs.rand(3, gr.N_FREQ, 37)
    batch = audio.inv_mel_spectrogram(_dev(mels), angles=r, iters=8)
    assert batch.shape == (3, gr.HOP * 36) and batch.is_cuda
    for b in range(3):
        single = audio.inv_mel_spectrogram(_dev(mels[b]), angles=r[b], iters=8)
        assert single.shape == (gr.HOP * 36,)
        assert torch.equal(batch[b], single)


def test_repeated_calls_and_streams_give_identical_bits():
    mel, r = _dev(_mel("synthetic")), _rand01("synthetic")
    a = audio.inv_mel_spectrogram(mel, angles=r, iters=10)
    b, wall = stream_tools.timed(lambda: audio.inv_mel_spectrogram(mel, angles=r, iters=10))
    torch.cuda.synchronize()
    # On a side stream that is still busy (tests/stream_tools.py): the inputs arrive behind a delay and hold NaN until then,
    # so a launch on any other stream than the caller's reads NaN.  audio.inv_mel_spectrogram itself uploads the initial
    # phase from pageable memory (audio._initial_phase: .to(device)), which waits for the stream: its three launches are
    # made here as it makes them, on a staged phase.
    n_fft, hop, win = audio._stft_parameters()
    phase = audio._initial_phase(r, None, 1, mel.shape[1], "cpu")
    side = stream_tools.side_stream()
    with stream_tools.delayed(side, stream_tools.delay_ms(wall)) as put:
        S = audio._mel_to_linear_device(put(_mel("synthetic"))[None], audio.hparams.power)
        y = _native.griffin_lim(S, put(phase), audio.griffin_lim_tables(S.device), 10, None, n_fft, hop, win)
        c = _native.inv_preemphasis(y, audio.hparams.preemphasis)[0]
        stream_tools.assert_busy(put, "inv_mel_spectrogram's launches")
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_seed_repeats_and_differs_between_seeds():
    mel = _mel("synthetic")
    a, b, c = (audio.inv_mel_spectrogram(mel, seed=s, iters=3) for s in (5, 5, 6))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # seed=s is the draw the reference makes after np.random.seed(s)
    np.random.seed(5)
    assert np.array_equal(a, audio.inv_mel_spectrogram(mel, angles=np.random.rand(gr.N_FREQ, mel.shape[1]), iters=3))
    np.random.seed(5)
    assert np.array_equal(a, audio.inv_mel_spectrogram(mel, iters=3))      # seed=None: the global NumPy state


def test_numpy_in_numpy_out_tensor_in_tensor_out():
    mel, r = _mel("synthetic"), _rand01("synthetic")
    a = audio.inv_mel_spectrogram(mel, angles=r, iters=2)
    t = audio.inv_mel_spectrogram(_dev(mel), angles=r, iters=2)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 1
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), a)
    assert hparams.griffin_lim_iters == 60 and hparams.power == 1.5


def test_values_outside_the_unit_interval_are_clipped():
    mel, r = _mel("synthetic"), _rand01("synthetic")
    wide = mel * 3 - 1
    a = audio.inv_mel_spectrogram(wide, angles=r, iters=2)
    assert np.all(np.isfinite(a)) and np.array_equal(a, audio.inv_mel_spectrogram(np.clip(wide, 0, 1), angles=r, iters=2))


def test_bad_input_raises():
    ok = np.random.RandomState(41).rand(80, 6)
    assert audio.inv_mel_spectrogram(ok, seed=0, iters=1).shape == (1200,)
    with pytest.raises(ValueError):
        audio.inv_mel_spectrogram(ok[:, :5], seed=0)         # 240 * 4 < 1025 samples: cannot be reflect-padded
    with pytest.raises(ValueError):
        audio.inv_mel_spectrogram(np.zeros((79, 20)), seed=0)
    with pytest.raises(ValueError):
        audio.inv_mel_spectrogram(ok, angles=np.zeros((gr.N_FREQ, 7)))
    with pytest.raises(_native.NativeError):
        audio.inv_mel_spectrogram(torch.zeros(80, 20))       # a host tensor
    with pytest.raises(_native.NativeError):
        audio.inv_mel_spectrogram(torch.zeros(80, 20, dtype=torch.float64, device="cuda"))
    tab, S = audio.griffin_lim_tables("cuda"), torch.ones(1, 5, gr.N_FREQ, device="cuda")
    ph = torch.ones(1, 5, gr.N_FREQ, dtype=torch.complex64, device="cuda")
    with pytest.raises(_native.NativeError, match="T=5"):
        _native.griffin_lim(S, ph, tab, 1)
    with pytest.raises(_native.NativeError, match="n_fft=1024"):
        _native.istft(torch.ones(1, 8, 513, dtype=torch.complex64, device="cuda"), tab, n_fft=1024, hop=240,
                      win_length=1024)
    with pytest.raises(_native.NativeError):
        _native.stft_complex(torch.zeros(1, 1024, device="cuda"), tab)     # shorter than the reflect padding needs


# ---------------------------------------------------------------------------
# 7. flows
# ---------------------------------------------------------------------------

def _launcher(mode, *args):
    return subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), *args],
                          env=dict(os.environ, MODE=mode), cwd=cases.ROOT, capture_output=True, text=True, timeout=600)


def _checkpoint(tmp_path):
    from fastvocoder_amd.synthetic import seeded_state_dict
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    sd = seeded_state_dict("hifigan", cfg, seed=0)
    ck = str(tmp_path / "hifigan.pth.tar")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    return ck, os.path.join(cases.ROOT, "conf/hifigan/light.yaml")


def test_mode_synthesize_writes_the_griffin_lim_wav(tmp_path):
    ck, conf = _checkpoint(tmp_path)
    T = 120
    np.save(tmp_path / "in.npy", _demo_mel()[:, :T])
    outs = []
    for run in range(2):
        wav = str(tmp_path / f"run{run}" / "out.wav")
        os.makedirs(os.path.dirname(wav))
        r = _launcher("synthesize", "--checkpoint_path", ck, "--mel_path", str(tmp_path / "in.npy"), "--wav_path", wav,
                      "--model_name", "hifigan", "--config", conf, "--gl_seed", "7")
        assert r.returncode == 0, r.stdout + r.stderr
        assert "skipped" not in r.stdout
        assert sorted(os.listdir(os.path.dirname(wav))) == ["out.bias.wav", "out.gl.wav", "out.remove.wav", "out.wav"]
        with open(wav[:-3] + "gl.wav", "rb") as f:
            outs.append(f.read())
        sr, data = scipy.io.wavfile.read(wav[:-3] + "gl.wav")
        assert sr == 24000 and data.dtype == np.int16 and data.shape == (gr.HOP * (T - 1),)
        assert abs(int(np.abs(data.astype(np.int32)).max()) - 32767 * hparams.rescale_out) <= 1
    assert outs[0] == outs[1]
    # the file is the library call on the same mel and seed
    y = audio.inv_mel_spectrogram(_demo_mel()[:, :T].astype(F32), seed=7)
    y *= 32767 / max(0.01, np.max(np.abs(y))) * hparams.rescale_out
    assert np.abs(data.astype(np.int32) - y.astype(np.int16)).max() <= 1


def test_mode_evaluation_with_griffin_lim(tmp_path):
    import re
    ck, conf = _checkpoint(tmp_path)
    rs = np.random.RandomState(29)
    audio_idx, mel_idx = tmp_path / "eval_audio", tmp_path / "eval_mel"
    names = []
    for i in range(2):
        n = 9000 + 2400 * i
        wav = (0.4 * np.sin(2 * np.pi * (180 + 60 * i) * np.arange(n) / 24000) + 0.02 * rs.randn(n)).astype(F32)
        mel = audio.melspectrogram(wav)
        np.save(tmp_path / f"u{i}.npy", wav)
        np.save(tmp_path / f"u{i}.mel.npy", mel)
        names.append(str(tmp_path / f"u{i}"))
    audio_idx.write_text("".join(n + ".npy\n" for n in names))
    mel_idx.write_text("".join(n + ".mel.npy\n" for n in names))
    args = ["--checkpoint_path", ck, "--audio_index_path", str(audio_idx), "--mel_index_path", str(mel_idx),
            "--config", conf, "--model_name", "hifigan", "--num", "2"]
    r = _launcher("evaluation", "--griffin_lim", *args)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^eval-gl (\d+) samples=(\d+) sc=(\S+) mag=(\S+)$", r.stdout, re.M)
    mean = re.findall(r"^eval-gl mean utterances=2 sc=(\S+) mag=(\S+)$", r.stdout, re.M)
    assert [ln[0] for ln in lines] == ["0", "1"] and len(mean) == 1, r.stdout
    assert all(np.isfinite(float(v)) and float(v) > 0 for ln in lines for v in ln[2:])
    assert abs(float(mean[0][0]) - np.mean([float(ln[2]) for ln in lines])) <= 1e-7
    # Griffin-Lim of the utterance's own mel is a better estimate than a generator with seeded random weights
    ev = re.findall(r"^eval (\d+) \S+ samples=\d+ sc=(\S+) mag=(\S+)$", r.stdout, re.M)
    assert len(ev) == 2 and all(float(g[2]) < float(e[1]) for g, e in zip(lines, ev))
    again = _launcher("evaluation", "--griffin_lim", *args)
    assert again.stdout == r.stdout                           # seeded: repeatable
    plain = _launcher("evaluation", *args)
    assert plain.returncode == 0 and "eval-gl" not in plain.stdout, plain.stdout + plain.stderr
    assert [ln for ln in r.stdout.splitlines() if not ln.startswith("eval-gl")] == plain.stdout.splitlines()
