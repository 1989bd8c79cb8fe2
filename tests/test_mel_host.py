"""CPU tests of the mel front end's host side: the float64 test oracle (tests/mel_reference.py)
against the reference's own data, the mel filter basis the kernel's table is built from, the
hparams it reads, the table layout the kernel expects and load_wav."""
import os
import re

import numpy as np
import pytest
import scipy.io.wavfile

from fastvocoder_amd import _native, audio, hparams
from tests import cases
from tests import mel_reference


def test_oracle_matches_the_reference_demo_mel(golden_dir):
    """The demo wav of the reference against the mel it was synthesised from (test.mel.npy): equal up to the
    constant dB offset of the wav's peak normalisation.  Pins the oracle's conventions (preemphasis, magnitude,
    Slaney filters, fmin 40) to reference data."""
    d = np.load(os.path.join(golden_dir, "mel_demo.npz"))
    wav, ref = d["wav"], d["mel"].astype(np.float64)
    assert wav.dtype == np.int16 and ref.shape == (80, 585) and wav.shape[0] == 585 * 240
    mel = mel_reference.melspectrogram(wav / 32768.0)
    assert mel.shape == (80, 1 + wav.shape[0] // 240)
    mae, corr = mel_reference.offset_free_agreement(mel[:, :ref.shape[1]], ref)
    assert mae <= 0.03 and corr >= 0.98, (mae, corr)


def test_mel_basis_is_librosas_slaney_basis():
    got, ref = audio._build_mel_basis(), mel_reference.mel_basis()
    assert got.shape == ref.shape == (80, 1025)
    assert float(np.abs(got - ref).max()) <= 1e-6
    assert int((got > 0).sum(axis=0).max()) <= 2                     # every bin in at most two filters
    assert int((got > 0).sum()) <= 2050


def test_hparams_carry_the_reference_values():
    want = dict(num_mels=80, num_freq=1025, frame_length_ms=50, frame_shift_ms=10, fmin=40, hop_size=240,
                sample_rate=24000, min_level_db=-100, ref_level_db=20, preemphasize=True, preemphasis=0.97,
                rescale_out=0.4, signal_normalization=True, train_size=9000, valid_size=500, eval_size=100)
    for k, v in want.items():
        assert getattr(hparams, k) == v, k
    assert audio._stft_parameters() == (2048, 240, 1200)


def test_numpy_helpers_follow_the_reference():
    x = np.random.RandomState(0).randn(500)
    p = audio.preemphasis(x)
    assert np.allclose(p[0], x[0]) and np.allclose(p[1:], x[1:] - 0.97 * x[:-1])
    assert audio._amp_to_db(np.array([0.0, 1.0]))[0] == -100.0
    assert np.array_equal(audio._normalize(np.array([-150.0, -50.0, 10.0])), [0.0, 0.5, 1.0])


def test_mel_table_layout_matches_the_header():
    header = open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")).read()
    defs = dict(re.findall(r"#define (FV_MEL_\w+) (\d+)", header))
    assert (int(defs["FV_MEL_TAB_WINDOW"]), int(defs["FV_MEL_TAB_TWIDDLE"]), int(defs["FV_MEL_TAB_SPLIT"]),
            int(defs["FV_MEL_TAB_FILTERS"]), int(defs["FV_MEL_TAB_WEIGHTS"]), int(defs["FV_MEL_MAX_WEIGHTS"])) == \
        (0, audio._MEL_TAB_TWIDDLE, audio._MEL_TAB_SPLIT, audio._MEL_TAB_FILTERS, audio._MEL_TAB_WEIGHTS,
         audio._MEL_MAX_WEIGHTS)
    tab = audio._mel_table_host().astype(np.float64)
    assert tab.dtype == np.float64 and tab.shape == (_native.mel_table_floats(),)
    assert np.allclose(tab[:1200], mel_reference.hann_window()[424:1624], atol=1e-7)
    # the filters rebuilt from (start, count, offset) + weights give the basis back
    basis = mel_reference.mel_basis()
    heads = tab[audio._MEL_TAB_FILTERS:audio._MEL_TAB_FILTERS + 240].reshape(80, 3).astype(int)
    rebuilt = np.zeros_like(basis)
    for m, (start, count, off) in enumerate(heads):
        rebuilt[m, start:start + count] = tab[audio._MEL_TAB_WEIGHTS + off:audio._MEL_TAB_WEIGHTS + off + count]
    assert float(np.abs(rebuilt - basis).max()) <= 1e-8
    tw = tab[audio._MEL_TAB_TWIDDLE:audio._MEL_TAB_TWIDDLE + 2048].reshape(1024, 2)
    assert np.allclose(tw[:, 0] + 1j * tw[:, 1], np.exp(-2j * np.pi * np.arange(1024) / 1024), atol=1e-7)


def test_load_wav_int16_float_stereo(tmp_path):
    rs = np.random.RandomState(1)
    s16 = rs.randint(-32768, 32768, size=4000).astype(np.int16)
    scipy.io.wavfile.write(str(tmp_path / "a.wav"), 24000, s16)
    y = audio.load_wav(str(tmp_path / "a.wav"), encode=False)
    assert y.dtype == np.float32 and np.array_equal(y, s16.astype(np.float32) / 32768.0)

    f32 = rs.uniform(-0.5, 0.5, size=3000).astype(np.float32)
    scipy.io.wavfile.write(str(tmp_path / "b.wav"), 24000, f32)
    assert np.array_equal(audio.load_wav(str(tmp_path / "b.wav"), encode=False), f32)

    st = rs.randint(-32768, 32768, size=(2000, 2)).astype(np.int16)
    scipy.io.wavfile.write(str(tmp_path / "c.wav"), 24000, st)
    y = audio.load_wav(str(tmp_path / "c.wav"), encode=False)
    assert y.shape == (2000,)
    assert np.allclose(y, st.astype(np.float64).mean(axis=1) / 32768.0, atol=1e-6)

    enc = audio.load_wav(str(tmp_path / "b.wav"))                   # encode=True: encode_16bits, as the reference
    assert enc.dtype == np.int16 and np.abs(enc).max() == 32767


def test_load_wav_refuses_another_sample_rate(tmp_path):
    scipy.io.wavfile.write(str(tmp_path / "a.wav"), 22050, np.zeros(100, np.int16))
    with pytest.raises(ValueError, match="22050"):
        audio.load_wav(str(tmp_path / "a.wav"))
    audio.load_wav(str(tmp_path / "a.wav"), sample_rate=22050)       # the rate asked for is accepted
