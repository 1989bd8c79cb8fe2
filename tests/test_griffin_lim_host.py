"""CPU cross-checks of tests/griffin_lim_reference.py, the float64 oracle of the GPU Griffin-Lim, against things that
are not itself: the transform pair's own inverse property, scipy.signal's STFT / ISTFT, tests/mel_reference.py's
magnitude (pinned to the reference's own mel) and the filter pair's inverse property."""
import os
import warnings

import numpy as np
import pytest
import scipy.signal

from tests import griffin_lim_reference as gr
from tests import mel_reference as mr


def _noise(n, seed):
    return np.random.RandomState(seed).randn(n)


@pytest.mark.parametrize("n", [1200, 2400, 4801, 7200 + 239, 24000 + 7])
def test_istft_inverts_stft_on_the_samples_it_covers(n):
    y = _noise(n, n)
    D = gr.stft(y)
    assert D.shape == (gr.N_FREQ, 1 + n // gr.HOP)
    back = gr.istft(D)
    assert back.shape == (gr.HOP * (D.shape[1] - 1),)       # the tail beyond 240 (T - 1) is dropped
    assert np.abs(back - y[:len(back)]).max() <= 1e-13 * np.abs(y).max()


def test_stft_agrees_with_scipy():
    """scipy.signal.stft with the padded window, hop 240, no boundary extension and no padding of its own, on the
    signal reflect-padded by hand, is the same transform up to scipy's 1 / sum(window) scaling -- every frame, the
    edges included."""
    y = _noise(240 * 40 + 100, 1)
    w = mr.hann_window()
    padded = np.pad(y, gr.N_FFT // 2, mode="reflect")
    _, _, Z = scipy.signal.stft(padded, window=w, nperseg=gr.N_FFT, noverlap=gr.N_FFT - gr.HOP, nfft=gr.N_FFT,
                                boundary=None, padded=False, return_onesided=True)
    D = gr.stft(y)
    assert Z.shape == D.shape
    assert np.abs(Z * w.sum() - D).max() <= 1e-12 * np.abs(D).max()


def test_istft_agrees_with_scipy():
    """scipy.signal.istft (window-sum-square normalised overlap-add, like librosa's) of the scaled spectrum, trimmed
    by 1024 on each side, on a spectrum that is NOT the transform of a signal (seeded complex noise)."""
    rs = np.random.RandomState(2)
    T = 30
    D = rs.randn(gr.N_FREQ, T) + 1j * rs.randn(gr.N_FREQ, T)
    D[0].imag = 0
    D[-1].imag = 0
    w = mr.hann_window()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)     # NOLA fails in the first / last 424 samples, which are trimmed
        _, x = scipy.signal.istft(D / w.sum(), window=w, nperseg=gr.N_FFT, noverlap=gr.N_FFT - gr.HOP, nfft=gr.N_FFT,
                                  input_onesided=True, boundary=False)
    x = x[gr.N_FFT // 2:gr.N_FFT // 2 + gr.HOP * (T - 1)]
    y = gr.istft(D)
    assert y.shape == x.shape
    assert np.abs(x - y).max() <= 1e-12 * np.abs(y).max()


def test_magnitude_of_preemphasised_stft_is_the_mel_oracles():
    y = _noise(240 * 25 + 13, 3)
    mag = mr.stft_magnitude(y)
    assert np.abs(np.abs(gr.stft(gr.preemphasis(y))) - mag).max() <= 1e-13 * mag.max()


def test_inv_preemphasis_inverts_preemphasis():
    y = _noise(50000, 4)
    assert np.abs(gr.inv_preemphasis(gr.preemphasis(y)) - y).max() <= 1e-12


def test_mel_to_linear_restates_the_reference_chain():
    """pinv(basis) @ A floored and raised to 1.5; through the filters again it gives the amplitudes back where the floor
    did not act (pinv is a right inverse of the full-row-rank filter matrix)."""
    mel = np.random.RandomState(5).rand(80, 12)
    A = 10 ** ((mel * 100 - 100 + 20) * 0.05)
    lin = np.linalg.pinv(mr.mel_basis()) @ A
    S = gr.mel_to_linear(mel)
    assert np.allclose(S, np.maximum(1e-10, lin) ** 1.5, rtol=1e-12, atol=0)
    assert np.abs(mr.mel_basis() @ lin - A).max() <= 1e-10
    assert np.array_equal(gr.mel_to_linear(mel * 3 - 1), gr.mel_to_linear(np.clip(mel * 3 - 1, 0, 1)))   # clipped


def test_griffin_lim_reduces_the_spectral_convergence_error():
    mel = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mel_demo.npz"))["mel"][:, :60]
    S = gr.mel_to_linear(mel)
    r = np.random.RandomState(6).rand(*S.shape)
    y, kept = gr.griffin_lim(S, r, 10, keep=(0, 5, 10))
    e = [gr.spectral_convergence(kept[k], S) for k in (0, 5, 10)]
    assert np.array_equal(y, kept[10]) and e[0] > e[1] > e[2]
    assert len(y) == gr.HOP * (S.shape[1] - 1)
    # angle(0) = 0: silence stays silence, no NaN
    assert np.array_equal(gr.project(S, np.zeros_like(y)), gr.istft(S.astype(complex)))


def test_float32_cast_runs_in_single_precision():
    S = gr.mel_to_linear(np.random.RandomState(7).rand(80, 12), np.float32)
    r = np.random.RandomState(8).rand(*S.shape)
    assert S.dtype == np.float32
    assert gr.stft(np.zeros(4000, np.float32), np.float32).dtype == np.complex64
    assert gr.griffin_lim(S, r, 2, np.float32).dtype == np.float32
    assert gr.inv_mel_spectrogram(np.random.RandomState(7).rand(80, 12), r, 1, np.float32).dtype == np.float32
