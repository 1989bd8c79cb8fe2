"""The numpy STFT the reference restatements share (mel_reference, stft_loss_reference, griffin_lim_reference):
centred frames with 'reflect' padding by n_fft / 2, a win_length window centred in n_fft (periodic Hann by default),
1 + n // hop frames, bins 0..n_fft / 2 -- librosa.stft and torch.stft alike.  Deliberately independent of
fastvocoder_amd (no import of it)."""
import numpy as np
import scipy.fft


def hann(win_length):
    """Periodic Hann (torch.hann_window(win_length), scipy get_window('hann', win_length, fftbins=True)):
    0.5 - 0.5 cos(2 pi i / win_length); one tap is [1] in torch."""
    if win_length == 1:
        return np.ones(1)
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)


def padded_window(n_fft, win_length, window=None):
    """The win_length window centred in n_fft with zeros around it (left offset (n_fft - win_length) // 2)."""
    w = hann(win_length) if window is None else np.asarray(window, dtype=np.float64)
    out = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    out[lpad:lpad + win_length] = w
    return out


def reflect_pad(x, p):
    """numpy 'reflect' (no edge repeat) by p on both sides of the last axis; needs p < x.shape[-1]."""
    n = x.shape[-1]
    assert p < n, (p, n)
    idx = np.concatenate([np.arange(p, 0, -1), np.arange(n), n - 2 - np.arange(p)])
    return x[..., idx]


def stft(x, n_fft, hop, win_length, window=None, dtype=np.float64):
    """Complex (..., 1 + n // hop, n_fft // 2 + 1) spectrum of x (..., n).  float32 runs the same arithmetic in single
    precision (scipy's pocketfft keeps float32 / complex64)."""
    x = np.asarray(x, dtype=dtype)
    padded = reflect_pad(x, n_fft // 2)
    T = 1 + x.shape[-1] // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return scipy.fft.rfft(padded[..., idx] * padded_window(n_fft, win_length, window).astype(dtype), axis=-1)
