"""Float64 numpy restatement of the reference's ``inv_mel_spectrogram`` (data/audio.py:66-95,179-190 with
hparams.py as shipped, librosa < 0.10 semantics): the test oracle of fastvocoder_amd.audio.inv_mel_spectrogram.
Deliberately independent of fastvocoder_amd (no import of it); the window and the mel filters are
tests/mel_reference.py's, which is pinned to the reference's own mel.

Every function takes ``dtype``: float64 is the oracle; float32 runs the SAME arithmetic with every array and
every transform (scipy's pocketfft keeps float32 / complex64) in single precision -- the "oracle cast to
float32" the GPU tests take their tolerances from (tests/test_gpu_griffin_lim.py)."""
import numpy as np
import scipy.fft
import scipy.signal

from . import mel_reference as mr
from . import stft_reference as sr

N_FFT, HOP, WIN = mr.N_FFT, mr.HOP, mr.WIN
N_FREQ = 1 + N_FFT // 2
POWER, ITERS = 1.5, 60
FLOOR = 1e-10                      # _mel_to_linear's np.maximum(1e-10, .)


def _cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def preemphasis(y):
    return scipy.signal.lfilter([1, -mr.PREEMPHASIS], [1], np.asarray(y, dtype=np.float64))


def inv_preemphasis(y, dtype=np.float64):
    """lfilter([1], [1, -0.97], y): o[n] = y[n] + 0.97 o[n-1]."""
    y = np.asarray(y, dtype=dtype)
    return scipy.signal.lfilter(np.array([1], dtype=dtype), np.array([1, -mr.PREEMPHASIS], dtype=dtype), y).astype(dtype)


def stft(y, dtype=np.float64):
    """librosa.stft(y, 2048, 240, 1200): centred, 'reflect' padding by 1024, periodic Hann of 1200 taps centred
    in 2048.  Complex [1025, 1 + len(y) // 240]."""
    return sr.stft(y, N_FFT, HOP, WIN, dtype=dtype).T.astype(_cdtype(dtype))


def window_sumsquare(T, dtype=np.float64):
    w2 = mr.hann_window().astype(dtype) ** 2
    wss = np.zeros(N_FFT + HOP * (T - 1), dtype=dtype)
    for t in range(T):
        wss[t * HOP:t * HOP + N_FFT] += w2
    return wss


def istft(D, dtype=np.float64):
    """librosa.istft(D, hop_length=240, win_length=1200): irfft of each frame, times the padded window,
    overlap-added at hop 240, divided by the overlap-added squared window where that exceeds tiny(float32),
    1024 samples trimmed from each end: 240 (T - 1) samples."""
    D = np.asarray(D, dtype=_cdtype(dtype))
    T = D.shape[1]
    frames = scipy.fft.irfft(D.T, n=N_FFT, axis=1).astype(dtype) * mr.hann_window().astype(dtype)[None, :]
    y = np.zeros(N_FFT + HOP * (T - 1), dtype=dtype)
    for t in range(T):
        y[t * HOP:t * HOP + N_FFT] += frames[t]
    wss = window_sumsquare(T, dtype)
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[N_FFT // 2:len(y) - N_FFT // 2]


def denormalize(mel, dtype=np.float64):
    return np.clip(np.asarray(mel, dtype=dtype), 0, 1) * dtype(-mr.MIN_LEVEL_DB) + dtype(mr.MIN_LEVEL_DB)


_inv_basis = None


def inv_mel_basis():
    global _inv_basis
    if _inv_basis is None:
        _inv_basis = np.linalg.pinv(mr.mel_basis())
    return _inv_basis


def mel_to_linear(mel, dtype=np.float64):
    """Normalised mel [80, T] -> S = max(1e-10, pinv(mel_basis) @ db_to_amp(denormalize(mel) + 20)) ** 1.5."""
    D = denormalize(mel, dtype)
    A = np.power(dtype(10.0), (D + dtype(mr.REF_LEVEL_DB)) * dtype(0.05)).astype(dtype)
    lin = np.maximum(dtype(FLOOR), inv_mel_basis().astype(dtype) @ A)
    return (lin ** dtype(POWER)).astype(dtype)


def initial_phase(rand01, dtype=np.float64):
    """exp(2j pi rand01), float64 arithmetic, rounded once for the float32 chain."""
    return np.exp(2j * np.pi * np.asarray(rand01, dtype=np.float64)).astype(_cdtype(dtype))


def project(S, y, dtype=np.float64):
    """One Griffin-Lim iteration: istft(S * exp(1j * angle(stft(y)))); angle(0) = 0."""
    X = stft(y, dtype)
    ph = np.exp(1j * np.angle(X)).astype(_cdtype(dtype))
    return istft(np.asarray(S, dtype=dtype) * ph, dtype)


def griffin_lim(S, rand01, iters=ITERS, dtype=np.float64, keep=()):
    """y0 = istft(S * exp(2j pi rand01)); ``iters`` projections.  ``keep``: iteration counts whose iterate is
    returned too (a dict count -> waveform) as the second result."""
    S = np.asarray(S, dtype=dtype)
    y = istft(S * initial_phase(rand01, dtype), dtype)
    kept = {0: y.copy()} if 0 in keep else {}
    for i in range(iters):
        y = project(S, y, dtype)
        if i + 1 in keep:
            kept[i + 1] = y.copy()
    return (y, kept) if keep else y


def inv_mel_spectrogram(mel, rand01, iters=ITERS, dtype=np.float64):
    return inv_preemphasis(griffin_lim(mel_to_linear(mel, dtype), rand01, iters, dtype), dtype)


def spectral_convergence(y, S):
    """||abs(stft(y)) - S||_F / ||S||_F in float64."""
    S = np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(np.abs(stft(np.asarray(y, dtype=np.float64))) - S) / np.linalg.norm(S))
