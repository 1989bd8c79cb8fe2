"""Float64 numpy restatement of the reference's ``melspectrogram`` (data/audio.py:58-61 with
hparams.py:4-15, librosa < 0.10 semantics): the test oracle of fastvocoder_amd.audio.melspectrogram.
Deliberately independent of fastvocoder_amd (no import of it)."""
import numpy as np

from . import stft_reference as sr

SR, N_FFT, HOP, WIN, N_MELS, FMIN = 24000, 2048, 240, 1200, 80, 40.0
PREEMPHASIS, MIN_LEVEL_DB, REF_LEVEL_DB = 0.97, -100.0, 20.0


def hz_to_mel(f):
    """Slaney's mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, log above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_basis(sr=SR, n_fft=N_FFT, n_mels=N_MELS, fmin=FMIN, fmax=None):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin), htk=False, Slaney area normalisation: [n_mels, 1+n_fft//2]."""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def hann_window():
    """Periodic Hann of WIN taps (scipy.signal.get_window('hann', WIN, fftbins=True)), centred in N_FFT."""
    return sr.padded_window(N_FFT, WIN)


def stft_magnitude(y):
    """|librosa.stft(preemphasis(y), n_fft, hop, win, center=True, pad_mode='reflect')|: [1+N_FFT//2, 1+n//HOP]."""
    y = np.asarray(y, dtype=np.float64)
    p = np.empty_like(y)
    p[0] = y[0]
    p[1:] = y[1:] - PREEMPHASIS * y[:-1]                   # lfilter([1, -0.97], [1], y)
    return np.abs(sr.stft(p, N_FFT, HOP, WIN)).T


def melspectrogram(y):
    """[N_MELS, 1 + len(y)//HOP] float64 in [0, 1]."""
    mel = mel_basis() @ stft_magnitude(y)
    S = 20 * np.log10(np.maximum(1e-5, mel)) - REF_LEVEL_DB
    return np.clip((S - MIN_LEVEL_DB) / -MIN_LEVEL_DB, 0, 1)


def offset_free_agreement(a, b):
    """(MAE after removing the median difference, correlation): a constant shift in dB (peak normalisation of a
    wav) is a constant shift of the normalised mel, so the two are compared up to that offset."""
    d = a - b
    mae = float(np.mean(np.abs(d - np.median(d))))
    corr = float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    return mae, corr
