"""The audio side of the reference (data/audio.py): the wav sink of the synthesize flow
(encode_16bits / save_wav, data/audio.py:12-26), and the mel front end that makes a generator's
input from a wav (load_wav / melspectrogram, data/audio.py:17-21,58-61) for copy-synthesis and
MODE=preprocess.  Griffin-Lim, the linear ``spectrogram`` and the TensorFlow helpers of the
reference stay out of scope.

``encode_16bits`` / ``save_wav`` take what the reference's take (a float numpy array, scaled IN
PLACE) and, additionally, a float32 tensor on the ROCm device: then the peak reduction, scaling and
int16 conversion run on the GPU (csrc/wav_sink.hip, fv_encode_16bits) and only the int16 samples
are copied to the host -- half the PCIe bytes of the fp32 waveform.
Both routes give the same int16 samples bit for bit.

``melspectrogram`` computes the reference's mel (librosa < 0.10 semantics: preemphasis, reflect-
padded STFT with a periodic Hann window, magnitude, Slaney mel filters, dB, normalise) in one HIP
launch (csrc/mel.hip, fv_melspectrogram); there is no CPU arithmetic path.  The small numpy helpers
below carry the reference's names; ``_build_mel_basis`` is the float64 restatement of
``librosa.filters.mel`` the kernel's filter table is built from.
"""
import numpy as np
import scipy.io.wavfile
import scipy.signal
import torch

from . import _native
from . import hparams


def encode_16bits(x, rescale_out=1.0):
    """Peak-normalise to int16 full scale times ``rescale_out``.  Like the
    reference this scales ``x`` IN PLACE (callers see the mutation).  A device
    tensor ([n] or [B,n], normalised per row) returns a device int16 tensor."""
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise _native.NativeError("encode_16bits: a tensor argument must live on the ROCm device; "
                                      "pass a numpy array for the host route")
        return _native.encode_16bits(x, rescale_out, scale_in_place=True)[0]
    x *= 32767 / max(0.01, np.max(np.abs(x))) * rescale_out
    return x.astype(np.int16)


def load_wav(filename, sample_rate=24000, encode=True):
    """The reference's ``load_wav`` without librosa: the samples as float32 (16-bit integer wavs divided by
    32768, as librosa returns them; float wavs as stored), multi-channel averaged to mono.  Unlike ``librosa.load`` it does not resample: a file at another rate raises ValueError.
    ``encode=True`` applies ``encode_16bits`` as the reference does."""
    sr, x = scipy.io.wavfile.read(filename)
    if sr != sample_rate:
        raise ValueError(f"{filename}: sample rate {sr} Hz, expected {sample_rate} Hz "
                         "(load_wav does not resample; convert the file first)")
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768.0
    elif x.dtype in (np.float32, np.float64):
        x = x.astype(np.float32)
    else:
        raise ValueError(f"{filename}: {x.dtype} samples; load_wav reads 16-bit integer or float wavs")
    if x.ndim == 2:
        x = x.mean(axis=1, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if encode:
        x = encode_16bits(x)
    return x


def save_wav(y, filename, sample_rate, rescale_out=1.0):
    y = encode_16bits(y, rescale_out)
    if torch.is_tensor(y):
        y = y.cpu().numpy()
    scipy.io.wavfile.write(filename, sample_rate, y.astype(np.int16))


def preemphasis(x):
    return scipy.signal.lfilter([1, -hparams.preemphasis], [1], x)


def _stft_parameters():
    n_fft = (hparams.num_freq - 1) * 2
    hop_length = int(hparams.frame_shift_ms / 1000 * hparams.sample_rate)
    win_length = int(hparams.frame_length_ms / 1000 * hparams.sample_rate)
    return n_fft, hop_length, win_length


def _hz_to_mel(f):
    """Slaney's mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep,
                    f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (np.maximum(m, min_log_mel) - min_log_mel)),
                    f_sp * m)


def _build_mel_basis():
    """librosa.filters.mel(sample_rate, n_fft, n_mels=num_mels, fmin=fmin) of librosa < 0.10 in float64:
    fmax = sr/2, Slaney scale, triangles normalised to area 2 / (f[i+2] - f[i]).  [num_mels, num_freq]."""
    n_fft = (hparams.num_freq - 1) * 2
    sr, n_mels = hparams.sample_rate, hparams.num_mels
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(hparams.fmin), _hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    lower = -ramps[:n_mels] / fdiff[:n_mels, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0, np.minimum(lower, upper))
    return weights * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def _amp_to_db(x):
    return 20 * np.log10(np.maximum(1e-5, x))


def _normalize(S):
    return np.clip((S - hparams.min_level_db) / -hparams.min_level_db, 0, 1)


def _mel_table_host():
    """The fp32 table fv_melspectrogram reads (include/fastvocoder_hip.h, FV_MEL_TAB_*), built in float64."""
    n_fft, _, win_length = _stft_parameters()
    nc = n_fft // 2
    tab = np.zeros(_MEL_TAB_WEIGHTS + _MEL_MAX_WEIGHTS, dtype=np.float64)
    tab[0:win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)   # periodic Hann
    tw = np.exp(-2j * np.pi * np.arange(nc) / nc)
    sp = np.exp(-2j * np.pi * np.arange(nc) / n_fft)
    tab[_MEL_TAB_TWIDDLE:_MEL_TAB_TWIDDLE + 2 * nc] = np.stack([tw.real, tw.imag], 1).ravel()
    tab[_MEL_TAB_SPLIT:_MEL_TAB_SPLIT + 2 * nc] = np.stack([sp.real, sp.imag], 1).ravel()
    basis = _build_mel_basis()
    off = 0
    for m, row in enumerate(basis):
        nz = np.nonzero(row)[0]
        start, count = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if len(nz) else (0, 0)
        if off + count > _MEL_MAX_WEIGHTS:
            raise _native.NativeError("mel filters hold more weights than fv_melspectrogram's table")
        tab[_MEL_TAB_FILTERS + 3 * m:_MEL_TAB_FILTERS + 3 * m + 3] = (start, count, off)
        tab[_MEL_TAB_WEIGHTS + off:_MEL_TAB_WEIGHTS + off + count] = row[start:start + count]
        off += count
    return tab.astype(np.float32)


# include/fastvocoder_hip.h FV_MEL_TAB_* (offsets in floats)
_MEL_TAB_TWIDDLE, _MEL_TAB_SPLIT, _MEL_TAB_FILTERS, _MEL_TAB_WEIGHTS, _MEL_MAX_WEIGHTS = 1200, 3248, 5296, 5536, 2050
_mel_tables = {}


def mel_tables(device):
    """The device copy of the mel table, built once per device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _native.NativeError(f"mel tables live on the ROCm device, not {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _mel_tables:
        _mel_tables[device] = torch.from_numpy(_mel_table_host()).to(device)
    return _mel_tables[device]


def melspectrogram(y):
    """The reference's ``melspectrogram`` on the GPU (one fv_melspectrogram launch).

    - numpy 1-D array of n samples -> numpy float32 [num_mels, 1 + n // hop_size] (computed on the
      current ROCm device);
    - fp32 device tensor [n] or [B, n] -> device tensor [B, num_mels, 1 + n // hop_size], the generators'
      ``forward`` layout, enqueued on the current stream with no host copy.
    n must be at least n_fft // 2 + 1 = 1025 samples (reflect padding)."""
    n_fft, hop, win_length = _stft_parameters()
    if torch.is_tensor(y):
        if not y.is_cuda:
            raise _native.NativeError("melspectrogram: a tensor argument must live on the ROCm device; "
                                      "pass a numpy array for the host route")
        if y.dtype != torch.float32 or y.dim() not in (1, 2):
            raise _native.NativeError(f"melspectrogram: expected a float32 [n] or [B, n] tensor, got "
                                      f"{y.dtype} {tuple(y.shape)}")
        x = y.reshape(1, -1) if y.dim() == 1 else y
        return _native.melspectrogram(x.contiguous(), mel_tables(y.device), hparams.sample_rate, n_fft, hop,
                                      win_length, hparams.num_mels, float(hparams.fmin))
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"melspectrogram: expected a 1-D waveform, got shape {y.shape}")
    if not torch.cuda.is_available():
        raise _native.NativeError("melspectrogram runs on the ROCm device (there is no CPU path in fastvocoder_amd)")
    x = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to("cuda")
    return melspectrogram(x)[0].cpu().numpy()
