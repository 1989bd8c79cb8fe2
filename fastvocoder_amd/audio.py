"""The audio side of the reference (data/audio.py): the wav sink of the synthesize flow
(encode_16bits / save_wav, data/audio.py:12-26), and the mel front end that makes a generator's
input from a wav (load_wav / melspectrogram, data/audio.py:17-21,58-61) for copy-synthesis and
MODE=preprocess, and the inverse direction: Griffin-Lim (inv_mel_spectrogram / inv_spectrogram,
data/audio.py:37-47,66-95,179-190), the baseline the synthesize flow writes beside the vocoder's wav.
The resampling inside the reference's ``load_wav`` is ``resample`` here; its TensorFlow helpers stay out of scope.

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

``resample`` is the sample-rate conversion ``librosa.load(sr=...)`` does inside the reference's ``load_wav``
(librosa < 0.10: resampy's ``kaiser_best``, band-limited interpolation with a Kaiser-windowed sinc) as one HIP launch
(csrc/resample.hip, fv_resample); ``load_wav(resample=True)`` and ``MODE=preprocess --resample`` run it on files
at another rate.  ``_resample_table_host`` is the float64 statement of the filter the kernel's table is built from.

``inv_mel_spectrogram`` is the reference's chain mel -> linear magnitude (pseudo-inverse of the mel
filters, ** power) -> Griffin-Lim (griffin_lim_iters projections) -> inverse preemphasis, all on the
GPU (csrc/griffin_lim.hip: fv_mel_to_linear, fv_griffin_lim, fv_inv_preemphasis).  The reference draws
the initial phase from the global NumPy state; here the draw is an argument (``angles`` / ``seed``), so a
run can be repeated.  Device tensors hold spectra FRAMES-MAJOR ([B, T, 1025], as the kernels read them);
the numpy-facing helpers (``_stft``, ``_istft``, ``_mel_to_linear``, ``_griffin_lim``) take and return
librosa's [1025, T].
"""
import math

import numpy as np
import scipy.io.wavfile
import scipy.signal
import scipy.special
import torch

from . import _abi
from . import _native
from . import hparams
from ._stft_tables import device_cached, periodic_hann, rfft_twiddles


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


def load_wav(filename, sample_rate=24000, encode=True, resample=False, keep_on_device=False):
    """The reference's ``load_wav`` without librosa: the samples as float32 (16-bit integer wavs divided by
    32768, as librosa returns them; float wavs as stored), multi-channel averaged to mono.
    A file at another rate raises ValueError unless ``resample=True``: then it is converted to ``sample_rate`` on
    the GPU (``resample`` below, what ``librosa.load(sr=sample_rate)`` does in the reference) -- a mono 16-bit file goes to
    the device as int16, stereo and float files after the host conversion to mono float32.  A file already at the
    rate never touches the GPU.  ``keep_on_device=True`` returns a resampled waveform as the device tensor it was
    computed into instead of copying it to the host (a file at the rate is a host array all the same).
    ``encode=True`` applies ``encode_16bits`` as the reference does."""
    sr, x = scipy.io.wavfile.read(filename)
    if sr != sample_rate and not resample:
        raise ValueError(f"{filename}: sample rate {sr} Hz, expected {sample_rate} Hz "
                         "(load_wav does not resample; convert the file first)")
    if x.dtype != np.int16 and x.dtype not in (np.float32, np.float64):
        raise ValueError(f"{filename}: {x.dtype} samples; load_wav reads 16-bit integer or float wavs")
    if sr != sample_rate and x.dtype == np.int16 and x.ndim == 1:
        x = _resample(_to_device(x, "load_wav(resample=True)", np.int16), int(sr), sample_rate)
    else:
        if x.dtype == np.int16:
            x = x.astype(np.float32) / 32768.0
        else:
            x = x.astype(np.float32)
        if x.ndim == 2:
            x = x.mean(axis=1, dtype=np.float32)
        x = np.ascontiguousarray(x, dtype=np.float32)
        if sr != sample_rate:
            x = _resample(_to_device(x, "load_wav(resample=True)"), int(sr), sample_rate)
    if torch.is_tensor(x) and not keep_on_device:
        x = x.cpu().numpy()
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
    tab = np.zeros(_MEL_TAB_WEIGHTS + _MEL_MAX_WEIGHTS, dtype=np.float64)
    tab[0:win_length] = periodic_hann(win_length)
    tab[_MEL_TAB_TWIDDLE:_MEL_TAB_SPLIT], tab[_MEL_TAB_SPLIT:_MEL_TAB_FILTERS] = rfft_twiddles(n_fft)
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


_C = _abi.constants()       # offsets in floats
_MEL_TAB_TWIDDLE, _MEL_TAB_SPLIT, _MEL_TAB_FILTERS = _C["FV_MEL_TAB_TWIDDLE"], _C["FV_MEL_TAB_SPLIT"], _C["FV_MEL_TAB_FILTERS"]
_MEL_TAB_WEIGHTS, _MEL_MAX_WEIGHTS = _C["FV_MEL_TAB_WEIGHTS"], _C["FV_MEL_MAX_WEIGHTS"]
_mel_tables = {}


def mel_tables(device):
    """The device copy of the mel table, built once per device."""
    return device_cached(_mel_tables, device, (), _mel_table_host, "mel tables")


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


# ---------------------------------------------------------------------------
# sample-rate conversion (csrc/resample.hip)
# ---------------------------------------------------------------------------

# resampy's kaiser_best: zero crossings of the sinc kept on each side, cutoff as a fraction of the lower Nyquist rate, Kaiser beta
RESAMPLE_NUM_ZEROS, RESAMPLE_ROLLOFF, RESAMPLE_BETA = 64, 0.9475937167399596, 14.769656459379492
_resample_tables = {}


def _resample_geometry(orig_sr, target_sr):
    """(L, M, scale, half) of the polyphase filter orig_sr -> target_sr; ValueError for rates that are not positive
    integers and for a pair beyond fv_resample's limits (include/fastvocoder_hip.h): a table of (2 half + 2) L floats
    above 2^20 (4 MiB; every pair of the usual rates 8000 ... 96000 Hz stays below 2^18) or a block's input window above
    16384 floats of LDS (ratios beyond about 1 : 50)."""
    for name, sr in (("orig_sr", orig_sr), ("target_sr", target_sr)):
        if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or sr <= 0:
            raise ValueError(f"resample: {name}={sr!r}; sample rates are positive integers")
    g = math.gcd(int(orig_sr), int(target_sr))
    L, M = int(target_sr) // g, int(orig_sr) // g
    scale = min(1.0, L / M) * RESAMPLE_ROLLOFF
    half = math.ceil(RESAMPLE_NUM_ZEROS / scale)
    table, window = (2 * half + 2) * L, (L - 1 + 255 * M) // L + 2 * half + 2
    if (max(L, M) > _native.RESAMPLE_MAX_FACTOR or table > _native.RESAMPLE_MAX_TABLE_FLOATS
            or window > _native.RESAMPLE_MAX_WINDOW):
        raise ValueError(f"resample: {orig_sr} -> {target_sr} Hz is the ratio {L}/{M}: a filter table of {table} floats "
                         f"(at most {_native.RESAMPLE_MAX_TABLE_FLOATS}) and an input window of {window} per block (at most "
                         f"{_native.RESAMPLE_MAX_WINDOW}); convert through a rate with a larger common divisor")
    return L, M, scale, half


def _resample_table_host(orig_sr, target_sr):
    """The fp32 table fv_resample reads for orig_sr -> target_sr, built in float64 and rounded once: [2 half + 2, L]
    (tap-major), entry [t, r] = scale h(scale (half - t + p_r / L)) with p_r = (r M) mod L, the coefficient output
    j = r (mod L) applies to x[c - half + t];  h(u) = sinc(u) I0(beta sqrt(1 - (u / zeros)^2)) / I0(beta), |u| < zeros."""
    L, M, scale, half = _resample_geometry(orig_sr, target_sr)
    frac = (np.arange(L, dtype=np.int64) * M % L) / L
    u = scale * (half - np.arange(2 * half + 2, dtype=np.float64)[:, None] + frac[None, :])
    inside = np.abs(u) < RESAMPLE_NUM_ZEROS
    arg = np.sqrt(np.where(inside, 1.0 - (u / RESAMPLE_NUM_ZEROS) ** 2, 0.0))
    h = np.where(inside, np.sinc(u) * scipy.special.i0(RESAMPLE_BETA * arg) / scipy.special.i0(RESAMPLE_BETA), 0.0)
    return np.ascontiguousarray(scale * h).astype(np.float32)


def resample_tables(device, orig_sr, target_sr):
    """The device copy of the filter table for orig_sr -> target_sr, built once per device and pair."""
    return device_cached(_resample_tables, device, (int(orig_sr), int(target_sr)),
                         lambda: _resample_table_host(orig_sr, target_sr), "resampling tables")


def resample(y, orig_sr, target_sr):
    """``librosa.resample(y, orig_sr, target_sr)`` of librosa < 0.10 (res_type='kaiser_best', fix=True) on the GPU, one
    fv_resample launch: ceil(n target_sr / orig_sr) samples.

    - numpy 1-D array (float32 or float64) -> numpy float32 (computed on the current ROCm device);
    - float32 or int16 (PCM, read as s / 32768) device tensor [n] or [B, n] -> float32 device tensor of the same rank,
      enqueued on the current stream with no host copy.
    ``orig_sr == target_sr`` returns the samples as float32 with no launch.  The filter is resampy's kaiser_best DESIGN
    evaluated exactly per phase (resampy interpolates in a table): the same filter, not the same bits."""
    L, M, _, half = _resample_geometry(orig_sr, target_sr)
    if torch.is_tensor(y):
        if not y.is_cuda:
            raise _native.NativeError("resample: a tensor argument must live on the ROCm device; pass a numpy array for "
                                      "the host route")
        if y.dtype not in (torch.float32, torch.int16) or y.dim() not in (1, 2):
            raise _native.NativeError(f"resample: expected a float32 or int16 [n] or [B, n] tensor, got {y.dtype} "
                                      f"{tuple(y.shape)}")
        if y.shape[-1] == 0:
            raise ValueError("resample: an empty waveform")
        if L == M:
            return y.to(torch.float32) / 32768.0 if y.dtype == torch.int16 else y
        x = (y.reshape(1, -1) if y.dim() == 1 else y).contiguous()
        out = _native.resample(x, resample_tables(y.device, orig_sr, target_sr), L, M, half)
        return out[0] if y.dim() == 1 else out
    y = np.asarray(y)
    if y.ndim != 1 or y.dtype not in (np.float32, np.float64):
        raise ValueError(f"resample: expected a 1-D float32 or float64 waveform, got {y.dtype} {y.shape}")
    if y.shape[0] == 0:
        raise ValueError("resample: an empty waveform")
    if L == M:
        return y.astype(np.float32)
    return resample(_to_device(y, "resample"), orig_sr, target_sr).cpu().numpy()


_resample = resample      # for load_wav, whose ``resample`` argument hides the function


# ---------------------------------------------------------------------------
# the inverse direction: Griffin-Lim (csrc/griffin_lim.hip)
# ---------------------------------------------------------------------------

def inv_preemphasis(x):
    """lfilter([1], [1, -preemphasis], x) on the GPU (fv_inv_preemphasis): numpy 1-D -> numpy float32; fp32 device
    tensor [n] or [B, n] -> device tensor of the same shape."""
    if torch.is_tensor(x):
        _need_device_f32(x, "inv_preemphasis", (1, 2))
        return _native.inv_preemphasis(x.reshape(1, -1) if x.dim() == 1 else x.contiguous(),
                                       hparams.preemphasis).reshape(x.shape)
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError(f"inv_preemphasis: expected a 1-D waveform, got shape {x.shape}")
    return inv_preemphasis(_to_device(x, "inv_preemphasis")).cpu().numpy()


def _denormalize(S):
    return (np.clip(S, 0, 1) * -hparams.min_level_db) + hparams.min_level_db


def _db_to_amp(x):
    return np.power(10.0, x * 0.05)


def _need_device_f32(t, who, dims):
    if not t.is_cuda:
        raise _native.NativeError(f"{who}: a tensor argument must live on the ROCm device; pass a numpy array for "
                                  "the host route")
    if t.dtype != torch.float32 or t.dim() not in dims:
        raise _native.NativeError(f"{who}: expected a float32 tensor of {' or '.join(map(str, dims))} dimensions, got "
                                  f"{t.dtype} {tuple(t.shape)}")


def _to_device(a, who, dtype=np.float32):
    if not torch.cuda.is_available():
        raise _native.NativeError(f"{who} runs on the ROCm device (there is no CPU path in fastvocoder_amd)")
    _native.lib()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def _gl_table_host():
    """The fp32 table the Griffin-Lim kernels read (include/fastvocoder_hip.h, FV_GL_TAB_*), built in float64: the
    window, twiddle and split parts of the mel table, then the squared window."""
    n_fft, _, win_length = _stft_parameters()
    tab = np.zeros(_GL_TAB_WIN2 + win_length, dtype=np.float64)
    w = periodic_hann(win_length)
    tab[0:win_length] = w
    tab[_MEL_TAB_TWIDDLE:_MEL_TAB_SPLIT], tab[_MEL_TAB_SPLIT:_GL_TAB_WIN2] = rfft_twiddles(n_fft)
    tab[_GL_TAB_WIN2:] = w * w
    return tab.astype(np.float32)


def _inv_mel_basis_host():
    """pinv(_build_mel_basis()) in float64, transposed to [num_mels, num_freq] (a wave reads consecutive bins) and
    rounded once to fp32."""
    return np.ascontiguousarray(np.linalg.pinv(_build_mel_basis()).T).astype(np.float32)


_GL_TAB_WIN2 = _C["FV_GL_TAB_WIN2"]
_gl_tables, _inv_bases = {}, {}


def griffin_lim_tables(device):
    """The device copy of the Griffin-Lim table, built once per device."""
    return device_cached(_gl_tables, device, (), _gl_table_host, "Griffin-Lim tables")


def inv_mel_basis(device):
    """The device copy of the transposed pseudo-inverse of the mel filters, built once per device."""
    return device_cached(_inv_bases, device, (), _inv_mel_basis_host, "Griffin-Lim tables")


def _stft(y):
    """librosa.stft(y, n_fft, hop, win) on the GPU (fv_stft): numpy 1-D -> complex64 numpy [num_freq, T]; fp32 device
    tensor [n] / [B, n] -> complex64 device tensor [B, T, num_freq] (frames-major)."""
    n_fft, hop, win_length = _stft_parameters()
    if torch.is_tensor(y):
        _need_device_f32(y, "_stft", (1, 2))
        return _native.stft_complex((y.reshape(1, -1) if y.dim() == 1 else y).contiguous(),
                                    griffin_lim_tables(y.device), n_fft, hop, win_length)
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"_stft: expected a 1-D waveform, got shape {y.shape}")
    return np.ascontiguousarray(_stft(_to_device(y, "_stft"))[0].cpu().numpy().T)


def _istft(D):
    """librosa.istft(D, hop, win) on the GPU (fv_istft): complex numpy [num_freq, T] -> float32 numpy
    [hop (T - 1)]; complex64 device tensor [B, T, num_freq] (frames-major) -> device tensor [B, hop (T - 1)]."""
    n_fft, hop, win_length = _stft_parameters()
    if torch.is_tensor(D):
        if not D.is_cuda:
            raise _native.NativeError("_istft: a tensor argument must live on the ROCm device")
        return _native.istft(D, griffin_lim_tables(D.device), n_fft, hop, win_length)
    D = np.asarray(D)
    if D.ndim != 2 or D.shape[0] != hparams.num_freq:
        raise ValueError(f"_istft: expected [{hparams.num_freq}, T], got shape {D.shape}")
    d = _to_device(D.T[None], "_istft", np.complex64)
    return _istft(d)[0].cpu().numpy()


def _initial_phase(angles, seed, B, T, device):
    """exp(2j pi u) for the reference's uniform draw u [num_freq, T] (given, or drawn on the host from
    RandomState(seed) / the global NumPy state), computed in float64, rounded once: complex64 device [B, T, num_freq]."""
    F = hparams.num_freq
    if angles is None:
        rng = np.random if seed is None else np.random.RandomState(seed)
        angles = rng.rand(F, T) if B == 1 else np.stack([rng.rand(F, T) for _ in range(B)])
    angles = np.asarray(angles, dtype=np.float64)
    if angles.shape == (F, T):
        angles = np.broadcast_to(angles, (B, F, T))
    if angles.shape != (B, F, T):
        raise ValueError(f"angles: expected [{F}, {T}] or [{B}, {F}, {T}], got {angles.shape}")
    ph = np.exp(2j * np.pi * angles.transpose(0, 2, 1)).astype(np.complex64)
    return torch.from_numpy(np.ascontiguousarray(ph)).to(device)


def _griffin_lim_device(S, angles, seed, iters):
    """S: fp32 device [B, T, num_freq] -> y [B, hop (T - 1)]."""
    n_fft, hop, win_length = _stft_parameters()
    B, T = S.shape[:2]
    if hop * (T - 1) < n_fft // 2 + 1:
        raise ValueError(f"Griffin-Lim needs at least {(n_fft // 2 + 1 + hop - 1) // hop + 1} frames (its iterate of "
                         f"{hop} (T - 1) samples is reflect-padded by {n_fft // 2}), got T={T}")
    ph = _initial_phase(angles, seed, B, T, S.device)
    return _native.griffin_lim(S, ph, griffin_lim_tables(S.device), int(iters), None, n_fft, hop, win_length)


def _griffin_lim(S, angles=None, seed=None, iters=None):
    """The reference's ``_griffin_lim`` on the GPU (fv_griffin_lim): S numpy [num_freq, T] magnitudes -> float32 numpy
    [hop (T - 1)]; fp32 device tensor [B, T, num_freq] (frames-major) -> device tensor [B, hop (T - 1)].
    ``angles``: the uniform [0, 1) draw the reference takes from np.random.rand(num_freq, T) ([B, num_freq, T] for a
    batch); absent, it is drawn from np.random.RandomState(seed), or the global NumPy state for seed=None."""
    iters = hparams.griffin_lim_iters if iters is None else iters
    if torch.is_tensor(S):
        _need_device_f32(S, "_griffin_lim", (3,))
        return _griffin_lim_device(S.contiguous(), angles, seed, iters)
    S = np.abs(np.asarray(S))
    if S.ndim != 2 or S.shape[0] != hparams.num_freq:
        raise ValueError(f"_griffin_lim: expected [{hparams.num_freq}, T], got shape {S.shape}")
    return _griffin_lim_device(_to_device(S.T[None], "_griffin_lim"), angles, seed, iters)[0].cpu().numpy()


def _mel_to_linear(mel_spectrogram, power=1.0):
    """max(1e-10, pinv(mel_basis) @ mel_spectrogram) ** power on the GPU (fv_mel_to_linear).  NOTE the argument: as in
    the reference's chain this is the AMPLITUDE mel (``_db_to_amp(_denormalize(mel) + ref_level_db)``) for numpy
    [num_mels, T] -> float32 numpy [num_freq, T]; the kernel takes the normalised mel, so the amplitudes are mapped back
    (exactly invertible above the 1e-5 floor of ``_amp_to_db``)."""
    A = np.asarray(mel_spectrogram, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != hparams.num_mels:
        raise ValueError(f"_mel_to_linear: expected [{hparams.num_mels}, T], got shape {A.shape}")
    mel = (20 * np.log10(np.maximum(1e-300, A)) - hparams.ref_level_db - hparams.min_level_db) / -hparams.min_level_db
    if mel.min() < 0 or mel.max() > 1:
        raise ValueError("_mel_to_linear: amplitudes outside the range of a normalised mel "
                         f"([{_db_to_amp(hparams.min_level_db + hparams.ref_level_db):g}, "
                         f"{_db_to_amp(hparams.ref_level_db):g}])")
    S = _mel_to_linear_device(_to_device(mel[None], "_mel_to_linear"), power)
    return np.ascontiguousarray(S[0].cpu().numpy().T)


def _mel_to_linear_device(mel, power):
    """Normalised mel, fp32 device [B, num_mels, T] -> S [B, T, num_freq] = _mel_to_linear(...) ** power."""
    return _native.mel_to_linear(mel.contiguous(), inv_mel_basis(mel.device), power)


def inv_mel_spectrogram(mel_spectrogram, angles=None, seed=None, iters=None):
    """The reference's ``inv_mel_spectrogram`` on the GPU: normalised mel -> waveform by Griffin-Lim.

    - numpy [num_mels, T] -> 1-D float32 numpy array of hop_size (T - 1) samples;
    - fp32 device tensor [num_mels, T] or [B, num_mels, T] -> device tensor [hop_size (T - 1)] / [B, hop_size (T - 1)]
      (chains after ``melspectrogram`` with no host round trip).
    ``angles`` / ``seed``: the initial phase draw, see ``_griffin_lim``.  ``iters``: hparams.griffin_lim_iters.
    T must be at least 6 frames.  Values outside [0, 1] are clipped, as the reference's ``_denormalize`` does."""
    iters = hparams.griffin_lim_iters if iters is None else iters
    if torch.is_tensor(mel_spectrogram):
        mel = mel_spectrogram
        _need_device_f32(mel, "inv_mel_spectrogram", (2, 3))
        m3 = mel.unsqueeze(0) if mel.dim() == 2 else mel
        if m3.shape[1] != hparams.num_mels:
            raise ValueError(f"inv_mel_spectrogram: expected {hparams.num_mels} mel channels, got {tuple(mel.shape)}")
        S = _mel_to_linear_device(m3, hparams.power)
        y = _native.inv_preemphasis(_griffin_lim_device(S, angles, seed, iters), hparams.preemphasis)
        return y[0] if mel.dim() == 2 else y
    mel = np.asarray(mel_spectrogram)
    if mel.ndim != 2 or mel.shape[0] != hparams.num_mels:
        raise ValueError(f"inv_mel_spectrogram: expected [{hparams.num_mels}, T], got shape {mel.shape}")
    return inv_mel_spectrogram(_to_device(mel, "inv_mel_spectrogram"), angles, seed, iters).cpu().numpy()
