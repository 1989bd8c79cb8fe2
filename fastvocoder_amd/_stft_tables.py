"""Host side of the shared STFT core (csrc/stft_core.hpp): the float64 pieces every kernel table is built from (the
mel, Griffin-Lim and STFT-distance tables round them once to fp32) and the per-device cache of the device copies."""
import numpy as np
import torch

from . import _native


def rfft_twiddles(n_fft):
    """(FFT twiddles exp(-2 pi i t / nc), split twiddles exp(-2 pi i k / n_fft)) for t, k < nc = n_fft // 2, each as
    2 nc float64 with real and imaginary parts interleaved."""
    nc = n_fft // 2
    tw, sp = np.exp(-2j * np.pi * np.arange(nc) / nc), np.exp(-2j * np.pi * np.arange(nc) / n_fft)
    return tuple(np.stack([c.real, c.imag], 1).ravel() for c in (tw, sp))


def periodic_hann(win_length):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)


def device_cached(cache, key_device, key_rest, make, what):
    """cache[(device, *key_rest)]: the device copy of the numpy array ``make()``, built once.  ``what`` names the
    tables in the error for a device that is not the ROCm device."""
    device = torch.device(key_device)
    if device.type != "cuda":
        raise _native.NativeError(f"{what} live on the ROCm device, not {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, *key_rest)
    if key not in cache:
        cache[key] = torch.from_numpy(make()).to(device)
    return cache[key]
