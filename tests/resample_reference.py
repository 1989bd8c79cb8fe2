"""float64 oracle of the resampler (audio.resample / fv_resample): band-limited interpolation with a Kaiser-windowed
sinc, the design of resampy's ``kaiser_best`` (what librosa < 0.10's ``load(sr=...)`` runs in the reference's load_wav).
Written independently of fastvocoder_amd/audio.py's table builder -- the formula is stated twice on purpose.

For sr_in -> sr_out:  g = gcd, L = sr_out / g, M = sr_in / g, scale = min(1, L / M) ROLLOFF, half = ceil(NUM_ZEROS / scale),
    h(u) = sinc(u) I0(BETA sqrt(1 - (u / NUM_ZEROS)^2)) / I0(BETA) for |u| < NUM_ZEROS, else 0
    n_out = ceil(n_in L / M);   c, p = divmod(j M, L)
    y[j] = scale sum_{i = c - half}^{c + half + 1} x[i] h(scale (c + p / L - i)),   x[i] = 0 outside [0, n_in)
The constants are resampy's published kaiser_best design as remembered (neither librosa nor resampy is a dependency):
this file, not bit parity with resampy, defines the filter.
"""
from functools import lru_cache
from math import gcd

import numpy as np

NUM_ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492

# the rate pairs of the tests: the reference's corpora (48, 44.1, 22.05 kHz -> 24 kHz), small and large ratios, and the
# two whose tables exceed a CU's LDS
PAIRS = [(48000, 24000), (44100, 24000), (22050, 24000), (16000, 24000), (8000, 24000), (96000, 24000),
         (48000, 22050), (11025, 24000)]


def window_sinc(u):
    """h(u), float64, any shape."""
    u = np.asarray(u, dtype=np.float64)
    inside = np.abs(u) < NUM_ZEROS
    v = np.where(inside, u, 0.0)
    kaiser = np.i0(BETA * np.sqrt(1.0 - (v / NUM_ZEROS) ** 2)) / np.i0(BETA)
    return np.where(inside, np.sinc(v) * kaiser, 0.0)


def geometry(sr_in, sr_out):
    """(L, M, scale, half)."""
    g = gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    scale = min(1.0, L / M) * ROLLOFF
    return L, M, scale, int(np.ceil(NUM_ZEROS / scale))


def out_len(n_in, L, M):
    return -((-n_in * L) // M)


@lru_cache(maxsize=None)
def coefficients(sr_in, sr_out):
    """[L, 2 half + 2] float64: row r = j mod L holds what output j multiplies x[c - half + t] by, t = 0 .. 2 half + 1.
    Computed once per pair and shared: read-only."""
    L, M, scale, half = geometry(sr_in, sr_out)
    rows = []
    for r in range(L):
        p = (r * M) % L
        i_rel = np.arange(-half, half + 2)                 # i - c
        rows.append(scale * window_sinc(scale * (p / L - i_rel)))
    H = np.array(rows)
    H.setflags(write=False)
    return H


def resample(x, sr_in, sr_out, start=0, stop=None):
    """Outputs [start, stop) (all of them by default) of x resampled sr_in -> sr_out, float64."""
    x = np.asarray(x, dtype=np.float64)
    L, M, scale, half = geometry(sr_in, sr_out)
    n_in = len(x)
    n_out = out_len(n_in, L, M)
    stop = n_out if stop is None else stop
    assert 0 <= start <= stop <= n_out, (start, stop, n_out)
    H = coefficients(sr_in, sr_out)
    i_rel = np.arange(-half, half + 2, dtype=np.int64)
    y = np.empty(stop - start, dtype=np.float64)
    for lo in range(start, stop, 4096):                     # one gathered product per block of outputs
        j = np.arange(lo, min(lo + 4096, stop), dtype=np.int64)
        c = (j * M) // L
        i = c[:, None] + i_rel[None, :]
        valid = (i >= 0) & (i < n_in)
        X = np.where(valid, x[np.clip(i, 0, n_in - 1)], 0.0)
        y[lo - start:lo - start + len(j)] = np.einsum("jt,jt->j", X, H[j % L])
    return y


def error_bound(sr_in, sr_out, peak):
    """|fp32 kernel - oracle| for inputs of magnitude <= peak: every coefficient rounded once (relative 2^-24) and a chain
    of taps fp32 FMAs whose partial sums stay below ||h_r||_1 peak:  (taps + 2) 2^-24 max_r ||h_r||_1 peak."""
    H = coefficients(sr_in, sr_out)
    return (H.shape[1] + 2) * 2.0 ** -24 * np.abs(H).sum(axis=1).max() * peak


def scipy_fir(sr_in, sr_out):
    """The same filter as the FIR scipy.signal.resample_poly(x, L, M, window=hf) / L applies:
    hf[n] = scale h(scale n / L), |n| <= ceil(NUM_ZEROS L / scale)."""
    L, M, scale, _ = geometry(sr_in, sr_out)
    reach = int(np.ceil(NUM_ZEROS * L / scale))
    n = np.arange(-reach, reach + 1)
    return L, M, scale * window_sinc(scale * n / L)
