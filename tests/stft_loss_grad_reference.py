"""Float64 numpy gradient of the reference's STFT loss with respect to the estimate: the analytic adjoint of
tests/stft_loss_reference.py, the test oracle of fastvocoder_amd.loss with ``differentiable`` set.  Deliberately
independent of fastvocoder_amd (no import of it).

With spec = stft(x), X = sqrt(max(|spec|^2, 1e-7)) and Y the same of y:
    dS_diff/dX = -2 (Y - X),   dS_log/dX = -sign(ln Y - ln X) / X,   dX/dspec = spec / X where |spec|^2 > 1e-7, else 0
and the adjoint of frames -> rfft is  f[i] = Re sum_{k=0..n_fft/2} C[k] exp(+2 pi i k i / n_fft)  =  n_fft *
irfft(C with its interior bins halved); the window, the overlap-add at hop and the fold of the reflect padding
follow."""
import numpy as np
import scipy.fft

from . import stft_loss_reference as ref
from .stft_reference import padded_window, stft

RESOLUTIONS = ref.RESOLUTIONS
CLAMP = 1e-7


def _reflect_source(n, p):
    """index of the sample each padded position reads (stft_reference.reflect_pad)"""
    return np.concatenate([np.arange(p, 0, -1), np.arange(n), n - 2 - np.arange(p)])


def stft_adjoint(C, n, n_fft, hop, win_length, window=None):
    """C (B, T, n_fft/2 + 1) complex = dL/dre + i dL/dim of stft(x) -> dL/dx (B, n)."""
    C = np.array(C, dtype=np.complex128)
    C[..., 1:-1] *= 0.5
    frames = n_fft * scipy.fft.irfft(C, n=n_fft, axis=-1) * padded_window(n_fft, win_length, window)
    B, T = C.shape[0], C.shape[1]
    assert T == 1 + n // hop
    gpad = np.zeros((B, n + 2 * (n_fft // 2)))
    idx = (np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]).reshape(-1)
    for b in range(B):
        np.add.at(gpad[b], idx, frames[b].reshape(-1))
    gx = np.zeros((B, n))
    src = _reflect_source(n, n_fft // 2)
    for b in range(B):
        np.add.at(gx[b], src, gpad[b])
    return gx


def bin_gradients(x, y, n_fft, hop, win_length, window=None):
    """(dS_diff/dspec, dS_log/dspec): complex (B, T, bins) each, dL/dre + i dL/dim of stft(x)."""
    sx = stft(np.atleast_2d(np.asarray(x, np.float64)), n_fft, hop, win_length, window)
    sy = stft(np.atleast_2d(np.asarray(y, np.float64)), n_fft, hop, win_length, window)
    px, py = sx.real ** 2 + sx.imag ** 2, sy.real ** 2 + sy.imag ** 2
    X, Y = np.sqrt(np.maximum(px, CLAMP)), np.sqrt(np.maximum(py, CLAMP))
    dX = np.where(px > CLAMP, 1.0, 0.0) * sx / X
    return -2.0 * (Y - X) * dX, -np.sign(np.log(Y) - np.log(X)) / X * dX


def grad_sums(x, y, n_fft, hop, win_length, window=None):
    """(dS_diff/dx, dS_log/dx), float64 (B, n) each: the gradients of partial_sums' first and third column."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    cd, cl = bin_gradients(x, y, n_fft, hop, win_length, window)
    n = x.shape[-1]
    return (stft_adjoint(cd, n, n_fft, hop, win_length, window), stft_adjoint(cl, n, n_fft, hop, win_length, window))


def _safe_inv(v):
    return np.where(v > 0, 1.0 / np.where(v > 0, v, 1.0), 0.0)


def multi_resolution_stft_loss(x, y, resolutions=RESOLUTIONS):
    """(d sc / dx, d mag / dx) of MultiResolutionSTFTLoss()(x, y), float64 (B, n) each.  Where S_diff = 0 the
    spectral convergence has the gradient 0 (torch.norm's subgradient, as the reference's autograd gives it)."""
    x, y = np.atleast_2d(np.asarray(x, np.float64)), np.atleast_2d(np.asarray(y, np.float64))
    B, n = x.shape
    g_sc, g_mag = np.zeros((B, n)), np.zeros((B, n))
    for nf, hop, wl in resolutions:
        sums = ref.partial_sums(x, y, nf, hop, wl).sum(axis=0)
        gd, gl = grad_sums(x, y, nf, hop, wl)
        g_sc += 0.5 * _safe_inv(np.sqrt(sums[0]) * np.sqrt(sums[1])) * gd
        g_mag += gl / (B * (1 + n // hop) * (nf // 2 + 1))
    return g_sc / len(resolutions), g_mag / len(resolutions)


def per_utterance(x, y, resolutions=RESOLUTIONS):
    """(d sc_b / dx_b, d mag_b / dx_b): row b holds the gradient of row b's own terms (scored alone)."""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    rows = [multi_resolution_stft_loss(x[b:b + 1], y[b:b + 1], resolutions) for b in range(x.shape[0])]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


def loss_single_band(est, wav):
    """d Loss()(est, wav)[0] / d est."""
    return sum(multi_resolution_stft_loss(est, wav))


def pqmf_synthesis_adjoint_filter(synthesis_filter):
    """[S, taps + 1] synthesis bank -> the analysis-form filter of the synthesis' adjoint, S * flip(g_k)."""
    g = np.asarray(synthesis_filter, np.float64)
    return g.shape[0] * g[:, ::-1]


def pqmf_analysis(x, h):
    """x (B, T), h [S, taps + 1] -> (B, S, T // S): zero padding by taps / 2, the FIR, decimation by S (the
    reference's PQMF.analysis)."""
    S, ntaps = h.shape
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (ntaps // 2, ntaps // 2)))
    T = x.shape[-1] // S
    idx = S * np.arange(T)[:, None] + np.arange(ntaps)[None, :]
    return np.einsum("btj,kj->bkt", xp[:, idx], h)


def pqmf_synthesis(x, g):
    """x (B, S, Tsub), g [S, taps + 1] -> (B, S Tsub): zero stuffing times S, zero padding, the FIR summed over the
    bands (the reference's PQMF.synthesis)."""
    B, S, Tsub = x.shape
    ntaps = g.shape[1]
    u = np.zeros((B, S, S * Tsub))
    u[:, :, ::S] = S * np.asarray(x, np.float64)
    up = np.pad(u, ((0, 0), (0, 0), (ntaps // 2, ntaps // 2)))
    idx = np.arange(S * Tsub)[:, None] + np.arange(ntaps)[None, :]
    return np.einsum("bkmj,kj->bm", up[:, :, idx], g)


def loss_multiband(est_sub, wav, analysis_filter, synthesis_filter):
    """d Loss()(est_sub, wav, pqmf=...)[0] / d est_sub, (B, S, Tsub), given the PQMF's two banks [S, taps + 1]."""
    est_sub = np.asarray(est_sub, np.float64)
    B, S, Tsub = est_sub.shape
    wav_sub = pqmf_analysis(wav, np.asarray(analysis_filter, np.float64))
    est_full = pqmf_synthesis(est_sub, np.asarray(synthesis_filter, np.float64))
    g_sub = sum(multi_resolution_stft_loss(est_sub.reshape(B * S, Tsub), wav_sub.reshape(B * S, Tsub)))
    g_full = sum(multi_resolution_stft_loss(est_full, wav))
    back = pqmf_analysis(g_full, pqmf_synthesis_adjoint_filter(synthesis_filter))
    return (g_sub.reshape(B, S, Tsub) + back) / 2.0
