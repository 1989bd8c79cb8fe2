"""Float64 numpy restatement of the reference's STFT loss (model/loss/stft_loss.py with torch.stft defaults,
model/loss/loss.py): the test oracle of fastvocoder_amd.loss.  Deliberately independent of fastvocoder_amd
(no import of it)."""
import numpy as np

from .stft_reference import padded_window, stft  # noqa: F401  (test_stft_loss_host reads padded_window from here)

RESOLUTIONS = ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))   # (n_fft, hop, win_length)


def stft_magnitude(x, n_fft, hop, win_length, window=None):
    """sqrt(max(|torch.stft(x, n_fft, hop, win_length, window)|^2, 1e-7)): (B, 1 + n // hop, n_fft // 2 + 1)."""
    spec = stft(np.atleast_2d(np.asarray(x, dtype=np.float64)), n_fft, hop, win_length, window)
    return np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, 1e-7))


def partial_sums(x, y, n_fft, hop, win_length):
    """[B, 3] float64: sum (|Y| - |X|)^2, sum |Y|^2, sum |ln|Y| - ln|X|| per row."""
    X, Y = stft_magnitude(x, n_fft, hop, win_length), stft_magnitude(y, n_fft, hop, win_length)
    return np.stack([((Y - X) ** 2).sum(axis=(1, 2)), (Y ** 2).sum(axis=(1, 2)),
                     np.abs(np.log(Y) - np.log(X)).sum(axis=(1, 2))], axis=1)


def stft_loss(x, y, n_fft, hop, win_length):
    """(sc, mag) of STFTLoss: ||Y - X||_F / ||Y||_F and mean |log Y - log X| over the whole batch."""
    X, Y = stft_magnitude(x, n_fft, hop, win_length), stft_magnitude(y, n_fft, hop, win_length)
    return float(np.linalg.norm(Y - X) / np.linalg.norm(Y)), float(np.mean(np.abs(np.log(Y) - np.log(X))))


def multi_resolution_stft_loss(x, y, resolutions=RESOLUTIONS):
    terms = np.array([stft_loss(x, y, *r) for r in resolutions])
    return float(terms[:, 0].mean()), float(terms[:, 1].mean())


def per_utterance(x, y, resolutions=RESOLUTIONS):
    """[B, 2]: each row's (sc, mag) as if scored alone."""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    return np.array([multi_resolution_stft_loss(x[b:b + 1], y[b:b + 1], resolutions) for b in range(x.shape[0])])


def loss_single_band(est, wav):
    """Loss()(est, wav)[0]: sc + mag of the multi-resolution loss."""
    return sum(multi_resolution_stft_loss(est, wav))


def loss_multiband(est_sub, wav, wav_sub, est_full):
    """Loss()(est_sub, wav, pqmf=...)[0] given the PQMF analysis of wav (B, S, T/S) and synthesis of est_sub (B, T)."""
    S = est_sub.shape[1]
    sub = sum(multi_resolution_stft_loss(est_sub.reshape(-1, est_sub.shape[-1]), wav_sub.reshape(-1, wav_sub.shape[-1])))
    full = sum(multi_resolution_stft_loss(est_full, wav))
    assert wav_sub.shape[1] == S
    return (sub + full) / 2.0
