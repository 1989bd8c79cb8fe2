"""Float64 numpy restatement of the reference's STFT loss (model/loss/stft_loss.py with torch.stft defaults,
model/loss/loss.py): the test oracle of fastvocoder_amd.loss.  Deliberately independent of fastvocoder_amd
(no import of it)."""
import numpy as np

RESOLUTIONS = ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))   # (n_fft, hop, win_length)


def hann(win_length):
    """torch.hann_window(win_length), periodic: 0.5 - 0.5 cos(2 pi i / win_length); one tap is [1] in torch."""
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


def stft_magnitude(x, n_fft, hop, win_length, window=None):
    """sqrt(max(|torch.stft(x, n_fft, hop, win_length, window)|^2, 1e-7)): (B, 1 + n // hop, n_fft // 2 + 1)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1]
    padded = reflect_pad(x, n_fft // 2)
    T = 1 + n // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    frames = padded[:, idx] * padded_window(n_fft, win_length, window)[None, None, :]
    spec = np.fft.rfft(frames, axis=-1)
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
