"""STFT-based distances of the reference (model/loss/stft_loss.py) on the MI355X, with an opt-in gradient.

``stft`` returns the reference's clamped magnitudes (B, #frames, #bins) from one fv_stft_magnitude launch.
``STFTLoss`` and ``MultiResolutionSTFTLoss`` keep the reference's names, constructor arguments and batch-level
results, but never build the magnitudes: one fv_stft_distance call (two launches) returns, per resolution and
utterance, the float64 sums S_diff = sum (|Y| - |X|)^2, S_ref = sum |Y|^2 and S_log = sum |ln|Y| - ln|X||, and the
terms are formed from them:

    SC  = sqrt(sum_b S_diff) / sqrt(sum_b S_ref)          (SpectralConvergenceLoss: ||Y - X||_F / ||Y||_F)
    mag = sum_b S_log / (B * frames * bins)                (LogSTFTMagnitudeLoss: F.l1_loss(log Y, log X))

each averaged over the resolutions.  ``per_utterance`` gives the same two terms for every row on its own from the
same sums.  By default the loss is inference-only: an input that requires grad while grad mode is on is refused
rather than have its gradient dropped.

``differentiable = True`` on a module (STFTLoss, MultiResolutionSTFTLoss, or Loss in loss.py; a policy attribute,
not a constructor argument) switches the gradient with respect to the estimate on: the sums then come from one
autograd Function whose forward is the same fv_stft_distance call (the same bits) and whose backward hands
dL/dS_diff and dL/dS_log per (resolution, row) to fv_stft_distance_grad, which returns dL/dx [B, n] in fp32.  Only x,
y, the tables and the sums are kept for backward, never spectra or magnitudes.  The target has no gradient.
"""
import numpy as np
import torch

from .. import _native
from .._stft_tables import device_cached, rfft_twiddles

_tables = {}


def _window_fn(window):
    fn = getattr(torch, window, None) if isinstance(window, str) else None
    if not (isinstance(window, str) and window.endswith("_window") and callable(fn)):
        raise _native.NativeError(f"window must name a torch window function such as 'hann_window', got {window!r}")
    return fn


def _stft_table_host(n_fft, win_length, window="hann_window"):
    """The fp32 table of one resolution (include/fastvocoder_hip.h FV_STFT_TAB_*), built in float64: the FFT and
    split twiddles, then the win_length window taps (``getattr(torch, window)(win_length)`` in float64, or the values
    of a window tensor)."""
    n_fft, win_length = int(n_fft), int(win_length)
    if n_fft not in (512, 1024, 2048) or not 1 <= win_length <= n_fft:
        raise _native.NativeError(f"stft: n_fft must be 512, 1024 or 2048 and 1 <= win_length <= n_fft "
                                  f"(got n_fft={n_fft} win_length={win_length})")
    if torch.is_tensor(window):
        w = window.detach().to("cpu", torch.float64).numpy().reshape(-1)
    else:
        w = _window_fn(window)(win_length, dtype=torch.float64).numpy()
    if w.shape != (win_length,):
        raise _native.NativeError(f"stft: the window has {w.size} taps, win_length is {win_length}")
    return np.concatenate([*rfft_twiddles(n_fft), w]).astype(np.float32)


def stft_tables(device, n_fft, win_length, window="hann_window"):
    """The device copy of one resolution's table, built once per (device, n_fft, win_length, window name)."""
    return device_cached(_tables, device, (int(n_fft), int(win_length), window),
                         lambda: _stft_table_host(n_fft, win_length, window), "stft tables")


def _signal(t, name, differentiable=False):
    """A [B, n] fp32 contiguous device tensor, or a clear error.  ``differentiable``: t may require grad."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise _native.NativeError(f"{name} lives on {t.device}; the STFT loss runs on the ROCm device "
                                  "(there is no CPU path in fastvocoder_amd)")
    if t.requires_grad and torch.is_grad_enabled() and not differentiable:
        if name == "x":
            raise RuntimeError("x requires grad: the fastvocoder_amd STFT loss is inference-only (forward, no "
                               "autograd) unless the module's `differentiable` attribute is set; set it, call the "
                               "loss under torch.no_grad() or pass a detached tensor")
        raise RuntimeError(f"{name} requires grad: the fastvocoder_amd STFT loss is inference-only (forward, no "
                           "autograd) and has no gradient with respect to the target; call it under "
                           "torch.no_grad() or pass a detached tensor")
    if t.dim() != 2:
        raise ValueError(f"{name} must be (B, T), got shape {tuple(t.shape)}")
    if not t.is_floating_point():
        raise TypeError(f"{name} must be a floating-point signal, got {t.dtype}")
    return t.to(torch.float32).contiguous()


def _table_for(t, n_fft, win_length, window):
    if torch.is_tensor(window):
        return torch.from_numpy(_stft_table_host(n_fft, win_length, window)).to(t.device)
    return stft_tables(t.device, n_fft, win_length, window)


def stft(x, fft_size, hop_size, win_length, window):
    """Magnitude spectrogram (B, #frames, fft_size // 2 + 1) of x (B, T), as the reference's ``stft``: torch.stft
    defaults (center=True, reflect padding), sqrt(max(re^2 + im^2, 1e-7)).  ``window`` is a torch window name
    ('hann_window') or a window tensor of win_length taps (the reference passes STFTLoss's buffer)."""
    x = _signal(x, "x")
    return _native.stft_magnitude(x, _table_for(x, fft_size, win_length, window), int(fft_size), int(hop_size),
                                  int(win_length))


class _DistanceSums(torch.autograd.Function):
    """float64 [R, B, 3] sums of fv_stft_distance with the gradient of fv_stft_distance_grad with respect to x."""

    @staticmethod
    def forward(ctx, x, y, geometry, *tables):
        sums = _native.stft_distance(x, y, list(tables), *geometry)
        ctx.geometry = geometry
        ctx.save_for_backward(x, y, sums, *tables)
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sums):
        x, y, sums, *tables = ctx.saved_tensors
        # S_ref does not depend on x.  A row with S_diff == 0 has X == Y in every bin, so dS_diff/dx is exactly 0
        # there, whatever the coefficient: sqrt'(0) = inf of the spectral convergence must not make it inf * 0.
        c_diff = torch.where(sums[:, :, 0] == 0, torch.zeros_like(grad_sums[:, :, 0]), grad_sums[:, :, 0])
        coef = torch.stack([c_diff, grad_sums[:, :, 2]], dim=2).float().contiguous()
        gx = _native.stft_distance_grad(x, y, tables, *ctx.geometry, coef)
        return (gx, None, None) + (None,) * len(tables)


def _sums(x, y, resolutions, differentiable=False):
    """float64 [R, B, 3] partial sums of (x, y) over resolutions [(n_fft, hop, win_length, window)].
    ``differentiable``: the sums carry the gradient with respect to x when x requires grad."""
    x, y = _signal(x, "x", differentiable), _signal(y, "y")
    if x.shape != y.shape:
        raise ValueError(f"x and y must have the same shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise _native.NativeError(f"x and y live on different devices ({x.device}, {y.device})")
    tables = [_table_for(x, nf, wl, w) for nf, _, wl, w in resolutions]
    geometry = ([r[0] for r in resolutions], [r[1] for r in resolutions], [r[2] for r in resolutions])
    if differentiable and x.requires_grad and torch.is_grad_enabled():
        return _DistanceSums.apply(x, y, geometry, *tables)
    return _native.stft_distance(x, y, tables, *geometry)


_counts_on_device = {}     # (device, geometry, n) -> _counts there


def _counts(resolutions, n):
    """frames * bins per utterance for each resolution, float64 [R]."""
    return torch.tensor([(1 + n // hop) * (nf // 2 + 1) for nf, hop, _, _ in resolutions], dtype=torch.float64)


def _counts_on(device, resolutions, n):
    """``_counts`` on ``device``, uploaded once per geometry and length: the copy comes from pageable memory and waits for
    the stream, which made every call of the loss a host synchronisation (tests/test_gpu_stft_loss_grad.py's stream
    test, behind a busy stream, was inconclusive for it)."""
    key = (torch.device(device), tuple((int(nf), int(hop)) for nf, hop, _, _ in resolutions), int(n))
    hit = _counts_on_device.get(key)
    if hit is None:
        if len(_counts_on_device) >= 256:
            _counts_on_device.clear()
        hit = _counts_on_device[key] = _counts(resolutions, n).to(device)
    return hit


def _batch_terms(sums, counts):
    """(sc, mag) 0-d fp32 tensors, the reference's batch-level terms averaged over the resolutions."""
    tot = sums.sum(dim=1)                                      # [R, 3]
    B = sums.shape[1]
    sc = tot[:, 0].sqrt() / tot[:, 1].sqrt()
    mag = tot[:, 2] / (B * counts)
    return sc.mean().float(), mag.mean().float()


def _utterance_terms(sums, counts):
    """[B, 2] fp32: (sc, mag) of every row on its own, averaged over the resolutions."""
    sc = sums[:, :, 0].sqrt() / sums[:, :, 1].sqrt()            # [R, B]
    mag = sums[:, :, 2] / counts[:, None]
    return torch.stack([sc.mean(dim=0), mag.mean(dim=0)], dim=1).float()


class SpectralConvergenceLoss(torch.nn.Module):
    """||Y - X||_F / ||Y||_F on given magnitudes (stft_loss.py:42-60); small torch reductions, kept for the
    reference's module tree.  STFTLoss does not go through it."""

    def forward(self, x_mag, y_mag):
        return torch.norm(y_mag - x_mag, p="fro") / torch.norm(y_mag, p="fro")


class LogSTFTMagnitudeLoss(torch.nn.Module):
    """mean |log Y - log X| on given magnitudes (stft_loss.py:63-80)."""

    def forward(self, x_mag, y_mag):
        return torch.nn.functional.l1_loss(torch.log(y_mag), torch.log(x_mag))


class STFTLoss(torch.nn.Module):
    """One resolution of the reference's STFT loss (stft_loss.py:83-121).  ``differentiable`` (default False)
    switches the gradient with respect to x on."""

    differentiable = False

    def __init__(self, fft_size=1024, shift_size=120, win_length=600, window="hann_window"):
        super().__init__()
        _stft_table_host(fft_size, win_length, window)          # refuse unsupported parameters up front
        if int(shift_size) < 1:
            raise _native.NativeError(f"stft: hop must be >= 1, got {shift_size}")
        self.fft_size = fft_size
        self.shift_size = shift_size
        self.win_length = win_length
        self.window_name = window
        self.spectral_convergence_loss = SpectralConvergenceLoss()
        self.log_stft_magnitude_loss = LogSTFTMagnitudeLoss()
        self.register_buffer("window", _window_fn(window)(win_length))

    def resolution(self):
        return (int(self.fft_size), int(self.shift_size), int(self.win_length), self.window_name)

    def partial_sums(self, x, y):
        """float64 [1, B, 3]: S_diff, S_ref, S_log per row (include/fastvocoder_hip.h fv_stft_distance)."""
        return _sums(x, y, [self.resolution()], self.differentiable)

    def forward(self, x, y):
        """x predicted, y ground truth, both (B, T) -> (sc_loss, mag_loss), 0-d fp32 device tensors."""
        sums = self.partial_sums(x, y)
        return _batch_terms(sums, _counts_on(sums.device, [self.resolution()], x.shape[-1]))

    def per_utterance(self, x, y):
        """[B, 2] fp32 device tensor: (sc_loss, mag_loss) of each row as if scored alone."""
        sums = self.partial_sums(x, y)
        return _utterance_terms(sums, _counts_on(sums.device, [self.resolution()], x.shape[-1]))


class MultiResolutionSTFTLoss(torch.nn.Module):
    """The reference's multi-resolution STFT loss (stft_loss.py:124-155): all resolutions in one call.
    ``differentiable`` (default False) switches the gradient with respect to x on, here and in the STFTLoss
    children."""

    def __init__(self, fft_sizes=[2048, 1024, 512], hop_sizes=[240, 120, 50], win_lengths=[1200, 600, 240],
                 window="hann_window"):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.stft_losses = torch.nn.ModuleList()
        for fs, ss, wl in zip(fft_sizes, hop_sizes, win_lengths):
            self.stft_losses += [STFTLoss(fs, ss, wl, window)]

    @property
    def differentiable(self):
        return all(f.differentiable for f in self.stft_losses)

    @differentiable.setter
    def differentiable(self, value):
        for f in self.stft_losses:
            f.differentiable = bool(value)

    def resolutions(self):
        return [f.resolution() for f in self.stft_losses]

    def partial_sums(self, x, y):
        """float64 [R, B, 3]: S_diff, S_ref, S_log per resolution and row, from one fv_stft_distance call."""
        return _sums(x, y, self.resolutions(), self.differentiable)

    def forward(self, x, y):
        """x predicted, y ground truth, both (B, T) -> (sc_loss, mag_loss), 0-d fp32 device tensors with the
        reference's batch-level semantics, averaged over the resolutions."""
        sums = self.partial_sums(x, y)
        return _batch_terms(sums, _counts_on(sums.device, self.resolutions(), x.shape[-1]))

    def per_utterance(self, x, y):
        """[B, 2] fp32 device tensor: (sc_loss, mag_loss) of each row as if scored alone (B = 1), from the same
        partial sums as ``forward``."""
        sums = self.partial_sums(x, y)
        return _utterance_terms(sums, _counts_on(sums.device, self.resolutions(), x.shape[-1]))
