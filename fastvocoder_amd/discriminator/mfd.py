"""Multi-resolution STFT discriminators (reference: model/discriminator/mfd.py) on the MI355X."""
import torch

from .. import _native
from ..loss.stft_loss import _stft_table_host, _window_fn
from .common import (ConvStack, DiscriminatorModule, NotDifferentiable, cached, check_activation, check_pad,
                     checked_input, wants_grad)


class _MagnitudeBins(torch.autograd.Function):
    """fv_stft_magnitude_bins with its adjoint fv_stft_magnitude_bins_grad.  Saves the signal only: the backward
    recomputes the spectrum (the forward's FFT code, so the clamp decisions are the forward's)."""

    @staticmethod
    def forward(ctx, x, table, geometry):
        ctx.table, ctx.geometry = table, geometry
        ctx.save_for_backward(x)
        return _native.stft_magnitude_bins(x, table, *geometry)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return _native.stft_magnitude_bins_grad(x, g.to(torch.float32).contiguous(), ctx.table, *ctx.geometry), \
            None, None


class STFTDiscriminator(NotDifferentiable, ConvStack):
    """mfd.py:44-136: the clamped STFT magnitude (B, bins, frames) -- bins as channels, no transpose -- then a conv
    stack: reflect-padded Conv1d(bins -> channels, prod(kernel_sizes)), grouped strided downsamples (k = 6 s + 1),
    Conv1d(k0), Conv1d(k1 -> 1).  Weight norm is applied at construction, as in the reference.  The window is the
    registered buffer ``window`` (its loaded values are used)."""

    def __init__(self, fft_size=1024, shift_size=120, win_length=600, window="hann_window", out_channels=1,
                 kernel_sizes=[5, 3], channels=64, max_downsample_channels=1024, bias=True, downsample_scales=[4, 4],
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2},
                 pad="ReflectionPad1d", pad_params={}):
        super().__init__()
        if out_channels != 1:
            raise NotImplementedError(f"STFTDiscriminator: out_channels={out_channels} (the discriminator path "
                                      "supports 1)")
        if fft_size not in (512, 1024, 2048) or int(shift_size) < 1 or not 1 <= win_length <= fft_size:
            raise NotImplementedError(f"STFTDiscriminator: fft_size={fft_size} shift_size={shift_size} "
                                      f"win_length={win_length} (the FFT kernel takes n_fft 512, 1024 or 2048)")
        slope = check_activation(nonlinear_activation, nonlinear_activation_params)
        check_pad(pad, pad_params)
        self.fft_size = fft_size
        self.shift_size = shift_size
        self.win_length = win_length
        self.register_buffer("window", _window_fn(window)(win_length))
        self._build_stack(fft_size // 2 + 1, out_channels, kernel_sizes, channels, max_downsample_channels, bias,
                          downsample_scales, slope, lambda s: s * 6 + 1, pad, pad_params)
        self.apply_weight_norm()

    def min_length(self):
        """Shortest input: the STFT's reflect pad needs n > fft_size / 2, the first conv's more frames than its pad."""
        return max(self.fft_size // 2 + 1, self._first_pad * self.shift_size)

    def _table(self):
        return cached(self, "table", lambda: torch.from_numpy(
            _stft_table_host(self.fft_size, self.win_length, self.window)).to(self._device()))

    def _forward(self, x, graph):
        """x (B, T) -> list of every layer's output (the reference's STFTDiscriminator takes the squeezed signal).  On
        the graph the magnitude runs through _MagnitudeBins and the stack through _LayersGrad."""
        x = checked_input(self, x, 2, graph, mono=False)
        grad = wants_grad(x, graph)
        geometry = (self.fft_size, self.shift_size, self.win_length)
        mag = _MagnitudeBins.apply(x, self._table(), geometry) if grad else \
            _native.stft_magnitude_bins(x, self._table(), *geometry)
        return self._stack(mag, grad)

    def _param_forward(self, x):
        """``forward`` on the parameters' graph (loss.discriminator_step_terms(..., stft_grad=True)): the clamped
        magnitude is a constant of the parameters, the stack runs through _LayersParamGrad (ConvStack._param_grad,
        csrc/disc_wgrad.hip) -- the launches and bits of the plain forward."""
        x = checked_input(self, x, 2, False, mono=False)
        mag = _native.stft_magnitude_bins(x, self._table(), self.fft_size, self.shift_size, self.win_length)
        return self._stack(mag, False, True)


class MultiResolutionSTFTDiscriminator(NotDifferentiable, DiscriminatorModule):
    """mfd.py:139-178: one STFTDiscriminator per (fft_size, hop_size, win_length)."""

    def __init__(self, fft_sizes=[2048, 1024, 512], hop_sizes=[240, 120, 50], win_lengths=[1200, 600, 240],
                 window="hann_window", downsample_pooling="AvgPool1d",
                 downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 1, "count_include_pad": False}):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.stft_discriminator = torch.nn.ModuleList()
        for fs, ss, wl in zip(fft_sizes, hop_sizes, win_lengths):
            self.stft_discriminator += [STFTDiscriminator(fft_size=fs, shift_size=ss, win_length=wl, window=window)]

    def min_length(self):
        return max(d.min_length() for d in self.stft_discriminator)

    def _forward(self, x, graph):
        """x (B, 1, T) -> list over the resolutions of each one's list of layer outputs; on the graph autograd sums
        the resolutions' gradients into x."""
        x = checked_input(self, x, 3, graph).squeeze(1)
        return [f._forward(x, graph) for f in self.stft_discriminator]

    def _param_forward(self, x):
        """``_forward`` with every resolution on its parameters' graph (loss.discriminator_step_terms), in the order
        of the list; the resolutions share no parameter."""
        x = checked_input(self, x, 3, False).squeeze(1)
        return [f._param_forward(x) for f in self.stft_discriminator]
