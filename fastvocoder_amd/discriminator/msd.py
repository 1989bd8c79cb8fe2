"""MelGAN discriminators (reference: model/discriminator/msd.py) on the MI355X."""
import torch

from .. import _native
from .common import (ConvStack, DiscriminatorModule, check_activation, check_pad, checked_input, first_length,
                     wants_grad)


class _AvgPool(torch.autograd.Function):
    """fv_avg_pool1d with its adjoint fv_avg_pool1d_input_grad."""

    @staticmethod
    def forward(ctx, x, pool):
        ctx.pool, ctx.tin = pool, x.shape[-1]
        return _native.avg_pool1d(x, *pool)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _native.avg_pool1d_input_grad(g.to(torch.float32).contiguous(), ctx.tin, *ctx.pool), None


class MelGANDiscriminator(ConvStack):
    """msd.py:13-118: reflect-padded Conv1d(1 -> channels, prod(kernel_sizes)), grouped strided downsamples
    (k = 10 s + 1, groups = in_chs // 4), Conv1d(k0) and Conv1d(k1 -> 1); LeakyReLU after all but the last.
    ``differentiable``: see ConvStack (the gradient with respect to x; the parameters' ``.grad`` stays None).
    ``parameter_grad``: see ConvStack (the gradient of the conv parameters, csrc/disc_wgrad.hip)."""

    def __init__(self, in_channels=1, out_channels=1, kernel_sizes=[5, 3], channels=16, max_downsample_channels=1024,
                 bias=True, downsample_scales=[4, 4, 4, 4], nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, pad="ReflectionPad1d", pad_params={}):
        super().__init__()
        if in_channels != 1 or out_channels != 1:
            raise NotImplementedError(f"MelGANDiscriminator: in_channels={in_channels} out_channels={out_channels} "
                                      "(the discriminator path supports 1 and 1)")
        slope = check_activation(nonlinear_activation, nonlinear_activation_params)
        check_pad(pad, pad_params)
        self._build_stack(in_channels, out_channels, kernel_sizes, channels, max_downsample_channels, bias,
                          downsample_scales, slope, lambda s: s * 10 + 1, pad, pad_params)

    def min_length(self):
        """Shortest input the reflection pad accepts (more samples than the pad)."""
        return self._first_pad + 1

    def _forward(self, x, graph, params=None):
        """x (B, 1, T) -> list of every layer's output.  ``params``: the parameters' graph (None: as the
        ``parameter_grad`` attribute says)."""
        x = checked_input(self, x, 3, graph)
        return self._stack(x, wants_grad(x, graph), self.parameter_grad if params is None else params)

    def _param_forward(self, x):
        """``forward`` on the parameters' graph whatever ``parameter_grad`` says (loss.discriminator_step_terms)."""
        return self._forward(x, self.differentiable, True)


class MelGANMultiScaleDiscriminator(DiscriminatorModule):
    """msd.py:121-241: ``scales`` MelGANDiscriminators, the input average-pooled between scales; weight norm applied
    and the weights re-drawn from N(0, 0.02) at construction, as in the reference."""

    _RESET_STD = 0.02   # msd.py:240

    def __init__(self, in_channels=1, out_channels=1, scales=3, downsample_pooling="AvgPool1d",
                 downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 1, "count_include_pad": False},
                 kernel_sizes=[5, 3], channels=16, max_downsample_channels=1024, bias=True,
                 downsample_scales=[4, 4, 4, 4], nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, pad="ReflectionPad1d", pad_params={},
                 use_weight_norm=True):
        super().__init__()
        pp = dict(downsample_pooling_params)
        if downsample_pooling != "AvgPool1d" or pp.get("count_include_pad", True) or pp.get("ceil_mode", False) \
                or pp.get("divisor_override") is not None:
            raise NotImplementedError(f"pooling {downsample_pooling}{downsample_pooling_params}: the pool kernel is "
                                      "AvgPool1d with count_include_pad=False and ceil_mode=False")
        self.discriminators = torch.nn.ModuleList()
        for _ in range(scales):
            self.discriminators += [MelGANDiscriminator(
                in_channels=in_channels, out_channels=out_channels, kernel_sizes=kernel_sizes, channels=channels,
                max_downsample_channels=max_downsample_channels, bias=bias, downsample_scales=downsample_scales,
                nonlinear_activation=nonlinear_activation, nonlinear_activation_params=nonlinear_activation_params,
                pad=pad, pad_params=pad_params)]
        self.pooling = getattr(torch.nn, downsample_pooling)(**downsample_pooling_params)
        k = pp["kernel_size"]
        self._pool = (k, pp.get("stride") or k, pp.get("padding", 0))
        if use_weight_norm:
            self.apply_weight_norm()
        self.reset_parameters()

    @property
    def differentiable(self):
        """True when every scale carries the gradient with respect to its input (ConvStack.differentiable); setting
        it sets every scale.  The pool between the scales then runs through its own autograd Function, and the
        gradient of x is the sum over the scales."""
        return all(d.differentiable for d in self.discriminators)

    @differentiable.setter
    def differentiable(self, value):
        for d in self.discriminators:
            d.differentiable = bool(value)

    @property
    def parameter_grad(self):
        """True when every scale carries the gradient of its parameters (ConvStack.parameter_grad); setting it sets
        every scale."""
        return all(d.parameter_grad for d in self.discriminators)

    @parameter_grad.setter
    def parameter_grad(self, value):
        for d in self.discriminators:
            d.parameter_grad = bool(value)

    def _pooled_length(self, n):
        k, s, p = self._pool
        return (n + 2 * p - k) // s + 1

    def min_length(self):
        """Shortest input for which every scale's input is longer than its reflection pad."""
        def ok(n):
            for i, d in enumerate(self.discriminators):
                if n < d.min_length():
                    return False
                if i + 1 < len(self.discriminators):
                    n = self._pooled_length(n)
            return True
        return first_length(ok)

    def _forward(self, x, graph, params=None):
        """x (B, 1, T) -> list over the scales of each scale's list of layer outputs.  The scales run as ``_stack``,
        without their own input checks: min_length() above already guarantees every pooled length, and
        ``differentiable`` is "all scales" -- with only some set, an x that requires grad is refused right here.
        ``params``: the parameters' graph for every scale (None: as each scale's ``parameter_grad`` says)."""
        x = checked_input(self, x, 3, graph)
        grad = wants_grad(x, graph)
        outs = []
        for i, f in enumerate(self.discriminators):
            outs += [f._stack(x, grad, f.parameter_grad if params is None else params)]
            if i + 1 < len(self.discriminators):
                x = _AvgPool.apply(x, self._pool) if grad else _native.avg_pool1d(x, *self._pool)
        return outs

    def _param_forward(self, x):
        """``forward`` on the parameters' graph whatever ``parameter_grad`` says (loss.discriminator_step_terms)."""
        return self._forward(x, self.differentiable, True)
