"""HiFi-GAN's multi-period discriminator (reference: model/discriminator/mpd.py:131-164, 288-304) on the MI355X.

``DiscriminatorP(p)`` reflect-pads the waveform to a multiple of p, views it as [B, 1, H, p] and runs six weight-normed
Conv2d((k, 1)) layers along H.  Here the first layer reads the raw waveform (fv_mpd_conv_first: pad and view are
address arithmetic), the three strided 32 -> 128 -> 512 -> 1024 layers run on the fp32 matrix cores
(fv_period_conv, csrc/mpd.hip), and the two stride-1 layers are dilated conv1ds on the flattened axis n = h p + c
(fv_conv1d_fused with dilation p and zero padding 2 p / p).  The convs live in the reference's containers
(``convs.<j>``, ``conv_post``) so that ``state_dict`` keys and 4-D shapes match; their ``forward`` is never called.

``grad_precision`` ("f32" | "bf16", on DiscriminatorP and MultiPeriodDiscriminator) is the arithmetic of the weight
gradients on the parameters' graph (loss.discriminator_step_terms(..., period_grad=True)): "bf16" rounds both operands
of layers 1-5 to bf16 (nearest even) and multiplies them on the bf16 matrix cores with fp32 accumulation
(fv_period_conv_weight_grad_bf16, csrc/gen_grad_bf16.hip).  The first layer, every bias gradient, the forwards, the
data gradients, the input gradient of loss.generator_adversarial_terms, the parameters and the optimizer state stay
fp32.  Read at backward time: nothing cached depends on it."""
import torch
from torch.nn.utils import weight_norm

from .. import _native
from ..generator.engine import PAD_ZERO, effective_weight
from .common import DiscriminatorModule, NotDifferentiable, cached, checked_input, first_length, wants_grad

LRELU_SLOPE = 0.1
PERIODS = (2, 3, 5, 7, 11)


def period_heights(T, period, stride=3, layers=4):
    """(n_pad, [H, H_1 .. H_layers]): the reflect tail of T samples and the map heights, H' = (H - 1) // stride + 1."""
    n_pad = _native.mpd_reflect_tail(T, period)
    hs = [(T + n_pad) // period]
    for _ in range(layers):
        hs.append((hs[-1] - 1) // stride + 1)
    return n_pad, hs


def _folded(conv):
    """The weight of a (k, 1) conv with weight norm folded, as [Cout, Cin, k]."""
    w = effective_weight(conv)
    return w.reshape(w.shape[0], w.shape[1], w.shape[2])


class DiscriminatorP(NotDifferentiable, DiscriminatorModule):
    """mpd.py:131-164."""

    _MATERIALIZE_GRADS = False    # a map without a gradient arrives as None: _input_grad skips the layers above it
    _grad_precision = "f32"

    @property
    def grad_precision(self):
        """"f32" (the default) or "bf16": the arithmetic of ``_param_grad``'s weight gradients of layers 1-5."""
        return self._grad_precision

    @grad_precision.setter
    def grad_precision(self, value):
        if value not in _native.GRAD_PRECISIONS:
            raise ValueError(f"{type(self).__name__}.grad_precision: {value!r} ('f32' or 'bf16')")
        self._grad_precision = value

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False):
        super().__init__()
        if use_spectral_norm:
            raise NotImplementedError("DiscriminatorP(use_spectral_norm=True): the period convs fold weight norm only "
                                      "(the reference's MultiPeriodDiscriminator never asks for spectral norm)")
        if kernel_size != 5 or stride != 3:
            raise NotImplementedError(f"DiscriminatorP(kernel_size={kernel_size}, stride={stride}): the period conv "
                                      "kernel has 5 taps and stride 3, the reference's only configuration")
        if period not in PERIODS:
            raise NotImplementedError(f"DiscriminatorP(period={period}): the period conv kernel is built for periods "
                                      f"{PERIODS}")
        self.period = period
        conv = torch.nn.Conv2d
        self.convs = torch.nn.ModuleList([
            weight_norm(conv(1, 32, (kernel_size, 1), (stride, 1), padding=(2, 0))),
            weight_norm(conv(32, 128, (kernel_size, 1), (stride, 1), padding=(2, 0))),
            weight_norm(conv(128, 512, (kernel_size, 1), (stride, 1), padding=(2, 0))),
            weight_norm(conv(512, 1024, (kernel_size, 1), (stride, 1), padding=(2, 0))),
            weight_norm(conv(1024, 1024, (kernel_size, 1), 1, padding=(2, 0))),
        ])
        self.conv_post = weight_norm(conv(1024, 1, (3, 1), 1, padding=(1, 0)))

    def min_length(self):
        """Shortest T whose reflect tail (period - T % period samples) is shorter than T, as torch's pad demands."""
        p = self.period
        return first_length(lambda n: all(_native.mpd_reflect_tail(t, p) < t for t in range(n, max(n, p) + 1)))

    def _convs(self):
        return list(self.convs) + [self.conv_post]

    def _native_layers(self):
        """[(weight, bias)]: layer 0 folded [32, 5]; layers 1-3 packed for fv_period_conv; layers 4-5 packed for
        fv_conv1d_fused.  Cached against the module state."""
        def build():
            layers = []
            for j, conv in enumerate(self._convs()):
                w = _folded(conv)
                b = None if conv.bias is None else conv.bias.detach().contiguous().float()
                if j == 0:
                    w = w.reshape(32, 5).contiguous()
                elif j < 4:
                    w = _native.pack_period_conv(w)
                else:
                    w = _native.pack_conv1d(w)
                layers.append((w, b))
            return layers
        return cached(self, "layers", build)

    def _native_grad_layers(self):
        """Per layer what its input gradient reads: layer 0 the folded weight [32, 5] (the forward's tensor); layers
        1-3 packed for fv_period_conv_input_grad; layers 4-5 the packed W'[ci, co, j] = W[co, ci, k-1-j] of
        fv_conv1d_fused.  Cached against the module state."""
        def build():
            layers = [self._native_layers()[0][0]]
            for j, conv in enumerate(self._convs()[1:], 1):
                w = _folded(conv)
                if j < 4:
                    layers.append(_native.pack_period_conv_grad(w))
                else:
                    layers.append(_native.pack_conv1d(w.flip(2).transpose(0, 1).contiguous()))
            return layers
        return cached(self, "grad_layers", build)

    def _run_layers(self, x):
        """x [B, 1, T] fp32 device -> the six feature maps [B, C, H_l, p]: one launch per layer."""
        p = self.period
        layers = self._native_layers()
        x = _native.mpd_conv_first(x, layers[0][0], layers[0][1], p, LRELU_SLOPE)
        fmap = [x]
        for j in (1, 2, 3):
            x = _native.period_conv(x, layers[j][0], layers[j][1], self.convs[j].out_channels, LRELU_SLOPE)
            fmap.append(x)
        B, C, H, _ = x.shape
        x = _native.conv1d_fused(x.view(B, C, H * p), layers[4][0], layers[4][1], 1024, 5, dil=p, pad=2 * p,
                                 pad_mode=PAD_ZERO, act_slope=LRELU_SLOPE)
        fmap.append(x.view(B, 1024, H, p))
        x = _native.conv1d_fused(x, layers[5][0], layers[5][1], 1, 3, dil=p, pad=p, pad_mode=PAD_ZERO)
        fmap.append(x.view(B, 1, H, p))
        return fmap

    def _input_grad(self, x, outs, grads):
        """d/dx of sum_l <grads[l], outs[l]> (None = zero), walking the six layers downwards: conv_post and the
        dilated 1024 -> 1024 layer as fv_conv1d_fused on flipped, transposed weights behind fv_disc_map_grad, the
        three strided layers as fv_period_conv_input_grad and the first as fv_mpd_first_input_grad, both of which
        apply the LeakyReLU mask of the layer's stored output while they stage the gradient."""
        p = self.period
        layers = self._native_grad_layers()
        gm = [None if g is None else g.to(torch.float32).contiguous() for g in grads]
        B, _, H, _ = outs[5].shape
        g_up = None
        if gm[5] is not None:                              # conv_post: no activation; its map's gradient alone
            g_up = _native.conv1d_fused(gm[5].view(B, 1, H * p), layers[5], None, 1024, 3, dil=p, pad=p,
                                        pad_mode=PAD_ZERO).view(B, 1024, H, p)
        if g_up is not None or gm[4] is not None:
            g_pre = _native.disc_map_grad(g_up, gm[4], outs[4], LRELU_SLOPE)
            g_up = _native.conv1d_fused(g_pre.view(B, 1024, H * p), layers[4], None, 1024, 5, dil=p, pad=2 * p,
                                        pad_mode=PAD_ZERO).view(B, 1024, H, p)
        for j in (3, 2, 1):
            if g_up is None and gm[j] is None:
                continue
            g_up = _native.period_conv_input_grad(g_up, gm[j], outs[j], layers[j], self.convs[j].in_channels,
                                                  outs[j - 1].shape[2], LRELU_SLOPE)
        if g_up is None and gm[0] is None:
            return torch.zeros_like(x)
        return _native.mpd_first_input_grad(g_up, gm[0], outs[0], layers[0], x.shape[-1], LRELU_SLOPE)

    def _param_grad(self, x, outs, params, grads, need_x, need):
        """The backward of _LayersParamGrad, the layer walk of _input_grad: per layer g_pre once (fv_disc_map_grad;
        conv_post has no activation), the weight and bias gradient (fv_period_conv_weight_grad from g_pre and the
        layer's stored input, fv_mpd_first_weight_grad from the waveform; csrc/mpd_wgrad.hip), the weight-norm adjoint
        under ``grad_precision = "bf16"`` fv_period_conv_weight_grad_bf16 for layers 1-5), the weight-norm adjoint
        on the 4-D ``weight_v`` viewed as [Cout, Cin k], and the data gradient for the layer below with the kernels
        of _input_grad.  ``need``: one flag per entry of ``params``; the walk ends at the lowest layer with a flagged
        parameter.  The waveform gets no gradient on this route (``need_x`` is refused: loss.discriminator_step_terms
        detaches the estimate and refuses an input that requires grad).  -> (None, [gradient or None per
        parameter])."""
        if need_x:
            raise NotImplementedError("DiscriminatorP: the parameters' graph carries no input gradient")
        p = self.period
        precision = self.grad_precision                     # read here, at backward time
        layers = self._native_grad_layers()
        convs = self._convs()
        first, wanted = self._param_plan(need)
        stop = min([l for l, w in enumerate(wanted) if w], default=len(convs))
        out = [None] * len(params)
        gm = [None if g is None else g.to(torch.float32).contiguous() for g in grads]
        B, _, H, _ = outs[5].shape
        g_up = None
        for l in range(5, stop - 1, -1):
            if g_up is None and gm[l] is None:
                continue
            if l == 5:
                g_pre = gm[5]
            else:
                g_pre = _native.disc_map_grad(g_up, gm[l], outs[l], LRELU_SLOPE)
            if wanted[l]:
                conv, at = convs[l], first[l]
                want_dw, want_db = self._param_wants(conv, need, at)
                if l == 0:
                    dw, db = _native.mpd_first_weight_grad(g_pre, x, want_dw, want_db)
                else:
                    dw, db = _native.period_conv_weight_grad(g_pre, outs[l - 1], conv.kernel_size[0], conv.stride[0],
                                                             want_dw, want_db, precision=precision)
                self._param_store(conv, params, need, at, dw, db, out)
            if l == stop:
                break
            if l == 5:
                g_up = _native.conv1d_fused(g_pre.view(B, 1, H * p), layers[5], None, 1024, 3, dil=p, pad=p,
                                            pad_mode=PAD_ZERO).view(B, 1024, H, p)
            elif l == 4:
                g_up = _native.conv1d_fused(g_pre.view(B, 1024, H * p), layers[4], None, 1024, 5, dil=p, pad=2 * p,
                                            pad_mode=PAD_ZERO).view(B, 1024, H, p)
            else:
                g_up = _native.period_conv_input_grad(g_pre, None, None, layers[l], convs[l].in_channels,
                                                      outs[l - 1].shape[2], 1.0)
        return None, out

    def _param_forward(self, x):
        """``forward`` on the parameters' graph (loss.discriminator_step_terms(..., period_grad=True)): the launches
        and bits of the plain forward through _LayersParamGrad, whose backward is ``_param_grad``."""
        x = checked_input(self, x, 3, False)
        fmap = self._stack(x, False, True)
        return fmap[5].flatten(1), fmap

    def _forward(self, x, graph):
        """x (B, 1, T) -> (score [B, H_6 p], the six feature maps [B, C, H_l, p]).  On the graph
        (loss.generator_adversarial_terms(..., period_grad=True)) the same launches run through _LayersGrad, whose
        backward is the input gradient of csrc/mpd_grad.hip; the parameters are constants (``.grad`` stays None)."""
        x = checked_input(self, x, 3, graph)
        fmap = self._stack(x, wants_grad(x, graph))
        return fmap[5].flatten(1), fmap


class MultiPeriodDiscriminator(NotDifferentiable, DiscriminatorModule):
    """mpd.py:288-304, the single-input form: one list per period, its six maps followed by the score [B, 1, H p]."""

    def __init__(self):
        super().__init__()
        self.discriminators = torch.nn.ModuleList([DiscriminatorP(p) for p in PERIODS])

    @property
    def grad_precision(self):
        """The five periods' ``grad_precision``: setting it sets all of them; reading it needs them to agree."""
        values = {d.grad_precision for d in self.discriminators}
        if len(values) != 1:
            raise ValueError(f"MultiPeriodDiscriminator.grad_precision: the periods disagree ({sorted(values)})")
        return values.pop()

    @grad_precision.setter
    def grad_precision(self, value):
        if value not in _native.GRAD_PRECISIONS:
            raise ValueError(f"{type(self).__name__}.grad_precision: {value!r} ('f32' or 'bf16')")
        for d in self.discriminators:
            d.grad_precision = value

    def min_length(self):
        """Shortest input every period's reflect pad accepts."""
        return max(d.min_length() for d in self.discriminators)

    def _forward(self, x, graph):
        """The periods in the order of PERIODS.  On the graph autograd adds their gradients into x in the reverse of
        that order (a node built later runs earlier), period 11 first and period 2 last: the same order, hence the
        same bits, on every call."""
        x = checked_input(self, x, 3, graph)
        outs = []
        for d in self.discriminators:
            score, fmap = d._forward(x, graph)
            outs.append(fmap + [score.unsqueeze(1)])
        return outs

    def _param_forward(self, x):
        """``_forward`` with every period on its parameters' graph (loss.discriminator_step_terms), in the order of
        PERIODS; the periods share no parameter, and autograd runs their backward nodes in the reverse of that
        order."""
        x = checked_input(self, x, 3, False)
        outs = []
        for d in self.discriminators:
            score, fmap = d._param_forward(x)
            outs.append(fmap + [score.unsqueeze(1)])
        return outs
