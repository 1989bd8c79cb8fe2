"""What the discriminators share: the argument checks, the cache of packed weights (``cached``), the one forward path
(``DiscriminatorModule``: ``forward`` and ``_graph_forward`` over a module's ``_forward(x, graph)``), the autograd
Functions of a layer stack (``_LayersGrad``: the input gradient; ``_LayersParamGrad``: the parameters' gradient, and
the input's when asked for) and the native run of one conv stack.

A sub-discriminator keeps its convs in the reference's containers (``layers.<i>`` Sequentials of pad / Conv1d /
LeakyReLU) so that ``state_dict`` keys match; their ``forward`` is never called.  ``ConvStack`` folds weight norm and
packs the dense convs once (engine.effective_weight on the GPU, _native.pack_conv1d), caches the result against the
module state (engine.NativeModule._fv_state: identity and version of every parameter and buffer), and runs the stack
as one launch per layer."""
import numpy as np
import torch

from .. import _native
from ..generator.engine import (PAD_REFLECT, PAD_ZERO, NativeModule, cached, conv_params, effective_weight,  # noqa: F401
                                param_store, param_wants)


def check_activation(nonlinear_activation, nonlinear_activation_params):
    if nonlinear_activation != "LeakyReLU":
        raise NotImplementedError(f"activation {nonlinear_activation}: the discriminator kernels fuse LeakyReLU only")
    return float(nonlinear_activation_params.get("negative_slope", 0.01))


def check_pad(pad, pad_params):
    if pad != "ReflectionPad1d" or pad_params:
        raise NotImplementedError(f"padding {pad}{pad_params}: the discriminator kernels fuse ReflectionPad1d only")


def check_grouped(in_chs):
    if in_chs < 4 or in_chs % 4:
        raise NotImplementedError(f"a downsample layer with {in_chs} input channels: groups = in_chs // 4 must give "
                                  "4 input channels per group (in_chs a multiple of 4)")


def device_input(x, name, dims, differentiable=False):
    """x as a contiguous fp32 device tensor of rank ``dims``, or a clear error (the checks of fastvocoder_amd.loss).
    ``differentiable``: x may require grad (the module's ``differentiable`` attribute is set)."""
    if not torch.is_tensor(x):
        raise TypeError(f"{name} must be a tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise _native.NativeError(f"{name} lives on {x.device}; the discriminators run on the ROCm device "
                                  "(there is no CPU path in fastvocoder_amd)")
    if x.requires_grad and torch.is_grad_enabled() and not differentiable:
        raise RuntimeError(f"{name} requires grad: the fastvocoder_amd discriminators are inference-only (forward, no "
                           "autograd); call them under torch.no_grad() or pass a detached tensor")
    if x.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimensions, got shape {tuple(x.shape)}")
    if not x.is_floating_point():
        raise TypeError(f"{name} must be a floating-point signal, got {x.dtype}")
    return x.to(torch.float32).contiguous()


def check_length(module, n):
    need = module.min_length()
    if n < need:
        raise ValueError(f"{type(module).__name__}: an input of {n} samples is too short; its reflection pads need at "
                         f"least {need} samples")


def checked_input(module, x, dims, graph, mono=True):
    """What every ``_forward`` starts with: device_input (``graph``: x may require grad), the (B, 1, T) check of a
    waveform (``mono``) and check_length."""
    x = device_input(x, "x", dims, graph)
    if mono and x.shape[1] != 1:
        raise ValueError(f"x must be (B, 1, T), got {tuple(x.shape)}")
    check_length(module, x.shape[-1])
    return x


def wants_grad(x, graph):
    """Whether a ``_forward`` runs through the autograd Functions: the caller permits it and autograd asks for it."""
    return bool(graph) and x.requires_grad and torch.is_grad_enabled()


def first_length(ok, start=1):
    """Smallest n >= start with ok(n), for ok monotone in n."""
    hi = max(start, 1)
    while not ok(hi):
        hi *= 2
    lo = max(start, hi // 2)
    while lo < hi:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


class NotDifferentiable:
    """Mix-in of the modules without an input gradient: ``differentiable`` reads False, and setting it raises.
    ``parameter_grad`` behaves the same way: the parameter gradient of these modules (the STFT discriminators, the
    period discriminators, Discriminator()) is opt-in per call, through
    fastvocoder_amd.loss.discriminator_step_terms with its keywords stft_grad=True / period_grad=True, never through
    an attribute."""

    @property
    def parameter_grad(self):
        return False

    @parameter_grad.setter
    def parameter_grad(self, value):
        if value:
            raise NotImplementedError(
                f"{type(self).__name__} has no parameter gradient yet: parameter_grad is supported by the MelGAN "
                "multi-scale discriminator only (MelGANDiscriminator, MelGANMultiScaleDiscriminator)")

    @property
    def differentiable(self):
        return False

    @differentiable.setter
    def differentiable(self, value):
        if value:
            raise NotImplementedError(
                f"{type(self).__name__} is not differentiable through this attribute: only the MelGAN multi-scale "
                "discriminator (MelGANDiscriminator, MelGANMultiScaleDiscriminator) takes it.  The generator-side "
                "gradient through the STFT discriminators and Discriminator() comes from "
                "fastvocoder_amd.loss.generator_adversarial_terms, for the period convs of the MPD with its keyword "
                "period_grad=True")


class _LayersGrad(torch.autograd.Function):
    """``module._run_layers`` with the gradient with respect to the input: the outputs are all the layer maps, the
    saved tensors the input and the maps.  The parameters are constants."""

    @staticmethod
    def forward(ctx, module, x):
        outs = module._run_layers(x)
        ctx.module = module
        ctx.set_materialize_grads(module._MATERIALIZE_GRADS)
        ctx.save_for_backward(x, *outs)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        x, *outs = ctx.saved_tensors
        return None, ctx.module._input_grad(x, outs, grads)


class _LayersParamGrad(torch.autograd.Function):
    """``module._run_layers`` with the conv parameters as inputs of the graph: the same forward launches as
    _LayersGrad, the backward ``module._param_grad`` (csrc/disc_wgrad.hip), which also hands down the input gradient
    when x requires grad.  A map without a gradient arrives as None and costs no launch."""

    @staticmethod
    def forward(ctx, module, x, *params):
        outs = module._run_layers(x)
        ctx.module, ctx.n_outs = module, len(outs)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, *outs, *params)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        x, *rest = ctx.saved_tensors
        outs, params = rest[:ctx.n_outs], rest[ctx.n_outs:]
        gx, gparams = ctx.module._param_grad(x, outs, params, grads, ctx.needs_input_grad[1],
                                             ctx.needs_input_grad[2:])
        return (None, gx) + tuple(gparams)


class DiscriminatorModule(NativeModule):
    """Base of every discriminator: one ``_forward(x, graph)`` per module, ``graph`` the permission for x to require
    grad (then the launches run through the autograd Functions: the same launches, the same bits)."""

    def forward(self, x):
        return self._forward(x, self.differentiable)

    def _graph_forward(self, x):
        """``forward`` on the graph of x whatever ``differentiable`` says (loss.generator_adversarial_terms)."""
        return self._forward(x, True)

    def _conv_params(self):
        """Per layer (``_convs()``) the conv's parameters in the order _LayersParamGrad takes them: (weight_g,
        weight_v[, bias]) under weight norm, (weight[, bias]) without."""
        return [conv_params(conv) for conv in self._convs()]

    def _stack(self, x, grad, params=False):
        """``_run_layers(x)`` of a module with layers of its own: on the parameters' graph (_LayersParamGrad, backward
        the module's ``_param_grad``) when ``params`` and grad is enabled and a conv parameter requires grad; else
        through _LayersGrad (backward: the module's ``_input_grad``) when ``grad``."""
        if params and torch.is_grad_enabled():
            flat = [q for ps in self._conv_params() for q in ps]
            if any(q.requires_grad for q in flat):
                return list(_LayersParamGrad.apply(self, x, *flat))
        return list(_LayersGrad.apply(self, x)) if grad else self._run_layers(x)

    def _param_plan(self, need):
        """What both ``_param_grad`` walks start from: (index of each layer's first parameter, whether a parameter of
        the layer is flagged in ``need``)."""
        counts = [len(ps) for ps in self._conv_params()]
        first = [sum(counts[:l]) for l in range(len(counts))]
        return first, [any(need[first[l]:first[l] + counts[l]]) for l in range(len(counts))]

    # (engine.param_wants / engine.param_store: shared with the generators' parameter gradient)
    _param_wants = staticmethod(param_wants)
    _param_store = staticmethod(param_store)


class ConvStack(DiscriminatorModule):
    """Base of the two sub-discriminators: ``layers`` as in the reference, ``_spec`` one entry per layer.

    ``differentiable`` (default False): with True, a forward whose input requires grad runs the same launches through
    an autograd Function (the same bits) whose backward is the input gradient of csrc/disc_grad.hip.  The parameters
    are constants of that graph: their ``.grad`` stays None.

    ``parameter_grad`` (default False): with True, grad enabled and at least one conv parameter requiring grad, the
    same launches run through _LayersParamGrad, whose inputs are the conv parameters: autograd accumulates into the
    ``.grad`` of ``weight_g`` / ``weight_v`` / ``bias`` (``weight`` without weight norm) from the kernels of
    csrc/disc_wgrad.hip.  A frozen parameter gets no gradient and costs no launch.  An x that requires grad still
    needs ``differentiable``."""

    differentiable = False
    parameter_grad = False
    _MATERIALIZE_GRADS = True     # a map without a gradient arrives as zeros: _input_grad launches for every layer

    def _build_stack(self, in_channels, out_channels, kernel_sizes, channels, max_downsample_channels, bias,
                     downsample_scales, slope, tap, pad_name, pad_params):
        """The reference's layer list (msd.py:54-103, mfd.py:76-121); ``tap(s)`` = the downsample kernel of scale s."""
        assert len(kernel_sizes) == 2
        assert kernel_sizes[0] % 2 == 1
        assert kernel_sizes[1] % 2 == 1
        act = lambda: torch.nn.LeakyReLU(slope)  # noqa: E731
        k0 = int(np.prod(kernel_sizes))
        self.layers = torch.nn.ModuleList()
        self.layers += [torch.nn.Sequential(getattr(torch.nn, pad_name)((k0 - 1) // 2, **pad_params),
                                            torch.nn.Conv1d(in_channels, channels, k0, bias=bias), act())]
        spec = [("dense", k0, (k0 - 1) // 2, PAD_REFLECT, slope)]
        in_chs = channels
        for s in downsample_scales:
            check_grouped(in_chs)
            out_chs = min(in_chs * s, max_downsample_channels)
            k = tap(s)
            self.layers += [torch.nn.Sequential(
                torch.nn.Conv1d(in_chs, out_chs, kernel_size=k, stride=s, padding=(k - 1) // 2, groups=in_chs // 4,
                                bias=bias), act())]
            spec.append(("grouped", k, (k - 1) // 2, s, slope))
            in_chs = out_chs
        out_chs = min(in_chs * 2, max_downsample_channels)
        self.layers += [torch.nn.Sequential(
            torch.nn.Conv1d(in_chs, out_chs, kernel_sizes[0], padding=(kernel_sizes[0] - 1) // 2, bias=bias), act())]
        spec.append(("dense", kernel_sizes[0], (kernel_sizes[0] - 1) // 2, PAD_ZERO, slope))
        self.layers += [torch.nn.Conv1d(out_chs, out_channels, kernel_sizes[1], padding=(kernel_sizes[1] - 1) // 2,
                                        bias=bias)]
        spec.append(("dense", kernel_sizes[1], (kernel_sizes[1] - 1) // 2, PAD_ZERO, 1.0))
        self._spec = spec
        self._first_pad = (k0 - 1) // 2

    def _convs(self):
        out = []
        for layer in self.layers:
            if isinstance(layer, torch.nn.Conv1d):
                out.append(layer)
            else:
                out.append(next(m for m in layer if isinstance(m, torch.nn.Conv1d)))
        return out

    def _native_layers(self):
        """[(spec, weight, bias)] with weight norm folded (grouped: [Cout, 4, k]; dense: packed), cached against the
        module state."""
        def build():
            layers = []
            for spec, conv in zip(self._spec, self._convs()):
                w = effective_weight(conv)
                b = None if conv.bias is None else conv.bias.detach().contiguous().float()
                layers.append((spec, w.contiguous() if spec[0] == "grouped" else _native.pack_conv1d(w), b,
                               conv.out_channels))
            return layers
        return cached(self, "layers", build)

    def _native_grad_layers(self):
        """Per layer what its input gradient reads: the folded weight [Cout, 4, k] of a grouped layer (the forward's
        tensor), the packed W'[ci, co, j] = W[co, ci, k-1-j] of a dense one.  Cached against the module state."""
        def build():
            layers = []
            for (spec, w, _, _), conv in zip(self._native_layers(), self._convs()):
                if spec[0] != "grouped":
                    w = _native.pack_conv1d(effective_weight(conv).flip(2).transpose(0, 1).contiguous())
                layers.append((spec, w, conv.in_channels))
            return layers
        return cached(self, "grad_layers", build)

    def _param_grad(self, x, outs, params, grads, need_x, need):
        """The backward of _LayersParamGrad, walking the layers downwards: per layer g_pre once (fv_disc_map_grad), the
        weight and bias gradient from g_pre and the layer's stored input, the weight-norm adjoint, and the data
        gradient for the layer below with the kernels of _input_grad.  ``need``: one flag per entry of ``params``; the
        walk ends at the lowest layer with a flagged parameter unless ``need_x``.  -> (gx or None, [gradient or None
        per parameter])."""
        layers = self._native_grad_layers()
        convs = self._convs()
        first, wanted = self._param_plan(need)
        stop = 0 if need_x else min([l for l, w in enumerate(wanted) if w], default=len(layers))
        out = [None] * len(params)
        g_up = None
        for l in range(len(layers) - 1, stop - 1, -1):
            spec, w, cin = layers[l]
            g_map = None if grads[l] is None else grads[l].to(torch.float32).contiguous()
            if g_up is None and g_map is None:
                continue
            xin = outs[l - 1] if l else x
            slope = spec[4]
            if slope != 1.0 or (g_up is not None and g_map is not None):
                g_pre = _native.disc_map_grad(g_up, g_map, outs[l] if slope != 1.0 else None, slope)
            else:
                g_pre = g_up if g_up is not None else g_map
            if wanted[l]:
                conv, at = convs[l], first[l]
                want_dw, want_db = self._param_wants(conv, need, at)
                if spec[0] == "grouped":
                    dw, db = _native.grouped_conv1d_weight_grad(g_pre, xin, spec[1], spec[3], spec[2], want_dw, want_db)
                else:
                    dw, db = _native.conv1d_weight_grad(g_pre, xin, spec[1], spec[2], spec[3], want_dw, want_db)
                self._param_store(conv, params, need, at, dw, db, out)
            if l == stop and not need_x:
                break
            tin = xin.shape[-1]
            if spec[0] == "grouped":
                _, k, pad, stride, _ = spec
                g_up = _native.grouped_conv1d_input_grad(g_pre, None, None, w, cin, tin, k, stride, pad, 1.0)
                continue
            _, k, pad, mode, _ = spec
            if mode == PAD_REFLECT:
                g_up = _native.reflect_pad_fold(_native.conv1d_fused(g_pre, w, None, cin, k, pad=k - 1), pad)
            else:
                g_up = _native.conv1d_fused(g_pre, w, None, cin, k, pad=k - 1 - pad)
        gx = None
        if need_x:
            gx = torch.zeros_like(x) if g_up is None else g_up
        return gx, out

    def _input_grad(self, x, outs, grads):
        """d/dx of sum_l <grads[l], outs[l]> (None = zero), walking the layers downwards: the LeakyReLU mask of a
        layer from its stored output, then the layer's data gradient, to which the next map's gradient is added."""
        layers = self._native_grad_layers()
        g_up = None
        for l in range(len(layers) - 1, -1, -1):
            spec, w, cin = layers[l]
            g_map = None if grads[l] is None else grads[l].to(torch.float32).contiguous()
            if g_up is None and g_map is None:
                continue
            tin = (outs[l - 1] if l else x).shape[-1]
            if spec[0] == "grouped":
                _, k, pad, stride, slope = spec
                g_up = _native.grouped_conv1d_input_grad(g_up, g_map, outs[l] if slope != 1.0 else None, w, cin, tin,
                                                         k, stride, pad, slope)
                continue
            _, k, pad, mode, slope = spec
            if slope != 1.0 or (g_up is not None and g_map is not None):
                g_pre = _native.disc_map_grad(g_up, g_map, outs[l] if slope != 1.0 else None, slope)
            else:
                g_pre = g_up if g_up is not None else g_map
            if mode == PAD_REFLECT:      # the gradient of the padded input (pad' = k - 1), folded back onto the input
                g_up = _native.reflect_pad_fold(_native.conv1d_fused(g_pre, w, None, cin, k, pad=k - 1), pad)
            else:
                g_up = _native.conv1d_fused(g_pre, w, None, cin, k, pad=k - 1 - pad)
        return torch.zeros_like(x) if g_up is None else g_up

    def _run_layers(self, x):
        """x [B, C, T] fp32 device -> the list of every layer's output (the reference's ``outs``)."""
        outs = []
        for (spec, w, b, cout) in self._native_layers():
            if spec[0] == "grouped":
                _, k, pad, stride, slope = spec
                x = _native.grouped_conv1d(x, w, b, k, stride, pad, slope)
            else:
                _, k, pad, mode, slope = spec
                x = _native.conv1d_fused(x, w, b, cout, k, pad=pad, pad_mode=mode, act_slope=slope)
            outs.append(x)
        return outs
