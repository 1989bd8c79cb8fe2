"""MelGAN's training forward and parameter gradient (``MelGANGenerator.stack_grad`` / ``parameter_grad``).

The training forward runs the graph of melgan.py conv by conv on the exact-fp32 entries (_native.conv1d_fused with its
``pad_mode``, _native.conv1d_2src_fused, _native.conv_transpose1d_fused) and keeps what the backward reads.  Per
ResidualStack ``y = P(lrelu(h)) + S(x)``, ``h = D(reflection_pad(lrelu(x)))``: x raw (the skip conv's input) and
lrelu(x) (the dilated conv's), and lrelu(h) (the pointwise conv's).  A LeakyReLU keeps the sign of its input, so the
mask of an activation is read off its OUTPUT: the raw h and the raw tensors in front of the upsamplers and of the last
conv are not kept.  Per upsampler the activated input; the mel; the tanh output.

The backward walks the graph downwards.  Per stack, from g_y = dL/dy: the weight and bias gradients of P and S (k = 1,
fv_conv1d_weight_grad_dilated), g_h = mask(h) P^T g_y, the weight gradient of D through the reflection pad
(fv_conv1d_weight_grad_dilated_mode), and g_x = S^T g_y + mask(x) D^T g_h with D^T through the pad in one launch
(fv_conv1d_input_grad_reflect, fv_residual_merge_grad).  The two k = 7 edge convs sit behind the same pad and use the
same two entries.  Every arithmetic step is a HIP launch; torch allocates.

Folded weights and their packed images are cached against the module state (engine.cached), as generator/grad.py does.
"""
import torch

from .. import _native
from .engine import PAD_REFLECT, POST_NONE, cached, conv_params, effective_weight, param_store, param_wants
from .grad import train_convs
from .modules import LastLayer, ResidualStack


def check_supported(gen):
    """What ``stack_grad = True`` refuses: the graphs whose backward does not exist."""
    name = type(gen).__name__
    if gen._config["use_causal_conv"]:
        raise NotImplementedError(
            f"{name}(use_causal_conv=True): stack_grad needs the backward of CausalConv1d (a two-sided pad whose "
            "output is cut to the input's length), which does not exist yet; the non-causal ResidualStack has one")
    if gen._config["nonlinear_activation"] != "LeakyReLU" or gen._config["pad"] != "ReflectionPad1d":
        raise NotImplementedError(
            f"{name}(nonlinear_activation={gen._config['nonlinear_activation']!r}, pad={gen._config['pad']!r}): "
            "stack_grad exists for LeakyReLU behind ReflectionPad1d only: the data gradient "
            "(fv_conv1d_input_grad_reflect) folds a reflection pad, and the activation masks are read off LeakyReLU "
            "outputs")
    if gen._slope <= 0.0:
        raise NotImplementedError(f"{name}: stack_grad reads the activation masks off the LeakyReLU outputs, which needs "
                                  f"a positive negative_slope, got {gen._slope}")


def _graph(gen):
    """The Sequential as (first conv, [(upsampler, [stacks])], LastLayer); None for a trunk that ends at its last
    ResidualStack (Basis-MelGAN, whose head is generator/basis_grad.py)."""
    mods = list(gen.melgan)
    first = next(m for m in mods if isinstance(m, torch.nn.Conv1d))
    stages = []
    for m in mods:
        if isinstance(m, torch.nn.ConvTranspose1d):
            stages.append((m, []))
        elif isinstance(m, ResidualStack):
            stages[-1][1].append(m)
    return first, stages, next((m for m in mods if isinstance(m, LastLayer)), None)


def _stack_convs(stack):
    dilated, pointwise = (stack.stack[i] for i in stack._conv_at)
    return dilated, pointwise, stack.skip_layer


def _layers(gen):
    """What the launches read.  id(conv) -> (the forward's packed weight, the bias, the data gradient's weight): for a
    conv behind the pad W with its first two axes swapped, for a 1x1 conv the packed transpose, for a
    ConvTranspose1d the folded weight itself.  id(stack) -> the packed [P ; S] and the summed bias of the one-launch
    pointwise + skip."""
    def bias(conv):
        return None if conv.bias is None else conv.bias.detach().contiguous().float()

    def build():
        out = {}
        for conv in train_convs(gen):
            w = effective_weight(conv)
            if isinstance(conv, torch.nn.ConvTranspose1d):
                out[id(conv)] = (_native.pack_conv_transpose1d(w, conv.stride[0], conv.padding[0]), bias(conv),
                                 w.contiguous())
            elif conv.kernel_size[0] == 1:
                out[id(conv)] = (_native.pack_conv1d(w), bias(conv), _native.pack_conv1d(w.transpose(0, 1).contiguous()))
            else:
                out[id(conv)] = (_native.pack_conv1d(w), bias(conv), w.transpose(0, 1).contiguous())
        for stack in (m for m in gen.melgan if isinstance(m, ResidualStack)):
            _, p, s = _stack_convs(stack)
            if stack.channels > 4:                       # the forward plan's condition for the one-launch form
                bp, bs = bias(p), bias(s)
                both = bp if bs is None else (bs if bp is None else (bp + bs).contiguous())
                out[id(stack)] = (_native.pack_conv1d(torch.cat([effective_weight(p), effective_weight(s)],
                                                                dim=1).contiguous()), both)
        return out
    return cached(gen, "stack_train_layers", build)


def _twin(x, cout, tout):
    return torch.empty((x.shape[0], cout, tout), dtype=torch.float32, device=x.device)


def train_forward(gen, mel):
    """mel [B, C, T] fp32 device -> (y [B, out_channels, T'], tape).  Without a LastLayer the graph ends at the last
    ResidualStack's raw output, which is y; its activated twin is not formed."""
    L = _layers(gen)
    slope = gen._slope
    first, stages, last = _graph(gen)
    pad = gen._first_pad[0]
    packed, b, _ = L[id(first)]
    xa = _twin(mel, first.out_channels, mel.shape[2])
    _native.conv1d_fused(mel, packed, b, first.out_channels, first.kernel_size[0], pad=pad, pad_mode=PAD_REFLECT,
                         out_act=xa, act_slope=slope)
    tape = {"mel": mel, "stages": []}
    for up, stacks in stages:
        packed, b, _ = L[id(up)]
        k, s, p, op = up.kernel_size[0], up.stride[0], up.padding[0], up.output_padding[0]
        tout = (xa.shape[2] - 1) * s - 2 * p + k + op
        ya = _twin(xa, up.out_channels, tout)
        y = _native.conv_transpose1d_fused(xa, packed, b, up.out_channels, k, s, p, op, out_act=ya, act_slope=slope)
        stage = {"up_in": xa, "stacks": []}
        for stack in stacks:
            d, pw, sk = _stack_convs(stack)
            ch = stack.channels
            x, xa = y, ya
            ends = last is None and up is stages[-1][0] and stack is stacks[-1]
            packed, b, _ = L[id(d)]
            ha = _twin(x, ch, x.shape[2])
            _native.conv1d_fused(xa, packed, b, ch, d.kernel_size[0], dil=d.dilation[0], pad=stack._pad,
                                 pad_mode=PAD_REFLECT, out_act=ha, act_slope=slope)
            ya = None if ends else _twin(x, ch, x.shape[2])
            if id(stack) in L:
                packed, b = L[id(stack)]
                y = _native.conv1d_2src_fused(ha, x, packed, b, ch, out_act=ya, act_slope=slope)
            else:
                skip = _native.conv1d_fused(x, L[id(sk)][0], L[id(sk)][1], ch, 1)
                y = _native.conv1d_fused(ha, L[id(pw)][0], L[id(pw)][1], ch, 1, res=skip, out_act=ya, act_slope=slope)
            stage["stacks"].append((x, xa, ha))
        stage["ya"] = ya                               # lrelu of the stage's output: the next conv's input
        tape["stages"].append(stage)
        xa = ya
    if last is None:
        return y, tape
    packed, b, _ = L[id(last.conv)]
    out = _native.conv1d_fused(xa, packed, b, last.conv.out_channels, last.conv.kernel_size[0], pad=last._pad,
                               pad_mode=PAD_REFLECT, post=gen._final_post)
    return out, tape


def train_backward(gen, tape, y, params, need, g):
    """g = dL/dy -> one gradient (or None) per entry of ``params`` (the convs' parameters, train_convs order).  Without
    a LastLayer, y is the last ResidualStack's raw output and the walk starts there."""
    L = _layers(gen)
    slope = gen._slope
    first, stages, last = _graph(gen)
    convs = train_convs(gen)
    first_at, at = {}, 0
    for conv in convs:
        first_at[id(conv)] = at
        at += len(conv_params(conv))
    order = {id(c): n for n, c in enumerate(convs)}    # module order is forward order
    wanted = [any(param_wants(c, need, first_at[id(c)])) for c in convs]
    if not any(wanted):
        return [None] * len(params)
    lowest = wanted.index(True)
    out = [None] * len(params)

    def below(conv):
        """A conv in front of ``conv`` wants a gradient: the walk has to go on past it."""
        return lowest < order[id(conv)]

    precision = gen.grad_precision                      # read here, at backward time

    def wgrad(conv, g_pre, xin, pad=0, pad_mode=None):
        want_dw, want_db = param_wants(conv, need, first_at[id(conv)])
        if not (want_dw or want_db):
            return
        if isinstance(conv, torch.nn.ConvTranspose1d):
            dw, db = _native.conv_transpose1d_weight_grad(g_pre, xin, conv.kernel_size[0], conv.stride[0],
                                                          conv.padding[0], conv.output_padding[0], want_dw, want_db,
                                                          precision=precision)
        else:
            dw, db = _native.conv1d_weight_grad_dilated(g_pre, xin, conv.kernel_size[0], conv.dilation[0], pad, want_dw,
                                                        want_db, pad_mode=pad_mode, precision=precision)
        param_store(conv, params, need, first_at[id(conv)], dw, db, out)

    def through_pad(conv, g_pre, tin, pad):
        return _native.conv1d_input_grad_reflect(g_pre, L[id(conv)][2], tin, conv.dilation[0], pad)

    if last is None:
        d = g
    else:
        g_z = _native.tanh_grad(g, y) if gen._final_post != POST_NONE else g
        post_in = tape["stages"][-1]["ya"]
        wgrad(last.conv, g_z, post_in, last._pad, PAD_REFLECT)
        if not below(last.conv):
            return out
        d = through_pad(last.conv, g_z, post_in.shape[2], last._pad)    # the gradient of lrelu(y) of the last stack
        del g_z
    for n in range(len(stages) - 1, -1, -1):
        up, stacks = stages[n]
        stage = tape["stages"][n]
        g_y = d if stage["ya"] is None else _native.disc_map_grad(d, None, stage["ya"], slope)
        del d
        for m in range(len(stacks) - 1, -1, -1):
            dil, pw, sk = _stack_convs(stacks[m])
            x, xa, ha = stage["stacks"][m]
            wgrad(pw, g_y, ha)
            wgrad(sk, g_y, x)
            if not below(pw):                          # the dilated conv and everything in front of it are frozen
                return out
            g_h = _native.disc_map_grad(_native.conv1d_fused(g_y, L[id(pw)][2], None, pw.in_channels, 1), None, ha, slope)
            wgrad(dil, g_h, xa, stacks[m]._pad, PAD_REFLECT)
            if not below(dil):
                return out
            g_y = _native.residual_merge_grad(_native.conv1d_fused(g_y, L[id(sk)][2], None, sk.in_channels, 1),
                                              through_pad(dil, g_h, xa.shape[2], stacks[m]._pad), xa, slope)
            del g_h
            stage["stacks"][m] = None                  # the stack's activations are not read again
        tape["stages"][n] = None
        wgrad(up, g_y, stage["up_in"])
        if not below(up):
            return out
        d = _native.conv_transpose1d_input_grad(g_y, L[id(up)][2], stage["up_in"].shape[2], up.stride[0], up.padding[0],
                                                up.output_padding[0])
        del g_y
    # d: the gradient of the first upsampler's input, lrelu of the first conv's output
    wgrad(first, _native.disc_map_grad(d, None, stage["up_in"], slope), tape["mel"], gen._first_pad[0], PAD_REFLECT)
    return out


class StackParamGrad(torch.autograd.Function):
    """``train_forward`` with the conv parameters as inputs of the graph; the backward is ``train_backward``.  The mel
    is a constant.  A frozen parameter gets None and costs no launch."""

    @staticmethod
    def forward(ctx, gen, mel, *params):
        y, tape = train_forward(gen, mel)
        ctx.gen, ctx.tape = gen, tape
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y, *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y, *params = ctx.saved_tensors
        tape, ctx.tape = ctx.tape, None
        if g is None or tape is None:
            if g is None:
                return (None, None) + (None,) * len(params)
            raise RuntimeError("the generator's training graph was already released: a second backward needs a "
                               "second forward (retain_graph is not supported)")
        grads = train_backward(ctx.gen, tape, y, params, ctx.needs_input_grad[2:], g.to(torch.float32).contiguous())
        return (None, None) + tuple(grads)


def wants_param_grad(gen):
    """Whether ``forward`` runs the training forward: the attribute, autograd, and a conv parameter that requires grad."""
    if not gen.parameter_grad or not torch.is_grad_enabled():
        return False
    return any(q.requires_grad for conv in train_convs(gen) for q in conv_params(conv))


def run(gen, mel):
    """The training forward of ``gen`` on mel [B, in_channels, T] -> y [B, out_channels, T'] on the parameters' graph."""
    check_supported(gen)
    if torch.is_tensor(mel) and mel.requires_grad:
        raise RuntimeError("the mel requires grad: the generator's parameter gradient treats its input as a constant "
                           "(there is no gradient with respect to the mel); pass a detached tensor")
    x = gen._prepare(mel)
    if x.dim() != 3 or x.shape[1] != gen._in_channels:
        raise ValueError(f"mel must be (B, {gen._in_channels}, T), got {tuple(x.shape)}")
    if x.shape[2] <= gen._first_pad[0]:
        raise ValueError(f"the reflection pad of {gen._first_pad[0]} needs more than {x.shape[2]} mel frames")
    flat = [q for conv in train_convs(gen) for q in conv_params(conv)]
    return StackParamGrad.apply(gen, x, *flat)
