"""The HiFi-GAN generators' training forward and parameter gradient (``_HiFiGANBase.parameter_grad``).

The training forward runs the graph of hifigan.py conv by conv on the exact-fp32 entries (_native.conv1d_fused,
_native.conv_transpose1d_fused) and keeps what the backward reads: every conv's input as the conv saw it (the
``y_act`` twin of the tensor in front of it), the raw tensor in front of every LeakyReLU, and the tanh output.  The
backward (csrc/gen_grad.hip) walks the graph downwards: per conv the mask of the activation behind it, the weight and
bias gradient, the weight-norm adjoint, and the data gradient for the layer below.  Every arithmetic step is a HIP
launch; torch allocates.

Folded weights and their packed images (the forward's, and W'[ci, co, j] = W[co, ci, k-1-j] for the data gradient of a
Conv1d) are cached against the module state (engine.cached): an ``optimizer.step()`` moves the parameters' versions
and the next forward packs again.
"""
import torch

from .. import _native
from .engine import POST_NONE, POST_TANH, cached, conv_params, effective_weight, param_store, param_wants
from .modules import LRELU_SLOPE, ResBlock1, UpsampleLayer

POST_SLOPE = 0.01       # F.leaky_relu's default, in front of conv_post (reference hifigan.py:104)


def _is_conv(m):
    return isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d))


def train_convs(gen):
    """The generator's convs in module order: conv_pre, ups, the ResBlocks' convs, conv_post."""
    return [m for m in gen.modules() if _is_conv(m)]


def check_supported(gen):
    if any(isinstance(up, UpsampleLayer) for up in gen.ups):
        raise NotImplementedError(
            f"{type(gen).__name__}(transposedconv=False): parameter_grad needs the backward of UpsampleLayer (nearest "
            "repeat + Conv1d in phase form), which does not exist yet; the ConvTranspose1d upsamplers have one")


def _layers(gen):
    """id(conv) -> what its launches read: the forward's packed weight, the bias, and the data gradient's weight (a
    packed flipped transpose for a Conv1d, the folded weight itself for a ConvTranspose1d)."""
    def build():
        out = {}
        for conv in train_convs(gen):
            w = effective_weight(conv)
            b = None if conv.bias is None else conv.bias.detach().contiguous().float()
            if isinstance(conv, torch.nn.ConvTranspose1d):
                out[id(conv)] = (_native.pack_conv_transpose1d(w, conv.stride[0], conv.padding[0]), b, w.contiguous())
            else:
                out[id(conv)] = (_native.pack_conv1d(w), b,
                                 _native.pack_conv1d(w.flip(2).transpose(0, 1).contiguous()))
        return out
    return cached(gen, "train_layers", build)


def _conv(L, conv, x, res=None, acc_in=None, out_div=1.0, act_slope=None, post=POST_NONE):
    """One forward conv launch on the activated input x -> (raw output, lrelu(output, act_slope) or None)."""
    packed, bias, _ = L[id(conv)]
    k, dil, pad = conv.kernel_size[0], conv.dilation[0], conv.padding[0]
    twin = None
    if act_slope is not None:
        twin = torch.empty((x.shape[0], conv.out_channels, x.shape[2] + 2 * pad - dil * (k - 1)), dtype=torch.float32,
                           device=x.device)
    y = _native.conv1d_fused(x, packed, bias, conv.out_channels, k, dil=dil, pad=pad, res=res, acc_in=acc_in,
                             out_div=out_div, post=post, out_act=twin, act_slope=1.0 if act_slope is None else act_slope)
    return y, twin


def train_forward(gen, mel):
    """mel [B, 80, T] fp32 device -> (y [B, C, T'] = tanh(conv_post(...)), tape): the tape holds, per conv, the
    tensors its backward reads."""
    L = _layers(gen)
    nk, n_up = gen.num_kernels, gen.num_upsamples
    tape = {"mel": mel, "stages": []}
    x, xa = _conv(L, gen.conv_pre, mel, act_slope=LRELU_SLOPE)
    tape["pre"] = x                                    # raw, for the mask in front of the first upsampler
    for i in range(n_up):
        up = gen.ups[i]
        packed, bias, _ = L[id(up)]
        k, s, p, op = up.kernel_size[0], up.stride[0], up.padding[0], up.output_padding[0]
        tout = (xa.shape[2] - 1) * s - 2 * p + k + op
        ua = torch.empty((xa.shape[0], up.out_channels, tout), dtype=torch.float32, device=xa.device)
        u = _native.conv_transpose1d_fused(xa, packed, bias, up.out_channels, k, s, p, op, out_act=ua,
                                           act_slope=LRELU_SLOPE)
        stage = {"up_in": xa, "u": u, "blocks": []}
        next_slope = LRELU_SLOPE if i + 1 < n_up else POST_SLOPE
        acc = None                                     # the running sum (r_0 + r_1) + ... of the stage
        for j in range(nk):
            blk = gen.resblocks[i * nk + j]
            final = j == nk - 1
            steps = []
            cur, cur_a = u, ua
            pairs = list(zip(blk.convs1, blk.convs2)) if isinstance(blk, ResBlock1) else [(c, None) for c in blk.convs]
            for pi, (c1, c2) in enumerate(pairs):
                last = pi == len(pairs) - 1
                # the block's last conv carries the stage's running sum, the final block's also the mean and the twin
                tail = dict(res=cur, acc_in=acc if last else None, out_div=float(nk) if (last and final) else 1.0,
                            act_slope=(next_slope if final else None) if last else LRELU_SLOPE)
                if c2 is None:                         # ResBlock2: x <- x + c(lrelu(x))
                    nxt, nxt_a = _conv(L, c1, cur_a, **tail)
                    steps.append((c1, None, cur, cur_a, None, None))
                else:                                  # ResBlock1: x <- x + c2(lrelu(c1(lrelu(x))))
                    h, ha = _conv(L, c1, cur_a, act_slope=LRELU_SLOPE)
                    nxt, nxt_a = _conv(L, c2, ha, **tail)
                    steps.append((c1, c2, cur, cur_a, h, ha))
                cur, cur_a = nxt, nxt_a
            stage["blocks"].append(steps)
            acc = cur
        stage["s"] = x = cur                           # raw stage output ((r_0 + r_1) + r_2) / nk
        xa = cur_a                                     # lrelu(s, next_slope)
        tape["stages"].append(stage)
    tape["post_in"] = xa
    y, _ = _conv(L, gen.conv_post, xa, post=POST_TANH)
    return y, tape


def _wgrad(conv, g_pre, xin, params, need, at, out, precision="f32"):
    want_dw, want_db = param_wants(conv, need, at)
    if not (want_dw or want_db):
        return
    k = conv.kernel_size[0]
    if isinstance(conv, torch.nn.ConvTranspose1d):
        dw, db = _native.conv_transpose1d_weight_grad(g_pre, xin, k, conv.stride[0], conv.padding[0],
                                                      conv.output_padding[0], want_dw, want_db, precision=precision)
    else:
        dw, db = _native.conv1d_weight_grad_dilated(g_pre, xin, k, conv.dilation[0], conv.padding[0], want_dw, want_db,
                                                    precision=precision)
    param_store(conv, params, need, at, dw, db, out)


def _dgrad(L, conv, g_pre):
    """The gradient of a Conv1d's (activated) input: the conv of g_pre with the flipped, transposed weight."""
    k, dil, pad = conv.kernel_size[0], conv.dilation[0], conv.padding[0]
    return _native.conv1d_fused(g_pre, L[id(conv)][2], None, conv.in_channels, k, dil=dil, pad=dil * (k - 1) - pad)


def train_backward(gen, tape, y, params, need, g):
    """g = dL/dy -> one gradient (or None) per entry of ``params`` (the convs' parameters, train_convs order)."""
    L = _layers(gen)
    convs = train_convs(gen)
    first, at = {}, 0
    for conv in convs:
        first[id(conv)] = at
        at += len(conv_params(conv))
    wanted = {id(c): any(param_wants(c, need, first[id(c)])) for c in convs}
    nk, n_up = gen.num_kernels, gen.num_upsamples
    # below[i]: a conv under stage i's ResBlocks wants a gradient (conv_pre, the upsamplers up to i, earlier stages)
    below, seen = [], wanted[id(gen.conv_pre)]
    for i in range(n_up):
        seen = seen or wanted[id(gen.ups[i])]
        below.append(seen)
        seen = seen or any(wanted[id(c)] for j in range(nk) for c in gen.resblocks[i * nk + j].modules() if _is_conv(c))
    out = [None] * len(params)

    precision = gen.grad_precision                      # read here, at backward time

    def wgrad(conv, g_pre, xin):
        _wgrad(conv, g_pre, xin, params, need, first[id(conv)], out, precision)

    g_z = _native.tanh_grad(g, y)
    wgrad(gen.conv_post, g_z, tape["post_in"])
    if not seen:
        return out
    slope = POST_SLOPE
    d = _dgrad(L, gen.conv_post, g_z)                   # the gradient of lrelu(s, slope)
    del g_z
    for i in range(n_up - 1, -1, -1):
        stage = tape["stages"][i]
        g_s = _native.disc_map_grad(d, None, stage["s"], slope)
        g_r = _native.grad_div(g_s, float(nk)) if nk > 1 else g_s      # the mean's adjoint: every r_j receives it
        del d, g_s
        g_u = None                                      # the sum of the blocks' input gradients
        for j in range(nk - 1, -1, -1):
            steps = stage["blocks"][j]
            g_x = g_r
            for pi in range(len(steps) - 1, -1, -1):
                c1, c2, cur, cur_a, h, ha = steps[pi]
                earlier = any(wanted[id(c)] for st in steps[:pi] for c in st[:2] if c is not None)
                g_pre = g_x
                if c2 is not None:
                    wgrad(c2, g_x, ha)
                    if not (wanted[id(c1)] or earlier or below[i]):
                        break
                    g_pre = _native.disc_map_grad(_dgrad(L, c2, g_x), None, h, LRELU_SLOPE)
                wgrad(c1, g_pre, cur_a)
                if not (earlier or below[i]):
                    break
                g_x = _native.residual_merge_grad(g_x, _dgrad(L, c1, g_pre), cur, LRELU_SLOPE,
                                                  acc=g_u if pi == 0 else None)
            else:
                g_u = g_x
            stage["blocks"][j] = None                   # the block's activations are not read again
        del g_r
        tape["stages"][i] = None
        if not below[i]:
            return out
        up = gen.ups[i]
        wgrad(up, g_u, stage["up_in"])
        lower = wanted[id(gen.conv_pre)] if i == 0 else below[i - 1] or any(
            wanted[id(c)] for j in range(nk) for c in gen.resblocks[(i - 1) * nk + j].modules() if _is_conv(c))
        if not lower:
            return out
        d = _native.conv_transpose1d_input_grad(g_u, L[id(up)][2], stage["up_in"].shape[2], up.stride[0], up.padding[0],
                                                up.output_padding[0])
        del g_u
        slope = LRELU_SLOPE
    wgrad(gen.conv_pre, _native.disc_map_grad(d, None, tape["pre"], LRELU_SLOPE), tape["mel"])
    return out


class GeneratorParamGrad(torch.autograd.Function):
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
    """The training forward of ``gen`` on mel [B, 80, T] -> y [B, C, T'] on the parameters' graph."""
    check_supported(gen)
    if torch.is_tensor(mel) and mel.requires_grad:
        raise RuntimeError("the mel requires grad: the generator's parameter gradient treats its input as a constant "
                           "(there is no gradient with respect to the mel); pass a detached tensor")
    x = gen._prepare(mel)
    if x.dim() != 3 or x.shape[1] != gen.conv_pre.in_channels:
        raise ValueError(f"mel must be (B, {gen.conv_pre.in_channels}, T), got {tuple(x.shape)}")
    flat = [q for conv in train_convs(gen) for q in conv_params(conv)]
    return GeneratorParamGrad.apply(gen, x, *flat)
