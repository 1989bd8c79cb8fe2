"""Basis-MelGAN's training forward and parameter gradient (``BasisMelGANGenerator.basis_grad`` / ``parameter_grad``).

The reference's ``forward`` (basis_melgan.py:140-162) runs the trunk twice, on the mel and on ``zeros_like(mel)``, and
returns the two differences; the parameter gradient flows through both passes.  All B rows of its zero pass are equal,
so here ONE all-zero row is appended and generator/stack_grad.py's conv-by-conv training forward runs once over
[B + 1, in_channels, T].  Every op is per row, so this is exact, and row B's output gradient is minus the sum of the
other rows', which the weight-gradient kernels add over the batch as they add any row.

The trunk ends at the last ResidualStack's raw output Y [B+1, C, F].  The head (csrc/basis_grad.hip):
``D = relu(Y[:B]) - relu(Y[B])`` (fv_basis_head_forward), ``weight = D^T`` (a view) and
``est = crop(overlap_add(basis D))`` (fv_basis_ola on D: the overlap-add is linear).  Its adjoint is one launch
(fv_basis_head_grad) from the two cotangents to g_Y, where stack_grad.train_backward starts.

The basis (``basis_signal.layer.weight``) is a constant of this graph: the reference never steps it (train.py:64,
329-331), and it gets no gradient here.
"""
import torch

from .. import _native
from . import stack_grad
from .engine import cached, conv_params
from .grad import train_convs


def check_supported(gen):
    """What ``basis_grad = True`` refuses: stack_grad's graphs, and the heads and upsamplers without a backward."""
    stack_grad.check_supported(gen)
    name = type(gen).__name__
    if gen._config["lastlinear"]:
        raise NotImplementedError(f"{name}(lastlinear=True): basis_grad needs the backward of LastLinear's BatchNorm "
                                  "head, which does not exist yet")
    if not gen._config["transposedconv"]:
        raise NotImplementedError(f"{name}(transposedconv=False): basis_grad needs the backward of UpsampleLayer (nearest "
                                  "repeat + Conv1d), which does not exist yet")
    if not gen._config["use_final_nonlinear_activation"]:
        raise NotImplementedError(f"{name}(use_final_nonlinear_activation=False): basis_grad exists for the trunk that "
                                  "ends in ReLU only, whose mask the head's adjoint (fv_basis_head_grad) applies")


def _basis(gen):
    """(the basis [L, C] as the head's adjoint reads it, its packed image for the overlap-add)."""
    def build():
        w = gen.basis_signal.layer.weight.detach().contiguous().float()
        return w, _native.pack_basis(w)
    return cached(gen, "basis_train", build)


class BasisParamGrad(torch.autograd.Function):
    """The trunk over B + 1 rows and the head, with the trunk's conv parameters as inputs of the graph; the mel and the
    basis are constants.  Returns (est [B, F hop], weight [B, F, C]); the backward takes either cotangent as None."""

    @staticmethod
    def forward(ctx, gen, rows, *params):
        Y, tape = stack_grad.train_forward(gen, rows)
        basis, packed = _basis(gen)
        D = _native.basis_head_forward(Y)
        F = D.shape[2]
        est = _native.basis_ola(D, packed, gen.L)[:, 0, : F * (gen.L // 2)]
        ctx.gen, ctx.tape = gen, tape
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(Y, basis, *params)
        return est, D.transpose(1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_est, g_w):
        Y, basis, *params = ctx.saved_tensors
        none = (None, None) + (None,) * len(params)
        if g_est is None and g_w is None:
            return none
        tape, ctx.tape = ctx.tape, None
        if tape is None:
            raise RuntimeError("the generator's training graph was already released: a second backward needs a "
                               "second forward (retain_graph is not supported)")
        if g_est is not None:
            g_est = g_est.to(torch.float32).contiguous()
        if g_w is not None:                    # [B, F, C]; loss.BasisWeightL1 hands it over in [B, C, F] storage
            g_w = g_w.to(torch.float32).transpose(1, 2).contiguous()
        g_Y = _native.basis_head_grad(g_est, g_w, Y, basis)
        return (None, None) + tuple(stack_grad.train_backward(ctx.gen, tape, Y, params, ctx.needs_input_grad[2:], g_Y))


def wants_param_grad(gen):
    """Whether ``forward`` runs the training forward: the attribute, autograd, and a trunk parameter that requires grad
    (the basis does not count: it is a constant)."""
    if not gen.parameter_grad or not torch.is_grad_enabled():
        return False
    return any(q.requires_grad for conv in train_convs(gen) for q in conv_params(conv))


def run(gen, mel):
    """The training forward of ``gen`` on mel [B, in_channels, T] -> (est [B, F L/2], weight [B, F, C]) on the trunk
    parameters' graph."""
    check_supported(gen)
    if torch.is_tensor(mel) and mel.requires_grad:
        raise RuntimeError("the mel requires grad: the generator's parameter gradient treats its input as a constant "
                           "(there is no gradient with respect to the mel); pass a detached tensor")
    x = gen._prepare(mel)
    if x.dim() != 3 or x.shape[1] != gen._in_channels:
        raise ValueError(f"mel must be (B, {gen._in_channels}, T), got {tuple(x.shape)}")
    if x.shape[2] <= gen._first_pad[0]:
        raise ValueError(f"the reflection pad of {gen._first_pad[0]} needs more than {x.shape[2]} mel frames")
    rows = torch.cat([x, x.new_zeros((1,) + tuple(x.shape[1:]))])
    flat = [q for conv in train_convs(gen) for q in conv_params(conv)]
    return BasisParamGrad.apply(gen, rows, *flat)
