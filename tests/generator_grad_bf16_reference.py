"""Float64 oracles of the generators' bf16 weight gradients (csrc/gen_grad_bf16.hip, ``grad_precision = "bf16"``):
``bf16_round`` (numpy, round-to-nearest-even on the uint32 image), the closed forms of
tests/generator_grad_reference.py / tests/melgan_grad_reference.py applied to rounded operands, and the chain oracle
``param_grad_bf16``: ``gref.param_grad`` / ``mref.param_grad`` run while ``F.conv1d`` and ``F.conv_transpose1d`` are
replaced by autograd Functions whose forward and data gradient are the real op, whose weight gradient is the real
op's on bf16(x), bf16(g) and whose bias gradient is g.sum((0, 2)).  oracle/torch_port.py calls the ops as ``F....``, so
the weight-norm adjoint and MelGAN's ``F.pad(..., "reflect")`` come from autograd unchanged (a reflected sample is the
rounded sample: rounding commutes with the pad).

TEST INFRASTRUCTURE ONLY; nothing here runs on the GPU."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import generator_grad_reference as gref
from tests import melgan_grad_reference as mref


def bf16_round(a):
    """The fp32 values of ``a`` rounded to bfloat16, nearest even, as fp32: on the uint32 image u,
    ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16.  Finite values and infinities; a NaN is not preserved."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xffffffff).astype(np.uint32).view(np.float32)


# ---- closed forms of the kernels: those of the fp32 entries on rounded operands ----
def dilated_weight_grad(g, xa, k, dil, pad):
    return gref.dilated_weight_grad(bf16_round(g), bf16_round(xa), k, dil, pad)


def reflect_weight_grad(g, xa, k, dil, pad):
    return mref.reflect_weight_grad(bf16_round(g), bf16_round(xa), k, dil, pad)


def convt_weight_grad(g, xa, k, s, p):
    return gref.convt_weight_grad(bf16_round(g), bf16_round(xa), k, s, p)


def ties(shape, seed):
    """fp32 values that all lie exactly half way between two bf16 neighbours (low half 0x8000), the kept bit 0 on every
    even flat index and 1 on every odd one, signs and exponents (2^-3 .. 2^3) random."""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    sign = rs.randint(0, 2, n).astype(np.uint32) << 31
    expo = rs.randint(124, 131, n).astype(np.uint32) << 23
    mant = (rs.randint(0, 64, n).astype(np.uint32) << 17) | ((np.arange(n, dtype=np.uint32) & 1) << 16)
    return (sign | expo | mant | np.uint32(0x8000)).view(np.float32).reshape(shape)


# ---- the whole chain ----
def _round_tensor(t):
    """bf16(fp32(t)) in t's dtype: the kernels round the fp32 value."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _patched(real, rounding):
    """``real`` (F.conv1d or F.conv_transpose1d) with the bf16 mode's backward; ``rounding`` False: the same Function
    with the rounding left out, i.e. the exact gradient by another route."""
    rnd = _round_tensor if rounding else (lambda t: t)

    class Op(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b, kw):
            ctx.save_for_backward(x, w)
            ctx.kw, ctx.bias = kw, b is not None
            return real(x, w, b, **kw)

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            with torch.enable_grad():
                xd = x.detach().requires_grad_(True)
                (dx,) = torch.autograd.grad(real(xd, w.detach(), None, **ctx.kw), xd, g)
                wd = w.detach().requires_grad_(True)
                (dw,) = torch.autograd.grad(real(rnd(x.detach()), wd, None, **ctx.kw), wd, rnd(g))
            return dx, dw, (g.sum((0, 2)) if ctx.bias else None), None

    def op(x, w, b=None, **kw):
        if not (torch.is_grad_enabled() and w.requires_grad):       # a constant filter (the PQMF), or no graph
            return real(x, w, b, **kw)
        return Op.apply(x, w, b, kw)
    return op


@contextlib.contextmanager
def bf16_weight_gradients(rounding=True):
    """While active, the weight gradient of every F.conv1d / F.conv_transpose1d whose weight requires grad is taken
    from bf16-rounded operands (the ``recorded_margins`` patching pattern)."""
    real = F.conv1d, F.conv_transpose1d
    F.conv1d, F.conv_transpose1d = _patched(real[0], rounding), _patched(real[1], rounding)
    try:
        yield
    finally:
        F.conv1d, F.conv_transpose1d = real


def chain_case(tag):
    """("hifigan" | "multiband-hifigan" | "melgan", cfg, state dict, mel, cotangent) of a chain case."""
    if tag in mref.CHAIN_MEL_SEED:
        return ("melgan",) + mref.chain_case(tag)
    return gref.chain_case(tag)


def param_grad_exact(name, cfg, sd, mel, c, dtype=torch.float64):
    if name == "melgan":
        return mref.param_grad(cfg, sd, mel, c, dtype)
    return gref.param_grad(name, cfg, sd, mel, c, dtype)


def param_grad_bf16(name, cfg, sd, mel, c, dtype=torch.float64, rounding=True):
    """The bf16 mode's gradient of <c, G(mel)> per state-dict key, evaluated in ``dtype`` -> (output, {key: ndarray})."""
    with bf16_weight_gradients(rounding):
        return param_grad_exact(name, cfg, sd, mel, c, dtype)


def is_weight(key):
    return key.endswith((".weight_v", ".weight"))


def chain_figures(tag):
    """(a) the yardstick: the float32 evaluation of the bf16 oracle against its float64 evaluation (YARDSTICK_THREADS
    threads), worst over the tensors of more than one element; (b) the routing floor: the smallest distance between
    the bf16 oracle and the exact float64 gradient over the weight_v / weight tensors; then the largest such distance,
    and the worst distance of the bias gradients (which the mode leaves exact)."""
    name, cfg, sd, mel, c = chain_case(tag)
    n = torch.get_num_threads()
    torch.set_num_threads(gref.YARDSTICK_THREADS)
    try:
        _, b64 = param_grad_bf16(name, cfg, sd, mel, c)
        _, b32 = param_grad_bf16(name, cfg, sd, mel, c, dtype=torch.float32)
    finally:
        torch.set_num_threads(n)
    _, e64 = param_grad_exact(name, cfg, sd, mel, c)
    yard = max(gref.rel_err(b32[k], b64[k]) for k in b64 if b64[k].size > 1)
    dist = [gref.rel_err(b64[k], e64[k]) for k in b64 if is_weight(k)]
    bias = max(gref.rel_err(b64[k], e64[k]) for k in b64 if k.endswith(".bias"))
    return yard, min(dist), max(dist), bias


# Recorded by tests/test_generator_grad_bf16_host.py (which recomputes and checks them): per chain case
# (yardstick (a), routing floor (b)).  (a) is a count of operands that the float32 and the float64 evaluation round to
# different bf16 neighbours, not smooth rounding noise, so the GPU chain tests allow 4 x (a).
CHAIN_FIGURES = {"hifigan_s": (5.41e-4, 1.38e-3), "mb_s": (5.50e-4, 1.97e-3), "melgan_s": (3.87e-4, 1.10e-3)}
# How closely a recomputation has to meet the recorded figures.  (b) is a float64 evaluation: the same on every
# machine up to the recorded digits.  (a) holds a float32 CPU evaluation, whose sums another BLAS or thread split
# orders differently, and every operand that thereby crosses a rounding boundary moves it by a whole step: a factor 2.
FLOOR_RTOL = 0.01
YARDSTICK_BAND = 2.0
YARDSTICK_FACTOR = 4.0
