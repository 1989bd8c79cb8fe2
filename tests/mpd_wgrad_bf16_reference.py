"""Float64 oracles of the multi-period discriminator's bf16 weight gradients (fv_period_conv_weight_grad_bf16,
csrc/gen_grad_bf16.hip; ``DiscriminatorP.grad_precision = "bf16"``): the closed form of
tests/mpd_wgrad_reference.py on operands rounded to bf16 (``generator_grad_bf16_reference.bf16_round``), and the chain
oracle ``param_grad_bf16``: ``mpd_wgrad_reference.param_grad`` run while ``F.conv2d`` is replaced by an autograd
Function whose forward and data gradient are the real op, whose weight gradient is the real op's on bf16(x), bf16(g)
when the layer has more than one input channel (the first layer, straight from the waveform, stays exact) and whose
bias gradient is g.sum((0, 2, 3)).  The shapes of the kernel tests live here so that the CPU test
(tests/test_mpd_wgrad_bf16_host.py) proves on them what the GPU test (tests/test_gpu_mpd_wgrad_bf16.py) asserts.

TEST INFRASTRUCTURE ONLY; nothing here runs on the GPU."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import generator_grad_bf16_reference as bref
from tests import mpd_wgrad_reference as wref

PERIODS = wref.PERIODS
U = 64                                            # flat positions per unit (gen_grad_bf16.hip kBfTK)
FLOOR_RTOL, YARDSTICK_BAND, YARDSTICK_FACTOR = bref.FLOOR_RTOL, bref.YARDSTICK_BAND, bref.YARDSTICK_FACTOR
CHAIN_CASES = [f"p{p}" for p in PERIODS] + ["mpd"]


# ---- the closed form of the kernel ----
def period_conv_weight_grad(g_pre, x, k, stride):
    """(dw from the rounded operands, db from the un-rounded g_pre), float64."""
    dw, _ = wref.period_conv_weight_grad(bref.bf16_round(g_pre), bref.bf16_round(x), k, stride)
    return dw, np.asarray(g_pre, np.float64).sum(axis=(0, 2, 3))


def rows(hout, stride):
    """The smallest input height whose output has ``hout`` rows."""
    return stride * (hout - 1) + 1


def _kernel_shapes():
    """(Cin, Cout, k, stride, p, H, B) of the kernel tests: the smallest shapes at which the staging can go wrong."""
    out = []
    for cin, cout, k, s in wref.KERNEL_LAYERS:            # H' p one row past a unit; units never align with rows
        out += [(cin, cout, k, s, p, s * (U // p) + 1, 3) for p in PERIODS]
    for p in PERIODS:                                     # H' p just below, at (where p divides), just above 64 and 128
        for n in (U, 2 * U):
            hs = [n // p, n // p + 1] + ([n // p - 1] if n % p == 0 else [])
            for hout in sorted(hs):
                out.append((32, 128, 5, 3, p, rows(hout, 3), 2))       # 160 columns: a partial column tile
                out.append((48, 40, 5, 1, p, hout, 2))                 # stride 1: the dilated route
    out += [(32, 128, 5, 3, 3, rows(21, 3), 3), (32, 128, 5, 3, 7, rows(9, 3), 3),     # 63 flat positions, B odd: the
            (128, 512, 5, 3, 11, rows(5, 3), 1), (48, 40, 3, 1, 5, 13, 3)]             # pair straddles a row end
    out += [(32, 128, 5, 3, 3, 7, 2), (32, 128, 5, 3, 11, 4, 2), (1024, 1, 3, 1, 5, 3, 2)]   # H' p < 32: dead halves
    for H in (1, 2, 3):                                   # only some taps meet a row
        out += [(32, 128, 5, 3, 2, H, 2), (32, 128, 5, 3, 7, H, 2), (64, 64, 5, 1, 3, H, 2), (1024, 1, 3, 1, 11, H, 1)]
    for H in (9, 10, 11):                                 # H = 0, 1, 2 mod 3: the bottom padding row read or not
        out += [(128, 512, 5, 3, 5, H, 2), (32, 128, 5, 3, 2, H + 21, 2)]
    out += [(16, 64, 5, 3, 3, 40, 2), (16, 64, 5, 2, 7, 21, 2), (16, 64, 5, 2, 2, 66, 1)]   # 64 rows x 80 columns
    # 20 x 8 tiles -> 4 splits; 240 flat positions are 4 units a row: B = 1, 2, 3 give splits of one, two, three units
    out += [(512, 1024, 5, 3, 3, rows(80, 3), B) for B in (1, 2, 3)]
    seen = []
    for s in out:
        if s not in seen:
            seen.append(s)
    return seen


KERNEL_SHAPES = _kernel_shapes()
SPLIT_SHAPES = [s for s in KERNEL_SHAPES if s[:2] == (512, 1024) and s[5] == rows(80, 3)]
REFUSED_SHAPE = (32, 32, 5, 3, 3, 10, 2)          # strided with Cout < 64: the fp32 entry's plain kernel, no bf16 twin


# ---- the whole chain ----
def _patched(real, rounding):
    """F.conv2d with the bf16 mode's backward; ``rounding`` False: the same Function without the rounding."""
    rnd = bref._round_tensor if rounding else (lambda t: t)

    class Op(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b, kw):
            ctx.save_for_backward(x, w)
            ctx.kw, ctx.bias = kw, b is not None
            return real(x, w, b, **kw)

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            r = rnd if x.shape[1] > 1 else (lambda t: t)          # the first layer stays exact
            with torch.enable_grad():
                xd = x.detach().requires_grad_(True)
                (dx,) = torch.autograd.grad(real(xd, w.detach(), None, **ctx.kw), xd, g)
                wd = w.detach().requires_grad_(True)
                (dw,) = torch.autograd.grad(real(r(x.detach()), wd, None, **ctx.kw), wd, r(g))
            return dx, dw, (g.sum((0, 2, 3)) if ctx.bias else None), None

    def op(x, w, b=None, **kw):
        if not (torch.is_grad_enabled() and w.requires_grad):
            return real(x, w, b, **kw)
        return Op.apply(x, w, b, kw)
    return op


@contextlib.contextmanager
def bf16_weight_gradients(rounding=True):
    real = F.conv2d
    F.conv2d = _patched(real, rounding)
    try:
        yield
    finally:
        F.conv2d = real


def param_grad_bf16(kind, est, real, sd, dtype=torch.float64, rounding=True, **kw):
    """``mpd_wgrad_reference.param_grad`` in the bf16 mode: the same arguments, the same four results."""
    with bf16_weight_gradients(rounding):
        return wref.param_grad(kind, est, real, sd, dtype, **kw)


def is_first(key):
    """A parameter of a DiscriminatorP's first layer (1 -> 32, from the waveform: fp32 in both modes)."""
    return ".convs.0." in "." + key


def is_rounded_weight(key):
    """A weight tensor whose gradient the mode takes from rounded operands: layers 1-5."""
    return key.endswith((".weight_v", ".weight")) and not is_first(key)


def chain_case(name):
    """(kind, kw, est, real, state dict) of "p<period>" (TINY_T, B = 2) or "mpd" (FULL_T)."""
    kind, kw = wref.case_kind(name)
    est, real = wref.case_signals(name)
    return kind, kw, est, real, wref.case_state_dict(name)


def chain_figures(name):
    """(a) the yardstick: the float32 evaluation of the bf16 oracle against its float64 evaluation
    (YARDSTICK_THREADS threads; for "mpd" float64 takes float32's leaky-ReLU sides, as the fp32 yardstick of the full
    cases does), worst over the tensors of more than one element; (b) the routing floor: the smallest distance between
    the bf16 oracle and the exact float64 gradient over the rounded weight tensors; then the largest such distance,
    and the worst distance over the tensors the mode leaves exact (every bias, the first layer)."""
    kind, kw, est, real, sd = chain_case(name)
    n = torch.get_num_threads()
    torch.set_num_threads(wref.YARDSTICK_THREADS)
    try:
        b32, _, e32, r32 = param_grad_bf16(kind, est, real, sd, torch.float32, **kw)
        adopt = dict(est_maps=e32, real_maps=r32) if name == "mpd" else {}
        b64 = param_grad_bf16(kind, est, real, sd, **adopt, **kw)[0]
    finally:
        torch.set_num_threads(n)
    e64 = wref.param_grad(kind, est, real, sd, **adopt, **kw)[0]
    yard = max(wref.rel_err(b32[k], b64[k]) for k in b64 if b64[k].size > 1)
    dist = [wref.rel_err(b64[k], e64[k]) for k in b64 if is_rounded_weight(k)]
    exact = max(wref.rel_err(b64[k], e64[k]) for k in b64 if k.endswith(".bias") or is_first(k))
    return yard, min(dist), max(dist), exact


# Recorded by tests/test_mpd_wgrad_bf16_host.py (which recomputes and checks them): per chain case
# (yardstick (a), routing floor (b)), the method of generator_grad_bf16_reference.CHAIN_FIGURES.
CHAIN_FIGURES = {"p2": (5.00e-4, 1.596e-3), "p3": (3.61e-4, 1.729e-3), "p5": (1.67e-4, 1.061e-3),
                 "p7": (1.90e-4, 9.131e-4), "p11": (1.35e-4, 5.828e-4), "mpd": (2.51e-4, 3.772e-4)}
