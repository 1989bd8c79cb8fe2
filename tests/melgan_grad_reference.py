"""Float64 oracles of MelGAN's parameter gradient (csrc/gen_grad.hip fv_conv1d_weight_grad_dilated_mode and
fv_conv1d_input_grad_reflect, generator/stack_grad.py): numpy closed forms of the two kernels, and float64 torch
autograd through oracle/torch_port.melgan_trunk -- the un-fused restatement of the reference's forward, which is
differentiable as it stands.  The float32 yardstick and the kink-margin recorder are those of
tests/generator_grad_reference.py: they wrap F.leaky_relu whatever its slope, so MelGAN's 0.2 from the config needs
nothing of its own.

TEST INFRASTRUCTURE ONLY; nothing here runs on the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_port
from tests.generator_grad_reference import (KINK, YARDSTICK_THREADS, bias_grad, cotangent, is_param,  # noqa: F401
                                            kernel_inputs, recorded_margins, rel_err)

# the golden case (tests/golden/make_melgan_param_grad_golden.py)
GOLDEN_CFG = dict(in_channels=80, out_channels=1, kernel_size=7, channels=[16, 8, 4], upsample_scales=[4, 3],
                  stack_kernel_size=3, stacks=3, use_weight_norm=True, use_causal_conv=False)
GOLDEN_WEIGHT_SEED = 3
GOLDEN_SHAPE = (2, 80, 6)


# ---- closed forms of the kernels ----
def reflect_index(i, T):
    """r(i): -i below zero, 2 (T - 1) - i from T on, i otherwise."""
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= T, 2 * (T - 1) - i, i))


def reflect_weight_grad(g, xa, k, dil, pad):
    """dw[co, ci, j] = sum_{b, t} g[b, co, t] xa[b, ci, r(t + j dil - pad)], float64."""
    g, xa = np.asarray(g, np.float64), np.asarray(xa, np.float64)
    tout = g.shape[2]
    assert tout == xa.shape[2] + 2 * pad - dil * (k - 1) and pad < xa.shape[2]
    xp = np.pad(xa, ((0, 0), (0, 0), (pad, pad)), mode="reflect") if pad else xa
    return np.stack([np.einsum("bot,bit->oi", g, xp[:, :, j * dil:j * dil + tout]) for j in range(k)], axis=2)


def reflect_input_grad(g, w, tin, dil, pad):
    """dxa[b, ci, i] = sum_{p, r(p - pad) = i} sum_{co, j} w[co, ci, j] g[b, co, p - j dil]: the gradient of the padded
    tensor, then the explicit fold of its 2 pad border samples onto their mirror images; float64."""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    B, cout, tout = g.shape
    k = w.shape[2]
    assert tout == tin + 2 * pad - dil * (k - 1) and pad < tin
    gp = np.zeros((B, w.shape[1], tin + 2 * pad))
    for j in range(k):
        gp[:, :, j * dil:j * dil + tout] += np.einsum("oi,bot->bit", w[:, :, j], g)
    dx = np.zeros((B, w.shape[1], tin))
    np.add.at(dx, (slice(None), slice(None), reflect_index(np.arange(tin + 2 * pad) - pad, tin)), gp)
    return dx


# ---- the whole chain ----
def output_length(cfg, frames):
    n = frames
    for s in cfg["upsample_scales"]:
        n *= s
    return n


def forward(cfg, sd, mel, dtype=torch.float64):
    """MelGANGenerator.forward on leaf copies of the state dict's parameters -> (output [B, T'], {key: leaf})."""
    leaves = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v))
        if is_param(k):
            t = t.to(dtype).clone().requires_grad_(True)
        leaves[k] = t
    y = torch.tanh(torch_port.melgan_trunk(torch.as_tensor(np.asarray(mel, np.float32)).to(dtype), leaves, cfg))
    return y[:, 0, :], {k: t for k, t in leaves.items() if is_param(k)}


def param_grad(cfg, sd, mel, c, dtype=torch.float64, margins=None):
    """d <c, G(mel)> / d parameter per state-dict key -> (output ndarray, {key: gradient ndarray}) in ``dtype``."""
    with recorded_margins([] if margins is None else margins):
        y, leaves = forward(cfg, sd, mel, dtype)
    (y * torch.as_tensor(np.asarray(c)).to(dtype)).sum().backward()
    return y.detach().numpy(), {k: t.grad.numpy() for k, t in leaves.items()}


def float32_yardstick(cfg, sd, mel, c):
    """The float32 eager-autograd error of the chain per parameter tensor, relative to the tensor's largest float64
    gradient -> (worst over the tensors of more than one element, its key, worst over the one-element tensors)."""
    n = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        _, g64 = param_grad(cfg, sd, mel, c)
        _, g32 = param_grad(cfg, sd, mel, c, dtype=torch.float32)
    finally:
        torch.set_num_threads(n)
    errs = {k: rel_err(g32[k], g64[k]) for k in g64}
    many = {k: e for k, e in errs.items() if g64[k].size > 1}
    worst = max(many, key=many.get)
    return many[worst], worst, max([e for k, e in errs.items() if g64[k].size == 1], default=0.0)


def kink_sides(cfg, sd, mel, dtype):
    """The side (x > 0) of every pre-activation of the forward evaluated in ``dtype``, one array per leaky ReLU."""
    out, real = [], F.leaky_relu

    def spy(x, *a, **kw):
        out.append((x.detach() > 0).numpy().copy())
        return real(x, *a, **kw)
    F.leaky_relu = spy
    try:
        with torch.no_grad():
            forward(cfg, sd, mel, dtype)
    finally:
        F.leaky_relu = real
    return out


def golden_inputs(seed):
    """(mel, cotangent) of the golden case from one RandomState seed."""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(-4.0, 1.0, GOLDEN_SHAPE).astype(np.float32)
    c = rs.randn(GOLDEN_SHAPE[0], output_length(GOLDEN_CFG, GOLDEN_SHAPE[2])).astype(np.float32)
    return mel, c


# The chain cases of tests/cases.py at SMALL_B x SMALL_T.  As for HiFi-GAN (tests/generator_grad_reference.py), the mel
# seed of each case is the one in 5..44 with the largest kink margin of the float64 forward, recorded beside it;
# tests/test_melgan_grad_host.py checks the margin and that the float32 CPU forward takes the same side of every kink.
CHAIN_SEARCH = range(5, 45)
CHAIN_MEL_SEED = {"melgan_s": (30, 1.11e-6), "melgan_nown": (25, 5.03e-6)}
CHAIN_WEIGHT_SEED = 1
CHAIN_COTANGENT_SEED = 7


def chain_case(tag, mel_seed=None):
    """(cfg, state dict, mel, cotangent) of a chain case of tests/cases.py."""
    from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
    from tests import cases
    cfg = next(c for t, _, c in cases.SMALL if t == tag)
    sd = seeded_state_dict("melgan", cfg, seed=CHAIN_WEIGHT_SEED, weight_norm=cfg.get("use_weight_norm", True))
    mel = seeded_mel(cases.SMALL_T, seed=CHAIN_MEL_SEED[tag][0] if mel_seed is None else mel_seed, batch=cases.SMALL_B)
    c = cotangent((cases.SMALL_B, output_length(cfg, cases.SMALL_T)), CHAIN_COTANGENT_SEED)
    return cfg, sd, mel, c


def chain_margin(tag, mel_seed=None):
    """The smallest kink margin of the float64 forward of a chain case."""
    cfg, sd, mel, _ = chain_case(tag, mel_seed)
    margins = []
    with torch.no_grad(), recorded_margins(margins):
        forward(cfg, sd, mel)
    return min(margins)
