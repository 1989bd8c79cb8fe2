"""Float64 oracles of the HiFi-GAN generators' parameter gradient (csrc/gen_grad.hip, generator/grad.py): numpy closed
forms of the three kernels, and float64 torch autograd through oracle/torch_port.hifigan_trunk -- the un-fused
restatement of the reference's forward, which is differentiable as it stands (its state dict may hold leaf tensors
that require grad; torch_port.forward itself runs under no_grad, so the trunk is called directly).

TEST INFRASTRUCTURE ONLY; nothing here runs on the GPU."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_port

# the golden case (tests/golden/make_hifigan_param_grad_golden.py)
_H = dict(resblock_kernel_sizes=[3, 7, 11], resblock_type="1",
          resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], transposedconv=True, bias=True)
GOLDEN_CFG = dict(_H, upsample_rates=[4, 3], upsample_kernel_sizes=[8, 7], upsample_initial_channel=16)
GOLDEN_WEIGHT_SEED = 3
GOLDEN_SHAPE = (2, 80, 6)
KINK = 1e-5                 # a pre-activation closer to zero than this fraction of its map's peak counts as on a kink
YARDSTICK_THREADS = 4


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---- closed forms of the kernels ----
def dilated_weight_grad(g, xa, k, dil, pad):
    """dw[co, ci, j] = sum_{b, t} g[b, co, t] xa[b, ci, t + j dil - pad] (zero padding), float64."""
    g, xa = np.asarray(g, np.float64), np.asarray(xa, np.float64)
    tout = g.shape[2]
    assert tout == xa.shape[2] + 2 * pad - dil * (k - 1)
    xp = np.pad(xa, ((0, 0), (0, 0), (pad, pad)))
    return np.stack([np.einsum("bot,bit->oi", g, xp[:, :, j * dil:j * dil + tout]) for j in range(k)], axis=2)


def bias_grad(g):
    return np.asarray(g, np.float64).sum(axis=(0, 2))


def convt_out_len(tin, k, s, p, op):
    return (tin - 1) * s - 2 * p + k + op


def _gather(g, tin, k, s, p):
    """G[b, co, j, i] = g[b, co, i s + j - p], zero outside the row."""
    g = np.asarray(g, np.float64)
    B, cout, tout = g.shape
    out = np.zeros((B, cout, k, tin))
    for j in range(k):
        pos = np.arange(tin) * s + j - p
        ok = (pos >= 0) & (pos < tout)
        out[:, :, j, ok] = g[:, :, pos[ok]]
    return out


def convt_input_grad(g, w, tin, s, p):
    """dxa[b, ci, i] = sum_{co, j} w[ci, co, j] g[b, co, i s + j - p], float64."""
    w = np.asarray(w, np.float64)
    return np.einsum("coj,bojn->bcn", w, _gather(g, tin, w.shape[2], s, p))


def convt_weight_grad(g, xa, k, s, p):
    """dw[ci, co, j] = sum_{b, i} xa[b, ci, i] g[b, co, i s + j - p], float64."""
    xa = np.asarray(xa, np.float64)
    return np.einsum("bcn,bojn->coj", xa, _gather(g, xa.shape[2], k, s, p))


def kernel_inputs(shape_g, shape_x, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(*shape_g).astype(np.float32), rs.randn(*shape_x).astype(np.float32)


# ---- the whole chain ----
def is_param(key):
    return key.endswith((".weight", ".weight_g", ".weight_v", ".bias"))


@contextlib.contextmanager
def recorded_margins(store):
    """While active, every F.leaky_relu call appends min |x| / max |x| of its input to ``store``."""
    real = F.leaky_relu

    def spy(x, *a, **kw):
        with torch.no_grad():
            store.append(float(x.abs().min() / x.abs().max().clamp_min(1e-300)))
        return real(x, *a, **kw)
    F.leaky_relu = spy
    try:
        yield store
    finally:
        F.leaky_relu = real


def forward(name, cfg, sd, mel, dtype=torch.float64):
    """The generator's forward on leaf copies of the state dict's parameters -> (output, {key: leaf})."""
    leaves = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v))
        if is_param(k):
            t = t.to(dtype).clone().requires_grad_(True)
        leaves[k] = t
    y = torch_port.hifigan_trunk(torch.as_tensor(np.asarray(mel, np.float32)).to(dtype), leaves, cfg)
    if name == "hifigan":
        y = y[:, 0, :]
    else:
        assert name == "multiband-hifigan", name
    return y, {k: t for k, t in leaves.items() if is_param(k)}


def param_grad(name, cfg, sd, mel, c, dtype=torch.float64, margins=None):
    """d <c, G(mel)> / d parameter per state-dict key -> (output ndarray, {key: gradient ndarray}), evaluated in
    ``dtype``; ``margins``: a list that receives the kink margin of every activation."""
    with recorded_margins([] if margins is None else margins):
        y, leaves = forward(name, cfg, sd, mel, dtype)
    (y * torch.as_tensor(np.asarray(c)).to(dtype)).sum().backward()
    return y.detach().numpy(), {k: t.grad.numpy() for k, t in leaves.items()}


def float32_yardstick(name, cfg, sd, mel, c):
    """The float32 eager-autograd error of the same chain per parameter tensor, relative to the tensor's largest
    float64 gradient -> (worst, its key)."""
    n = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        _, g64 = param_grad(name, cfg, sd, mel, c)
        _, g32 = param_grad(name, cfg, sd, mel, c, dtype=torch.float32)
    finally:
        torch.set_num_threads(n)
    errs = {k: rel_err(g32[k], g64[k]) for k in g64}
    worst = max(errs, key=errs.get)
    return errs[worst], worst


def output_length(cfg, frames):
    """Samples the generator makes of ``frames`` mel frames (hifigan.py:44-51: padding u // 2 + u % 2, output
    padding u % 2)."""
    n = frames
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        n = convt_out_len(n, k, u, u // 2 + u % 2, u % 2)
    return n


def golden_inputs(seed):
    """(mel, cotangent) of the golden case from one RandomState seed."""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(-4.0, 1.0, GOLDEN_SHAPE).astype(np.float32)
    n = output_length(GOLDEN_CFG, GOLDEN_SHAPE[2])
    c = rs.randn(GOLDEN_SHAPE[0], n).astype(np.float32)
    return mel, c


def cotangent(shape, seed):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


# The chain cases of tests/cases.py at SMALL_B x SMALL_T.  Their maps hold up to 10^5 pre-activations each, so some lie
# within float32 rounding of a leaky-ReLU kink whatever the input: a float32 forward (eager torch on the CPU as much as
# the GPU's) that lands on the other side of one differs from float64 by a whole masked term -- with mel seed 5 the
# float32 CPU autograd of mb_s errs by 1.7e-2 on resblocks.5.convs1.2.weight_v through ONE such element (margin 1.1e-8).
# The mel seed of each case is therefore the one in 5..44 with the largest kink margin of the float64 forward
# (recorded beside it; tests/test_generator_grad_host.py checks the margin and that the float32 CPU forward takes the
# same side of every kink).
CHAIN_SEARCH = range(5, 45)
CHAIN_MEL_SEED = {"hifigan_s": (9, 2.60e-7), "hifigan_rb2": (35, 4.68e-6), "mb_s": (35, 6.16e-7)}
CHAIN_WEIGHT_SEED = 1
CHAIN_COTANGENT_SEED = 7


def chain_case(tag, mel_seed=None):
    """(model name, cfg, state dict, mel, cotangent) of a chain case of tests/cases.py."""
    from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
    from tests import cases
    name, cfg = next((n, c) for t, n, c in cases.SMALL if t == tag)
    sd = seeded_state_dict(name, cfg, seed=CHAIN_WEIGHT_SEED)
    mel = seeded_mel(cases.SMALL_T, seed=CHAIN_MEL_SEED[tag][0] if mel_seed is None else mel_seed, batch=cases.SMALL_B)
    n = output_length(cfg, cases.SMALL_T)
    c = cotangent((cases.SMALL_B, n) if name == "hifigan" else (cases.SMALL_B, 4, n), CHAIN_COTANGENT_SEED)
    return name, cfg, sd, mel, c


def kink_sides(name, cfg, sd, mel, dtype):
    """The side (x > 0) of every pre-activation of the forward evaluated in ``dtype``, one array per leaky ReLU."""
    out, real = [], F.leaky_relu

    def spy(x, *a, **kw):
        out.append((x.detach() > 0).numpy().copy())
        return real(x, *a, **kw)
    F.leaky_relu = spy
    try:
        with torch.no_grad():
            forward(name, cfg, sd, mel, dtype)
    finally:
        F.leaky_relu = real
    return out
