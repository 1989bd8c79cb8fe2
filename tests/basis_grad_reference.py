"""Float64 oracles of Basis-MelGAN's parameter gradient (csrc/basis_grad.hip, generator/basis_grad.py,
loss.BasisWeightL1): numpy closed forms of the three kernels, and float64 / float32 torch autograd of the reference's
TWO-PASS graph (basis_melgan.py:140-162: the trunk on the mel and on zeros_like(mel), the two differences), composed
from oracle/torch_port.melgan_trunk(..., with_last=False), torch.relu, F.linear and torch_port.overlap_and_add.  The
one-pass form the GPU runs (B + 1 rows, the zero mel last) is restated here too, so that the host test can show on the
CPU that the two have one gradient.  The basis is a constant of both, as in the code under test.

The kink-margin recorder of tests/generator_grad_reference.py (every leaky ReLU) is extended to the final ReLU of BOTH
passes and, for the weight term, to ``weight - target``, whose sign the L1 gradient is.

TEST INFRASTRUCTURE ONLY; nothing here runs on the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_port
from tests.generator_grad_reference import (KINK, YARDSTICK_THREADS, cotangent, is_param, recorded_margins,  # noqa: F401
                                            rel_err)

BASIS_KEY = "basis_signal.layer.weight"

# the golden case (tests/golden/make_basis_param_grad_golden.py)
GOLDEN_CFG = dict(in_channels=80, out_channels=8, kernel_size=7, channels=[16, 8, 8], upsample_scales=[3, 2], L=6,
                  stack_kernel_size=3, stacks=3, use_weight_norm=True, use_causal_conv=False, transposedconv=True)
GOLDEN_WEIGHT_SEED = 3
GOLDEN_SHAPE = (2, 80, 6)


# ---- closed forms of the kernels ----
def head_forward(Y):
    """D[b] = relu(Y[b]) - relu(Y[B]), Y [B+1, C, F] -> [B, C, F], float64."""
    Y = np.asarray(Y, np.float64)
    return np.maximum(Y[:-1], 0.0) - np.maximum(Y[-1:], 0.0)


def head_grad(g_est, g_w, Y, basis):
    """g_Y [B+1, C, F] from g_est [B, F hop] or None and g_w [B, C, F] or None, float64:
    g_post[b, c, f] = sum_{j < L, f hop + j < F hop} basis[j, c] g_est[b, f hop + j] + g_w[b, c, f];
    rows b < B masked by Y[b] > 0, row B minus the batch sum masked by Y[B] > 0."""
    Y, basis = np.asarray(Y, np.float64), np.asarray(basis, np.float64)
    B, C, Fr = Y.shape[0] - 1, Y.shape[1], Y.shape[2]
    L = basis.shape[0]
    hop = L // 2
    post = np.zeros((B, C, Fr))
    if g_est is not None:
        ge = np.zeros((B, Fr * hop + L))                  # zeros behind the crop
        ge[:, :Fr * hop] = np.asarray(g_est, np.float64)
        for j in range(L):
            post += basis[j][None, :, None] * ge[:, None, j:j + Fr * hop:hop]
    if g_w is not None:
        post += np.asarray(g_w, np.float64)
    out = np.empty_like(Y)
    out[:B] = np.where(Y[:B] > 0, post, 0.0)
    out[B] = np.where(Y[B] > 0, -post.sum(axis=0), 0.0)
    return out


def weight_l1(D, target):
    """(mean |D^T - target|, mean D) of D [B, C, F] against target [B, F, C], float64."""
    D, target = np.asarray(D, np.float64), np.asarray(target, np.float64)
    return float(np.abs(D.transpose(0, 2, 1) - target).mean()), float(D.mean())


def weight_l1_grad(D, target, coef=1.0):
    """coef sign(D^T - target) / (B F C) in D's [B, C, F] storage; the difference is taken in float32, as the kernel and
    torch's L1 take it, so that sign(0) = 0 falls on the same elements."""
    diff = np.asarray(D, np.float32) - np.asarray(target, np.float32).transpose(0, 2, 1)
    return float(coef) * np.sign(diff).astype(np.float64) / diff.size


# ---- the whole chain ----
def frames(cfg, mel_frames):
    n = mel_frames
    for s in cfg["upsample_scales"]:
        n *= s
    return n


def _leaves(sd, dtype):
    leaves = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v))
        if is_param(k):
            t = t.to(dtype).clone()
            if k != BASIS_KEY:                              # the basis is a constant: the reference never steps it
                t.requires_grad_(True)
        leaves[k] = t
    return leaves


def _margin(x, store):
    if store is not None:
        with torch.no_grad():
            store.append(float(x.abs().min() / x.abs().max().clamp_min(1e-300)))


def forward(cfg, sd, mel, dtype=torch.float64, one_pass=False, relu_margins=None, sides=None):
    """BasisMelGANGenerator.forward on leaf copies of the state dict's trunk parameters -> (est [B, F hop], weight
    [B, F, C], {key: leaf}).  ``one_pass``: the B + 1-row form, the zero mel as the last row of ONE trunk call.
    ``relu_margins`` receives the kink margin of the final ReLU's input of every trunk call, ``sides`` its sign map."""
    leaves = _leaves(sd, dtype)
    L = cfg.get("L", 30)
    W = leaves[BASIS_KEY]
    x = torch.as_tensor(np.asarray(mel, np.float32)).to(dtype)

    def trunk(inp):
        y = torch_port.melgan_trunk(inp, leaves, cfg, with_last=False)
        _margin(y, relu_margins)
        if sides is not None:
            sides.append((y.detach() > 0).numpy().copy())
        return torch.relu(y)

    def head(w):
        w = w.contiguous().transpose(1, 2)
        s = torch_port.overlap_and_add(F.linear(w, W), L // 2)
        return s[:, : w.size(1) * (L // 2)], w

    if one_pass:
        r = trunk(torch.cat([x, torch.zeros_like(x[:1])]))
        est, weight = head(r[:-1] - r[-1:])
    else:
        zs, zw = head(trunk(torch.zeros_like(x)))
        s, w = head(trunk(x))
        est, weight = s - zs, w - zw
    return est, weight, {k: t for k, t in leaves.items() if is_param(k) and k != BASIS_KEY}


def param_grad(cfg, sd, mel, c_est, c_w, dtype=torch.float64, one_pass=False, margins=None):
    """d (<c_est, est> + <c_w, weight>) / d trunk parameter per state-dict key (either cotangent may be None) ->
    (est ndarray, weight ndarray, {key: gradient ndarray}) in ``dtype``; ``margins`` receives the kink margin of every
    leaky ReLU and of the final ReLU of both passes."""
    store = [] if margins is None else margins
    with recorded_margins(store):
        est, weight, leaves = forward(cfg, sd, mel, dtype, one_pass, relu_margins=store)
    total = 0.0
    if c_est is not None:
        total = total + (est * torch.as_tensor(np.asarray(c_est)).to(dtype)).sum()
    if c_w is not None:
        total = total + (weight * torch.as_tensor(np.asarray(c_w)).to(dtype)).sum()
    total.backward()
    return est.detach().numpy(), weight.detach().numpy(), {k: t.grad.numpy() for k, t in leaves.items()}


def float32_yardstick(cfg, sd, mel, c_est, c_w):
    """The float32 eager-autograd error of the two-pass chain per trunk parameter tensor, relative to the tensor's
    largest float64 gradient -> (worst over the tensors of more than one element, its key, worst over the one-element
    tensors)."""
    n = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        _, _, g64 = param_grad(cfg, sd, mel, c_est, c_w)
        _, _, g32 = param_grad(cfg, sd, mel, c_est, c_w, dtype=torch.float32)
    finally:
        torch.set_num_threads(n)
    errs = {k: rel_err(g32[k], g64[k]) for k in g64}
    many = {k: e for k, e in errs.items() if g64[k].size > 1}
    worst = max(many, key=many.get)
    return many[worst], worst, max([e for k, e in errs.items() if g64[k].size == 1], default=0.0)


def kink_sides(cfg, sd, mel, dtype):
    """The side (x > 0) of every pre-activation of the two-pass forward evaluated in ``dtype``: one array per leaky
    ReLU and per final ReLU, in call order."""
    out, real = [], F.leaky_relu

    def spy(x, *a, **kw):
        out.append((x.detach() > 0).numpy().copy())
        return real(x, *a, **kw)
    F.leaky_relu = spy
    try:
        with torch.no_grad():
            forward(cfg, sd, mel, dtype, sides=out)
    finally:
        F.leaky_relu = real
    return out


def golden_inputs(seed):
    """(mel, cotangent of est, target weights) of the golden case from one RandomState seed."""
    rs = np.random.RandomState(seed)
    mel = rs.uniform(-4.0, 1.0, GOLDEN_SHAPE).astype(np.float32)
    Fr = frames(GOLDEN_CFG, GOLDEN_SHAPE[2])
    c = rs.randn(GOLDEN_SHAPE[0], Fr * (GOLDEN_CFG["L"] // 2)).astype(np.float32)
    target = rs.uniform(0.0, 0.5, (GOLDEN_SHAPE[0], Fr, GOLDEN_CFG["out_channels"])).astype(np.float32)
    return mel, c, target


# The chain case of tests/cases.py at SMALL_B x SMALL_T.  As for MelGAN (tests/melgan_grad_reference.py), its mel seed
# is the one in 5..44 with the largest kink margin of the float64 forward, recorded beside it -- here the smallest
# over every leaky ReLU, the final ReLU of both passes and ``weight - target`` of the L1 term;
# tests/test_basis_grad_host.py checks the margin and that the float32 CPU forward takes the same side of every kink.
CHAIN_SEARCH = range(5, 45)
CHAIN_MEL_SEED = {"basis_s": (13, 3.29e-6)}
CHAIN_WEIGHT_SEED = 1
CHAIN_COTANGENT_SEED = 7
CHAIN_TARGET_SEED = 11


def chain_case(tag, mel_seed=None):
    """(cfg, state dict, mel, cotangent of est, cotangent of weight, target weights) of a chain case of tests/cases.py."""
    from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict
    from tests import cases
    cfg = next(c for t, _, c in cases.SMALL if t == tag)
    sd = seeded_state_dict("basis-melgan", cfg, seed=CHAIN_WEIGHT_SEED)
    mel = seeded_mel(cases.SMALL_T, seed=CHAIN_MEL_SEED[tag][0] if mel_seed is None else mel_seed, batch=cases.SMALL_B)
    Fr = frames(cfg, cases.SMALL_T)
    c_est = cotangent((cases.SMALL_B, Fr * (cfg["L"] // 2)), CHAIN_COTANGENT_SEED)
    c_w = cotangent((cases.SMALL_B, Fr, cfg["out_channels"]), CHAIN_COTANGENT_SEED + 1)
    target = np.random.RandomState(CHAIN_TARGET_SEED).uniform(0.0, 0.5, c_w.shape).astype(np.float32)
    return cfg, sd, mel, c_est, c_w, target


def chain_margin(tag, mel_seed=None):
    """The smallest kink margin of the float64 two-pass forward of a chain case: the leaky ReLUs, both final ReLUs and
    the L1 term's weight - target."""
    cfg, sd, mel, _, _, target = chain_case(tag, mel_seed)
    margins = []
    with torch.no_grad(), recorded_margins(margins):
        _, weight, _ = forward(cfg, sd, mel, relu_margins=margins)
        _margin(weight - torch.as_tensor(target).double(), margins)
    return min(margins)
