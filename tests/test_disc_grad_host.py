"""Host tests of the discriminator input gradient: the oracle (float64 autograd through
tests/discriminator_reference.py) against the reference's own gradient (tests/golden/discriminator_grad.npz); the
closed forms of tests/disc_grad_reference.py, which the kernels of csrc/disc_grad.hip evaluate, against float64 torch
autograd; the distance of the committed inputs from the kinks of the chain; the error of float32 eager autograd, the
yardstick of the GPU tolerances; the ``differentiable`` attribute; the ABI."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANDiscriminator,
                                           MelGANMultiScaleDiscriminator, MultiPeriodDiscriminator,
                                           MultiResolutionSTFTDiscriminator, STFTDiscriminator)
from fastvocoder_amd.loss.discriminator_loss import grad_coefficients
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import cases
from tests import disc_grad_reference as gref
from tests import discriminator_reference as ref

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_KW = dict(SMALL_MSD, downsample_scales=(4, 2))
GOLDEN_RTOL = 1e-9       # float64 against float64

# (Cin, Cout, k, stride, pad, Tin): (Tin + 2 pad - k) % stride != 0, Tin < k, stride > k, one output, Cout/groups 1..16
GROUPED_CASES = [(8, 8, 7, 1, 3, 33), (4, 1, 11, 1, 5, 40), (8, 4, 13, 2, 6, 100), (4, 8, 31, 3, 15, 77),
                 (12, 48, 51, 5, 25, 97), (8, 32, 13, 2, 6, 3), (4, 16, 41, 4, 20, 30), (4, 16, 41, 4, 0, 46),
                 (4, 4, 3, 5, 0, 40), (16, 64, 41, 4, 20, 130), (4, 4, 9, 2, 1, 24)]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "discriminator_grad.npz"))
    return g, seeded_discriminator_state_dict("msd", int(g["seed"]), **SMALL_MSD)


def test_oracle_meets_the_reference_golden(golden_dir):
    g, sd = _golden(golden_dir)
    for case in ("short", "long"):
        est, real = g[f"{case}_est"], g[f"{case}_real"]
        errs = {"grad": _rel(gref.chain_grad(est, real, sd, **SMALL_KW)[0], g[f"{case}_grad"]),
                "fake": _rel(gref.chain_grad(est, real, sd, ("fake",), **SMALL_KW)[0], g[f"{case}_grad_fake"]),
                "scale1": _rel(gref.chain_grad(est, real, sd, scale=1, **SMALL_KW)[0], g[f"{case}_grad_scale1"])}
        print(case, errs)
        assert max(errs.values()) <= GOLDEN_RTOL, (case, errs)


def test_polyphase_grouped_input_gradient_meets_autograd():
    rs = np.random.RandomState(1)
    for cin, cout, k, s, pad, T in GROUPED_CASES:
        x = torch.from_numpy(rs.randn(2, cin, T)).requires_grad_(True)
        w = rs.randn(cout, 4, k)
        y = F.conv1d(x, torch.from_numpy(w), stride=s, padding=pad, groups=cin // 4)
        g = rs.randn(*y.shape)
        y.backward(torch.from_numpy(g))
        got = gref.grouped_input_grad(g, w, cin, T, k, s, pad)
        assert _rel(got, x.grad.numpy()) <= 1e-13, (cin, cout, k, s, pad, T)
        last = (y.shape[-1] - 1) * s - pad + k
        assert not got[:, :, max(last, 0):].any()


def test_dense_fold_pool_and_mask_meet_autograd():
    rs = np.random.RandomState(2)
    for cin, cout, k, pad, T in ((1, 4, 15, 0, 40), (4, 16, 5, 2, 9), (16, 1, 3, 1, 2), (3, 5, 5, 2, 3)):
        x = torch.from_numpy(rs.randn(2, cin, T)).requires_grad_(True)
        w = rs.randn(cout, cin, k)
        y = F.conv1d(x, torch.from_numpy(w), padding=pad)
        g = rs.randn(*y.shape)
        y.backward(torch.from_numpy(g))
        assert _rel(gref.dense_input_grad(g, w, pad), x.grad.numpy()) <= 1e-13, (cin, cout, k, pad, T)
    for T, P in ((8, 7), (9, 7), (30, 7), (5, 0), (2, 1), (16, 2)):                # T = P + 1 among them
        x = torch.from_numpy(rs.randn(2, 3, T)).requires_grad_(True)
        y = F.pad(x, (P, P), mode="reflect") if P else x * 1.0
        g = rs.randn(*y.shape)
        y.backward(torch.from_numpy(g))
        assert _rel(gref.reflect_fold(g, P), x.grad.numpy()) <= 1e-15, (T, P)
    for T in (2, 3, 5, 8, 31, 32):                                                 # odd T: a partial last window
        for k, s, p in ((4, 2, 1), (4, 2, 2), (3, 1, 1), (5, 3, 0), (2, 3, 0)):
            if T + 2 * p < k:
                continue
            x = torch.from_numpy(rs.randn(2, 1, T)).requires_grad_(True)
            y = ref.avg_pool(x, k, s, p)
            assert torch.allclose(y, F.avg_pool1d(x, k, s, p, count_include_pad=False), rtol=1e-13, atol=0)
            g = rs.randn(*y.shape)
            y.backward(torch.from_numpy(g))
            assert _rel(gref.avg_pool_input_grad(g, T, k, s, p), x.grad.numpy()) <= 1e-14, (T, k, s, p)
    pre = torch.from_numpy(rs.randn(2, 3, 50))
    pre[..., ::5] = 0.0
    pre.requires_grad_(True)
    y = F.leaky_relu(pre, 0.2)
    g = rs.randn(2, 3, 50)
    y.backward(torch.from_numpy(g))
    assert np.array_equal(gref.map_grad(g[None][0] * 0.5, g * 0.5, y.detach().numpy(), 0.2), pre.grad.numpy())
    assert np.array_equal(gref.map_grad(None, g, None, 1.0), g)


def test_score_gradient_formula_and_divisors_meet_autograd():
    rs = np.random.RandomState(3)
    lengths, B = [3, 2, 3], 2                                   # the divisor uses the FIRST list's length for all
    shapes = [[(B, 2, 7), (B, 3, 5), (B, 1, 4)], [(B, 2, 6), (B, 1, 3)], [(B, 4, 3), (B, 2, 2), (B, 1, 2)]]
    est_p = [[torch.from_numpy(rs.randn(*s)).requires_grad_(True) for s in lst] for lst in shapes]
    p = [[torch.from_numpy(rs.randn(*s)) for s in lst] for lst in shapes]
    with torch.no_grad():
        est_p[0][0][0, 0, :3] = p[0][0][0, 0, :3]               # e == r: sign 0
    g_terms = [0.7, -1.3, 5.0, 0.4, 0.25]
    t = gref.terms(est_p, p)
    sum(c * t[k] for c, k in zip(g_terms, ("adversarial", "feature_map", "real", "fake", "discriminator"))).backward()
    flat_e = [m for lst in est_p for m in lst]
    flat_r = [m for lst in p for m in lst]
    counts = [m[0].numel() for m in flat_e]
    coef = gref.score_coefficients(g_terms, counts, lengths, B)
    lib_coef = grad_coefficients(g_terms, counts, lengths, B)
    for m, (e, r) in enumerate(zip(flat_e, flat_r)):
        assert np.allclose(coef[m], lib_coef[m], rtol=1e-15, atol=0), m
        want = e.grad.numpy()
        assert _rel(gref.score_grad(e.detach().numpy(), r.numpy(), *coef[m]), want) <= 1e-14, m
    assert not est_p[0][0].grad[0, 0, :3].any()
    want = ref.scores([[m.detach() for m in lst] for lst in est_p], p)
    assert all(abs(float(t[k]) - v) <= 1e-14 * abs(v) for k, v in want.items())


def test_the_short_case_keeps_clear_of_every_kink(golden_dir):
    """A float32 forward and the float64 oracle must not disagree on the side of zero of a pre-activation or of a
    feature-map difference: no value of the oracle lies within 1e-4 x its map's largest magnitude of zero for the
    short case (B = 2, 45 samples, 2000 values; seeds searched on the CPU).  At about 2000 samples a count of 0 cannot
    be had by choosing seeds: 84 136 values, of which 150 to 210 lie inside the band for every seed tried (a smooth
    density near zero times the band's width); the long case is compared on the GPU all the same, nothing
    excluded, and its count is printed here."""
    g, sd = _golden(golden_dir)
    _, est_p, p = gref.chain_grad(g["short_est"], g["short_real"], sd, **SMALL_KW)
    assert gref.kink_count(est_p, p) == 0
    _, est_p, p = gref.chain_grad(g["long_est"], g["long_real"], sd, **SMALL_KW)
    n = sum(m.numel() for lst in est_p for m in lst[:-1])
    print(f"long case: {gref.kink_count(est_p, p)} of {n} values within 1e-4 of a kink")


def test_float32_eager_autograd_error_is_the_yardstick(golden_dir):
    """The error of float32 eager autograd on the CPU against the float64 oracle, on the cases of the GPU tests: the
    figures the GPU tolerances are set from (times 10) until an MI355X run has produced measured ones."""
    g, sd = _golden(golden_dir)
    worst = 0.0
    for case in ("short", "long"):
        est, real = g[f"{case}_est"], g[f"{case}_real"]
        for which in (("adversarial", "feature_map"), ("fake",)):
            want = gref.chain_grad(est, real, sd, which, **SMALL_KW)[0]
            got = gref.chain_grad(est, real, sd, which, dtype=torch.float32, **SMALL_KW)[0]
            err = _rel(got, want)
            worst = max(worst, err)
            print(f"float32 eager small MSD {case} {which}: {err:.2e}")
    rs = np.random.RandomState(1)
    kworst = 0.0
    for cin, cout, k, s, T in ((4, 16, 41, 4, 2001), (16, 64, 41, 4, 1030), (12, 48, 51, 5, 4097)):
        pad = (k - 1) // 2
        w = (rs.randn(cout, 4, k) / np.sqrt(4 * k)).astype(np.float32)
        gy = rs.randn(3, cout, (T + 2 * pad - k) // s + 1).astype(np.float32)
        x = torch.zeros(3, cin, T, requires_grad=True)
        F.conv1d(x, torch.from_numpy(w), stride=s, padding=pad, groups=cin // 4).backward(torch.from_numpy(gy))
        kworst = max(kworst, _rel(x.grad.numpy(), gref.grouped_input_grad(gy, w, cin, T, k, s, pad)))
    print(f"float32 eager: worst chain error {worst:.2e}, worst grouped conv backward {kworst:.2e}")
    assert worst <= 1e-4 and kworst <= 1e-5                      # float32-class: the yardstick itself is sane


def test_differentiable_defaults_setters_and_refusals():
    one, msd = MelGANDiscriminator(**SMALL_MSD), MelGANMultiScaleDiscriminator(**SMALL_MSD)
    assert one.differentiable is False and msd.differentiable is False
    keys = list(msd.state_dict())
    msd.differentiable = True
    assert msd.differentiable is True and all(d.differentiable is True for d in msd.discriminators)
    assert list(msd.state_dict()) == keys
    assert MelGANMultiScaleDiscriminator(**SMALL_MSD).differentiable is False     # not shared state
    msd.differentiable = False
    assert all(d.differentiable is False for d in msd.discriminators)
    for module in (Discriminator(), STFTDiscriminator(), MultiResolutionSTFTDiscriminator(), DiscriminatorP(3),
                   MultiPeriodDiscriminator()):
        assert module.differentiable is False
        module.differentiable = False
        with pytest.raises(NotImplementedError, match="not differentiable"):
            module.differentiable = True
        assert module.differentiable is False


def test_header_and_sources():
    with open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    for name in ("fv_grouped_conv1d_input_grad", "fv_disc_map_grad", "fv_reflect_pad_fold", "fv_avg_pool1d_input_grad",
                 "fv_disc_score_grad"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert hasattr(_native.lib(), name)
    assert "disc_grad.hip" in _native.SOURCES
