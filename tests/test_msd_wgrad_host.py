"""Host tests of the multi-scale discriminator's parameter gradient: the closed forms of tests/msd_wgrad_reference.py,
which the kernels of csrc/disc_wgrad.hip evaluate, against float64 torch autograd; the oracle ``param_grad`` against
the reference's own gradient (tests/golden/msd_param_grad.npz); the distance of the short case from every kink, for
both signals; the error of float32 eager autograd, the yardstick of the GPU tolerances; the ``parameter_grad``
attribute; the ABI."""
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
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import cases
from tests import msd_wgrad_reference as wref

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_KW = dict(SMALL_MSD, downsample_scales=(4, 2))
GOLDEN_RTOL = 1e-12      # float64 against float64


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "msd_param_grad.npz"))
    return g, seeded_discriminator_state_dict("msd", int(g["seed"]), **SMALL_MSD)


def test_dense_weight_and_bias_gradient_meet_autograd():
    rs = np.random.RandomState(1)
    for cin, cout, k, pad, mode, T in ((1, 4, 15, 7, "reflect", 45), (1, 4, 15, 7, "reflect", 8), (4, 16, 5, 2, "zero", 9),
                                       (16, 1, 3, 1, "zero", 2), (3, 5, 5, 2, "zero", 1), (5, 3, 4, 0, "zero", 11)):
        x = torch.from_numpy(rs.randn(2, cin, T))
        w = torch.from_numpy(rs.randn(cout, cin, k)).requires_grad_(True)
        b = torch.from_numpy(rs.randn(cout)).requires_grad_(True)
        xp = F.pad(x, (pad, pad), mode="reflect") if mode == "reflect" else F.pad(x, (pad, pad))
        y = F.conv1d(xp, w, b)
        g = rs.randn(*y.shape)
        y.backward(torch.from_numpy(g))
        assert _rel(wref.dense_weight_grad(g, x.numpy(), k, pad, mode), w.grad.numpy()) <= 1e-13, (cin, cout, k, T)
        assert _rel(wref.bias_grad(g), b.grad.numpy()) <= 1e-13
    got = wref.dense_weight_grad(rs.randn(1, 16, 1), rs.randn(1, 16, 1), 5, 2)     # one sample: only the centre tap
    assert got[:, :, 2].all() and not got[:, :, [0, 1, 3, 4]].any()


def test_grouped_weight_gradient_meets_autograd():
    rs = np.random.RandomState(2)
    for cin, cout, k, s, pad, T in ((8, 8, 7, 1, 3, 33), (4, 1, 11, 1, 5, 40), (8, 4, 13, 2, 6, 100),
                                    (12, 48, 51, 5, 25, 97), (8, 32, 13, 2, 6, 3), (4, 16, 41, 4, 20, 45),
                                    (4, 8, 3, 5, 1, 40), (16, 64, 41, 4, 20, 130), (4, 16, 41, 4, 0, 46)):
        x = torch.from_numpy(rs.randn(2, cin, T))
        w = torch.from_numpy(rs.randn(cout, 4, k)).requires_grad_(True)
        y = F.conv1d(x, w, stride=s, padding=pad, groups=cin // 4)
        g = rs.randn(*y.shape)
        y.backward(torch.from_numpy(g))
        assert _rel(wref.grouped_weight_grad(g, x.numpy(), k, s, pad), w.grad.numpy()) <= 1e-13, (cin, cout, k, s, T)


def test_weight_norm_adjoint_meets_autograd():
    rs = np.random.RandomState(3)
    for shape in ((4, 1, 15), (16, 4, 41), (3, 1, 1), (2, 1024, 5)):
        v = torch.from_numpy(rs.randn(*shape)).requires_grad_(True)
        g = torch.from_numpy(rs.randn(shape[0], 1, 1)).requires_grad_(True)
        with torch.no_grad():
            g[0] = 0.0                                              # a row with g = 0: dv is 0, dg is not
        w = v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
        dw = rs.randn(*shape)
        w.backward(torch.from_numpy(dw))
        dv, dg = wref.weight_norm_grad(dw, v.detach().numpy(), g.detach().numpy())
        # a row of length 1 has dv = 0 by cancellation: the error is held against the size of the terms cancelled
        n = np.sqrt((v.detach().numpy() ** 2).sum(axis=(1, 2), keepdims=True))
        size = np.abs(g.detach().numpy() / n * dw).max()
        assert np.abs(dv - v.grad.numpy()).max() <= 1e-13 * size, shape
        assert _rel(dg, g.grad.numpy().reshape(-1)) <= 1e-13, shape
        assert not dv[0].any() and dg[0] != 0.0


def test_oracle_meets_the_reference_golden(golden_dir):
    g, sd = _golden(golden_dir)
    for case in ("short", "long"):
        grads, terms, _, _ = wref.param_grad(g[f"{case}_est"], g[f"{case}_real"], sd, **SMALL_KW)
        assert sorted(grads) == sorted(sd)
        errs = {k: _rel(grads[k], g[f"{case}_grad/{k}"]) for k in sd}
        worst = max(errs, key=errs.get)
        print(f"{case}: worst {worst} {errs[worst]:.2e}")
        assert errs[worst] <= GOLDEN_RTOL, (case, worst, errs[worst])
        assert abs(terms["real"] - float(g[f"{case}_real_loss"])) <= 1e-13 * abs(terms["real"])
        assert abs(terms["fake"] - float(g[f"{case}_fake_loss"])) <= 1e-13 * abs(terms["fake"])


def test_the_short_case_keeps_clear_of_every_kink_for_both_signals(golden_dir):
    """The real signal carries a gradient here too: no pre-activation of either signal's float64 forward lies within
    1e-4 x its map's largest magnitude of zero (RandomState(113); the short case of discriminator_grad.npz, seed 37,
    has one such value in the real signal's maps).  The long case's count is printed."""
    g, sd = _golden(golden_dir)
    _, _, est_p, p = wref.param_grad(g["short_est"], g["short_real"], sd, **SMALL_KW)
    assert wref.preactivation_kink_count(est_p) == 0
    assert wref.preactivation_kink_count(p) == 0
    _, _, est_p, p = wref.param_grad(g["long_est"], g["long_real"], sd, **SMALL_KW)
    print(f"long case: {wref.preactivation_kink_count(est_p)} (estimate) and {wref.preactivation_kink_count(p)} (real) "
          "pre-activations within 1e-4 of a kink")


def test_float32_eager_autograd_error_is_the_yardstick(golden_dir):
    """The error of float32 eager autograd of the same chain on the CPU against float64, per parameter tensor and
    relative to that tensor's largest magnitude: the figure a GPU error is held against (measured: 6.8e-7 for the
    short case, 9.3e-7 for the long one)."""
    g, sd = _golden(golden_dir)
    for case in ("short", "long"):
        want = wref.param_grad(g[f"{case}_est"], g[f"{case}_real"], sd, **SMALL_KW)[0]
        got = wref.param_grad(g[f"{case}_est"], g[f"{case}_real"], sd, dtype=torch.float32, **SMALL_KW)[0]
        errs = {k: _rel(got[k], want[k]) for k in sd}
        worst = max(errs, key=errs.get)
        print(f"float32 eager small MSD {case}: worst {worst} {errs[worst]:.2e}")
        assert errs[worst] <= 1e-5                               # float32-class: the yardstick itself is sane


def test_parameter_grad_defaults_setters_and_refusals():
    one, msd = MelGANDiscriminator(**SMALL_MSD), MelGANMultiScaleDiscriminator(**SMALL_MSD)
    assert one.parameter_grad is False and msd.parameter_grad is False
    keys = list(msd.state_dict())
    msd.parameter_grad = True
    assert msd.parameter_grad is True and all(d.parameter_grad is True for d in msd.discriminators)
    assert msd.differentiable is False                           # the two attributes are independent
    assert list(msd.state_dict()) == keys
    assert MelGANMultiScaleDiscriminator(**SMALL_MSD).parameter_grad is False    # not shared state
    msd.parameter_grad = False
    assert all(d.parameter_grad is False for d in msd.discriminators)
    msd.discriminators[1].parameter_grad = True
    assert msd.parameter_grad is False                           # "all scales"
    for module in (Discriminator(), STFTDiscriminator(), MultiResolutionSTFTDiscriminator(), DiscriminatorP(3),
                   MultiPeriodDiscriminator()):
        assert module.parameter_grad is False
        module.parameter_grad = False
        with pytest.raises(NotImplementedError, match="MelGANMultiScaleDiscriminator"):
            module.parameter_grad = True
        assert module.parameter_grad is False


def test_step_terms_refuses_the_other_modules():
    from fastvocoder_amd.loss import discriminator_step_terms
    x = torch.zeros(1, 1, 4000)
    for module in (Discriminator(), STFTDiscriminator(), MultiResolutionSTFTDiscriminator(), DiscriminatorP(3),
                   MultiPeriodDiscriminator()):
        with pytest.raises(NotImplementedError, match="MelGANMultiScaleDiscriminator"):
            discriminator_step_terms(module, x, x)


def test_header_and_sources():
    with open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    for name in ("fv_conv1d_weight_grad", "fv_grouped_conv1d_weight_grad", "fv_weight_norm_grad"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert hasattr(_native.lib(), name)
    assert re.search(r"^int64_t fv_conv_weight_grad_workspace_bytes\(", header, re.M)
    assert hasattr(_native.lib(), "fv_conv_weight_grad_workspace_bytes")
    assert re.search(r"^#define FV_ABI_VERSION 18\b", header, re.M)
    assert "disc_wgrad.hip" in _native.SOURCES
    L = _native.lib()
    # the query refuses what the entries refuse, and sizes S records of Cout Cin k + Cout floats
    assert L.fv_conv_weight_grad_workspace_bytes(1, 1, 6, 3, 100, 5, 1, 2, 0) == _native.ERR_UNSUPPORTED
    assert L.fv_conv_weight_grad_workspace_bytes(1, 1, 8, 4, 100, 301, 1, 0, 0) == _native.ERR_INVALID_ARG
    assert L.fv_conv_weight_grad_workspace_bytes(0, 1, 4, 4, 10, 5, 1, 2, 7) == _native.ERR_UNSUPPORTED
    assert L.fv_conv_weight_grad_workspace_bytes(0, 1, 4, 4, 3, 15, 1, 7, 1) == _native.ERR_INVALID_ARG
    need = L.fv_conv_weight_grad_workspace_bytes(0, 2, 1024, 1024, 131, 5, 1, 2, 0)
    assert need > 0 and need % (4 * (1024 * 1024 * 5 + 1024)) == 0
