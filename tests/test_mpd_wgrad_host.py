"""CPU tests of the oracle behind tests/test_gpu_mpd_wgrad.py (tests/mpd_wgrad_reference.py): it meets the reference's
own parameter gradient (tests/golden/mpd_mfd_param_grad.npz), its closed forms meet float64 torch autograd, the
float32 eager-autograd yardsticks are the pinned ones, the tiny chain cases keep clear of the leaky-ReLU kinks, and
discriminator_step_terms admits the STFT and period discriminators only with their keywords."""
import os
import re

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANMultiScaleDiscriminator,
                                           MultiPeriodDiscriminator, MultiResolutionSTFTDiscriminator,
                                           STFTDiscriminator)
from fastvocoder_amd.loss import discriminator_step_terms
from tests import mpd_reference as ref
from tests import mpd_wgrad_reference as wref

GOLDEN_RTOL = 1e-9
TINY = [f"p{p}" for p in ref.PERIODS] + ["stft"]
GOLDEN_CASES = TINY + ["mfd", "discriminator_mpd"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mpd_mfd_param_grad.npz"))


@pytest.fixture
def four_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(wref.YARDSTICK_THREADS)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_the_oracle_meets_the_reference_gradient(golden, name):
    kind, kw = wref.case_kind(name)
    est, real = wref.case_signals(name)
    assert np.array_equal(est, golden[f"{name}_est"]) and np.array_equal(real, golden[f"{name}_real"])
    sd = wref.case_state_dict(name)
    grads, terms, _, _ = wref.param_grad(kind, est, real, sd, **kw)
    assert sorted(grads) == sorted(k for k in sd if wref.is_param(k))
    worst = 0.0
    for k, g in grads.items():
        got, norm = wref.sample(g)
        want = golden[f"{name}_grad/{k}"]
        assert got.shape == want.shape and (g.size <= wref.SAMPLE or got.size == wref.SAMPLE), k
        worst = max(worst, wref.rel_err(got, want) if np.abs(want).max() > 0 else float(np.abs(got).max()),
                    abs(norm - float(golden[f"{name}_norm/{k}"])) / max(float(golden[f"{name}_norm/{k}"]), 1e-300))
    print(f"{name}: oracle against the reference's gradient {worst:.2e}")
    assert worst <= GOLDEN_RTOL, worst
    assert abs(terms["real"] - float(golden[f"{name}_real_loss"])) <= GOLDEN_RTOL * terms["real"]
    assert abs(terms["fake"] - float(golden[f"{name}_fake_loss"])) <= GOLDEN_RTOL * terms["fake"]


def test_the_golden_is_small_and_data_only(golden_dir):
    path = os.path.join(golden_dir, "mpd_mfd_param_grad.npz")
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir)
                                        if f != "mpd_mfd_param_grad.npz")
    with np.load(path, allow_pickle=False) as g:
        assert all(g[k].dtype.kind in "fi" for k in g.files)


def test_the_closed_forms_meet_float64_autograd():
    for cin, cout, k, stride in ((3, 5, 5, 3), (4, 2, 5, 1), (6, 1, 3, 1), (2, 3, 3, 2)):
        for p in (2, 3, 11):
            for H in (1, 2, 3, 4, 5, 10):
                g, x = wref.kernel_inputs(cin, cout, k, stride, p, H, 2)
                dw, db = wref.period_conv_weight_grad(g, x, k, stride)
                adw, adb = wref.eager_weight_grad(g, x, k, stride, torch.float64)
                assert wref.rel_err(dw, adw) <= 1e-13 and wref.rel_err(db, adb) <= 1e-13, (cin, cout, k, stride, p, H)
    for p in ref.PERIODS:
        for T in (p // 2 + 1, 6 * p - 1, 6 * p, 6 * p + 1):
            g, x = wref.first_inputs(p, T, 2)
            dw, db = wref.first_weight_grad(g, x, p)
            adw, adb = wref.eager_first_weight_grad(g, x, p, torch.float64)
            assert wref.rel_err(dw, adw) <= 1e-13 and wref.rel_err(db, adb) <= 1e-13, (p, T)


def _pinned(name, got):
    want = wref.YARDSTICK[name]
    print(f"yardstick {name}: float32 eager autograd against float64 {got:.3e} (pinned {want:.3e})")
    assert abs(got - want) <= 0.05 * want, (name, got, want)


def test_float32_eager_autograd_error_of_the_kernels_is_the_yardstick(four_threads):
    for name, got in wref.kernel_yardsticks().items():
        _pinned(name, got)


@pytest.mark.parametrize("family", ["p", "stft", "full"])
def test_float32_eager_autograd_error_of_the_chains_is_the_yardstick(four_threads, family):
    _pinned(family, wref.chain_yardstick(family))


def test_the_tiny_cases_keep_clear_of_the_kinks():
    for name in TINY:
        count = wref.case_unresolved(name)
        print(f"{name}: {count} pre-activations within {wref.UNRESOLVED:g} of their map's peak of a kink")
        assert count == 0, name


def _modules():
    small = STFTDiscriminator(**wref.SMALL_STFT)
    return [(small, {"stft_grad"}, 2), (MultiResolutionSTFTDiscriminator(), {"stft_grad"}, 3),
            (DiscriminatorP(3), {"period_grad"}, 3), (MultiPeriodDiscriminator(), {"period_grad"}, 3),
            (Discriminator(), {"stft_grad"}, 3), (Discriminator(use_mpd=True), {"stft_grad", "period_grad"}, 3)]


def test_the_keywords_admit_the_modules_and_nothing_else_does():
    for module, need, dims in _modules():
        x = torch.zeros((1, 4000) if dims == 2 else (1, 1, 4000))
        name = type(module).__name__
        for given in (set(), {"stft_grad"}, {"period_grad"}, {"stft_grad", "period_grad"}):
            kw = {k: True for k in given}
            if need <= given:          # admitted: on CPU tensors the call reaches the device check
                with pytest.raises(_native.NativeError, match="ROCm device"):
                    discriminator_step_terms(module, x, x, **kw)
            else:
                with pytest.raises(NotImplementedError, match="MelGANMultiScaleDiscriminator") as e:
                    discriminator_step_terms(module, x, x, **kw)
                assert all(f"{k}=True" in str(e.value) for k in need - given), (name, str(e.value))
        with pytest.raises(NotImplementedError, match="MelGANMultiScaleDiscriminator"):
            module.parameter_grad = True                         # the attribute stays refused
        assert module.parameter_grad is False
    msd = MelGANMultiScaleDiscriminator()
    x = torch.zeros(1, 1, 4000)
    for kw in ({}, {"stft_grad": True}, {"period_grad": True}, {"stft_grad": True, "period_grad": True}):
        with pytest.raises(_native.NativeError, match="ROCm device"):
            discriminator_step_terms(msd, x, x, **kw)
    with pytest.raises(TypeError):
        discriminator_step_terms(msd, x, x, True)                # keyword-only
    with pytest.raises(NotImplementedError, match="MelGANMultiScaleDiscriminator"):
        discriminator_step_terms(torch.nn.Conv1d(1, 1, 1), x, x, stft_grad=True, period_grad=True)


def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    for name in ("fv_period_conv_weight_grad", "fv_period_conv_weight_grad_workspace_bytes",
                 "fv_mpd_first_weight_grad", "fv_mpd_first_weight_grad_workspace_bytes"):
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert "mpd_wgrad.hip" in _native.SOURCES
    assert os.path.exists(os.path.join(ROOT, "fastvocoder_amd", "csrc", "mpd_wgrad.hip"))
    assert _native.PERIOD_WGRAD_UNIT == 32 and _native.PERIOD_WGRAD_CHUNK == 1024
