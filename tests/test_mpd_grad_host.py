"""Host tests of the multi-period discriminator's input gradient: the oracle (tests/mpd_grad_reference.py, float64
numpy) against the reference's own gradient (tests/golden/mpd_grad.npz) and against float64 torch autograd; the
adjoint identities; a numpy restatement of the tiling and LDS addressing of csrc/mpd_grad.hip against the formula;
the distance of the tiny cases from the kinks; the error of float32 eager autograd, the yardstick of the GPU
tolerances; the refusals of loss.generator_adversarial_terms; the ABI.

The tiny cases and the kinks.  Even the smallest input (every map one row high) leaves 2 x 2720 p activated values
and as many differences e - r per case, and a band of 1e-4 of a map's peak around zero catches 44 (p = 2) to 349
(p = 11) of them at best over 30 signal seeds, 50 to 318 for the cases stored: no seed gives none.  What a float32
forward cannot decide is a value below its own rounding, so the seeds are chosen (the first that does) such that no
float64 value lies within UNRESOLVED = 3e-7 (5 float32 ulps of the map's peak) of a kink, the criterion of the
full-size STFT-discriminator case (tests/test_mfd_grad_host.py); that count is asserted to be 0, the 1e-4 count is
printed, and nothing is excluded from any GPU comparison."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import Discriminator, DiscriminatorP, MultiPeriodDiscriminator
from fastvocoder_amd.loss import generator_adversarial_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import cases
from tests import mpd_grad_reference as mref
from tests import mpd_reference as ref

GOLDEN_RTOL = 1e-9       # float64 against float64


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mpd_grad.npz"))


@pytest.fixture(scope="module")
def mpd_sd(golden):
    return seeded_discriminator_state_dict("mpd", int(golden["seed"]))


def test_oracle_meets_the_reference_golden(golden, mpd_sd):
    assert int(golden["seed"]) == mref.SEEDS["mpd"]
    for i, p in enumerate(mref.PERIODS):
        est, real = golden[f"tiny{p}_est"], golden[f"tiny{p}_real"]
        assert est.shape == (2, 1, mref.TINY_T[p]) and est.shape[-1] <= 64 and est.shape[-1] % p
        a, b = mref.signals(int(golden["tiny_seeds"][i]), mref.TINY_T[p])
        assert np.array_equal(a, est) and np.array_equal(b, real)
        psd = mref.sub_state_dict(mpd_sd, i)
        errs = {"grad": _rel(mref.objective_grad("p", est, real, psd, period=p)[0], golden[f"tiny{p}_grad"]),
                "adv": _rel(mref.objective_grad("p", est, None, psd, period=p)[0], golden[f"tiny{p}_grad_adv"])}
        print(p, errs)
        assert max(errs.values()) <= GOLDEN_RTOL, (p, errs)
    est, real = golden["n2311_est"], golden["n2311_real"]
    errs = {"grad": _rel(mref.objective_grad("mpd", est, real, mpd_sd)[0], golden["n2311_grad"]),
            "adv": _rel(mref.objective_grad("mpd", est, None, mpd_sd)[0], golden["n2311_grad_adv"])}
    print("n2311", errs)
    assert max(errs.values()) <= GOLDEN_RTOL, errs


def test_discriminator_with_mpd_oracle_is_the_sum_of_its_parts():
    """Discriminator(use_mpd=True): 11 lists, so the MPD lists weigh 5 / 11 of the MPD's own objective and the MSD
    and MFD lists 6 / 11 of Discriminator()'s (the feature-map divisor is 6 for both first lists)."""
    from tests import mfd_grad_reference as fref
    sd = seeded_discriminator_state_dict("discriminator", mref.SEEDS["discriminator"], use_mpd=True)
    est, real = mref.signals(5, 1700, B=1)
    got, terms, differ = mref.objective_grad("discriminator", est, real, sd)
    mpd_sd = {k[4:]: v for k, v in sd.items() if k.startswith("mpd.")}
    a = mref.objective_grad("mpd", est, real, mpd_sd)[0]
    b = fref.objective_grad("discriminator", est, real, {k: v for k, v in sd.items() if not k.startswith("mpd.")})[0]
    assert differ == [] and _rel(got, 5 / 11 * a + 6 / 11 * b) <= 1e-12
    # and with float64's own maps as the decisions nothing changes (mfd_grad_reference.typed_conv_stack rounds its
    # slope 0.2 to float32 on that path: 7.5e-9 of it)
    maps = [[torch.from_numpy(np.ascontiguousarray(m)) if not torch.is_tensor(m) else m for m in lst]
            for lst in ref.discriminator_with_mpd(est.astype(np.float64), sd)]
    rmaps = ref.discriminator_with_mpd(real.astype(np.float64), sd)
    again, _, differ = mref.objective_grad("discriminator", est, real, sd, maps, rmaps)
    assert differ == [] and _rel(again, got) <= 1e-7


def test_adjoints():
    """<conv_h(x), g> = <x, conv_h_adjoint(g)> and <view(x), g> = <x, view_adjoint(g)> in float64."""
    rs = np.random.RandomState(1)
    for p in mref.PERIODS:
        for H in (1, 2, 3, 4, 5, 17):
            for k, stride in ((5, 3), (5, 1), (3, 1)):
                x, w = rs.randn(2, 3, H, p), rs.randn(4, 3, k)
                y = ref.conv_h(x, w, np.zeros(4), stride)
                g = rs.randn(*y.shape)
                lhs, rhs = (y * g).sum(), (x * mref.conv_h_adjoint(g, w, H, stride)).sum()
                assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (p, H, k, stride)
        for T in (p + 1, 2 * p, 4 * p + 1, 5 * p - 1, 64):
            x = rs.randn(2, 1, T)
            v = ref.view(x, p)
            g = rs.randn(*v.shape)
            lhs, rhs = (v * g).sum(), (x * mref.view_adjoint(g, T)).sum()
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (p, T)


def kernel_restatement(g_pre, w, H, p, NT):
    """What period_grad_kernel evaluates, tile by tile as it addresses LDS: the gradient line gs[co][i] with its
    p-word halo (n = n0 - p + i, zero outside [0, Hout p)), the three phases from the words n and n - p, and the
    output line whose word (3 (m - m0) + ph) p + c lands on flat input position (3 m0 - 2) p + word."""
    B, Cout, Hout, _ = g_pre.shape
    Cin = w.shape[1]
    flat = g_pre.reshape(B, Cout, Hout * p)
    dx = np.full((B, Cin, H * p), np.nan)
    total = ((H + 1) // 3 + 1) * p
    for n0 in range(0, total, NT):
        m0 = n0 // p
        gs = np.zeros((B, Cout, NT + p))
        for i in range(NT + p):
            n = n0 - p + i
            if 0 <= n < Hout * p:
                gs[:, :, i] = flat[:, :, n]
        line = np.full((B, Cin, 3 * (NT + 2 * p)), np.nan)
        for col in range(NT):
            n = n0 + col
            m, c = divmod(n, p)
            g0, g1 = gs[:, :, p + col], gs[:, :, col]
            for ph in range(3):
                acc = np.einsum("oc,bo->bc", w[:, :, ph], g0)
                if ph < 2:
                    acc = acc + np.einsum("oc,bo->bc", w[:, :, ph + 3], g1)
                line[:, :, (3 * (m - m0) + ph) * p + c] = acc
        base = (3 * m0 - 2) * p
        for word in range(line.shape[2]):
            rr, cc = divmod(word, p)
            nn = (m0 + rr // 3) * p + cc
            at = base + word
            if n0 <= nn < n0 + NT and 0 <= at < H * p:
                assert np.isnan(dx[:, :, at]).all()             # every position is written once
                dx[:, :, at] = line[:, :, word]
    return dx.reshape(B, Cin, H, p)


@pytest.mark.parametrize("p", mref.PERIODS)
def test_kernel_tiling_restated_in_numpy_meets_the_formula(p):
    rs = np.random.RandomState(p)
    w = rs.randn(3, 2, 5)
    for NT in (64, 128):
        for H in list(range(1, 41)) + [3 * (NT // p) + 1, 3 * (2 * NT // p) + 2]:
            g = rs.randn(1, 3, (H - 1) // 3 + 1, p)
            got = kernel_restatement(g, w, H, p, NT)
            assert not np.isnan(got).any(), (p, NT, H)          # all of dx is written
            assert _rel(got, mref.conv_h_adjoint(g, w, H, 3)) <= 1e-13, (p, NT, H)


def test_the_tiny_cases_keep_clear_of_unresolvable_kinks(golden, mpd_sd):
    for i, p in enumerate(mref.PERIODS):
        psd = mref.sub_state_dict(mpd_sd, i)
        est, real = golden[f"tiny{p}_est"], golden[f"tiny{p}_real"]
        wide = mref.kink_count("p", est, real, psd, period=p)
        near = mref.kink_count("p", est, real, psd, period=p, rel=mref.UNRESOLVED)
        print(f"period {p}: {wide} values within {mref.KINK_BAND:g} of a kink, {near} within {mref.UNRESOLVED:g}")
        assert near == 0, p


def yardsticks(golden, mpd_sd):
    threads = torch.get_num_threads()
    torch.set_num_threads(mref.YARDSTICK_THREADS)
    try:
        return _yardsticks(golden, mpd_sd)
    finally:
        torch.set_num_threads(threads)


def _yardsticks(golden, mpd_sd):
    out = {}
    worst = 0.0
    for cin, cout, p, H in mref.YARDSTICK_SHAPES:
        w, g_up, g_map, y = mref.period_conv_inputs(cin, cout, p, H)
        x = torch.zeros(2, cin, H, p, requires_grad=True)
        g = (torch.from_numpy(g_up) + torch.from_numpy(g_map)) * torch.where(torch.from_numpy(y) > 0, 1.0, 0.1)
        F.conv2d(x, torch.from_numpy(w)[..., None], stride=(3, 1), padding=(2, 0)).backward(g)
        worst = max(worst, _rel(x.grad.numpy(), mref.period_conv_input_grad(g_up, g_map, y, w, H)))
    out["period_conv"] = worst
    worst = 0.0
    for i, p in enumerate(mref.PERIODS):
        w = ref.folded(mpd_sd, f"discriminators.{i}.convs.0")[0].astype(np.float32)
        for T in (2310, 2311):
            rs = np.random.RandomState(T + p)
            H = (T + ref.reflect_tail(T, p)) // p
            g_up, y = (rs.randn(2, 32, (H - 1) // 3 + 1, p).astype(np.float32) for _ in range(2))
            x = torch.zeros(2, 1, T, requires_grad=True)
            v = F.pad(x, (0, ref.reflect_tail(T, p)), "reflect") if T % p else x
            g = torch.from_numpy(g_up) * torch.where(torch.from_numpy(y) > 0, 1.0, 0.1)
            F.conv2d(v.view(2, 1, -1, p), torch.from_numpy(w)[..., None], stride=(3, 1), padding=(2, 0)).backward(g)
            worst = max(worst, _rel(x.grad.numpy(), mref.first_input_grad(mref.mask(g_up, y), w, T, p)))
    out["first"] = worst
    worst = 0.0
    for i, p in enumerate(mref.PERIODS):
        psd = mref.sub_state_dict(mpd_sd, i)
        for real in (golden[f"tiny{p}_real"], None):
            want = mref.objective_grad("p", golden[f"tiny{p}_est"], real, psd, period=p)[0]
            worst = max(worst, _rel(mref.eager_grad("p", golden[f"tiny{p}_est"], real, psd, period=p)[0], want))
    out["tiny"] = worst
    worst = 0.0
    for real in (golden["n2311_real"], None):
        got, e_maps, r_maps = mref.eager_grad("mpd", golden["n2311_est"], real, mpd_sd)
        want = mref.objective_grad("mpd", golden["n2311_est"], real, mpd_sd, e_maps, r_maps)[0]
        worst = max(worst, _rel(got, want))
    out["n2311"] = worst
    return out


def test_float32_eager_autograd_error_is_the_yardstick(golden, mpd_sd):
    """The figures the GPU tolerances of tests/test_gpu_mpd_grad.py are set from (times 10): mpd_grad_reference's
    YARDSTICK must be what this test computes, so the bounds cannot drift away from the yardstick."""
    y = yardsticks(golden, mpd_sd)
    print("float32 eager autograd against float64: " + ", ".join(f"{k} {v:.2e}" for k, v in y.items()))
    assert all(0.0 < v <= 2e-6 for v in y.values()), y     # float32-class: the yardstick itself is sane
    assert set(y) == set(mref.YARDSTICK)
    for k, v in y.items():
        assert abs(mref.YARDSTICK[k] - v) <= 0.05 * v, (k, v, mref.YARDSTICK[k])


def test_float64_torch_autograd_meets_the_numpy_oracle(golden, mpd_sd):
    p, i = 5, 2
    psd = mref.sub_state_dict(mpd_sd, i)
    for real in (golden[f"tiny{p}_real"], None):
        a = mref.eager_grad("p", golden[f"tiny{p}_est"], real, psd, dtype=torch.float64, period=p)[0]
        assert _rel(a, mref.objective_grad("p", golden[f"tiny{p}_est"], real, psd, period=p)[0]) <= 1e-12


def test_refusals_and_the_keyword():
    x = torch.zeros(1, 1, 3000, requires_grad=True)
    for module in (Discriminator(use_mpd=True), MultiPeriodDiscriminator(), DiscriminatorP(3)):
        with pytest.raises(NotImplementedError, match="period convs.*period_grad=True"):
            generator_adversarial_terms(module, x)
        with pytest.raises(NotImplementedError, match="period convs"):
            generator_adversarial_terms(module, x, period_grad=False)
        with pytest.raises(_native.NativeError, match="ROCm device"):
            generator_adversarial_terms(module, x, period_grad=True)
        with pytest.raises(NotImplementedError, match="not differentiable.*period_grad=True"):
            module.differentiable = True
        assert module.differentiable is False and hasattr(module, "_graph_forward")
    with pytest.raises(_native.NativeError, match="ROCm device"):
        generator_adversarial_terms(Discriminator(), x, period_grad=True)      # the keyword changes nothing here


def test_header_and_sources():
    with open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    for name in ("fv_period_conv_input_grad", "fv_mpd_first_input_grad", "fv_pack_period_conv_grad"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert hasattr(_native.lib(), name)
    assert re.search(r"^int64_t fv_packed_period_conv_grad_floats\(", header, re.M)
    assert "mpd_grad.hip" in _native.SOURCES
    for name in ("period_conv_input_grad", "mpd_first_input_grad", "pack_period_conv_grad"):
        assert callable(getattr(_native, name))
    L = _native.lib()                                          # the size function's checks need no device
    assert L.fv_packed_period_conv_grad_floats(1024, 512) == 1024 * 512 * 5
    assert L.fv_packed_period_conv_grad_floats(128, 32) == 128 * 32 * 5
    assert L.fv_packed_period_conv_grad_floats(512, 32) == 0 and L.fv_packed_period_conv_grad_floats(128, 48) == 0
