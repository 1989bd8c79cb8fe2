"""Host tests of the STFT discriminators' input gradient: the oracle (float64 autograd through
tests/mfd_grad_reference.py) against the reference's own gradient (tests/golden/mfd_grad.npz); the closed form the
kernel of csrc/stft_mag_grad.hip evaluates against float64 autograd; the distance of the seeded inputs from the clamp
and from the kinks of the chain; the error of float32 eager autograd, the yardstick of the GPU tolerances; the
refusals of loss.generator_adversarial_terms; the ABI."""
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
from tests import disc_grad_reference as gref
from tests import mfd_grad_reference as mref

GOLDEN_RTOL = 1e-9       # float64 against float64
from tests.mfd_grad_reference import DENSE_CASES, FULL_SEED, UNRESOLVED, full_signals  # noqa: E402


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "mfd_grad.npz"))
    return g, seeded_discriminator_state_dict("stft", int(g["seed"]), **mref.SMALL_STFT)


def test_oracle_meets_the_reference_golden(golden_dir):
    g, sd = _golden(golden_dir)
    for case in ("n400", "n1999"):
        est, real = g[f"{case}_est"], g[f"{case}_real"]
        errs = {"grad": _rel(mref.objective_grad("stft", est, real, sd, **mref.SMALL_STFT)[0], g[f"{case}_grad"]),
                "adv": _rel(mref.objective_grad("stft", est, None, sd, **mref.SMALL_STFT)[0], g[f"{case}_grad_adv"])}
        print(case, errs)
        assert max(errs.values()) <= GOLDEN_RTOL, (case, errs)


@pytest.mark.parametrize("n_fft,hop,win,n", mref.KERNEL_GRID)
def test_closed_form_meets_float64_autograd(n_fft, hop, win, n):
    x, gmag = mref.kernel_inputs(n_fft, hop, win, n)
    err = _rel(mref.magnitude_grad_closed_form(x, gmag, n_fft, hop, win),
               mref.magnitude_grad_autograd(x, gmag, n_fft, hop, win))
    print(f"closed form {(n_fft, hop, win, n)}: {err:.2e}")
    assert err <= 1e-12
    half = x.copy()
    half[:, :n // 2] = 0.0                          # silent frames: every bin clamped, no gradient through them
    err = _rel(mref.magnitude_grad_closed_form(half, gmag, n_fft, hop, win),
               mref.magnitude_grad_autograd(half, gmag, n_fft, hop, win))
    assert err <= 1e-12


def test_the_seeded_inputs_keep_clear_of_the_clamp_and_the_kinks(golden_dir):
    """A float32 forward and the float64 oracle must take the same side of the clamp and of every kink: no bin power
    of the kernel grid's inputs or of the n = 400 chain case lies within a factor 4 of 1e-7 (float64), and no
    pre-activation or e - r difference of the n = 400 case within 1e-4 x its map's largest magnitude of 0.  Nothing
    of the kind is asserted at n = 1999 (its count is printed); nothing is excluded from any GPU comparison."""
    for n_fft, hop, win, n in mref.KERNEL_GRID:
        x, _ = mref.kernel_inputs(n_fft, hop, win, n)
        assert mref.count_near_clamp(mref.bin_powers(x, n_fft, hop, win)) == 0, (n_fft, hop, win, n)
    g, sd = _golden(golden_dir)
    c = mref.SMALL_STFT
    for case in ("n400", "n1999"):
        _, est_p, p, _ = mref.objective_grad("stft", g[f"{case}_est"], g[f"{case}_real"], sd, **c)
        near = sum(mref.count_near_clamp(mref.bin_powers(g[f"{case}_{s}"], c["fft_size"], c["shift_size"],
                                                         c["win_length"], sd["window"])) for s in ("est", "real"))
        kinks = gref.kink_count(est_p, p)
        print(f"{case}: {near} bin powers near the clamp, {kinks} values within 1e-4 of a kink")
        if case == "n400":
            assert near == 0 and kinks == 0


def test_the_full_size_case_keeps_clear_of_unresolvable_kinks():
    """At n = 2400 the default modules hold 25 152 and 332 352 activated values, and hundreds of them lie within
    1e-4 of a kink for any signal; that cannot be avoided and is not asserted.  What float32 cannot do at all is
    give the sign of a pre-activation (or of e - r) that is smaller than its own rounding: a sum of float32
    products carries an error of a few ulps of the map's largest magnitude, so the side of zero of a float64 value
    below that is decided by the order of summation, not by the data, while one such mask deep in a stack is worth
    1e-3 of the input gradient's peak (DESIGN.md section 6.16 shows one in float64).  So the signal of the
    full-size case is seeded such that no float64 value of either module lies within 5 float32 ulps (3e-7) of its
    map's peak of a kink.  The criterion reads the float64 oracle only; nothing is excluded from the GPU
    comparison, and tests/test_gpu_mfd_grad.py's B = 16 case runs without any such choice."""
    est, real = full_signals()
    for kind in ("mfd", "discriminator"):
        sd = seeded_discriminator_state_dict(kind, FULL_SEED)
        _, est_p, p, _ = mref.objective_grad(kind, est, real, sd)
        n = sum(m.numel() for lst in est_p for m in lst[:-1])
        print(f"{kind}: {gref.kink_count(est_p, p)} of {n} values within 1e-4 of a kink, "
              f"{gref.kink_count(est_p, p, rel=UNRESOLVED)} within {UNRESOLVED:g}")
        assert gref.kink_count(est_p, p, rel=UNRESOLVED) == 0, kind


def yardsticks(golden_dir):
    """The error of float32 eager autograd on the CPU against float64, per case family of the GPU tests."""
    threads = torch.get_num_threads()
    torch.set_num_threads(mref.YARDSTICK_THREADS)
    try:
        return _yardsticks(golden_dir)
    finally:
        torch.set_num_threads(threads)


def _yardsticks(golden_dir):
    out = {}
    out["kernel"] = max(_rel(mref.magnitude_grad_autograd(*mref.kernel_inputs(*c), *c[:3], dtype=torch.float32),
                             mref.magnitude_grad_closed_form(*mref.kernel_inputs(*c), *c[:3]))
                        for c in mref.KERNEL_GRID)
    g, sd = _golden(golden_dir)
    worst = 0.0
    for case in ("n400", "n1999"):
        for real in (g[f"{case}_real"], None):
            want = mref.objective_grad("stft", g[f"{case}_est"], real, sd, **mref.SMALL_STFT)[0]
            got = mref.objective_grad("stft", g[f"{case}_est"], real, sd, dtype=torch.float32, **mref.SMALL_STFT)[0]
            worst = max(worst, _rel(got, want))
    out["small_chain"] = worst
    est, real = full_signals()
    worst = 0.0
    for kind in ("mfd", "discriminator"):
        sd = seeded_discriminator_state_dict(kind, FULL_SEED)
        for r in (real, None):
            want = mref.objective_grad(kind, est, r, sd)[0]
            worst = max(worst, _rel(mref.objective_grad(kind, est, r, sd, dtype=torch.float32)[0], want))
    out["full"] = worst
    worst = 0.0
    for cin, cout, k, T in DENSE_CASES:
        w, gy = mref.dense_grad_inputs(cin, cout, k, T)
        x = torch.zeros(gy.shape[0], cout, T + k - 1, requires_grad=True)
        F.conv1d(x, torch.from_numpy(w)).backward(torch.from_numpy(gy))
        worst = max(worst, _rel(x.grad.numpy(), gref.dense_input_grad(gy, w, 0)))
    out["dense"] = worst
    return out


def test_float32_eager_autograd_error_is_the_yardstick(golden_dir):
    """The figures the GPU tolerances of tests/test_gpu_mfd_grad.py are set from (times 10): mfd_grad_reference's
    YARDSTICK must be what this test computes, so the bounds cannot drift away from the yardstick."""
    y = yardsticks(golden_dir)
    print("float32 eager autograd against float64: " + ", ".join(f"{k} {v:.2e}" for k, v in y.items()))
    assert all(0.0 < v <= 2e-6 for v in y.values()), y     # float32-class: the yardstick itself is sane
    assert set(y) == set(mref.YARDSTICK)
    for k, v in y.items():
        assert abs(mref.YARDSTICK[k] - v) <= 0.05 * v, (k, v, mref.YARDSTICK[k])


def test_generator_adversarial_terms_refusals():
    x = torch.zeros(1, 1, 3000, requires_grad=True)
    for module in (Discriminator(use_mpd=True), MultiPeriodDiscriminator(), DiscriminatorP(3)):
        with pytest.raises(NotImplementedError, match="period convs"):
            generator_adversarial_terms(module, x)
    with pytest.raises(_native.NativeError, match="ROCm device"):
        generator_adversarial_terms(Discriminator(), x)
    with pytest.raises(TypeError):
        generator_adversarial_terms(torch.nn.Identity(), x)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        Discriminator().differentiable = True                  # the attribute still refuses


def test_header_and_sources():
    with open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert re.search(r"^int fv_stft_magnitude_bins_grad\(", header, re.M)
    assert re.search(r"^int64_t fv_stft_magnitude_bins_grad_workspace_bytes\(", header, re.M)
    for name in ("fv_stft_magnitude_bins_grad", "fv_stft_magnitude_bins_grad_workspace_bytes"):
        assert hasattr(_native.lib(), name)
    assert "stft_mag_grad.hip" in _native.SOURCES
    L = _native.lib()                                          # the size function's checks need no device
    assert L.fv_stft_magnitude_bins_grad_workspace_bytes(3, 700, 512, 50, 240) == 4 * 3 * 15 * 240
    assert L.fv_stft_magnitude_bins_grad_workspace_bytes(1, 700, 4096, 50, 240) == _native.ERR_UNSUPPORTED
    assert L.fv_stft_magnitude_bins_grad_workspace_bytes(1, 256, 512, 50, 240) == _native.ERR_INVALID_ARG
