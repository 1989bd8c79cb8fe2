"""Host tests of the STFT loss gradient: the float64 oracle (tests/stft_loss_grad_reference.py) against the
reference's own autograd values (tests/golden/stft_loss_grad.npz), against float64 torch autograd and against finite
differences; the ``differentiable`` attribute; the PQMF synthesis adjoint; the ABI."""
import os
import re

import numpy as np
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.loss import Loss, MultiResolutionSTFTLoss, STFTLoss
from tests import cases
from tests import stft_loss_grad_reference as gref
from tests import stft_loss_reference as ref
from tests.stft_reference import stft
from tests.test_gpu_stft_loss import _pairs

# float64 against float64: the oracle meets the reference's autograd within 3e-12 here (relative L2)
GOLDEN_RTOL = 1e-9


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_oracle_meets_the_reference_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "stft_loss_grad.npz"))
    assert d["x"].shape[1] >= 1025 and d["x"].shape[1] % 4 == 0
    x, y = d["x"].astype(np.float64), d["y"].astype(np.float64)
    g_sc, g_mag = gref.multi_resolution_stft_loss(x, y)
    errs = {"sc": _rel(g_sc, d["g_sc"]), "mag": _rel(g_mag, d["g_mag"]),
            "single": _rel(gref.loss_single_band(x, y), d["g_single"]),
            "multi": _rel(gref.loss_multiband(d["est_sub"].astype(np.float64), y, d["analysis_filter"],
                                              d["synthesis_filter"]), d["g_multi"])}
    print(errs)
    assert max(errs.values()) <= GOLDEN_RTOL, errs
    p_sc, p_mag = gref.per_utterance(x, y)                       # a row alone: B = 1 of the same function
    assert _rel(p_sc[1:], gref.multi_resolution_stft_loss(x[1:], y[1:])[0]) == 0.0 and p_mag.shape == x.shape


def _torch_chain(x, y, nf, hop, wl, w):
    def mag(v):
        S = torch.stft(v, nf, hop, wl, w, return_complex=True)
        return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-7))
    X, Y = mag(x), mag(y)
    return ((Y - X) ** 2).sum(), (torch.log(Y) - torch.log(X)).abs().sum()


def test_oracle_meets_float64_torch_autograd():
    rs = np.random.RandomState(11)
    for nf, hop, wl, n, window in ((1024, 77, 1024, 5003, "hann_window"), (2048, 333, 601, 7001, "hamming_window"),
                                   (512, 50, 240, 257, "hann_window"), (1024, 120, 600, 4000, "hamming_window")):
        x, y = rs.uniform(-1, 1, (2, n)), rs.uniform(-1, 1, (2, n))
        w = getattr(torch, window)(wl, dtype=torch.float64)
        for term in (0, 1):
            tx = torch.from_numpy(x).requires_grad_(True)
            _torch_chain(tx, torch.from_numpy(y), nf, hop, wl, w)[term].backward()
            got = gref.grad_sums(x, y, nf, hop, wl, window=w.numpy())[term]
            assert _rel(got, tx.grad.numpy()) <= GOLDEN_RTOL, (nf, hop, wl, n, window, term)


def test_oracle_meets_central_finite_differences():
    rs = np.random.RandomState(12)
    n = 1500
    x, y = rs.uniform(-1, 1, (1, n)), rs.uniform(-1, 1, (1, n))
    g = gref.loss_single_band(x, y)
    h = 1e-6
    for i in (0, 1, 7, 255, 256, 700, n - 2, n - 1):             # the reflected edges among them
        e = np.zeros_like(x)
        e[0, i] = h
        fd = (ref.loss_single_band(x + e, y) - ref.loss_single_band(x - e, y)) / (2 * h)
        assert abs(fd - g[0, i]) <= 1e-5 * np.abs(g).max(), (i, fd, g[0, i])


def test_identical_signals_have_a_zero_oracle_gradient():
    x = np.random.RandomState(13).uniform(-1, 1, (2, 3000))
    g_sc, g_mag = gref.multi_resolution_stft_loss(x, x.copy())
    assert not g_sc.any() and not g_mag.any()


def test_float32_keeps_the_broadband_bins_on_their_side_of_the_clamp(golden_dir):
    """The GPU test excludes the frames in which the device's float32 spectrum puts a bin on the other side of a jump
    of the mag gradient than float64, at most 1 % of them.  The signals fit that cap: with the float32 oracle in the
    device's place, the share of frames with a bin of x across the 1e-7 clamp stays under it for every pair."""
    for name, (x, _, _) in _pairs(golden_dir).items():
        x32 = x.astype(np.float32)
        for nf, hop, wl in ref.RESOLUTIONS:
            s64, s32 = stft(x32.astype(np.float64), nf, hop, wl), stft(x32, nf, hop, wl, dtype=np.float32)
            flip = ((s64.real ** 2 + s64.imag ** 2) > 1e-7) != ((s32.real ** 2 + s32.imag ** 2) > np.float32(1e-7))
            share = float(flip.any(axis=-1).mean())
            print(f"{name} n_fft={nf}: clamp flips in {100 * share:.3f} % of the frames")
            assert share <= 0.01, (name, nf, share)


def test_differentiable_defaults_and_propagates():
    f, mr, loss = STFTLoss(), MultiResolutionSTFTLoss(), Loss()
    assert f.differentiable is False and mr.differentiable is False and loss.differentiable is False
    assert all(c.differentiable is False for c in mr.stft_losses)
    mr.differentiable = True
    assert mr.differentiable is True and all(c.differentiable is True for c in mr.stft_losses)
    mr.differentiable = False
    assert all(c.differentiable is False for c in mr.stft_losses)
    loss.differentiable = True
    assert loss.stft_loss.differentiable is True and all(c.differentiable is True for c in loss.stft_loss.stft_losses)
    assert MultiResolutionSTFTLoss().differentiable is False      # a class-level default, not shared state
    f.differentiable = True
    assert STFTLoss().differentiable is False


def test_state_dict_keys_are_unchanged():
    want = [f"stft_losses.{i}.window" for i in range(3)]
    mr = MultiResolutionSTFTLoss()
    assert list(mr.state_dict()) == want
    mr.differentiable = True
    assert list(mr.state_dict()) == want
    loss = Loss()
    loss.differentiable = True
    assert list(loss.state_dict()) == ["stft_loss." + k for k in want]


def test_pqmf_synthesis_adjoint_is_analysis_with_the_flipped_filter():
    from fastvocoder_amd.generator.pqmf import design_pqmf_filters
    _, syn = design_pqmf_filters()
    rs = np.random.RandomState(14)
    x, g = rs.randn(2, 4, 300), rs.randn(2, 1200)
    adj = gref.pqmf_synthesis_adjoint_filter(syn)
    assert np.array_equal(adj, 4 * syn[:, ::-1])
    lhs = float((gref.pqmf_synthesis(x, syn) * g).sum())          # <synthesis(x), g> == <x, adjoint(g)>
    rhs = float((x * gref.pqmf_analysis(g, adj)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_abi_and_header():
    assert _native.ABI_VERSION == 18
    with open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define FV_ABI_VERSION 18\b", header)
    assert re.search(r"^int fv_stft_distance_grad\(", header, re.M)
    assert re.search(r"^int64_t fv_stft_distance_grad_workspace_bytes\(", header, re.M)
    assert "stft_loss_grad.hip" in _native.SOURCES
