"""CPU tests of the STFT loss's host side: the float64 test oracle (tests/stft_loss_reference.py) against the
reference's own values (tests/golden/stft_loss.npz), the tables the kernel reads, the header's table layout and the
argument checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.loss import stft_loss
from fastvocoder_amd.loss import MultiResolutionSTFTLoss, STFTLoss
from tests import cases
from tests import stft_loss_reference as ref


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "stft_loss.npz"))


def test_oracle_meets_the_reference_golden(golden_dir):
    """The reference computes in float32 torch; the oracle in float64: equal to fp32 round-off."""
    d = _golden(golden_dir)
    x, y = d["x"].astype(np.float64), d["y"].astype(np.float64)
    assert x.shape == y.shape == (2, 12000) and d["est_sub"].shape == (2, 4, 3000)
    for (nf, hop, wl), want in zip(ref.RESOLUTIONS, d["stft_terms"]):
        got = np.array(ref.stft_loss(x, y, nf, hop, wl))
        assert np.allclose(got, want, rtol=2e-6, atol=0), (nf, got, want)
    assert np.allclose(ref.multi_resolution_stft_loss(x, y), d["mr_terms"], rtol=2e-6, atol=0)
    assert np.isclose(ref.loss_single_band(x, y), d["loss_single"], rtol=2e-6, atol=0)


def test_oracle_magnitude_is_torch_stft():
    x = np.random.RandomState(3).randn(2, 3001)
    for nf, hop, wl in ref.RESOLUTIONS + ((1024, 77, 1024), (512, 13, 1)):
        S = torch.stft(torch.from_numpy(x), nf, hop, wl, torch.hann_window(wl, dtype=torch.float64),
                       return_complex=True).abs()
        want = torch.sqrt(torch.clamp(S ** 2, min=1e-7)).transpose(2, 1).numpy()
        got = ref.stft_magnitude(x, nf, hop, wl)
        assert got.shape == want.shape == (2, 1 + 3001 // hop, nf // 2 + 1)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (nf, hop, wl)


def test_oracle_partial_sums_give_the_batch_terms():
    rs = np.random.RandomState(4)
    x, y = rs.randn(3, 5000), rs.randn(3, 5000)
    for nf, hop, wl in ref.RESOLUTIONS:
        s = ref.partial_sums(x, y, nf, hop, wl).sum(axis=0)
        sc, mag = ref.stft_loss(x, y, nf, hop, wl)
        assert np.isclose(np.sqrt(s[0]) / np.sqrt(s[1]), sc, rtol=1e-12)
        assert np.isclose(s[2] / (3 * (1 + 5000 // hop) * (nf // 2 + 1)), mag, rtol=1e-12)


def test_tables_hold_the_window_and_exact_twiddles():
    for nf, hop, wl in ref.RESOLUTIONS + ((1024, 1, 601), (2048, 1, 2048), (512, 1, 1)):
        tab = stft_loss._stft_table_host(nf, wl)
        assert tab.dtype == np.float32 and tab.shape == (2 * nf + wl,)
        nc = nf // 2
        tw = tab[:nf].astype(np.float64).reshape(nc, 2)
        sp = tab[nf:2 * nf].astype(np.float64).reshape(nc, 2)
        assert np.array_equal(tw[:, 0] + 1j * tw[:, 1],
                              np.exp(-2j * np.pi * np.arange(nc) / nc).astype(np.complex64))
        assert np.array_equal(sp[:, 0] + 1j * sp[:, 1],
                              np.exp(-2j * np.pi * np.arange(nc) / nf).astype(np.complex64))
        # the window centred-padded into n_fft is torch's, as torch.stft pads it
        padded = np.zeros(nf)
        lpad = (nf - wl) // 2
        padded[lpad:lpad + wl] = tab[2 * nf:]
        want = torch.hann_window(wl, dtype=torch.float64).numpy()
        assert np.allclose(padded, ref.padded_window(nf, wl), atol=1e-7)
        assert np.array_equal(tab[2 * nf:], want.astype(np.float32))
    ham = stft_loss._stft_table_host(1024, 600, "hamming_window")
    assert np.array_equal(ham[2048:], torch.hamming_window(600, dtype=torch.float64).numpy().astype(np.float32))
    w = torch.hann_window(240)
    assert np.array_equal(stft_loss._stft_table_host(512, 240, w)[1024:], w.numpy())


def test_mel_griffin_lim_and_stft_tables_share_their_twiddles_bit_for_bit():
    """The three n_fft = 2048 tables come from one host helper: the same bits in each."""
    from fastvocoder_amd import audio
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    mel, gl, st = audio._mel_table_host(), audio._gl_table_host(), stft_loss._stft_table_host(2048, 1200)
    t0, s0 = audio._MEL_TAB_TWIDDLE, audio._MEL_TAB_SPLIT
    for tab in (mel, gl):
        assert np.array_equal(bits(tab[t0:t0 + 2048]), bits(st[:2048]))          # FFT twiddles
        assert np.array_equal(bits(tab[s0:s0 + 2048]), bits(st[2048:4096]))      # split twiddles
    assert np.array_equal(bits(mel[:1200]), bits(gl[:1200]))                     # window


def test_table_layout_matches_the_header():
    header = open(os.path.join(cases.ROOT, "include", "fastvocoder_hip.h")).read()
    defs = dict(re.findall(r"#define (FV_STFT_\w+(?:\(n_fft\))?) (.+)", header))
    assert defs["FV_STFT_TAB_TWIDDLE(n_fft)"].strip() == "0"
    assert defs["FV_STFT_TAB_SPLIT(n_fft)"].strip() == "(n_fft)"
    assert defs["FV_STFT_TAB_WINDOW(n_fft)"].strip() == "(2 * (n_fft))"
    assert int(defs["FV_STFT_MAX_RES"]) == 8
    for nf, wl in ((512, 240), (1024, 600), (2048, 1200), (2048, 1)):
        assert _native.stft_table_floats(nf, wl) == stft_loss._stft_table_host(nf, wl).size == 2 * nf + wl


def test_unsupported_parameters_raise_without_a_device():
    for nf, wl in ((256, 200), (4096, 1200), (1000, 600), (1024, 1025), (1024, 0)):
        with pytest.raises(_native.NativeError):
            stft_loss._stft_table_host(nf, wl)
        with pytest.raises(_native.NativeError):
            _native.stft_table_floats(nf, wl)
        with pytest.raises(_native.NativeError):
            STFTLoss(nf, 120, wl)
    with pytest.raises(_native.NativeError, match="hop"):
        STFTLoss(1024, 0, 600)
    with pytest.raises(_native.NativeError, match="torch window"):
        STFTLoss(1024, 120, 600, window="hann")
    with pytest.raises(AssertionError):
        MultiResolutionSTFTLoss(fft_sizes=[1024], hop_sizes=[120, 50], win_lengths=[600])


def test_cpu_tensors_and_grad_are_refused():
    m = MultiResolutionSTFTLoss()
    x = torch.zeros(2, 4000)
    with pytest.raises(_native.NativeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(_native.NativeError, match="no CPU path"):
        stft_loss.stft(x, 1024, 120, 600, "hann_window")
    with pytest.raises(_native.NativeError):
        stft_loss.stft_tables("cpu", 1024, 600)


def test_module_tree_mirrors_the_reference():
    m = MultiResolutionSTFTLoss()
    assert [(f.fft_size, f.shift_size, f.win_length) for f in m.stft_losses] == list(ref.RESOLUTIONS)
    assert sorted(m.state_dict()) == [f"stft_losses.{i}.window" for i in range(3)]
    assert torch.equal(m.stft_losses[1].window, torch.hann_window(600))
    assert m.resolutions() == [(2048, 240, 1200, "hann_window"), (1024, 120, 600, "hann_window"),
                               (512, 50, 240, "hann_window")]
