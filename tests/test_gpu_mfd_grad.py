"""GPU tests of the STFT discriminators' input gradient (csrc/stft_mag_grad.hip: fv_stft_magnitude_bins_grad; the
graph-mode forwards of fastvocoder_amd.discriminator; loss.generator_adversarial_terms) against the float64 closed
form and float64 autograd of tests/mfd_grad_reference.py on the same fp32 inputs, and the reference's own gradient
(tests/golden/mfd_grad.npz).

Tolerances: relative to the largest magnitude of the tensor compared, against float64.  Each is 10 x YARDSTICK, the
error of float32 eager autograd of the same case family on the CPU against float64
(tests/test_mfd_grad_host.py::test_float32_eager_autograd_error_is_the_yardstick printed them): the kernels sum the
same number of fp32 terms as eager does, in another order.
  family                                        yardstick   bound     measured worst on MI355X
  fv_stft_magnitude_bins_grad alone             5.88e-7     5.88e-6   8.36e-7 (half-silent 512 / 700; grid 7.17e-7)
  small STFTDiscriminator chain                 7.26e-7     7.26e-6   3.28e-6 (n = 1999; n = 400: 1.11e-6)
  default MFD / Discriminator()                 6.74e-7     6.74e-6   2.12e-6 (Discriminator(); MFD 1.18e-6)
  ragged dense data gradient                    3.88e-7     3.88e-6   1.81e-7
"""
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, MelGANMultiScaleDiscriminator,
                                           MultiResolutionSTFTDiscriminator, STFTDiscriminator)
from fastvocoder_amd.loss import generator_adversarial_terms
from fastvocoder_amd.loss.stft_loss import _stft_table_host
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import disc_grad_reference as gref
from tests import discriminator_reference as ref
from tests import mfd_grad_reference as mref
from tests.mfd_grad_reference import DENSE_CASES, DENSE_CASES_B16, FULL_SEED, YARDSTICK, full_signals

pytestmark = pytest.mark.gpu

KERNEL_RTOL = 10 * YARDSTICK["kernel"]        # fv_stft_magnitude_bins_grad alone
CHAIN_RTOL = 10 * YARDSTICK["small_chain"]    # estimate.grad of the small STFTDiscriminator, oracle and golden
FULL_RTOL = 10 * YARDSTICK["full"]            # estimate.grad of the default MFD and Discriminator()
DENSE_RTOL = 10 * YARDSTICK["dense"]          # the ragged dense data gradient through fv_conv1d_fused
VALUE_RTOL = 7e-6                             # the terms' values: SCORE_RTOL of tests/test_gpu_discriminator.py


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _rel(got, want):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _table(n_fft, win):
    return torch.from_numpy(_stft_table_host(n_fft, win, mref.hann(win, torch.float32))).to(_dev())


def _load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.to(_dev()).eval()


@pytest.mark.parametrize("n_fft,hop,win,n", mref.KERNEL_GRID)
def test_kernel_against_the_float64_closed_form(n_fft, hop, win, n):
    x, gmag = mref.kernel_inputs(n_fft, hop, win, n)
    got = _native.stft_magnitude_bins_grad(_t(x), _t(gmag), _table(n_fft, win), n_fft, hop, win)
    err = _rel(got, mref.magnitude_grad_closed_form(x, gmag, n_fft, hop, win))
    print(f"stft_magnitude_bins_grad {(n_fft, hop, win, n)}: {err:.2e}")
    assert err <= KERNEL_RTOL, err


@pytest.mark.parametrize("n_fft,hop,win,n", [(512, 50, 240, 700), (2048, 240, 1200, 4100)])
def test_kernel_exact_properties(n_fft, hop, win, n):
    x, gmag = mref.kernel_inputs(n_fft, hop, win, n)
    tab = _table(n_fft, win)
    run = lambda a, g: _native.stft_magnitude_bins_grad(a, g, tab, n_fft, hop, win)  # noqa: E731
    dx, dg = _t(x), _t(gmag)
    assert not run(torch.zeros_like(dx), dg).any()              # every bin clamped
    assert not run(dx, torch.zeros_like(dg)).any()
    half = x.copy()
    half[:, :n // 2] = 0.0
    err = _rel(run(_t(half), dg), mref.magnitude_grad_closed_form(half, gmag, n_fft, hop, win))
    print(f"half-silent {(n_fft, hop, win, n)}: {err:.2e}")
    assert err <= KERNEL_RTOL, err
    got = run(dx, dg)
    assert torch.equal(got, run(dx, dg))
    for b in range(x.shape[0]):
        assert torch.equal(run(dx[b:b + 1].contiguous(), dg[b:b + 1].contiguous()), got[b:b + 1]), b


@pytest.mark.parametrize("cin,cout,k,T", DENSE_CASES)
def test_ragged_dense_data_gradient(cin, cout, k, T):
    """The first STFT-discriminator layer's data gradient: fv_conv1d_fused with an output-channel count that is no
    multiple of 4 (W'[ci, co, j] = W[co, ci, k-1-j], zero padding k - 1)."""
    w, gy = mref.dense_grad_inputs(cin, cout, k, T)
    packed = _native.pack_conv1d(_t(w).flip(2).transpose(0, 1).contiguous())
    got = _native.conv1d_fused(_t(gy), packed, None, cout, k, pad=k - 1)
    err = _rel(got, gref.dense_input_grad(gy, w, 0))
    print(f"ragged dense gradient {(cin, cout, k, T)}: {err:.2e}")
    assert err <= DENSE_RTOL, err


@pytest.mark.parametrize("cin,cout,k,T", DENSE_CASES_B16)
def test_ragged_dense_data_gradient_batch_16(cin, cout, k, T):
    """B = 16 and lengths at which fv_conv1d_fused's grid cap makes a block walk several time tiles
    (tiles_per_run > 1), the ragged last output-channel tile among them; Cin = 64 are the MFD's own shapes at
    24 000 samples."""
    w, gy = mref.dense_grad_inputs(cin, cout, k, T, B=16)
    packed = _native.pack_conv1d(_t(w).flip(2).transpose(0, 1).contiguous())
    got = _native.conv1d_fused(_t(gy), packed, None, cout, k, pad=k - 1)
    err = _rel(got, gref.dense_input_grad(gy, w, 0))
    print(f"ragged dense gradient B=16 {(cin, cout, k, T)}: {err:.2e}")
    assert err <= DENSE_RTOL, err


def test_default_mfd_at_batch_16_and_24000_samples():
    """The training shape (the inputs of tools/mfd_grad_bench.py), no seed chosen: 5 million activated values, so
    some float64 pre-activations lie below float32's rounding and a float32 forward decides their side of zero
    differently from float64 (a row with one such mask is off by 1e-3 of the gradient's peak against the plain
    oracle, as float32 eager autograd on the device is on other rows; both are printed).  The kernels' arithmetic
    is therefore checked against float64 arithmetic that takes the kink decisions -- each leaky ReLU's side, each
    sign(e - r) -- from the device's own forward, within the bound of the B = 1 case; and every decision that
    differs from float64's own must sit on a float64 value smaller than the forward's error bound (MAP_RTOL of
    tests/test_gpu_discriminator.py, 2e-5 of the map's peak), so a wrong mask cannot hide in the adopted ones."""
    B, n = 16, 24000
    rs = np.random.RandomState(B)
    real = (0.5 * rs.randn(B, 1, n)).astype(np.float32)
    est = (real + 0.1 * rs.randn(B, 1, n).astype(np.float32)).astype(np.float32)
    sd = seeded_discriminator_state_dict("mfd", FULL_SEED)
    mfd = _load(MultiResolutionSTFTDiscriminator(), sd)
    x = _t(est).requires_grad_(True)
    sum(generator_adversarial_terms(mfd, x, _t(real)).values()).backward()
    with torch.no_grad():
        e_maps = [[m.cpu().numpy() for m in lst] for lst in mfd(_t(est))]
        r_maps = [[m.cpu().numpy() for m in lst] for lst in mfd(_t(real))]
    plain = mref.objective_grad("mfd", est, real, sd)[0]
    got = x.grad.cpu().double().numpy()
    rows = np.abs(got - plain).reshape(B, -1).max(1) / np.abs(plain).max()
    print("default MFD B=16 n=24000 against the plain float64 oracle, per row: " + " ".join(f"{v:.1e}" for v in rows))
    want, differ = mref.mfd_grad_with_decisions(est, real, sd, e_maps, r_maps)
    print(f"decisions that differ from float64's own (list, map, count, largest |value| / peak, kind): {differ}")
    err = _rel(x.grad, want)
    print(f"default MFD B=16 n=24000 against float64 with the device's kink decisions: {err:.2e}")
    assert all(d[3] <= 2e-5 for d in differ), differ
    assert err <= FULL_RTOL, err
    assert np.median(rows) <= FULL_RTOL                         # the rows without such a mask meet the plain oracle


@pytest.mark.parametrize("case", ["n400", "n1999"])
def test_small_stft_discriminator_matches_the_oracle_and_the_golden(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "mfd_grad.npz"))
    sd = seeded_discriminator_state_dict("stft", int(g["seed"]), **mref.SMALL_STFT)
    est, real = g[f"{case}_est"], g[f"{case}_real"]
    disc = _load(STFTDiscriminator(**mref.SMALL_STFT), sd)
    with pytest.raises(RuntimeError, match="inference-only"):
        disc(_t(est).requires_grad_(True))                      # the plain forward still refuses
    with torch.no_grad():
        plain = disc(_t(est))
        nograd = generator_adversarial_terms(disc, _t(est).requires_grad_(True), _t(real))
    for r, key in ((real, "grad"), (None, "grad_adv")):
        x = _t(est).requires_grad_(True)
        terms = generator_adversarial_terms(disc, x, None if r is None else _t(r))
        assert set(terms) == ({"adversarial", "feature_map"} if r is not None else {"adversarial"})
        assert all(v.dim() == 0 and v.dtype == torch.float32 and v.requires_grad for v in terms.values())
        sum(terms.values()).backward()
        want, est_p, p, _ = mref.objective_grad("stft", est, r, sd, **mref.SMALL_STFT)
        err, gerr = _rel(x.grad, want), _rel(x.grad, g[f"{case}_{key}"])
        print(f"small STFTDiscriminator {case} {key}: oracle {err:.2e} golden {gerr:.2e}")
        assert err <= CHAIN_RTOL and gerr <= CHAIN_RTOL, (key, err, gerr)
        if r is not None:
            scores = ref.scores([[m.detach() for m in lst] for lst in est_p], p)
            for k in terms:
                assert abs(float(terms[k]) - scores[k]) <= VALUE_RTOL * abs(scores[k]), k
                assert torch.equal(terms[k].detach(), nograd[k]) and not nograd[k].requires_grad
        assert all(q.grad is None for q in disc.parameters())
    maps = disc._graph_forward(_t(est).requires_grad_(True))     # the same launches: the same bits
    assert len(maps) == len(plain) and all(torch.equal(a, b) for a, b in zip(maps, plain))
    a = _t(est).requires_grad_(True)
    sum(generator_adversarial_terms(disc, a, _t(real)).values()).backward()
    b = _t(est).requires_grad_(True)
    sum(generator_adversarial_terms(disc, b, _t(real)).values()).backward()
    assert torch.equal(a.grad, b.grad)                          # twice the same bits


@pytest.mark.parametrize("kind", ["mfd", "discriminator"])
def test_default_modules_match_float64_autograd(kind):
    sd = seeded_discriminator_state_dict(kind, FULL_SEED)
    module = _load(MultiResolutionSTFTDiscriminator() if kind == "mfd" else Discriminator(), sd)
    est, real = full_signals()
    with torch.no_grad():
        plain = module(_t(est))
    for r in (real, None):
        x = _t(est).requires_grad_(True)
        terms = generator_adversarial_terms(module, x, None if r is None else _t(r))
        assert set(terms) == ({"adversarial", "feature_map"} if r is not None else {"adversarial"})
        sum(terms.values()).backward()
        want, _, _, values = mref.objective_grad(kind, est, r, sd)
        err = _rel(x.grad, want)
        print(f"default {kind} n={est.shape[-1]} real={'yes' if r is not None else 'None'}: {err:.2e}")
        assert err <= FULL_RTOL, err
        for k in terms:
            assert abs(float(terms[k]) - values[k]) <= VALUE_RTOL * abs(values[k]), k
        assert all(q.grad is None for q in module.parameters())
    maps = module._graph_forward(_t(est).requires_grad_(True))
    for la, lb in zip(maps, plain):
        assert len(la) == len(lb) and all(torch.equal(a, b) for a, b in zip(la, lb))
    assert module.differentiable is False


def test_entry_point_runs_the_msd_whatever_its_attribute_says():
    small = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
    sd = seeded_discriminator_state_dict("msd", 11, **small)
    msd = _load(MelGANMultiScaleDiscriminator(**small), sd)
    rs = np.random.RandomState(4)
    real = rs.uniform(-0.8, 0.8, (2, 1, 300)).astype(np.float32)
    est = (real + 0.3 * rs.randn(2, 1, 300)).astype(np.float32)
    x = _t(est).requires_grad_(True)
    assert msd.differentiable is False
    sum(generator_adversarial_terms(msd, x, _t(real)).values()).backward()
    want = gref.chain_grad(est, real, sd, **dict(small, downsample_scales=(4, 2)))[0]
    assert _rel(x.grad, want) <= 7e-6                           # test_gpu_disc_grad.py GRAD_RTOL
    with pytest.raises(ValueError, match="too short"):
        generator_adversarial_terms(Discriminator(), _t(est).requires_grad_(True))


def test_error_codes_at_the_abi():
    L = _native.lib()
    z = _t(np.zeros(1 << 16))
    p = z.data_ptr()
    n, B = 700, 1
    need = L.fv_stft_magnitude_bins_grad_workspace_bytes(B, n, 512, 50, 240)
    assert need == 4 * 15 * 240
    x, gm, tab, gx, ws = p, p + 4096, p + 4096 + 4 * 257 * 15, p + 65536, p + 131072

    def rc(n_fft=512, n=n, x=x, gm=gm, tab=tab, gx=gx, ws=ws, bytes_=need):
        return L.fv_stft_magnitude_bins_grad(x, gm, tab, B, n, n_fft, 50, 240, gx, ws, bytes_, None)
    assert rc(n_fft=4096) == _native.ERR_UNSUPPORTED
    assert rc(n=256) == _native.ERR_INVALID_ARG                 # n <= n_fft / 2
    for name in ("x", "gm", "tab", "gx", "ws"):
        assert rc(**{name: None}) == _native.ERR_INVALID_ARG, name
    assert rc(bytes_=need - 1) == _native.ERR_INVALID_ARG
    assert rc(gx=x) == _native.ERR_INVALID_ARG and rc(gx=gm + 8) == _native.ERR_INVALID_ARG   # gx aliases an input
    assert L.fv_stft_magnitude_bins_grad_workspace_bytes(B, n, 4096, 50, 240) == _native.ERR_UNSUPPORTED
    torch.cuda.synchronize()
