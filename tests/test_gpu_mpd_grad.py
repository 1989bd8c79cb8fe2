"""GPU tests of the multi-period discriminator's input gradient (csrc/mpd_grad.hip: fv_period_conv_input_grad,
fv_pack_period_conv_grad, fv_mpd_first_input_grad; DiscriminatorP / MultiPeriodDiscriminator /
Discriminator(use_mpd=True) behind loss.generator_adversarial_terms(..., period_grad=True)) against the float64 oracle
tests/mpd_grad_reference.py and the reference's own gradient (tests/golden/mpd_grad.npz).

Every bound is 10 x the error of float32 eager autograd against float64 for the same family of cases
(mpd_grad_reference.YARDSTICK, pinned by tests/test_mpd_grad_host.py), relative to the peak of the tensor compared:
the kernels sum the same number of fp32 terms as eager does, in another order.

Worst errors on MI355X: fv_period_conv_input_grad 2.3e-6 (bound 1.89e-5), fv_mpd_first_input_grad 3.8e-7 (2.95e-6),
the tiny chains 1.2e-6 (9.88e-6), the n2311 chains with the device's decisions 1.5e-6 (MPD) and 6.5e-6
(Discriminator(use_mpd=True)) (8.99e-6); DESIGN.md section 6.17.  The tests print them (run with -s)."""
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import Discriminator, DiscriminatorP, MultiPeriodDiscriminator
from fastvocoder_amd.loss import generator_adversarial_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import mpd_grad_reference as mref
from tests import mpd_reference as ref

pytestmark = pytest.mark.gpu

KERNEL_RTOL = 10 * mref.YARDSTICK["period_conv"]
FIRST_RTOL = 10 * mref.YARDSTICK["first"]
TINY_RTOL = 10 * mref.YARDSTICK["tiny"]
CHAIN_RTOL = 10 * mref.YARDSTICK["n2311"]
GOLDEN_RTOL = CHAIN_RTOL     # the oracle meets the golden within 1e-9 (tests/test_mpd_grad_host.py)
TERM_RTOL = 7e-6             # the terms' values, relative
MAP_RTOL = 2e-5              # tests/test_gpu_mpd.py: the forward's bound, the ceiling of an adopted decision

# m-space positions per block of period_grad_kernel (csrc/mpd_grad.hip NT), by the layer's input channels
TILE_N = {32: 128, 128: 64, 512: 64}


def _h_near_tile(p, tile, past):
    """An input height whose (H + 1) // 3 + 1 rows of m-space positions end as little as possible past (or short of)
    a tile boundary beyond the first tile: one position for the odd periods, one row of two for p = 2.  Past: the
    last row m holds phase 0 only (H = 3 m - 1); short: all three phases (H = 3 m + 1)."""
    want = (1 if past else tile - 1) if p % 2 else (2 if past else tile - 2)
    rows = next(r for r in range(tile // p + 1, 8 * tile) if (r * p) % tile == want)
    return 3 * rows - 4 if past else 3 * rows - 2


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _rel(got, want):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.to(_dev()).eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mpd_grad.npz"))


@pytest.fixture(scope="module")
def mpd_sd():
    return seeded_discriminator_state_dict("mpd", mref.SEEDS["mpd"])


@pytest.fixture(scope="module")
def mpd_module(mpd_sd):
    return _load(MultiPeriodDiscriminator(), mpd_sd)


@pytest.fixture(scope="module")
def full_sd():
    return seeded_discriminator_state_dict("discriminator", mref.SEEDS["discriminator"], use_mpd=True)


@pytest.fixture(scope="module")
def full_module(full_sd):
    return _load(Discriminator(use_mpd=True), full_sd)


def test_tile_heights_hit_the_boundary():
    for p in mref.PERIODS:
        for tile in set(TILE_N.values()):
            past, short = _h_near_tile(p, tile, True), _h_near_tile(p, tile, False)
            assert (((past + 1) // 3 + 1) * p) % tile == (1 if p % 2 else 2)
            assert (((short + 1) // 3 + 1) * p) % tile == tile - (1 if p % 2 else 2)
            assert ((past + 1) // 3 + 1) * p > tile and (past + 1) % 3 == 0 and (short + 1) % 3 == 2


@pytest.mark.parametrize("p", mref.PERIODS)
@pytest.mark.parametrize("cin,cout", mref.PERIOD_LAYERS)
def test_period_conv_input_grad_alone_against_float64(cin, cout, p):
    """fv_period_conv_input_grad on seeded float32 gradients and a seeded float32 y (the oracle reads the same y: no
    kink question arises): H = 1..5 (every H % 3, rows with missing taps, Hout = 1) and the two heights around a
    tile boundary, B = 1 and 3; with both gradients, either alone, and slope 1 without y; identical calls and the
    row of a smaller batch give identical bits."""
    tile = TILE_N[cin]
    worst = 0.0
    packed = None
    for H in (1, 2, 3, 4, 5, _h_near_tile(p, tile, True), _h_near_tile(p, tile, False)):
        w, g_up, g_map, y = mref.period_conv_inputs(cin, cout, p, H, B=3)
        if packed is None:
            wd = _t(w)
            packed = _native.pack_period_conv_grad(wd)
            w0 = w
        w = w0
        variants = [(g_up, g_map, y, 0.1)]
        if H in (4, 5):
            variants += [(g_up, None, y, 0.1), (None, g_map, y, 0.1), (g_up, g_map, None, 1.0)]
        for gu, gm, yy, slope in variants:
            args = (_t(gu), _t(gm), _t(yy))
            got3 = _native.period_conv_input_grad(*args, packed, cin, H, slope)
            assert tuple(got3.shape) == (3, cin, H, p)
            want = mref.period_conv_input_grad(gu, gm, yy, w, H, slope)
            err = _rel(got3, want)
            worst = max(worst, err)
            assert err <= KERNEL_RTOL, (cin, cout, p, H, gu is None, gm is None, slope, err)
            assert torch.equal(got3, _native.period_conv_input_grad(*args, packed, cin, H, slope))
            one = [None if a is None else a[:1].contiguous() for a in args]
            assert torch.equal(_native.period_conv_input_grad(*one, packed, cin, H, slope), got3[:1])
    print(f"period conv input grad {cin} -> {cout} period {p}: worst error relative to the peak {worst:.2e}")


@pytest.mark.parametrize("pi", range(5))
def test_first_input_grad_alone_against_float64(pi, mpd_sd):
    p = mref.PERIODS[pi]
    w = ref.folded(mpd_sd, f"discriminators.{pi}.convs.0")[0].astype(np.float32).reshape(32, 5)
    worst = 0.0
    for T in (2310, 2311):
        rs = np.random.RandomState(T + p)
        H = (T + ref.reflect_tail(T, p)) // p
        g_up, g_map, y = (rs.randn(3, 32, (H - 1) // 3 + 1, p).astype(np.float32) for _ in range(3))
        for gu, gm in ((g_up, g_map), (g_up, None), (None, g_map)):
            got = _native.mpd_first_input_grad(_t(gu), _t(gm), _t(y), _t(w), T, 0.1)
            g = (0 if gu is None else gu.astype(np.float64)) + (0 if gm is None else gm.astype(np.float64))
            err = _rel(got, mref.first_input_grad(mref.mask(g, y), w, T, p))
            worst = max(worst, err)
            assert err <= FIRST_RTOL, (p, T, err)
        assert torch.equal(got, _native.mpd_first_input_grad(None, _t(g_map), _t(y), _t(w), T, 0.1))
        one = _native.mpd_first_input_grad(None, _t(g_map[:1]), _t(y[:1]), _t(w), T, 0.1)
        assert torch.equal(one, got[:1])
        raw = _native.mpd_first_input_grad(_t(g_up), None, None, _t(w), T, 1.0)
        assert _rel(raw, mref.first_input_grad(g_up, w, T, p)) <= FIRST_RTOL
    print(f"first layer input grad period {p}: worst error relative to the peak {worst:.2e}")


def _chain(module, est, real, scale=1.0):
    x = _t(est).requires_grad_(True)
    terms = generator_adversarial_terms(module, x, _t(real), period_grad=True)
    (sum(terms.values()) * scale).backward()
    return x, terms


def _check_terms(terms, want):
    for k, v in terms.items():
        assert abs(float(v.detach()) - want[k]) <= TERM_RTOL * abs(want[k]), (k, float(v.detach()), want[k])


@pytest.mark.parametrize("pi", range(5))
def test_tiny_cases_against_the_oracle_and_the_golden(pi, golden, mpd_sd):
    p = mref.PERIODS[pi]
    psd = mref.sub_state_dict(mpd_sd, pi)
    module = _load(DiscriminatorP(p), psd)
    est, real = golden[f"tiny{p}_est"], golden[f"tiny{p}_real"]
    with torch.no_grad():
        plain = module(_t(est))[1]
    for r, key in ((real, "grad"), (None, "grad_adv")):
        x, terms = _chain(module, est, r)
        want, wterms, _ = mref.objective_grad("p", est, r, psd, period=p)
        err, gerr = _rel(x.grad, want), _rel(x.grad, golden[f"tiny{p}_{key}"])
        print(f"tiny period {p} {key}: oracle {err:.2e} golden {gerr:.2e}")
        assert err <= TINY_RTOL and gerr <= TINY_RTOL, (p, key, err, gerr)
        assert set(terms) == ({"adversarial", "feature_map"} if r is not None else {"adversarial"})
        _check_terms(terms, wterms)
        assert torch.equal(x.grad, _chain(module, est, r)[0].grad)         # twice the same bits
    maps = module._graph_forward(_t(est).requires_grad_(True))[1]
    assert all(torch.equal(a, b) for a, b in zip(maps, plain))              # the same launches: the same bits
    assert all(q.grad is None for q in module.parameters())
    assert module.differentiable is False


def _maps(module, v):
    with torch.no_grad():
        return [[m.cpu().numpy() for m in lst] for lst in module(_t(v))]


@pytest.mark.parametrize("kind", ["mpd", "discriminator"])
def test_n2311_against_float64_with_the_device_decisions(kind, golden, mpd_sd, mpd_module, full_sd, full_module):
    """B = 2, T = 2311.  Thousands of activated values: a float32 forward decides some kinks differently from
    float64, so the kernels' arithmetic is compared with float64 arithmetic that takes every kink decision from the
    device's own forward, and every decision that differs from float64's own must sit on a float64 value below the
    forward's error bound (MAP_RTOL).  The error against the plain oracle is printed."""
    module, sd = (mpd_module, mpd_sd) if kind == "mpd" else (full_module, full_sd)
    est, real = golden["n2311_est"], golden["n2311_real"]
    e_maps, r_maps = _maps(module, est), _maps(module, real)
    for r, key in ((real, "grad"), (None, "grad_adv")):
        x, terms = _chain(module, est, r)
        plain = mref.objective_grad(kind, est, r, sd)[0]
        want, wterms, differ = mref.objective_grad(kind, est, r, sd, e_maps, r_maps)
        err = _rel(x.grad, want)
        print(f"{kind} n2311 {key}: with the device's decisions {err:.2e}, plain oracle {_rel(x.grad, plain):.2e}" +
              (f", golden {_rel(x.grad, golden['n2311_' + key]):.2e}" if kind == "mpd" else ""))
        print(f"  decisions that differ from float64's own (list, map, count, largest |value| / peak, kind): {differ}")
        assert all(d[3] <= MAP_RTOL for d in differ), differ
        assert err <= CHAIN_RTOL, (kind, key, err)
        _check_terms(terms, wterms)
    assert all(q.grad is None for q in module.parameters())


def test_bits(golden, mpd_module, full_module, full_sd):
    est, real = golden["n2311_est"], golden["n2311_real"]
    with torch.no_grad():
        plain = mpd_module(_t(est))
    maps = mpd_module._graph_forward(_t(est).requires_grad_(True))
    for la, lb in zip(maps, plain):
        assert len(la) == len(lb) and all(torch.equal(a, b) for a, b in zip(la, lb))
    # row 0 of a batch of three against the batch of one: the coefficients carry 1 / B, so the terms of the batch of
    # three are scaled by 3 (3 / (3 k) and 1 / k round to the same coefficient)
    rs = np.random.RandomState(8)
    e3 = np.concatenate([est, (0.5 * rs.randn(1, 1, 2311)).astype(np.float32)])
    r3 = np.concatenate([real, (0.5 * rs.randn(1, 1, 2311)).astype(np.float32)])
    for module in (mpd_module, full_module):
        three = _chain(module, e3, r3, 3.0)[0].grad
        one = _chain(module, e3[:1], r3[:1])[0].grad
        assert torch.equal(three[:1], one)
        assert torch.equal(three, _chain(module, e3, r3, 3.0)[0].grad)      # twice the same bits
    # Discriminator(use_mpd=True) = 5 / 11 of the MPD's own objective + 6 / 11 of Discriminator()'s
    mpd_only = _load(MultiPeriodDiscriminator(), {k[4:]: v for k, v in full_sd.items() if k.startswith("mpd.")})
    rest = _load(Discriminator(), {k: v for k, v in full_sd.items() if not k.startswith("mpd.")})
    full = _chain(full_module, est, real)[0].grad
    a = _chain(mpd_only, est, real)[0].grad
    xr = _t(est).requires_grad_(True)
    sum(generator_adversarial_terms(rest, xr, _t(real)).values()).backward()
    err = _rel(full, (5 / 11) * a.double() + (6 / 11) * xr.grad.double())
    print(f"Discriminator(use_mpd=True) against the sum of its parts: {err:.2e}")
    assert err <= CHAIN_RTOL
    # the default keeps refusing, on the device too
    with pytest.raises(NotImplementedError, match="period convs"):
        generator_adversarial_terms(mpd_module, _t(est).requires_grad_(True))


def test_unsupported_shapes_return_codes():
    """FV_ERR_UNSUPPORTED first, with NULL pointers: nothing is launched."""
    L = _native.lib()
    U, I = _native.ERR_UNSUPPORTED, _native.ERR_INVALID_ARG
    assert L.fv_period_conv_input_grad(None, None, None, None, None, 1, 32, 128, 10, 4, 0.1, None) == U
    assert L.fv_period_conv_input_grad(None, None, None, None, None, 1, 64, 128, 10, 3, 0.1, None) == U
    assert L.fv_period_conv_input_grad(None, None, None, None, None, 1, 32, 512, 10, 3, 0.1, None) == U
    assert L.fv_period_conv_input_grad(None, None, None, None, None, 1, 32, 128, 10, 3, 0.1, None) == I
    assert L.fv_mpd_first_input_grad(None, None, None, None, None, 1, 100, 13, 0.1, None) == U
    assert L.fv_mpd_first_input_grad(None, None, None, None, None, 1, 100, 11, 0.1, None) == I
    assert L.fv_pack_period_conv_grad(None, None, 128, 48, None) == U
    assert L.fv_pack_period_conv_grad(None, None, 128, 32, None) == I
    assert L.fv_packed_period_conv_grad_floats(128, 48) == 0
    assert L.fv_version() == 18
