"""GPU tests of the multi-scale discriminator's input gradient (csrc/disc_grad.hip: fv_grouped_conv1d_input_grad,
fv_disc_map_grad, fv_reflect_pad_fold, fv_avg_pool1d_input_grad, fv_disc_score_grad; the ``differentiable``
attribute of fastvocoder_amd.discriminator and of loss.discriminator_terms) against the float64 closed forms of
tests/disc_grad_reference.py on the same fp32 inputs, float64 autograd through tests/discriminator_reference.py and
the reference's own gradient (tests/golden/discriminator_grad.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANDiscriminator,
                                           MelGANMultiScaleDiscriminator)
from fastvocoder_amd.loss import discriminator_terms, generator_adversarial_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import disc_grad_reference as gref

pytestmark = pytest.mark.gpu

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_KW = dict(SMALL_MSD, downsample_scales=(4, 2))

# Relative to the largest magnitude of the tensor compared, against float64: the worst errors measured on MI355X
#  times about 10.  The yardstick beside them: float32 eager autograd of the same chains on
# the CPU errs by 5.9e-7, of the grouped conv's backward by 6.9e-7 (tests/test_disc_grad_host.py).
KERNEL_RTOL = 6e-6       # one kernel alone (worst 5.7e-7: the grouped input gradient, 64 -> 256 channels)
GRAD_RTOL = 7e-6         # x.grad of a whole chain (worst 7.1e-7: the small MSD's `fake` term at 2001 samples)
GOLDEN_RTOL = 7e-6       # the same against the reference's float64 gradient (the oracle meets it within 1e-15)

# (Cin, Cout, k, stride, Tin)
GROUPED_GRID = [
    (8, 8, 7, 1, 1033), (4, 1, 11, 1, 999), (8, 4, 13, 2, 1000), (4, 8, 31, 3, 777), (12, 48, 51, 5, 4097),
    (8, 32, 13, 2, 3), (16, 16, 21, 2, 501), (4, 16, 41, 4, 2001),
    (16, 64, 41, 4, 1030), (64, 256, 41, 4, 515), (256, 1024, 41, 4, 130), (1024, 1024, 41, 4, 67),
]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _rel(got, want):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.to(_dev()).eval()


@pytest.mark.parametrize("cin,cout,k,s,T", GROUPED_GRID)
def test_grouped_input_grad_against_float64(cin, cout, k, s, T):
    rs = np.random.RandomState(cin + cout + k + T)
    pad = (k - 1) // 2
    tout = (T + 2 * pad - k) // s + 1
    w = (rs.randn(cout, 4, k) / np.sqrt(4 * k)).astype(np.float32)
    g_up = rs.randn(3, cout, tout).astype(np.float32)
    g_map = rs.randn(3, cout, tout).astype(np.float32)
    y = rs.randn(3, cout, tout).astype(np.float32)
    y[:, :, ::7] = 0.0                                           # y == 0 takes the slope
    worst = 0.0
    for slope, up, mp in ((0.2, g_up, g_map), (1.0, g_up, None), (0.2, None, g_map)):
        want = gref.grouped_input_grad(gref.map_grad(up, mp, y if slope != 1.0 else None, slope), w, cin, T, k, s, pad)
        args = (None if up is None else _t(up), None if mp is None else _t(mp), _t(y) if slope != 1.0 else None, _t(w))
        got3 = _native.grouped_conv1d_input_grad(*args, cin, T, k, s, pad, slope)
        err = _rel(got3, want)
        print(f"grouped input grad {(cin, cout, k, s, T)} slope {slope}: {err:.2e}")
        worst = max(worst, err)
        assert err <= KERNEL_RTOL, (slope, err)
        last = (tout - 1) * s - pad + k                          # first input position beyond the last window
        assert not got3[:, :, max(last, 0):].any()
        assert torch.equal(got3, _native.grouped_conv1d_input_grad(*args, cin, T, k, s, pad, slope))
        one = [None if a is None else a[:1].contiguous() for a in args[:3]]
        got1 = _native.grouped_conv1d_input_grad(*one, args[3], cin, T, k, s, pad, slope)
        assert torch.equal(got1, got3[:1])


def test_grouped_input_grad_positions_beyond_the_last_window_are_zero():
    # (Tin + 2 pad - k) % stride != 0: 1030 - 41 = 989 = 4 * 247 + 1 -> the last input sample meets no window
    rs = np.random.RandomState(5)
    g = _t(rs.randn(1, 64, 248))
    w = _t(rs.randn(64, 4, 41))
    dx = _native.grouped_conv1d_input_grad(g, None, None, w, 16, 1030, 41, 4, 0, 1.0)
    assert dx.shape == (1, 16, 1030) and not dx[:, :, 1029:].any() and dx[:, :, 1028].any()
    dx = _native.grouped_conv1d_input_grad(_t(rs.randn(1, 4, 8)), None, None, _t(rs.randn(4, 4, 3)), 4, 40, 3, 5, 0, 1.0)
    want = np.zeros(40, bool)
    want[[5 * t + j for t in range(8) for j in range(3)]] = True  # stride > k: the gaps between the windows too
    assert np.array_equal(dx[0, 0].cpu().numpy() != 0, want)


def test_grouped_input_grad_error_codes():
    L = _native.lib()
    z = _t(np.zeros(4096))
    p = z.data_ptr()

    def rc(cin, cout, tin, k, s, pad, g=p, y=None, slope=1.0, B=1):
        return L.fv_grouped_conv1d_input_grad(g, None, y, p + 4, p + 8, B, cin, cout, tin, k, s, pad,
                                              ctypes.c_float(slope), None)
    assert rc(6, 3, 100, 5, 1, 2) == _native.ERR_UNSUPPORTED           # not 4 channels per group
    assert rc(8, 3, 100, 5, 1, 2) == _native.ERR_UNSUPPORTED           # Cout no multiple of the 2 groups
    assert rc(8, 4, 100, 161, 16, 80) == _native.ERR_UNSUPPORTED       # beyond a block's shared memory
    assert rc(8, 4, 100, 5, 0, 2) == _native.ERR_UNSUPPORTED           # stride 0
    assert rc(8, 4, 100, 301, 1, 0) == _native.ERR_INVALID_ARG         # empty output
    assert rc(8, 4, 100, 5, 1, 2, g=None) == _native.ERR_INVALID_ARG   # no gradient at all
    assert rc(8, 4, 100, 5, 1, 2, slope=0.2) == _native.ERR_INVALID_ARG   # a mask without the layer's output
    assert rc(8, 4, 100, 5, 1, -1) == _native.ERR_INVALID_ARG
    assert rc(8, 4, 100, 5, 1, 2, B=0) == _native.ERR_INVALID_ARG
    torch.cuda.synchronize()


def test_map_grad_fold_pool_and_score_grad_against_float64():
    rs = np.random.RandomState(6)
    for n in (1, 255, 257, 4099):
        up, mp, y = (rs.randn(2, 3, n).astype(np.float32) for _ in range(3))
        y[..., ::3] = 0.0
        for a, b, yy, slope in ((up, mp, y, 0.2), (up, None, y, 0.2), (None, mp, y, 0.01), (up, mp, None, 1.0),
                                (up, None, None, 1.0)):
            got = _native.disc_map_grad(None if a is None else _t(a), None if b is None else _t(b),
                                        None if yy is None else _t(yy), slope)
            assert _rel(got, gref.map_grad(a, b, yy, slope)) <= 1e-7, (n, slope)
    for T, P in ((8, 7), (9, 7), (300, 7), (1027, 7), (5, 0), (2, 1), (600, 2)):
        gp = rs.randn(3, 2, T + 2 * P).astype(np.float32)
        assert _rel(_native.reflect_pad_fold(_t(gp), P), gref.reflect_fold(gp, P)) <= 2e-7, (T, P)
    for T in (2, 3, 5, 8, 1000, 1001, 4099):
        for k, s, p in ((4, 2, 1), (4, 2, 2), (3, 1, 1), (5, 3, 0), (1, 1, 0), (2, 3, 0)):
            if T + 2 * p < k:
                continue
            g = rs.randn(3, 1, (T + 2 * p - k) // s + 1).astype(np.float32)
            got = _native.avg_pool1d_input_grad(_t(g), T, k, s, p)
            assert _rel(got, gref.avg_pool_input_grad(g, T, k, s, p)) <= 3e-7, (T, k, s, p)
    es = [rs.randn(2, c, t).astype(np.float32) for c, t in ((1, 1), (3, 2049), (16, 700), (1, 5000))]
    rr = [rs.randn(*e.shape).astype(np.float32) for e in es]
    for e, r in zip(es, rr):
        r.reshape(-1)[::5] = e.reshape(-1)[::5]                  # e == r: sign 0
    coef = [(0.3, 0.0, 0.0), (1e-3, 0.0, 0.0), (0.0, 0.25, 0.5), (0.7, -0.2, 0.1)]
    got = _native.disc_score_grad([_t(e) for e in es], [_t(r) for r in rr], coef, skip=[False, True, False, False])
    assert got[1] is None
    for m in (0, 2, 3):
        assert _rel(got[m], gref.score_grad(es[m], rr[m], *coef[m])) <= 3e-7, m
    zero = _native.disc_score_grad([_t(es[2])], [_t(es[2])], [(0.5, 0.0, 0.0)])[0]
    assert not zero.any()


def _chain(module, est, real, which=("adversarial", "feature_map")):
    x = _t(est).requires_grad_(True)
    est_p = module(x)
    if torch.is_tensor(est_p[0]):
        est_p = [est_p]
    with torch.no_grad():
        p = module(_t(real))
        p = [p] if torch.is_tensor(p[0]) else p
    terms = discriminator_terms(est_p, p, differentiable=True)
    sum(terms[k] for k in which).backward()
    return x, est_p, p, terms


@pytest.mark.parametrize("case", ["short", "long"])
def test_small_msd_gradient_matches_the_oracle_and_the_golden(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "discriminator_grad.npz"))
    sd = seeded_discriminator_state_dict("msd", int(g["seed"]), **SMALL_MSD)
    est, real = g[f"{case}_est"], g[f"{case}_real"]
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    with pytest.raises(RuntimeError, match="inference-only"):
        msd(_t(est).requires_grad_(True))                       # differentiable = False still refuses
    with torch.no_grad():
        plain = msd(_t(est))
        plain_terms = discriminator_terms(plain, msd(_t(real)))
    msd.differentiable = True
    for which, key in ((("adversarial", "feature_map"), "grad"), (("fake",), "grad_fake")):
        x, est_p, p, terms = _chain(msd, est, real, which)
        want = gref.chain_grad(est, real, sd, which, **SMALL_KW)[0]
        err, gerr = _rel(x.grad, want), _rel(x.grad, g[f"{case}_{key}"])
        print(f"small MSD {case} {which}: oracle {err:.2e} golden {gerr:.2e}")
        assert err <= GRAD_RTOL and gerr <= GOLDEN_RTOL, (which, err, gerr)
        for la, lb in zip(est_p, plain):                        # the same launches: the same bits
            assert all(torch.equal(a, b) for a, b in zip(la, lb))
        assert all(torch.equal(terms[k], plain_terms[k]) for k in terms)
        assert all(q.grad is None for q in msd.parameters())
        assert all(not m.requires_grad and m.grad is None for lst in p for m in lst)
    one = MelGANDiscriminator(**SMALL_MSD)
    one.apply_weight_norm()
    one = _load(one, {k[len("discriminators.1."):]: v for k, v in sd.items() if k.startswith("discriminators.1.")})
    one.differentiable = True
    x, _, _, _ = _chain(one, est, real)
    want = gref.chain_grad(est, real, sd, scale=1, **SMALL_KW)[0]
    err, gerr = _rel(x.grad, want), _rel(x.grad, g[f"{case}_grad_scale1"])
    print(f"small MelGANDiscriminator {case}: oracle {err:.2e} golden {gerr:.2e}")
    assert err <= GRAD_RTOL and gerr <= GOLDEN_RTOL, (err, gerr)
    # estimate and real the same tensor: the feature-map term has an exactly zero gradient
    x, _, _, _ = _chain(msd, est, est, ("feature_map",))
    assert x.grad is not None and not x.grad.any()
    # twice the same bits
    a = _chain(msd, est, real)[0].grad
    assert torch.equal(a, _chain(msd, est, real)[0].grad)


def test_full_size_msd_gradient_matches_the_oracle():
    sd = seeded_discriminator_state_dict("msd", 13)
    msd = _load(MelGANMultiScaleDiscriminator(), sd)
    msd.differentiable = True
    n = msd.min_length() + 300
    rs = np.random.RandomState(21)
    real = (0.5 * rs.randn(1, 1, n)).astype(np.float32)
    est = (real + 0.2 * rs.randn(1, 1, n)).astype(np.float32)
    x, _, _, _ = _chain(msd, est, real)
    err = _rel(x.grad, gref.chain_grad(est, real, sd)[0])
    print(f"full-size MSD n={n}: {err:.2e}")
    assert err <= GRAD_RTOL, err
    assert all(q.grad is None for q in msd.parameters())


def test_out_of_scope_modules_refuse():
    with pytest.raises(NotImplementedError, match="not differentiable"):
        Discriminator().differentiable = True
    d = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), seeded_discriminator_state_dict("msd", 3, **SMALL_MSD))
    d.differentiable = True
    x = _t(np.random.RandomState(1).randn(2, 1, 100)).requires_grad_(True)
    out = d(x)
    with pytest.raises(RuntimeError, match="inference-only"):
        discriminator_terms(out, out)                           # the terms' own switch defaults to False
    with pytest.raises(NotImplementedError, match="per_utterance"):
        discriminator_terms(out, out, per_utterance=True, differentiable=True)
    with torch.no_grad():
        assert not d(x)[0][0].requires_grad


@pytest.mark.parametrize("make,T", [(lambda: MelGANMultiScaleDiscriminator(**SMALL_MSD), 100),
                                    (lambda: DiscriminatorP(3), 20)], ids=["small_msd", "period_3"])
def test_the_gradient_caches_follow_the_weights(make, T):
    """An in-place update of a weight reaches the cached forward and gradient weights ("layers", "grad_layers") of
    both autograd paths: the gradient after it is the gradient of a fresh module with the same state."""
    rs = np.random.RandomState(T)
    est, real = rs.randn(2, 1, T), rs.randn(2, 1, T)
    torch.manual_seed(T)

    def grad(module):
        x = _t(est).requires_grad_(True)
        terms = generator_adversarial_terms(module, x, _t(real), period_grad=True)
        (terms["adversarial"] + terms["feature_map"]).backward()
        return x.grad

    m = make().to(_dev()).eval()
    first = grad(m)
    with torch.no_grad():
        next(q for name, q in m.named_parameters() if name.endswith("weight_g")).mul_(1.5)
    second = grad(m)
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(second, grad(fresh.to(_dev()).eval()))
    assert not torch.equal(second, first)
