"""GPU tests of the HiFi-GAN generators' parameter gradient (csrc/gen_grad.hip: fv_conv1d_weight_grad_dilated,
fv_conv_transpose1d_input_grad, fv_conv_transpose1d_weight_grad and the elementwise steps; the ``parameter_grad``
attribute of HiFiGANGenerator / MultiBandHiFiGANGenerator, generator/grad.py) against the float64 closed forms and
float64 CPU autograd of tests/generator_grad_reference.py on the same fp32 inputs, and against the reference's own
gradient (tests/golden/hifigan_param_grad.npz).  The tests print every error they assert on (run with -s)."""
import functools
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import MelGANMultiScaleDiscriminator
from fastvocoder_amd.loss import MultiResolutionSTFTLoss, generator_adversarial_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_mel, seeded_state_dict
from tests import cases
from tests import generator_grad_reference as gref

pytestmark = pytest.mark.gpu

# Relative to the largest magnitude of the tensor compared, against float64: the worst errors measured on MI355X
#  times about 10.  The yardstick beside them: float32 eager autograd of the same chain on the
# CPU errs by 2.6e-6 (golden case) and 6.0e-6 (hifigan_s) per parameter tensor, both on conv_post.weight_g
# (tests/test_generator_grad_host.py).  That tensor is ONE number, dg = <dw, v> / |v| over 112 terms that cancel
# 128-fold in the golden case (sum |dw v| / |sum dw v| = 128), so the float32 rounding of dw (1.6e-7 of its peak) shows
# as 2e-5 of dg: the one-element tensors have a constant of their own, every other tensor the tighter one.
KERNEL_RTOL = 1.7e-5     # one kernel alone (worst 1.65e-6: the data gradient of 256 -> 128, k 20, a 2560-term chain)
GRAD_RTOL = 2.1e-5       # .grad of a whole chain (worst 2.11e-6: hifigan_s; the composition test 1.9e-6)
GOLDEN_RTOL = 9e-6       # the golden case against the reference's float64 gradient (worst 8.92e-7)
SCALAR_RTOL = 2.4e-4     # ... the one-element tensors, conv_post.weight_g (worst 2.35e-5 composition, 2.06e-5 golden)
SGD_RTOL = 3e-5          # the loss along three SGD steps against float64 (worst 3.16e-6)
WAVE_TOL = 1e-4          # the training forward's waveform: the generator parity tolerance (tests/test_gpu_parity.py TOL)

# (Cin, Cout, k, dil, Tin, B)
DILATED_GRID = [
    (16, 16, 3, 1, 13, 2),            # smallest regular case
    (16, 16, 11, 5, 40, 2),           # taps reaching past both ends
    (16, 16, 11, 5, 1, 1),            # only the centre tap alive
    (32, 32, 7, 3, 4099, 3),          # time split, length not a tile multiple
    (64, 64, 11, 5, 130, 2),
    (128, 128, 11, 5, 131, 2),
    (128, 128, 3, 1, 7, 2),           # reduction shorter than a tile
    (20, 12, 7, 3, 50, 2),            # channel counts that are no tile multiples
    (8, 8, 3, 3, 24, 2),
    (4, 4, 11, 1, 72, 2),
    (16, 1, 7, 1, 67, 3),             # conv_post
    (16, 4, 7, 1, 67, 2),             # the multiband conv_post
    (80, 64, 7, 1, 24, 2),            # conv_pre
]

# (Cin, Cout, k, s, p, op, Tin, B)
CONVT_GRID = [
    (256, 128, 16, 8, 4, 0, 5, 2),    # light upsampler 1
    (128, 64, 10, 5, 3, 1, 9, 2),     # light upsampler 2
    (64, 32, 6, 3, 2, 1, 11, 2),      # light upsampler 3
    (32, 16, 4, 2, 1, 0, 13, 3),      # light upsampler 4
    (256, 128, 20, 10, 5, 0, 4, 1),   # multiband upsampler 1
    (128, 64, 12, 6, 3, 0, 7, 2),     # multiband upsampler 2
    (128, 64, 8, 4, 2, 0, 5, 2),
    (64, 32, 7, 3, 2, 1, 6, 2),       # k % s != 0, k > 2 s
    (16, 8, 8, 4, 2, 0, 6, 2),
    (8, 4, 7, 3, 2, 1, 24, 2),
    (32, 16, 4, 2, 1, 0, 1, 1),       # one input sample
    (32, 16, 4, 2, 1, 0, 4099, 2),    # time split
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


def _nan(n):
    return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float32, device=_dev())


@pytest.mark.parametrize("cin,cout,k,dil,T,B", DILATED_GRID)
def test_dilated_weight_grad_against_float64(cin, cout, k, dil, T, B):
    pad = dil * (k - 1) // 2
    g, x = gref.kernel_inputs((B, cout, T), (B, cin, T), cin + cout + k + T)
    gd, xd = _t(g), _t(x)
    dw, none = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad)
    assert none is None
    err = _rel(dw, gref.dilated_weight_grad(g, x, k, dil, pad))
    dw2, db2 = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, True, True)
    berr = _rel(db2, gref.bias_grad(g))
    print(f"dilated weight grad {(cin, cout, k, dil, T, B)}: dw {err:.2e} db {berr:.2e}")
    assert err <= KERNEL_RTOL and berr <= KERNEL_RTOL, (err, berr)
    if T == 1:                                                   # only the centre tap meets the one sample
        other = [j for j in range(k) if j != (k - 1) // 2]
        assert not dw[:, :, other].any() and dw[:, :, (k - 1) // 2].any()
    # with the bias, the bias alone, a second call and a workspace full of NaN: equal bits
    ws = _nan(_native.conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, T, k, dil, pad))
    dw3, db3 = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, True, True, workspace=ws)
    none, db4 = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, False, True, workspace=_nan(ws.numel()))
    assert none is None
    assert torch.equal(dw, dw2) and torch.equal(dw, dw3)
    assert torch.equal(db2, db3) and torch.equal(db2, db4)
    assert torch.isfinite(dw3).all() and torch.isfinite(db4).all()


@pytest.mark.parametrize("cin,cout,k,s,p,op,T,B", CONVT_GRID)
def test_conv_transpose_gradients_against_float64(cin, cout, k, s, p, op, T, B):
    tout = gref.convt_out_len(T, k, s, p, op)
    g, x = gref.kernel_inputs((B, cout, tout), (B, cin, T), cin + cout + k + s + T)
    w = np.random.RandomState(k + s).randn(cin, cout, k).astype(np.float32)
    gd, xd, wd = _t(g), _t(x), _t(w)
    case = (cin, cout, k, s, p, op, T, B)
    # the data gradient: one launch; a row does not depend on the batch
    dx = _native.conv_transpose1d_input_grad(gd, wd, T, s, p, op)
    derr = _rel(dx, gref.convt_input_grad(g, w, T, s, p))
    assert torch.equal(dx, _native.conv_transpose1d_input_grad(gd, wd, T, s, p, op))
    assert torch.equal(dx[:1], _native.conv_transpose1d_input_grad(gd[:1].contiguous(), wd, T, s, p, op))
    # the weight and bias gradient
    dw, none = _native.conv_transpose1d_weight_grad(gd, xd, k, s, p, op)
    assert none is None
    werr = _rel(dw, gref.convt_weight_grad(g, x, k, s, p))
    dw2, db2 = _native.conv_transpose1d_weight_grad(gd, xd, k, s, p, op, True, True)
    berr = _rel(db2, gref.bias_grad(g))
    print(f"conv transpose grads {case}: dx {derr:.2e} dw {werr:.2e} db {berr:.2e}")
    assert derr <= KERNEL_RTOL and werr <= KERNEL_RTOL and berr <= KERNEL_RTOL, (derr, werr, berr)
    ws = _nan(_native.conv_transpose1d_weight_grad_workspace_floats(B, cin, cout, T, k, s, p, op))
    dw3, db3 = _native.conv_transpose1d_weight_grad(gd, xd, k, s, p, op, True, True, workspace=ws)
    none, db4 = _native.conv_transpose1d_weight_grad(gd, xd, k, s, p, op, False, True, workspace=_nan(ws.numel()))
    assert none is None
    assert torch.equal(dw, dw2) and torch.equal(dw, dw3) and torch.equal(db2, db3) and torch.equal(db2, db4)
    assert torch.isfinite(dw3).all() and torch.isfinite(db4).all()


def test_the_elementwise_steps_against_float64():
    rs = np.random.RandomState(5)
    n = (3, 7, 1031)
    g, d, x, acc = (rs.randn(*n).astype(np.float32) for _ in range(4))
    y = np.tanh(x)
    g64, d64, x64, acc64, y64 = (a.astype(np.float64) for a in (g, d, x, acc, y))
    assert _rel(_native.tanh_grad(_t(g), _t(y)), g64 * (1 - y64 * y64)) <= KERNEL_RTOL
    want = g64 + np.where(x64 > 0, 1.0, 0.1) * d64
    assert _rel(_native.residual_merge_grad(_t(g), _t(d), _t(x), 0.1), want) <= KERNEL_RTOL
    assert _rel(_native.residual_merge_grad(_t(g), _t(d), _t(x), 0.1, acc=_t(acc)), want + acc64) <= KERNEL_RTOL
    got = _native.grad_div(_t(g), 3.0)
    assert torch.equal(got.cpu(), torch.from_numpy(g) / 3.0)     # a true division, as torch's


# ---- the whole chain ----
def _model(name, cfg, sd, weight_norm=True):
    m = build_generator(name, cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    if not weight_norm:
        m.remove_weight_norm()
    return m.to(_dev())


@functools.lru_cache(maxsize=None)
def _case(tag):
    """(model name, cfg, state dict, mel, cotangent, float64 output, float64 gradients) of a chain case; the float64
    side is computed once and shared."""
    if tag == "golden":
        g = np.load(os.path.join(cases.ROOT, "tests", "golden", "hifigan_param_grad.npz"))
        sd = seeded_state_dict("hifigan", gref.GOLDEN_CFG, int(g["weight_seed"]))
        return ("hifigan", gref.GOLDEN_CFG, sd, g["mel"], g["c"], g["out"],
                {k[5:]: g[k] for k in g.files if k.startswith("grad/")})
    if tag == "light":
        name, path = next((n, p) for t, n, p in cases.SHIPPED if t == "hifigan_light")
        cfg = cases.load_conf(path)
        sd = seeded_state_dict(name, cfg, seed=gref.CHAIN_WEIGHT_SEED)
        mel = seeded_mel(8, seed=5, batch=2)
        c = gref.cotangent((2, gref.output_length(cfg, 8)), gref.CHAIN_COTANGENT_SEED)
    else:
        name, cfg, sd, mel, c = gref.chain_case(tag.replace("_nown", ""))
    ref_sd = sd
    if tag.endswith("_nown"):                                     # the parameters are the folded weights
        from oracle import torch_port
        ref_sd = {k: v.numpy() for k, v in torch_port.fold_state_dict(sd).items()}
    out, grads = gref.param_grad(name, cfg, ref_sd, mel, c)
    return name, cfg, sd, mel, c, out, grads


def _worst(tag, errs, g64):
    """(worst error of the tensors with more than one element, worst error of the one-element tensors), printed."""
    order = sorted(errs, key=errs.get, reverse=True)
    many = [k for k in order if g64[k].size > 1]
    one = [k for k in order if g64[k].size == 1]
    print(f"{tag}: worst .grad errors " + ", ".join(f"{errs[k]:.2e} ({k})" for k in many[:3]) +
          "; one-element tensors " + ", ".join(f"{errs[k]:.2e} ({k})" for k in one[:2]))
    return errs[many[0]], max([errs[k] for k in one], default=0.0)


def _chain(tag):
    name, cfg, sd, mel, c, out64, g64 = _case(tag)
    gen = _model(name, cfg, sd, weight_norm=not tag.endswith("_nown"))
    gen.parameter_grad = True
    y = gen(_t(mel))
    assert y.requires_grad and y.shape == out64.shape
    y.backward(_t(c))
    named = dict(gen.named_parameters())
    assert sorted(named) == sorted(g64)
    errs = {k: _rel(named[k].grad, g64[k]) for k in g64}
    wave = float(np.abs(y.detach().cpu().double().numpy() - out64).max())
    worst, scalar = _worst(tag, errs, g64)
    print(f"{tag}: waveform {wave:.2e}")
    return worst, scalar, wave


def test_golden_case_meets_the_reference_gradient():
    err, scalar, wave = _chain("golden")
    assert err <= GOLDEN_RTOL, err
    assert scalar <= SCALAR_RTOL, scalar
    assert wave <= WAVE_TOL, wave


@pytest.mark.parametrize("tag", ["hifigan_s", "hifigan_rb2", "mb_s", "hifigan_s_nown", "light"])
def test_chain_gradient_against_float64(tag):
    err, scalar, wave = _chain(tag)
    assert err <= GRAD_RTOL, err
    assert scalar <= SCALAR_RTOL, scalar
    assert wave <= WAVE_TOL, wave


def test_default_off_changes_nothing():
    name, cfg, sd, mel, c, _, _ = _case("golden")
    gen = _model(name, cfg, sd)
    before = gen(_t(mel))                                          # before the attribute was ever touched
    assert not before.requires_grad and all(q.grad is None for q in gen.parameters())
    gen.parameter_grad = True
    gen(_t(mel)).backward(_t(c))
    assert all(q.grad is not None for q in gen.parameters())
    with torch.no_grad():
        assert not gen(_t(mel)).requires_grad                      # no autograd, no training forward
    gen.parameter_grad = False
    gen.zero_grad(set_to_none=True)
    after = gen(_t(mel))
    assert not after.requires_grad and torch.equal(before, after)
    assert all(q.grad is None for q in gen.parameters())


def test_frozen_parameters_get_no_gradient_and_the_rest_the_same_bits():
    name, cfg, sd, mel, c, _, _ = _case("golden")
    gen = _model(name, cfg, sd)
    gen.parameter_grad = True
    gen(_t(mel)).backward(_t(c))
    full = {k: q.grad.clone() for k, q in gen.named_parameters()}
    gen.zero_grad(set_to_none=True)
    for k, q in gen.named_parameters():
        q.requires_grad_(k.startswith("conv_post."))
    gen(_t(mel)).backward(_t(c))
    for k, q in gen.named_parameters():
        if k.startswith("conv_post."):
            assert torch.equal(q.grad, full[k]), k
        else:
            assert q.grad is None, k
    # everything frozen: the inference path, no graph
    for q in gen.parameters():
        q.requires_grad_(False)
    assert not gen(_t(mel)).requires_grad


def test_three_sgd_steps_follow_float64():
    """The loss L = <c, G(mel)> along three SGD steps: a packed-weight cache that does not see optimizer.step() would
    keep the first step's loss."""
    name, cfg, sd, mel, c, _, _ = _case("golden")
    lr = 1e-5
    gen = _model(name, cfg, sd)
    gen.parameter_grad = True
    opt = torch.optim.SGD(gen.parameters(), lr=lr)
    cur = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    got, want = [], []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        y = gen(_t(mel))
        got.append(float((y.detach().double() * _t(c).double()).sum()))
        y.backward(_t(c))
        opt.step()
        out, grads = gref.param_grad(name, cfg, cur, mel, c)
        want.append(float((out * c.astype(np.float64)).sum()))
        cur = {k: v - lr * grads[k] for k, v in cur.items()}
    errs = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(f"SGD: losses {want}, relative errors {[f'{e:.2e}' for e in errs]}")
    assert abs(want[3] - want[0]) > 1e3 * SGD_RTOL * abs(want[0])   # the steps move the loss far beyond the tolerance
    assert max(errs) <= SGD_RTOL, errs


def test_composition_with_the_losses_and_an_optimizer_step():
    """total = 5 (sc + mag) + adversarial + feature_map through MultiResolutionSTFTLoss(differentiable) and
    generator_adversarial_terms on a small multi-scale discriminator: the parameter gradients equal the float64
    generator VJP of the cotangent the same losses hand to a detached waveform, so the test isolates the new link.
    Discriminator() takes no size arguments, so the small discriminator is its MSD part built with the SMALL_MSD
    kwargs of tests/test_gpu_disc_grad.py; both sides of the comparison share whatever discriminator produced the
    cotangent, so the choice does not bear on what is checked."""
    name, cfg, sd, mel, _, _, _ = _case("hifigan_s")
    B = mel.shape[0]
    small = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
    disc = MelGANMultiScaleDiscriminator(**small)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("msd", 3, **small).items()})
    disc = disc.to(_dev()).eval()
    mr = MultiResolutionSTFTLoss().to(_dev())
    mr.differentiable = True
    gen = _model(name, cfg, sd)
    gen.parameter_grad = True
    real = _t(0.3 * np.random.RandomState(9).randn(B, gref.output_length(cfg, cases.SMALL_T)))

    def total(wave):
        sc, mag = mr(wave, real)
        terms = generator_adversarial_terms(disc, wave.unsqueeze(1), real.unsqueeze(1))
        return 5.0 * (sc + mag) + terms["adversarial"] + terms["feature_map"]

    wave = gen(_t(mel))
    probe = wave.detach().clone().requires_grad_(True)
    total(probe).backward()
    c = probe.grad.cpu().numpy()
    total(wave).backward()
    _, g64 = gref.param_grad(name, cfg, sd, mel, c)
    named = dict(gen.named_parameters())
    errs = {k: _rel(named[k].grad, g64[k]) for k in g64}
    err, scalar = _worst("composition", errs, g64)
    assert err <= GRAD_RTOL, err
    assert scalar <= SCALAR_RTOL, scalar
    opt = torch.optim.Adam(gen.parameters(), lr=1e-3)
    norm = torch.nn.utils.clip_grad_norm_(gen.parameters(), 10.0)
    assert torch.isfinite(norm)
    opt.step()
    with torch.no_grad():
        assert not torch.equal(gen(_t(mel)), wave)
