"""GPU tests of MelGAN's parameter gradient (csrc/gen_grad.hip: fv_conv1d_weight_grad_dilated_mode and
fv_conv1d_input_grad_reflect; ``MelGANGenerator.stack_grad`` / ``parameter_grad``, generator/stack_grad.py;
``Trainer(stack_grad=True)``) against the float64 closed forms and float64 CPU autograd of
tests/melgan_grad_reference.py on the same fp32 inputs, and against the reference's own gradient
(tests/golden/melgan_param_grad.npz).  The tests print every error they assert on (run with -s)."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native, optim
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import MelGANMultiScaleDiscriminator
from fastvocoder_amd.loss import generator_adversarial_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_state_dict
from fastvocoder_amd.train import Trainer
from tests import cases
from tests import melgan_grad_reference as mref

pytestmark = pytest.mark.gpu

# Relative to the largest magnitude of the tensor compared, against float64: ten times the worst error measured on
# MI355X (the worst beside each constant).  The yardstick: float32 eager autograd of the same
# chain on the CPU errs by 5.5e-6 (golden case), 4.2e-6 (melgan_s) and 1.2e-6 (melgan_nown) per parameter tensor of more
# than one element, and by 1.8e-6 / 1.0e-4 / 2.1e-7 on the one-element tensors (tests/test_melgan_grad_host.py prints
# them): melgan_s's last conv has one output channel, so its weight_g gradient dg = <dw, v> / |v| is ONE number over
# 28 terms that cancel, and float32 rounding of dw shows magnified in it.  The one-element tensors therefore have a
# constant of their own, as in tests/test_gpu_generator_grad.py.  No measured error exceeds its yardstick.
KERNEL_RTOL = 1.3e-5     # one kernel alone (worst 1.27e-6: the data gradient of 160 -> 144, k 7, a 1120-term chain)
GRAD_RTOL = 3.4e-5       # .grad of a whole chain (worst 3.40e-6: melgan_s; through Trainer.step 8.3e-7; a resumed run 0)
GOLDEN_RTOL = 2.4e-5     # the golden case against the reference's float64 gradient (worst 2.40e-6)
SCALAR_RTOL = 3.7e-5     # ... the one-element tensors, the last conv's weight_g and bias (worst 3.72e-6: melgan_s)
SGD_RTOL = 1.9e-6        # the loss along three SGD steps against float64 (worst 1.89e-7)
WAVE_TOL = 1e-4          # the training forward's waveform: the generator parity tolerance (tests/test_gpu_parity.py TOL)

CHANNELS = [(4, 4), (16, 16), (32, 32), (48, 48), (80, 64), (32, 1)]         # every tile height, ragged ones, the edges
TAPS = [(3, 1), (3, 3), (3, 9), (7, 1)]                                       # (k, dil): the stacks' and the edge convs'
LENGTHS = ["pad+1", "2pad", "2pad+1", 33, 70]                                 # both mirrors on one column ... none
BATCHES = [1, 3]


def _length(name, pad):
    return {"pad+1": pad + 1, "2pad": 2 * pad, "2pad+1": 2 * pad + 1}.get(name, name)


def _grid():
    """The product thinned to at most 40 cases that keep every value of every axis: every eighth case of the product
    in a fixed order that walks all axes, and always T = pad + 1 with dil = 9 (each channel pair once)."""
    out = []
    cases_ = list(itertools.product(range(len(CHANNELS)), range(len(TAPS)), range(len(LENGTHS)), range(len(BATCHES))))
    for n, (a, b, c, d) in enumerate(cases_):
        (cin, cout), (k, dil), B = CHANNELS[a], TAPS[b], BATCHES[d]
        pad = dil * (k - 1) // 2
        forced = dil == 9 and LENGTHS[c] == "pad+1" and d == a % 2
        if forced or (a + 3 * b + 5 * c + 7 * d) % 8 == 0:
            out.append((cin, cout, k, dil, _length(LENGTHS[c], pad), B))
    return out


GRID = _grid()
assert len(GRID) <= 40, len(GRID)
assert {(g[0], g[1]) for g in GRID} == set(CHANNELS) and {(g[2], g[3]) for g in GRID} == set(TAPS)
assert {g[5] for g in GRID} == set(BATCHES) and {33, 70} <= {g[4] for g in GRID}
assert all(any(g[4] == _length(name, g[3] * (g[2] - 1) // 2) for g in GRID) for name in LENGTHS)
assert any(g[3] == 9 and g[4] == 10 for g in GRID)
# beyond that grid: more than one tile of rows with a ragged last one (MelGAN's wide stages), several column blocks
EXTRA = [(160, 144, 3, 3, 37, 2), (144, 160, 7, 1, 131, 2)]


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


@pytest.mark.parametrize("cin,cout,k,dil,T,B", GRID + EXTRA)
def test_reflect_weight_grad_against_float64(cin, cout, k, dil, T, B):
    pad = dil * (k - 1) // 2
    R = _native.PAD_REFLECT
    g, x = mref.kernel_inputs((B, cout, T), (B, cin, T), cin + cout + k + dil + T)
    gd, xd = _t(g), _t(x)
    dw, db = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, True, True, pad_mode=R)
    err = _rel(dw, mref.reflect_weight_grad(g, x, k, dil, pad))
    berr = _rel(db, mref.bias_grad(g))
    print(f"reflect weight grad {(cin, cout, k, dil, T, B)}: dw {err:.2e} db {berr:.2e}")
    assert err <= KERNEL_RTOL and berr <= KERNEL_RTOL, (err, berr)
    # the weight alone, the bias alone, a second call and a workspace full of NaN: equal bits
    ws = _nan(_native.conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, T, k, dil, pad, R))
    dw2, none = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, pad_mode=R, workspace=ws)
    assert none is None
    none, db2 = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, False, True, pad_mode=R, workspace=_nan(ws.numel()))
    assert none is None and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.isfinite(dw2).all() and torch.isfinite(db2).all()
    # zero padding through the new entry: the bits of the old one
    old = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, True, True)
    new = _native.conv1d_weight_grad_dilated(gd, xd, k, dil, pad, True, True, pad_mode=_native.PAD_ZERO)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    assert not torch.equal(old[0], dw)                              # ... and the pad mode is not ignored


def test_reflect_mode_needs_more_samples_than_pad():
    g, x = _t(np.ones((1, 4, 9))), _t(np.ones((1, 4, 9)))
    for T in (9, 5):                                                # pad = 9: T = pad and T < pad
        with pytest.raises(_native.NativeError):
            _native.conv1d_weight_grad_dilated(g[:, :, :T].contiguous(), x[:, :, :T].contiguous(), 3, 9, 9,
                                               pad_mode=_native.PAD_REFLECT)
        with pytest.raises(_native.NativeError):
            _native.conv1d_input_grad_reflect(g[:, :, :T].contiguous(), _t(np.ones((4, 4, 3))), T, 9, 9)
    _native.conv1d_weight_grad_dilated(g, x, 3, 9, 9)               # zero padding takes the same shape


@pytest.mark.parametrize("cin,cout,k,dil,T,B", GRID + EXTRA)
def test_reflect_input_grad_against_float64(cin, cout, k, dil, T, B):
    pad = dil * (k - 1) // 2
    g, _ = mref.kernel_inputs((B, cout, T), (1, 1, 1), cin + cout + k + dil + T)
    w = np.random.RandomState(k + dil + cin).randn(cout, cin, k).astype(np.float32)
    gd, wd = _t(g), _t(w)
    wt = wd.transpose(0, 1).contiguous()
    dx = _native.conv1d_input_grad_reflect(gd, wt, T, dil, pad)
    err = _rel(dx, mref.reflect_input_grad(g, w, T, dil, pad))
    # the two-pass form it replaces: the zero-padded full correlation [B, Cin, T + 2 pad], then the fold
    full = _native.conv1d_fused(gd, _native.pack_conv1d(wd.flip(2).transpose(0, 1).contiguous()), None, cin, k, dil=dil,
                                pad=dil * (k - 1))
    assert full.shape[2] == T + 2 * pad
    two = _rel(dx, _native.reflect_pad_fold(full, pad).cpu().double().numpy())
    print(f"reflect input grad {(cin, cout, k, dil, T, B)}: {err:.2e}; against the two-pass form {two:.2e}")
    assert err <= KERNEL_RTOL and two <= KERNEL_RTOL, (err, two)
    assert torch.equal(dx, _native.conv1d_input_grad_reflect(gd, wt, T, dil, pad))
    # one utterance alone and inside a batch of 3: the same bits
    g3 = _t(np.concatenate([g[:1] * 0.5, g[:1], g[:1] * -2.0]))
    alone = _native.conv1d_input_grad_reflect(gd[:1].contiguous(), wt, T, dil, pad)
    assert torch.equal(alone[0], _native.conv1d_input_grad_reflect(g3, wt, T, dil, pad)[1])
    assert torch.equal(alone[0], dx[0])


# ---- the whole chain ----
def _model(cfg, sd):
    m = build_generator("melgan", cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    return m.to(_dev())


@functools.lru_cache(maxsize=None)
def _case(tag):
    """(cfg, state dict, mel, cotangent, float64 output, float64 gradients) of a chain case; the float64 side is
    computed once and shared."""
    if tag == "golden":
        g = np.load(os.path.join(cases.ROOT, "tests", "golden", "melgan_param_grad.npz"))
        sd = seeded_state_dict("melgan", mref.GOLDEN_CFG, int(g["weight_seed"]))
        return (mref.GOLDEN_CFG, sd, g["mel"], g["c"], g["out"], {k[5:]: g[k] for k in g.files if k.startswith("grad/")})
    cfg, sd, mel, c = mref.chain_case(tag)
    out, grads = mref.param_grad(cfg, sd, mel, c)
    return cfg, sd, mel, c, out, grads


def _worst(tag, errs, g64):
    """(worst error of the tensors with more than one element, worst error of the one-element tensors), printed."""
    order = sorted(errs, key=errs.get, reverse=True)
    many = [k for k in order if g64[k].size > 1]
    one = [k for k in order if g64[k].size == 1]
    print(f"{tag}: worst .grad errors " + ", ".join(f"{errs[k]:.2e} ({k})" for k in many[:3]) +
          "; one-element tensors " + ", ".join(f"{errs[k]:.2e} ({k})" for k in one[:2]))
    return errs[many[0]], max([errs[k] for k in one], default=0.0)


def _trainable(gen):
    gen.stack_grad = True
    gen.parameter_grad = True
    return gen


def _chain(tag):
    cfg, sd, mel, c, out64, g64 = _case(tag)
    gen = _trainable(_model(cfg, sd))
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


@pytest.mark.parametrize("tag", ["melgan_s", "melgan_nown"])
def test_chain_gradient_against_float64(tag):
    err, scalar, wave = _chain(tag)
    assert err <= GRAD_RTOL, err
    assert scalar <= SCALAR_RTOL, scalar
    assert wave <= WAVE_TOL, wave


def test_default_off_changes_nothing():
    cfg, sd, mel, c, _, _ = _case("golden")
    gen = _model(cfg, sd)
    before = gen(_t(mel))                                          # before either attribute was ever touched
    assert not before.requires_grad and all(q.grad is None for q in gen.parameters())
    gen.stack_grad = True                                          # the opt-in alone: still the plans
    mid = gen(_t(mel))
    assert not mid.requires_grad and torch.equal(before, mid)
    gen.parameter_grad = True
    gen(_t(mel)).backward(_t(c))
    assert all(q.grad is not None for q in gen.parameters())
    with torch.no_grad():
        assert not gen(_t(mel)).requires_grad                      # no autograd, no training forward
    gen.parameter_grad = False
    gen.zero_grad(set_to_none=True)
    after = gen(_t(mel))
    assert not after.requires_grad and torch.equal(before, after)
    gen.stack_grad = False
    assert torch.equal(before, gen(_t(mel)))
    assert all(q.grad is None for q in gen.parameters())


def test_a_second_backward_is_refused():
    cfg, sd, mel, c, _, _ = _case("golden")
    gen = _trainable(_model(cfg, sd))
    y = gen(_t(mel))
    y.backward(_t(c), retain_graph=True)
    with pytest.raises(RuntimeError, match="second forward"):
        y.backward(_t(c))


def test_frozen_parameters_get_no_gradient_and_the_rest_the_same_bits():
    cfg, sd, mel, c, _, _ = _case("golden")
    gen = _trainable(_model(cfg, sd))
    gen(_t(mel)).backward(_t(c))
    full = {k: q.grad.clone() for k, q in gen.named_parameters()}
    # the walk stops under: the last conv; a pointwise conv in the middle; a dilated conv; the first upsampler
    for prefix in ("melgan.12.conv.", "melgan.9.stack.4.", "melgan.5.stack.2.", "melgan.3."):
        assert any(k.startswith(prefix) for k in full), prefix
        gen.zero_grad(set_to_none=True)
        for k, q in gen.named_parameters():
            q.requires_grad_(k.startswith(prefix))
        gen(_t(mel)).backward(_t(c))
        for k, q in gen.named_parameters():
            if k.startswith(prefix):
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
    cfg, sd, mel, c, _, _ = _case("golden")
    lr = 1e-4
    gen = _trainable(_model(cfg, sd))
    opt = torch.optim.SGD(gen.parameters(), lr=lr)
    cur = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    got, want = [], []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        y = gen(_t(mel))
        got.append(float((y.detach().double() * _t(c).double()).sum()))
        y.backward(_t(c))
        opt.step()
        out, grads = mref.param_grad(cfg, cur, mel, c)
        want.append(float((out * c.astype(np.float64)).sum()))
        cur = {k: v - lr * grads[k] for k, v in cur.items()}
    errs = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(f"SGD: losses {want}, relative errors {[f'{e:.2e}' for e in errs]}")
    assert abs(want[3] - want[0]) > 1e3 * SGD_RTOL * abs(want[0])   # the steps move the loss far beyond the tolerance
    assert max(errs) <= SGD_RTOL, errs


# ---- composition: Trainer.step ----
SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])


def _small_msd():
    disc = MelGANMultiScaleDiscriminator(**SMALL_MSD)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("msd", 3, **SMALL_MSD).items()})
    return disc.to(_dev())


def _trainer(gen, disc, start, lr=1e-4):
    # a clip threshold no gradient reaches: .grad keeps the backward's bits (scaled by min(1, ...) = 1)
    return Trainer(gen, disc, optim.Adam(gen.parameters(), lr=lr, eps=1e-6), optim.Adam(disc.parameters(), lr=5e-5, eps=1e-6),
                   lambda_stft=5.0, use_feature_map_loss=True, discriminator_train_start_steps=start,
                   grad_clip_thresh=1e9, stack_grad=True)


def _target(cfg, seed):
    n = mref.output_length(cfg, cases.SMALL_T)
    t = np.arange(n) / 24000.0
    rs = np.random.RandomState(seed)
    return _t(np.stack([0.4 * np.sin(2 * np.pi * (180.0 + 70 * b) * t) + 0.02 * rs.randn(n) for b in range(cases.SMALL_B)]))


@pytest.mark.parametrize("phase", ["stft_only", "adversarial"])
def test_a_trainer_step_carries_the_float64_gradient(phase):
    """``Trainer.step`` on melgan_s with a small multi-scale discriminator: the ``.grad`` it leaves on an early and on
    a late parameter equals the float64 generator VJP of the cotangent the same losses hand to a detached waveform, so
    the test isolates the new link (the losses' own gradients have their tests)."""
    cfg, sd, mel, _, _, _ = _case("melgan_s")
    gen, disc = _model(cfg, sd), _small_msd()
    trainer = _trainer(gen, disc, start=1 if phase == "stft_only" else 0)
    assert trainer.samples_per_frame == 240
    wav = _target(cfg, 9)

    probe = gen(_t(mel)).detach().clone().requires_grad_(True)       # the training forward's waveform
    stft, _ = trainer.vocoder_loss(probe, wav)
    total = 5.0 * stft
    if phase == "adversarial":
        terms = generator_adversarial_terms(disc, probe.unsqueeze(1), wav.unsqueeze(1))
        total = total + terms["adversarial"] + terms["feature_map"]
    total.backward()
    _, g64 = mref.param_grad(cfg, sd, mel, probe.grad.cpu().numpy())

    before = {k: q.detach().clone() for k, q in gen.named_parameters()}
    out = trainer.step(_t(mel), wav, 1)
    assert out["total"] == float(total.detach()) and np.isfinite(out["grad_norm"]) and out["grad_norm"] > 0.0
    assert (out["discriminator"] > 0.0) == (phase == "adversarial")
    named = dict(gen.named_parameters())
    early, late = "melgan.1.weight_v", "melgan.22.conv.weight_v"
    errs = {k: _rel(named[k].grad, g64[k]) for k in g64}
    print(f"trainer step {phase}: early {errs[early]:.2e} late {errs[late]:.2e}")
    err, scalar = _worst(f"trainer step {phase}", errs, g64)
    assert errs[early] <= GRAD_RTOL and errs[late] <= GRAD_RTOL, (errs[early], errs[late])
    assert err <= GRAD_RTOL and scalar <= SCALAR_RTOL, (err, scalar)
    assert all(not torch.equal(q, before[k]) for k, q in named.items())      # Adam moved every parameter


def test_thirty_steps_on_one_batch_lower_the_stft_loss():
    cfg, sd, mel, _, _, _ = _case("melgan_s")
    gen, disc = _model(cfg, sd), _small_msd()
    trainer = _trainer(gen, disc, start=10 ** 9, lr=1e-3)
    wav = _target(cfg, 2)
    losses = [trainer.step(_t(mel), wav, s + 1)["stft"] for s in range(30)]
    print("overfit: sc + mag " + " ".join(f"{v:.3f}" for v in losses))
    assert losses[-1] < losses[0], (losses[0], losses[-1])
