"""GPU tests of Basis-MelGAN's parameter gradient (csrc/basis_grad.hip: fv_basis_head_forward, fv_basis_head_grad,
fv_basis_weight_l1, fv_basis_weight_l1_grad; ``BasisMelGANGenerator.basis_grad`` / ``parameter_grad``,
generator/basis_grad.py; loss.BasisWeightL1; ``Trainer(basis_grad=True)``) against the float64 closed forms and float64
CPU autograd of the reference's two-pass graph (tests/basis_grad_reference.py) on the same fp32 inputs, and against the
reference's own gradient (tests/golden/basis_param_grad.npz).  The tests print every error they assert on (run with
-s)."""
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
from fastvocoder_amd.loss.loss import BasisWeightL1
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_state_dict
from fastvocoder_amd.train import KEYS, Trainer
from tests import basis_grad_reference as bref
from tests import cases
from tests.test_gpu_parity import TOL as WAVE_TOL

pytestmark = pytest.mark.gpu

# Relative to the largest magnitude of the tensor compared, against float64: ten times the worst error measured on
# MI355X (the worst beside each constant).  The yardstick: float32 eager autograd of the same
# two-pass chain on the CPU errs by 2.2e-6 (basis_s, both cotangents), 1.4e-6 (est alone), 1.5e-6 (weight alone) and
# 1.5e-6 (golden case) per trunk parameter tensor (tests/test_basis_grad_host.py prints them).  No trunk tensor of
# these cases has one element, so there is no constant for those (_worst asserts it).  One measured error exceeds its
# yardstick: the golden case's 2.03e-6 on melgan.11.stack.2.weight_g, an 8-element weight-norm gradient
# dg = <dw, v> / |v| over 24 terms that cancel; float32 eager autograd errs on that same tensor by 1.1e-6 to 1.8e-6
# depending on the thread count alone (the order of its sums), see DESIGN.md section 6.23.
KERNEL_RTOL = 2.5e-6     # one kernel alone (worst 2.46e-7: the head adjoint at C 32, L 30, F 17; the L1 gradient 5.9e-8)
L1_RTOL = 4.5e-7         # the two means of fv_basis_weight_l1 (worst 4.42e-8)
GRAD_RTOL = 1.4e-5       # .grad of a whole chain (worst 1.31e-6: basis_s, weight alone; through Loss and through
#                          Trainer.step 4.1e-7; a resumed run 0)
GOLDEN_RTOL = 2.1e-5     # the golden case against the reference's float64 gradient (worst 2.03e-6)

CHANNELS = [1, 24, 32, 80, 256]          # ragged channel tiles of 16 and of 64, and the shipped width
LENGTHS = [2, 8, 30]                     # L: hop 1, an aligned hop, the shipped odd 15
FRAMES = [1, 2, 17, 70]                  # only taps j < hop live; the cropped tail; ragged tiles; two frame tiles
BATCHES = [1, 3]


def _grid():
    """The product thinned to at most 40 cases that keep every value of every axis: every fourth case of the product in
    a fixed order that walks all axes, and always the corner C = 1, L = 2, F = 1."""
    out = []
    for a, b, c, d in itertools.product(range(len(CHANNELS)), range(len(LENGTHS)), range(len(FRAMES)), range(len(BATCHES))):
        if (a + 2 * b + 3 * c + d) % 4 == 0 or (a, b, c) == (0, 0, 0):
            out.append((CHANNELS[a], LENGTHS[b], FRAMES[c], BATCHES[d]))
    return out


GRID = _grid()
assert len(GRID) <= 40, len(GRID)
assert {g[0] for g in GRID} == set(CHANNELS) and {g[1] for g in GRID} == set(LENGTHS)
assert {g[2] for g in GRID} == set(FRAMES) and {g[3] for g in GRID} == set(BATCHES)
# beyond that grid: the shipped head shape on several tiles of both axes
EXTRA = [(256, 30, 70, 3), (80, 30, 130, 2)]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _rel(got, want):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _head_inputs(C, L, F, B):
    rs = np.random.RandomState(C + 3 * L + 7 * F + B)
    Y = rs.randn(B + 1, C, F).astype(np.float32)
    Y.reshape(-1)[::5] = 0.0                                 # exact zeros, some of them -0.0: the mask is > 0
    Y.reshape(-1)[::10] = -0.0
    basis = rs.randn(L, C).astype(np.float32)
    g_est = rs.randn(B, F * (L // 2)).astype(np.float32)
    g_w = rs.randn(B, C, F).astype(np.float32)
    return Y, basis, g_est, g_w


@pytest.mark.parametrize("C,L,F,B", GRID + EXTRA)
def test_head_forward_and_adjoint_against_float64(C, L, F, B):
    Y, basis, g_est, g_w = _head_inputs(C, L, F, B)
    Yd, bd, ged, gwd = _t(Y), _t(basis), _t(g_est), _t(g_w)
    D = _native.basis_head_forward(Yd)
    ferr = _rel(D, bref.head_forward(Y))
    errs = {}
    for name, ge, gw in (("both", g_est, g_w), ("est", g_est, None), ("weight", None, g_w)):
        got = _native.basis_head_grad(None if ge is None else ged, None if gw is None else gwd, Yd, bd)
        errs[name] = _rel(got, bref.head_grad(ge, gw, Y, basis))
        assert torch.equal(got, _native.basis_head_grad(None if ge is None else ged, None if gw is None else gwd, Yd, bd))
        assert bool((got[torch.from_numpy(Y == 0).to(_dev())] == 0).all())          # nothing passes an exact zero
    print(f"head {(C, L, F, B)}: forward {ferr:.2e}; adjoint " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert ferr <= KERNEL_RTOL and max(errs.values()) <= KERNEL_RTOL, (ferr, errs)
    assert torch.equal(D, _native.basis_head_forward(Yd))
    with pytest.raises(_native.NativeError):
        _native.basis_head_grad(None, None, Yd, bd)


@pytest.mark.parametrize("C,F,B", sorted({(g[0], g[2], g[3]) for g in GRID + EXTRA}))
def test_weight_l1_and_its_gradient_against_float64(C, F, B):
    rs = np.random.RandomState(C + 7 * F + B)
    D = rs.randn(B, C, F).astype(np.float32)
    target = rs.randn(B, F, C).astype(np.float32)
    same = rs.rand(B, F, C) < 0.25
    target[same] = D.transpose(0, 2, 1)[same]                # D == target elements: sign is 0
    Dd, td = _t(D), _t(target)
    out = _native.basis_weight_l1(Dd, td)
    want = bref.weight_l1(D, target)
    errs = [abs(float(out[i]) - want[i]) / max(abs(want[0]), abs(want[1])) for i in (0, 1)]
    coef = _t(np.array([-1.75]))
    g = _native.basis_weight_l1_grad(Dd, td, coef)
    g1 = _native.basis_weight_l1_grad(Dd, td)
    gerr = _rel(g, bref.weight_l1_grad(D, target, -1.75))
    gerr1 = _rel(g1, bref.weight_l1_grad(D, target))
    print(f"weight l1 {(C, F, B)}: mean |d| {errs[0]:.2e} mean D {errs[1]:.2e}; gradient {gerr:.2e} / {gerr1:.2e}")
    assert max(errs) <= L1_RTOL and gerr <= KERNEL_RTOL and gerr1 <= KERNEL_RTOL, (errs, gerr, gerr1)
    assert int((g == 0).sum()) == int(same.sum()) and bool((g.transpose(1, 2)[torch.from_numpy(same).to(_dev())] == 0).all())
    assert torch.equal(out, _native.basis_weight_l1(Dd, td)) and torch.equal(g, _native.basis_weight_l1_grad(Dd, td, coef))


# ---- the whole chain ----
def _model(cfg, sd):
    m = build_generator("basis-melgan", cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    return m.to(_dev())


def _trainable(gen):
    gen.basis_grad = True
    gen.parameter_grad = True
    return gen


@functools.lru_cache(maxsize=None)
def _case(tag):
    """(cfg, state dict, mel, cotangent of est, cotangent of weight, target) of a chain case."""
    return bref.chain_case(tag)


@functools.lru_cache(maxsize=None)
def _float64(tag, which):
    """The float64 (est, weight, gradients) of a chain case for both cotangents or one of them; computed once."""
    cfg, sd, mel, c_est, c_w, _ = _case(tag)
    return bref.param_grad(cfg, sd, mel, c_est if which != "weight" else None, c_w if which != "est" else None)


def _worst(tag, named, g64):
    errs = {k: _rel(named[k].grad, g64[k]) for k in g64}
    assert all(g64[k].size > 1 for k in g64)
    order = sorted(errs, key=errs.get, reverse=True)
    print(f"{tag}: worst .grad errors " + ", ".join(f"{errs[k]:.2e} ({k})" for k in order[:3]))
    return errs[order[0]]


def _trunk_keys(gen):
    return sorted(k for k, _ in gen.named_parameters() if k != bref.BASIS_KEY)


@pytest.mark.parametrize("which", ["both", "est", "weight"])
def test_chain_gradient_against_float64(which):
    cfg, sd, mel, c_est, c_w, _ = _case("basis_s")
    est64, w64, g64 = _float64("basis_s", which)
    gen = _trainable(_model(cfg, sd))
    est, weight = gen(_t(mel))
    assert est.requires_grad and weight.requires_grad and est.shape == est64.shape and weight.shape == w64.shape
    total = 0.0
    if which != "weight":
        total = total + (est * _t(c_est)).sum()
    if which != "est":
        total = total + (weight * _t(c_w)).sum()
    total.backward()
    named = dict(gen.named_parameters())
    assert _trunk_keys(gen) == sorted(g64) and named[bref.BASIS_KEY].grad is None
    err = _worst(f"basis_s ({which})", named, g64)
    eerr = float(np.abs(est.detach().cpu().double().numpy() - est64).max())
    werr = float(np.abs(weight.detach().cpu().double().numpy() - w64).max())
    print(f"basis_s ({which}): est {eerr:.2e} weight {werr:.2e}")
    assert err <= GRAD_RTOL and eerr <= WAVE_TOL and werr <= WAVE_TOL, (err, eerr, werr)


def test_golden_case_meets_the_reference_gradient():
    g = np.load(os.path.join(cases.ROOT, "tests", "golden", "basis_param_grad.npz"))
    cfg = bref.GOLDEN_CFG
    gen = _trainable(_model(cfg, seeded_state_dict("basis-melgan", cfg, int(g["weight_seed"]))))
    est, weight = gen(_t(g["mel"]))
    l1, average = BasisWeightL1.apply(weight, _t(g["target"]))
    ((est * _t(g["c"])).sum() + l1).backward()
    named = dict(gen.named_parameters())
    g64 = {k: g["grad/" + k] for k in _trunk_keys(gen)}
    err = _worst("golden", named, g64)
    eerr = float(np.abs(est.detach().cpu().double().numpy() - g["est"]).max())
    werr = float(np.abs(weight.detach().cpu().double().numpy() - g["weight"]).max())
    aerr = abs(float(average.detach()) - float(g["weight"].mean()))
    print(f"golden: est {eerr:.2e} weight {werr:.2e} weight average {aerr:.2e}")
    assert err <= GOLDEN_RTOL and eerr <= WAVE_TOL and werr <= WAVE_TOL and aerr <= WAVE_TOL, (err, eerr, werr, aerr)
    assert named[bref.BASIS_KEY].grad is None and not average.requires_grad


def test_default_off_changes_nothing_and_the_training_forward_meets_the_inference_forward():
    cfg, sd, mel, c_est, _, _ = _case("basis_s")
    gen = _model(cfg, sd)
    est0, w0 = gen(_t(mel))
    assert not est0.requires_grad and not w0.requires_grad
    gen.basis_grad = True                                          # the opt-in alone: still the plan
    est1, w1 = gen(_t(mel))
    assert not est1.requires_grad and torch.equal(est0, est1) and torch.equal(w0, w1)
    gen.parameter_grad = True
    est, weight = gen(_t(mel))
    eerr, werr = float((est.detach() - est0).abs().max()), float((weight.detach() - w0).abs().max())
    print(f"training forward against the inference forward: est {eerr:.2e} weight {werr:.2e}")
    assert est.shape == est0.shape and weight.shape == w0.shape and eerr <= WAVE_TOL and werr <= WAVE_TOL
    est.backward(_t(c_est), retain_graph=True)                     # the weight's cotangent is None
    with pytest.raises(RuntimeError, match="second forward"):
        est.backward(_t(c_est))
    with torch.no_grad():
        assert not gen(_t(mel))[0].requires_grad
    with pytest.raises(RuntimeError, match="mel requires grad"):
        gen(_t(mel).requires_grad_(True))
    # the basis alone requiring grad: the plain forward
    for k, q in gen.named_parameters():
        q.requires_grad_(k == bref.BASIS_KEY)
    est2, _ = gen(_t(mel))
    assert not est2.requires_grad and torch.equal(est0, est2)
    gen.basis_grad = False
    assert gen.parameter_grad is False


# ---- composition: Loss and Trainer.step ----
SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
LAMBDA_STFT = 5.0


def _small_msd():
    disc = MelGANMultiScaleDiscriminator(**SMALL_MSD)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("msd", 3, **SMALL_MSD).items()})
    return disc.to(_dev())


def _trainer(gen, disc, start, lr=1e-4):
    # a clip threshold no gradient reaches: .grad keeps the backward's bits (scaled by min(1, ...) = 1)
    return Trainer(gen, disc, optim.Adam(gen.melgan.parameters(), lr=lr, eps=1e-6),
                   optim.Adam(disc.parameters(), lr=5e-5, eps=1e-6), lambda_stft=LAMBDA_STFT, use_feature_map_loss=True,
                   discriminator_train_start_steps=start, grad_clip_thresh=1e9, basis_grad=True)


def _wav(cfg, seed):
    n = bref.frames(cfg, cases.SMALL_T) * (cfg["L"] // 2)
    t = np.arange(n) / 24000.0
    rs = np.random.RandomState(seed)
    return _t(np.stack([0.4 * np.sin(2 * np.pi * (180.0 + 70 * b) * t) + 0.02 * rs.randn(n) for b in range(cases.SMALL_B)]))


def _state(gen):
    return {k: v.detach().cpu().numpy().copy() for k, v in gen.state_dict().items()}


def _probe(trainer, gen, disc, mel, wav, target, adversarial):
    """The cotangents the step's losses hand to a detached (est, weight) of the training forward, and the total: the
    float64 generator VJP of them is what the step must leave in .grad (the losses' own gradients have their tests)."""
    est, weight = (t.detach().clone().requires_grad_(True) for t in gen(mel))
    stft, weight_loss = trainer.vocoder_loss(est, wav, est_weight=weight, weight=target)
    total = LAMBDA_STFT * stft
    if adversarial:
        terms = generator_adversarial_terms(disc, est.unsqueeze(1), wav.unsqueeze(1))
        total = total + terms["adversarial"] + terms["feature_map"]
    else:
        total = total + weight_loss
    total.backward()
    c_w = None if weight.grad is None else weight.grad.cpu().numpy()
    return est.grad.cpu().numpy(), c_w, float(total.detach()), float(weight_loss.detach()), float(weight.detach().mean())


def test_loss_carries_both_terms_to_the_float64_gradient():
    cfg, sd, mel, _, _, target = _case("basis_s")
    gen, disc = _trainable(_model(cfg, sd)), _small_msd()
    trainer = _trainer(gen, disc, start=10)
    wav = _wav(cfg, 9)
    c_est, c_w, _, w_l, _ = _probe(trainer, gen, disc, _t(mel), wav, _t(target), adversarial=False)
    weight = gen(_t(mel))[1].detach().cpu().double().numpy()        # the training forward's
    ref_l1 = float(np.abs(weight - target.astype(np.float64)).mean())
    print(f"weight loss through Loss {w_l:.8e}, float64 of the same weights {ref_l1:.8e}")
    assert abs(w_l - ref_l1) <= L1_RTOL * max(ref_l1, float(np.abs(weight).mean())), (w_l, ref_l1)
    _, _, g64 = bref.param_grad(cfg, sd, mel, c_est, c_w)
    est, weight = gen(_t(mel))
    stft, weight_loss = trainer.vocoder_loss(est, wav, est_weight=weight, weight=_t(target))
    (LAMBDA_STFT * stft + weight_loss).backward()
    err = _worst("basis_s through Loss", dict(gen.named_parameters()), g64)
    assert err <= GRAD_RTOL, err


def test_three_trainer_steps_in_the_weight_phase_carry_the_float64_gradient():
    cfg, sd, mel, _, _, target = _case("basis_s")
    gen, disc = _model(cfg, sd), _small_msd()
    trainer = _trainer(gen, disc, start=10)
    assert trainer.samples_per_frame == 4 * 4 * 15 and gen.parameter_grad is True
    wav, meld, td = _wav(cfg, 9), _t(mel), _t(target)
    basis = gen.basis_signal.layer.weight.detach().clone()
    for step in (1, 2, 3):
        cur = _state(gen)
        c_est, c_w, total, w_l, average = _probe(trainer, gen, disc, meld, wav, td, adversarial=False)
        _, _, g64 = bref.param_grad(cfg, cur, mel, c_est, c_w)
        out = trainer.step(meld, wav, step, td)
        assert tuple(out) == KEYS + ("weight", "weight_average")
        assert out["total"] == total and out["weight"] == w_l and out["discriminator"] == 0.0
        assert abs(out["weight_average"] - average) <= 1e-6 * max(abs(average), 1e-3), (out["weight_average"], average)
        named = dict(gen.named_parameters())
        err = _worst(f"trainer step {step}", named, g64)
        assert err <= GRAD_RTOL, err
        assert all(not np.array_equal(named[k].detach().cpu().numpy(), cur[k]) for k in g64)   # Adam moved the trunk
        assert named[bref.BASIS_KEY].grad is None and torch.equal(named[bref.BASIS_KEY], basis)


def test_a_trainer_step_in_the_adversarial_phase_leaves_the_weight_term_out():
    cfg, sd, mel, _, _, target = _case("basis_s")
    gen, disc = _model(cfg, sd), _small_msd()
    trainer = _trainer(gen, disc, start=0)
    wav, meld, td = _wav(cfg, 9), _t(mel), _t(target)
    c_est, c_w, total, w_l, _ = _probe(trainer, gen, disc, meld, wav, td, adversarial=True)
    assert c_w is None
    _, _, g64 = bref.param_grad(cfg, sd, mel, c_est, None)
    out = trainer.step(meld, wav, 1, td)
    assert out["total"] == total and w_l > 0.0 and out["weight"] == 0.0 and out["discriminator"] > 0.0
    assert np.isfinite(out["weight_average"]) and out["weight_average"] != 0.0
    assert abs(out["total"] - (LAMBDA_STFT * out["stft"] + out["adversarial"] + out["feature_map"])) <= 1e-5 * out["total"]
    err = _worst("trainer step, adversarial", dict(gen.named_parameters()), g64)
    assert err <= GRAD_RTOL, err


def test_a_resumed_run_repeats_the_uninterrupted_one():
    cfg, sd, mel, _, _, target = _case("basis_s")
    wav, meld, td = _wav(cfg, 9), _t(mel), _t(target)

    def fresh():
        gen, disc = _model(cfg, sd), _small_msd()
        return gen, disc, _trainer(gen, disc, start=2)

    gen, disc, trainer = fresh()
    for step in (1, 2, 3, 4):
        trainer.step(meld, wav, step, td)
    want = _state(gen)
    gen, disc, trainer = fresh()
    for step in (1, 2):
        trainer.step(meld, wav, step, td)
    saved = [m.state_dict() for m in (gen, trainer.optimizer, disc, trainer.discriminator_optimizer)]
    start = _state(gen)
    gen, disc, trainer = fresh()
    for module, state in zip((gen, trainer.optimizer, disc, trainer.discriminator_optimizer), saved):
        module.load_state_dict(state)
    for step in (3, 4):
        trainer.step(meld, wav, step, td)
    got = _state(gen)
    worst = max(bref.rel_err(got[k], want[k]) for k in want)
    moved = max(bref.rel_err(start[k], want[k]) for k in want if k != bref.BASIS_KEY)
    print(f"resumed run against the first: parameters {worst:.2e} (steps 3 and 4 moved them by {moved:.2e})")
    # the same rows in the same order, no atomics anywhere: the same bits
    assert all(np.array_equal(got[k], want[k]) for k in want), worst
    assert moved > GRAD_RTOL, moved
    assert np.array_equal(got[bref.BASIS_KEY], np.asarray(sd[bref.BASIS_KEY], np.float32))
