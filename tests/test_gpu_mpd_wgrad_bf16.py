"""GPU tests of the multi-period discriminator's bf16 weight gradients (csrc/gen_grad_bf16.hip:
fv_period_conv_weight_grad_bf16; ``grad_precision = "bf16"`` on DiscriminatorP, MultiPeriodDiscriminator and
Discriminator(use_mpd=True), ``Trainer(discriminator_grad_precision=)``, ``MODE=train --discriminator_grad_precision``)
against the float64 oracles of tests/mpd_wgrad_bf16_reference.py: the closed form of the fp32 kernel on operands
rounded to bf16 (nearest even), and float64 autograd whose conv2d weight gradients take rounded operands.  The tests
print every figure they assert on (run with -s).

A kernel's products are exact in fp32, so against the closed form on ROUNDED operands only the order of the fp32
additions is left: the bound is KERNEL_RTOL, the project's constant for one kernel alone.  Against the closed form on
the UN-rounded operands the same result has to sit 10 x KERNEL_RTOL away and more (tests/test_mpd_wgrad_bf16_host.py
shows on the CPU that every shape allows it: 1.8e-3 at the least): that is the assertion that the operands are rounded
at all.  The chain bounds are those of tests/test_gpu_generator_grad_bf16.py: YARDSTICK_FACTOR x the yardstick (a)
against the bf16 oracle, the routing floor (b) less FLOOR_RTOL away from the fp32 mode.

Measured on MI355X, the 100 kernel shapes: dw 1.7e-7 of the rounded closed form at the worst
(1024 -> 1024, p 3), 1.8e-3 .. 3.8e-3 of the un-rounded one, db 2.4e-7, representable operands within 2.2e-7 of the fp32
entry.  The chains, worst against the bf16 oracle beside 4 x (a): p2 5.0e-4 (2.0e-3), p3 3.6e-4 (1.4e-3), p5 6.3e-4
(6.7e-4), p7 1.8e-4 (7.6e-4), p11 2.7e-4 (5.4e-4), mpd 3.0e-4 (1.0e-3); least distance from the fp32 mode beside (b):
1.596e-3 (1.596e-3), 1.730e-3 (1.729e-3), 1.061e-3 (1.061e-3), 9.128e-4 (9.131e-4), 5.827e-4 (5.828e-4), 3.955e-4
(3.772e-4); bias gradients 1.4e-6 at the worst."""
import functools
import glob

import numpy as np
import pytest
import torch
import yaml

from fastvocoder_amd import _native, optim
from fastvocoder_amd.bin.synthesize import load_checkpoint
from fastvocoder_amd.discriminator import Discriminator
from fastvocoder_amd.loss import discriminator_step_terms, generator_adversarial_terms
from fastvocoder_amd.train import Trainer, samples_per_frame
from tests import generator_grad_bf16_reference as bref
from tests import mpd_wgrad_bf16_reference as pb
from tests import mpd_wgrad_reference as wref
from tests import test_gpu_mpd_wgrad as fp32_tests
from tests import test_gpu_train as train_tests
from tests.test_gpu_generator_grad import KERNEL_RTOL

pytestmark = pytest.mark.gpu

ROUNDED_FLOOR = 10 * KERNEL_RTOL       # a result this close to the un-rounded closed form did not round its operands
_dev, _t, _rel = fp32_tests._dev, fp32_tests._t, fp32_tests._rel


def _nan(n):
    return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float32, device=_dev())


# ---- the kernel ----
@pytest.mark.parametrize("cin,cout,k,stride,p,H,B", pb.KERNEL_SHAPES)
def test_period_conv_weight_grad_bf16_against_float64(cin, cout, k, stride, p, H, B):
    what = f"period conv {(cin, cout, k, stride)} p={p} H={H} B={B}"
    g, x = wref.kernel_inputs(cin, cout, k, stride, p, H, B)
    call = lambda gd, xd, w, b, ws, pr: _native.period_conv_weight_grad(  # noqa: E731
        gd, xd, k, stride, w, b, workspace=ws, precision=pr)
    floats = _native.period_conv_weight_grad_workspace_floats(B, cin, cout, H, p, k, stride, "bf16")
    rounded, exact_db = pb.period_conv_weight_grad(g, x, k, stride)
    exact = wref.period_conv_weight_grad(g, x, k, stride)[0]
    gd, xd = _t(g), _t(x)
    dw, none = call(gd, xd, True, False, None, "bf16")
    assert none is None and dw.shape == (cout, cin, k)
    err, away = _rel(dw, rounded), _rel(dw, exact)
    dw2, db2 = call(gd, xd, True, True, None, "bf16")
    berr = _rel(db2, exact_db)
    print(f"bf16 {what}: dw {err:.2e} of the rounded closed form, {away:.2e} of the un-rounded one; db {berr:.2e}")
    assert err <= KERNEL_RTOL, err
    assert away > ROUNDED_FLOOR, away
    assert berr <= KERNEL_RTOL, berr
    # a second call, a workspace full of NaN, the weight alone / with the bias / the bias alone: equal bits
    dw3, db3 = call(gd, xd, True, True, _nan(floats), "bf16")
    none, db4 = call(gd, xd, False, True, _nan(floats), "bf16")
    assert none is None
    assert torch.equal(dw, dw2) and torch.equal(dw, dw3) and torch.equal(db2, db3) and torch.equal(db2, db4)
    assert torch.isfinite(dw3).all() and torch.isfinite(db4).all()
    # operands that are bf16 values already: the fp32 entry computes the same sum
    gr, xr = _t(bref.bf16_round(g)), _t(bref.bf16_round(x))
    same = _rel(call(gr, xr, True, False, None, "bf16")[0], call(gr, xr, True, False, None, "f32")[0].cpu().double().numpy())
    print(f"bf16 {what}: representable operands, against the fp32 entry {same:.2e}")
    assert same <= KERNEL_RTOL, same
    if H == 1 and k == 5:                                        # one row: only the centre tap meets it
        assert not dw[:, :, [0, 1, 3, 4]].any() and dw[:, :, 2].any()


def test_a_strided_shape_below_64_output_channels_is_refused():
    cin, cout, k, stride, p, H, B = pb.REFUSED_SHAPE
    g, x = wref.kernel_inputs(cin, cout, k, stride, p, H, B)
    assert _native.period_conv_weight_grad(_t(g), _t(x), k, stride)[0].shape == (cout, cin, k)    # the fp32 entry runs it
    with pytest.raises(_native.NativeError, match="Cout >= 64"):
        _native.period_conv_weight_grad(_t(g), _t(x), k, stride, precision="bf16")
    with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
        _native.period_conv_weight_grad(_t(g), _t(x), k, stride, precision="f16")


# ---- the whole chain ----
def _np(grads):
    return {k: v.cpu().double().numpy() for k, v in grads.items()}


def _run(module, kind, est, real, precision):
    """(terms, gradients) of one discriminator step in ``precision``."""
    module.grad_precision = precision
    terms = fp32_tests._step(module, kind, est, real)
    return {k: v.detach().clone() for k, v in terms.items()}, fp32_tests._grads(module)


@functools.lru_cache(maxsize=None)
def _chain(name):
    """Everything a chain case compares, computed once and shared: the fp32-mode and bf16-mode runs of one module,
    the bf16 oracle and the exact oracle in float64 (for "mpd" both with the device's leaky-ReLU sides)."""
    module, sd, kind, kw = fp32_tests._build(name)
    est, real = wref.case_signals(name)
    fresh, _, _, _ = fp32_tests._build(name)                       # a module that never leaves "f32"
    terms_never, never = _run(fresh, kind, est, real, "f32")
    with torch.no_grad():
        maps = [fp32_tests._lists(module, module(_t(v))) for v in (est, real)]
    terms16, g16 = _run(module, kind, est, real, "bf16")
    with torch.no_grad():
        maps16 = [fp32_tests._lists(module, module(_t(v))) for v in (est, real)]
    terms_back, back = _run(module, kind, est, real, "f32")
    adopt = {}
    if name == "mpd":
        adopt = dict(est_maps=fp32_tests._np_lists(maps[0]), real_maps=fp32_tests._np_lists(maps[1]))
    oracle = pb.param_grad_bf16(kind, est, real, sd, **adopt, **kw)[0]
    exact = wref.param_grad(kind, est, real, sd, **adopt, **kw)[0]
    return dict(never=never, g16=g16, back=back, terms=(terms_never, terms16, terms_back), maps=(maps, maps16),
                oracle=oracle, exact=exact)


@pytest.mark.parametrize("name", pb.CHAIN_CASES)
def test_chain_gradient_in_bf16_mode(name):
    c = _chain(name)
    yard, floor = pb.CHAIN_FIGURES[name]
    bound = fp32_tests._bound(fp32_tests._family(name))
    g16, g32 = _np(c["g16"]), _np(c["never"])
    assert sorted(g16) == sorted(c["oracle"])
    errs = {k: wref.rel_err(g16[k], c["oracle"][k]) for k in g16 if g16[k].size > 1}
    worst = max(errs, key=errs.get)
    routed = {k: wref.rel_err(g16[k], g32[k]) for k in g16 if pb.is_rounded_weight(k)}
    least = min(routed, key=routed.get)
    bias = {k: wref.rel_err(g16[k], c["exact"][k]) for k in g16 if k.endswith(".bias")}
    bworst = max(bias, key=bias.get)
    print(f"{name} bf16: worst against the float64 bf16 oracle {errs[worst]:.2e} ({worst}), yardstick (a) {yard:.2e}, "
          f"bound {pb.YARDSTICK_FACTOR * yard:.2e}; least distance from the f32 mode {routed[least]:.3e} ({least}), "
          f"floor (b) {floor:.3e}; worst bias gradient against exact float64 {bias[bworst]:.2e} ({bworst}), "
          f"bound {bound:.2e}")
    assert len(routed) == 5 * (5 if name == "mpd" else 1)
    assert errs[worst] <= pb.YARDSTICK_FACTOR * yard, (worst, errs[worst])
    assert routed[least] >= floor * (1 - pb.FLOOR_RTOL), (least, routed[least])
    assert bias[bworst] <= bound, (bworst, bias[bworst])
    first = [k for k in g16 if pb.is_first(k)]
    assert len(first) == 3 * (5 if name == "mpd" else 1)
    for k in first:                                              # the first layer: fp32 in both modes
        assert torch.equal(c["g16"][k], c["never"][k]), k


@pytest.mark.parametrize("name", ["p5", "mpd"])
def test_the_attribute_does_not_reach_the_forward_and_leaves_no_trace(name):
    c = _chain(name)
    never, t16, back = c["terms"]
    for k in ("real", "fake", "discriminator"):                  # the three terms: equal bits in both modes
        assert torch.equal(never[k], t16[k]) and torch.equal(never[k], back[k]), k
    for la, lb in zip(c["maps"][0], c["maps"][1]):               # the maps and the scores of both signals
        for ma, mb in zip(la, lb):
            assert all(torch.equal(a, b) for a, b in zip(ma, mb))
    # "bf16" and back to "f32": the bits of a module that never left "f32"
    assert all(torch.equal(c["back"][k], c["never"][k]) for k in c["never"])
    assert any(not torch.equal(c["g16"][k], c["never"][k]) for k in c["never"])


def test_the_attribute_does_nothing_to_the_input_gradient():
    module, sd, kind, kw = fp32_tests._build("p7")
    est, real = wref.case_signals("p7")
    out = []
    for precision in ("f32", "bf16"):
        module.grad_precision = precision
        x = _t(est).requires_grad_(True)
        terms = generator_adversarial_terms(module, x, _t(real), period_grad=True)
        (terms["adversarial"] + terms["feature_map"]).backward()
        out.append((terms["adversarial"].detach().clone(), x.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][1].abs().max() > 0
    assert all(q.grad is None for q in module.parameters())


def test_the_discriminator_forwards_the_attribute_to_the_mpd_alone():
    name = "discriminator_mpd"
    module, sd, kind, kw = fp32_tests._build(name)
    est, real = wref.case_signals(name)
    terms32, g32 = _run(module, kind, est, real, "f32")
    terms16, g16 = _run(module, kind, est, real, "bf16")
    assert module.mpd.grad_precision == "bf16" and all(d.grad_precision == "bf16" for d in module.mpd.discriminators)
    assert all(torch.equal(terms32[k], terms16[k]) for k in terms32)
    moved = [k for k in g32 if not torch.equal(g32[k], g16[k])]
    rounded = [k for k in g32 if pb.is_rounded_weight(k) and k.startswith("mpd.")]
    away = min(_rel(g16[k], g32[k].cpu().double().numpy()) for k in rounded)
    print(f"Discriminator(use_mpd=True): {len(moved)} of {len(g32)} gradients moved, all of them the MPD's; the rounded "
          f"weights by at least {away:.2e}")
    assert len(rounded) == 25 and set(rounded) <= set(moved) and all(k.startswith("mpd.") for k in moved)
    assert away > ROUNDED_FLOOR
    assert all(torch.equal(g32[k], g16[k]) for k in g32 if k.startswith(("msd.", "mfd.")) or pb.is_first(k))
    with pytest.raises(NotImplementedError, match="no bf16 kernels"):
        Discriminator().grad_precision = "bf16"


# ---- the trainer and the command line ----
def _trainer(precision):
    name, cfg = train_tests.CONFIGS["hifigan"]
    torch.manual_seed(5)
    g, d = train_tests._generator(name, cfg, weight_seed=3), Discriminator(use_mpd=True).to(train_tests.DEV)
    kw = {} if precision is None else {"discriminator_grad_precision": precision}
    return g, d, Trainer(g, d, optim.Adam(g.parameters(), lr=1e-3, eps=1e-6),
                         optim.Adam(d.parameters(), lr=train_tests.LR_D, eps=1e-6), lambda_stft=train_tests.LAMBDA_STFT,
                         use_feature_map_loss=True, discriminator_train_start_steps=0, grad_clip_thresh=1.0, **kw)


def test_an_adversarial_step_with_the_discriminator_in_bf16_mode():
    runs = {}
    for precision in ("bf16", None):
        g, d, trainer = _trainer(precision)
        assert d.grad_precision == (precision or "f32") and g.grad_precision == "f32"
        g_before = {k: v.clone() for k, v in g.state_dict().items()}
        d_before = {k: v.clone() for k, v in d.state_dict().items()}
        mel, wav = train_tests._batch(samples_per_frame(g), seed=2)
        out = trainer.step(mel, wav, 1)
        assert all(np.isfinite(out[k]) for k in out) and out["adversarial"] > 0.0 and out["discriminator"] > 0.0
        assert any(not torch.equal(v, g_before[k]) for k, v in g.state_dict().items())
        assert any(not torch.equal(v, d_before[k]) for k, v in d.state_dict().items())
        runs[precision] = (out, {k: q.grad.clone() for k, q in g.named_parameters()},
                           {k: v.clone() for k, v in g.state_dict().items()},
                           {k: v.clone() for k, v in d.state_dict().items()})
    (o16, gg16, gs16, ds16), (o32, gg32, gs32, ds32) = runs["bf16"], runs[None]
    print(f"one adversarial step: discriminator gradient norm {o16['discriminator_grad_norm']:.6f} (bf16) "
          f"{o32['discriminator_grad_norm']:.6f} (f32)")
    assert all(o16[k] == o32[k] for k in ("stft", "total", "adversarial", "feature_map", "discriminator", "grad_norm"))
    assert all(torch.equal(gg16[k], gg32[k]) for k in gg32)      # the generator's gradients and step: the fp32 bits
    assert all(torch.equal(gs16[k], gs32[k]) for k in gs32)
    assert any(not torch.equal(ds16[k], ds32[k]) for k in ds32 if k.startswith("mpd."))
    assert all(torch.equal(ds16[k], ds32[k]) for k in ds32 if "convs.0." in k)   # the first layers


def test_mode_train_takes_the_flag_and_resumes_without_it(tmp_path):
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(train_tests.CLI_CFG))
    train_tests._dataset(tmp_path, "train", 5, seed=0)
    train_tests._dataset(tmp_path, "valid", 2, seed=1)
    out = train_tests._train(tmp_path, "--use_mpd", "1", "--discriminator_grad_precision", "bf16", "--max_steps", "2",
                             "--save_step", "2", "--valid_step", "100", "--discriminator_train_start_steps", "0")
    assert "---Start New Training---" in out and "save model at step 2 ..." in out
    train_tests._logged(out, 2)                                     # the log lines are the usual ones
    (ck,) = glob.glob(str(tmp_path / "checkpoint" / "*" / "checkpoint_2.pth.tar"))
    saved = load_checkpoint(ck, "cpu")
    assert sorted(saved) == ["discriminator", "discriminator_optimizer", "model", "optimizer"]
    assert any(k.startswith("mpd.") for k in saved["discriminator"])
    out = train_tests._train(tmp_path, "--checkpoint_path", ck, "--restore_step", "2", "--max_steps", "1",
                             "--save_step", "100", "--valid_step", "100", "--discriminator_train_start_steps", "0")
    assert "---Model Restored at Step 2---" in out
    train_tests._logged(out, 3)
