"""GPU tests of the multi-scale discriminator's parameter gradient (csrc/disc_wgrad.hip: fv_conv1d_weight_grad,
fv_grouped_conv1d_weight_grad, fv_weight_norm_grad; the ``parameter_grad`` attribute of
fastvocoder_amd.discriminator; loss.discriminator_step_terms) against the float64 closed forms of
tests/msd_wgrad_reference.py on the same fp32 inputs, float64 autograd of the discriminator's own loss and the
reference's own gradient (tests/golden/msd_param_grad.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import MelGANDiscriminator, MelGANMultiScaleDiscriminator
from fastvocoder_amd.loss import discriminator_step_terms, discriminator_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import msd_wgrad_reference as wref

pytestmark = pytest.mark.gpu

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_KW = dict(SMALL_MSD, downsample_scales=(4, 2))

# Relative to the largest magnitude of the tensor compared, against float64: the worst errors measured on MI355X
#  times about 10.  The yardstick beside them: float32 eager autograd of the same chain on the
# CPU errs by 6.8e-7 (short case) and 9.3e-7 (long case) per parameter tensor (tests/test_msd_wgrad_host.py).
KERNEL_RTOL = 4e-6       # one kernel alone (worst 4.2e-7: the dense 1024 -> 1024 weight gradient at 131 samples)
GRAD_RTOL = 1.4e-5       # .grad of a whole chain (worst 1.4e-6: the full-size MSD, discriminators.1.layers.6.weight_g)
GOLDEN_RTOL = 6e-6       # the small MSD against the reference's float64 gradient (worst 5.6e-7, the long case)
SGD_RTOL = 8e-7          # the loss along three SGD steps against float64 (worst 8.4e-8)

# (Cin, Cout, k, pad mode, Tin, B)
DENSE_GRID = [
    (1, 4, 15, "reflect", 45, 2),          # small first layer
    (1, 16, 15, "reflect", 4099, 3),       # first layer, time split, length not a tile multiple
    (16, 16, 5, "zero", 13, 2),            # small 16 -> 16 conv
    (16, 16, 5, "zero", 1, 1),             # every tap but the centre falls in padding
    (20, 12, 3, "zero", 130, 2),           # channel counts that are no tile multiple
    (1024, 1024, 5, "zero", 7, 2),         # the matrix-core shape with a reduction shorter than a tile
    (1024, 1024, 5, "zero", 131, 2),       # the matrix-core shape at the training column count
    (1024, 1, 3, "zero", 67, 3),           # the score layer
    (70, 100, 3, "zero", 50, 2),           # the matrix-core kernel's edge tiles: Cout and Cin k no tile multiples
    (33, 64, 7, "reflect", 40, 1),         # the matrix-core kernel with a reflection pad
]

# (Cin, Cout, k, stride, Tin, B)
GROUPED_GRID = [
    (4, 16, 41, 4, 45, 2),                 # small first grouped layer
    (16, 16, 21, 2, 12, 2),                # small second grouped layer
    (8, 32, 13, 2, 3, 3),                  # input shorter than the kernel
    (4, 8, 3, 5, 40, 1),                   # stride above k
    (12, 48, 51, 5, 4097, 1),              # time split, odd length
    (16, 64, 41, 4, 1030, 3),              # the last input sample meets no window
    (64, 256, 41, 4, 515, 2),              # full-size 64 -> 256 layer
    (256, 1024, 41, 4, 130, 2),            # full-size 256 -> 1024 layer
    (1024, 1024, 41, 4, 67, 2),            # 4 outputs per group
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
    module.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    return module.to(_dev()).eval()


def _nan_workspace(grouped, B, cin, cout, tin, k, stride, pad, mode):
    n = _native.conv_weight_grad_workspace_floats(grouped, B, cin, cout, tin, k, stride, pad, mode)
    return torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device=_dev())


@pytest.mark.parametrize("with_db", [False, True], ids=["dw", "dw_db"])
@pytest.mark.parametrize("cin,cout,k,mode,T,B", DENSE_GRID)
def test_dense_weight_grad_against_float64(cin, cout, k, mode, T, B, with_db):
    rs = np.random.RandomState(cin + cout + k + T)
    pad = (k - 1) // 2
    tout = T + 2 * pad - k + 1
    g = rs.randn(B, cout, tout).astype(np.float32)
    x = rs.randn(B, cin, T).astype(np.float32)
    pm = _native.PAD_REFLECT if mode == "reflect" else _native.PAD_ZERO
    dw, db = _native.conv1d_weight_grad(_t(g), _t(x), k, pad, pm, True, with_db)
    err = _rel(dw, wref.dense_weight_grad(g, x, k, pad, mode))
    print(f"dense weight grad {(cin, cout, k, mode, T, B)}: {err:.2e}")
    assert err <= KERNEL_RTOL, err
    assert (db is None) == (not with_db)
    if with_db:
        berr = _rel(db, wref.bias_grad(g))
        print(f"dense bias grad {(cin, cout, k, mode, T, B)}: {berr:.2e}")
        assert berr <= KERNEL_RTOL, berr
    if T == 1:                                                   # only the centre tap meets the one sample
        other = [j for j in range(k) if j != pad]
        assert not dw[:, :, other].any() and dw[:, :, pad].any()
    # a second call, and one on a workspace full of NaN: equal bits
    dw2, db2 = _native.conv1d_weight_grad(_t(g), _t(x), k, pad, pm, True, with_db)
    dw3, db3 = _native.conv1d_weight_grad(_t(g), _t(x), k, pad, pm, True, with_db,
                                          workspace=_nan_workspace(False, B, cin, cout, T, k, 1, pad, pm))
    assert torch.equal(dw, dw2) and torch.equal(dw, dw3)
    if with_db:
        assert torch.equal(db, db2) and torch.equal(db, db3)
        only_db = _native.conv1d_weight_grad(_t(g), _t(x), k, pad, pm, False, True)
        assert only_db[0] is None and torch.equal(only_db[1], db)


@pytest.mark.parametrize("with_db", [False, True], ids=["dw", "dw_db"])
@pytest.mark.parametrize("cin,cout,k,s,T,B", GROUPED_GRID)
def test_grouped_weight_grad_against_float64(cin, cout, k, s, T, B, with_db):
    rs = np.random.RandomState(cin + cout + k + T)
    pad = (k - 1) // 2
    tout = (T + 2 * pad - k) // s + 1
    g = rs.randn(B, cout, tout).astype(np.float32)
    x = rs.randn(B, cin, T).astype(np.float32)
    dw, db = _native.grouped_conv1d_weight_grad(_t(g), _t(x), k, s, pad, True, with_db)
    err = _rel(dw, wref.grouped_weight_grad(g, x, k, s, pad))
    print(f"grouped weight grad {(cin, cout, k, s, T, B)}: {err:.2e}")
    assert err <= KERNEL_RTOL, err
    if with_db:
        berr = _rel(db, wref.bias_grad(g))
        print(f"grouped bias grad {(cin, cout, k, s, T, B)}: {berr:.2e}")
        assert berr <= KERNEL_RTOL, berr
    dw2, db2 = _native.grouped_conv1d_weight_grad(_t(g), _t(x), k, s, pad, True, with_db)
    dw3, db3 = _native.grouped_conv1d_weight_grad(_t(g), _t(x), k, s, pad, True, with_db,
                                                  workspace=_nan_workspace(True, B, cin, cout, T, k, s, pad, 0))
    assert torch.equal(dw, dw2) and torch.equal(dw, dw3)
    if with_db:
        assert torch.equal(db, db2) and torch.equal(db, db3)


def test_grouped_weight_grad_without_padding_and_windows_that_skip_samples():
    # pad 0 and (Tin - k) % stride != 0: the last input sample meets no window; stride > k: gaps between the windows
    rs = np.random.RandomState(5)
    for cin, cout, k, s, T in ((16, 64, 41, 4, 1030), (4, 4, 3, 5, 40)):
        tout = (T - k) // s + 1
        g, x = rs.randn(1, cout, tout).astype(np.float32), rs.randn(1, cin, T).astype(np.float32)
        dw, _ = _native.grouped_conv1d_weight_grad(_t(g), _t(x), k, s, 0)
        assert _rel(dw, wref.grouped_weight_grad(g, x, k, s, 0)) <= KERNEL_RTOL
        x2 = x.copy()
        x2[:, :, (tout - 1) * s + k:] = 7.0                      # samples no window holds do not matter
        assert torch.equal(dw, _native.grouped_conv1d_weight_grad(_t(g), _t(x2), k, s, 0)[0])


def test_weight_grad_error_codes():
    L = _native.lib()
    z = _t(np.zeros(4096))
    p = z.data_ptr()
    nbytes = ctypes.c_size_t(4096 * 4 - 64)

    def grouped(cin, cout, tin, k, s, pad, g=p, B=1, ws=p + 64, dw=p + 16):
        return L.fv_grouped_conv1d_weight_grad(g, p + 4, dw, None, B, cin, cout, tin, k, s, pad, ws, nbytes, None)
    assert grouped(6, 3, 100, 5, 1, 2) == _native.ERR_UNSUPPORTED           # not 4 channels per group
    assert grouped(8, 3, 100, 5, 1, 2) == _native.ERR_UNSUPPORTED           # Cout no multiple of the 2 groups
    assert grouped(8, 4, 100, 161, 16, 80) == _native.ERR_UNSUPPORTED       # beyond a block's shared memory
    assert grouped(8, 4, 100, 5, 0, 2) == _native.ERR_UNSUPPORTED           # stride 0
    assert grouped(8, 4, 100, 5, 0, 2, g=None) == _native.ERR_UNSUPPORTED   # UNSUPPORTED comes first
    assert grouped(8, 4, 100, 301, 1, 0) == _native.ERR_INVALID_ARG         # empty output
    assert grouped(8, 4, 100, 5, 1, 2, g=None) == _native.ERR_INVALID_ARG   # no gradient
    assert grouped(8, 4, 100, 5, 1, 2, dw=None) == _native.ERR_INVALID_ARG  # nothing asked for
    assert grouped(8, 4, 100, 5, 1, -1) == _native.ERR_INVALID_ARG
    assert grouped(8, 4, 100, 5, 1, 2, B=0) == _native.ERR_INVALID_ARG
    assert grouped(8, 4, 100, 5, 1, 2, ws=None) == _native.ERR_INVALID_ARG  # no workspace
    assert grouped(8, 4, 100, 5, 1, 2, dw=p) == _native.ERR_INVALID_ARG     # dw aliases g_pre

    def dense(cin, cout, tin, k, pad, mode=0, g=p, B=1, ws=p + 64, size=nbytes):
        return L.fv_conv1d_weight_grad(g, p + 4, p + 16, None, B, cin, cout, tin, k, pad, mode, ws, size, None)
    assert dense(0, 4, 100, 5, 2) == _native.ERR_UNSUPPORTED
    assert dense(4, 4, 100, 5, 2, mode=2) == _native.ERR_UNSUPPORTED        # causal padding: no such conv here
    assert dense(4, 4, 100, 0, 0) == _native.ERR_UNSUPPORTED
    assert dense(4, 4, 3, 15, 7, mode=1) == _native.ERR_INVALID_ARG         # a reflection pad beyond the input
    assert dense(4, 4, 3, 15, 2) == _native.ERR_INVALID_ARG                 # empty output
    assert dense(4, 4, 100, 5, 2, g=None) == _native.ERR_INVALID_ARG
    assert dense(4, 4, 100, 5, 2, B=0) == _native.ERR_INVALID_ARG
    assert dense(4, 4, 100, 5, 2, size=ctypes.c_size_t(16)) == _native.ERR_INVALID_ARG   # a small workspace
    assert L.fv_weight_norm_grad(p, p + 4, p + 8, None, None, 1, 4, None) == _native.ERR_INVALID_ARG
    assert L.fv_weight_norm_grad(p, p + 4, p + 8, p + 16, None, 0, 4, None) == _native.ERR_INVALID_ARG
    assert L.fv_weight_norm_grad(p, p + 4, p + 8, p, None, 1, 4, None) == _native.ERR_INVALID_ARG    # dv aliases dw
    torch.cuda.synchronize()


def test_weight_norm_grad_against_float64():
    """dv is held against the size of the two terms it is the difference of, (g / n) dw: a row of length 1 has
    dv = 0 by exact cancellation in float64, which an fp32 difference meets only to rounding."""
    rs = np.random.RandomState(8)
    for rows, inner in ((5, (1, 1)), (4, (1, 15)), (16, (4, 41)), (3, (1024, 5))):
        v = rs.randn(rows, *inner).astype(np.float32)
        g = rs.randn(rows, 1, 1).astype(np.float32)
        g[1] = 0.0                                               # a row with g = 0: dv is exactly 0, dg is not
        dw = rs.randn(rows, *inner).astype(np.float32)
        want_dv, want_dg = wref.weight_norm_grad(dw, v, g)
        dv, dg = _native.weight_norm_grad(_t(dw), _t(v), _t(g))
        assert dv.shape == v.shape and dg.shape == g.shape
        n = np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True))
        size = max(np.abs(want_dv).max(), np.abs(g / n * dw).max())
        verr = float(np.abs(dv.cpu().double().numpy() - want_dv).max() / size)
        gerr = _rel(dg.reshape(-1), want_dg)
        print(f"weight norm grad rows of {int(np.prod(inner))}: dv {verr:.2e} dg {gerr:.2e}")
        assert verr <= KERNEL_RTOL and gerr <= KERNEL_RTOL, (inner, verr, gerr)
        assert not dv[1].any() and bool(dg[1].any())
        only = _native.weight_norm_grad(_t(dw), _t(v), _t(g), want_dv=False)
        assert only[0] is None and torch.equal(only[1], dg)
        only = _native.weight_norm_grad(_t(dw), _t(v), _t(g), want_dg=False)
        assert only[1] is None and torch.equal(only[0], dv)


# ---- the modules ----
def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "msd_param_grad.npz"))
    return g, seeded_discriminator_state_dict("msd", int(g["seed"]), **SMALL_MSD)


def _step(module, est, real, zero=True):
    if zero:
        module.zero_grad(set_to_none=True)
    terms = discriminator_step_terms(module, _t(est), _t(real))
    terms["discriminator"].backward()
    return terms


def _grads(module):
    return {k: None if q.grad is None else q.grad.clone() for k, q in module.named_parameters()}


def _worst(grads, want):
    errs = {k: _rel(grads[k], want[k]) for k in want}
    k = max(errs, key=errs.get)
    return k, errs[k]


@pytest.mark.parametrize("case", ["short", "long"])
def test_small_msd_parameter_gradient_matches_the_oracle_and_the_golden(golden_dir, case):
    g, sd = _golden(golden_dir)
    est, real = g[f"{case}_est"], g[f"{case}_real"]
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    assert msd.parameter_grad is False
    with torch.no_grad():
        plain_est, plain_real = msd(_t(est)), msd(_t(real))
        plain_terms = discriminator_terms(plain_est, plain_real)
        quiet = discriminator_step_terms(msd, _t(est), _t(real))
    terms = _step(msd, est, real)
    grads = _grads(msd)
    assert sorted(grads) == sorted(sd) and all(v is not None for v in grads.values())
    want = wref.param_grad(est, real, sd, **SMALL_KW)[0]
    (k1, err), (k2, gerr) = _worst(grads, want), _worst(grads, {k: g[f"{case}_grad/{k}"] for k in sd})
    print(f"small MSD {case}: oracle {err:.2e} ({k1}) golden {gerr:.2e} ({k2})")
    assert err <= GRAD_RTOL and gerr <= GOLDEN_RTOL, (k1, err, k2, gerr)
    # the same launches: the maps and the three terms hold the bits of the plain path
    for x, plain in ((est, plain_est), (real, plain_real)):
        for la, lb in zip(msd._param_forward(_t(x)), plain):
            assert all(a.requires_grad and torch.equal(a, b) for a, b in zip(la, lb))
    for k in ("real", "fake", "discriminator"):
        assert terms[k].dtype == torch.float32 and terms[k].dim() == 0 and terms[k].requires_grad
        assert torch.equal(terms[k], plain_terms[k]) and torch.equal(quiet[k], plain_terms[k])
        assert not quiet[k].requires_grad
    # twice the same bits; two backward passes without zero_grad: exactly twice the first
    _step(msd, est, real)
    again = _grads(msd)
    assert all(torch.equal(again[k], grads[k]) for k in grads)
    _step(msd, est, real, zero=False)
    assert all(torch.equal(q.grad, 2 * grads[k]) for k, q in msd.named_parameters())


def test_a_frozen_parameter_gets_no_gradient_and_the_others_keep_theirs(golden_dir):
    g, sd = _golden(golden_dir)
    est, real = g["short_est"], g["short_real"]
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    _step(msd, est, real)
    full = _grads(msd)
    named = dict(msd.named_parameters())
    frozen = ["discriminators.0.layers.0.1.weight_g", "discriminators.0.layers.0.1.weight_v",
              "discriminators.0.layers.0.1.bias",            # the whole lowest layer of scale 0: the walk ends above it
              "discriminators.1.layers.2.0.weight_v", "discriminators.2.layers.3.0.bias",
              "discriminators.2.layers.4.weight_g"]
    for k in frozen:
        named[k].requires_grad_(False)
    _step(msd, est, real)
    for k, q in named.items():
        if k in frozen:
            assert q.grad is None, k
        else:
            assert torch.equal(q.grad, full[k]), k
    for q in named.values():                                     # everything frozen: the values, no graph
        q.requires_grad_(False)
    terms = discriminator_step_terms(msd, _t(est), _t(real))
    assert not terms["discriminator"].requires_grad


def test_the_attribute_decides_the_plain_forward(golden_dir):
    g, sd = _golden(golden_dir)
    est = g["short_est"]
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    assert msd.parameter_grad is False
    out = msd(_t(est))                                           # grad enabled, parameters require grad: constants
    assert all(not m.requires_grad for lst in out for m in lst)
    assert all(q.grad is None for q in msd.parameters())
    msd.differentiable = True                                    # ... also with the input gradient switched on
    x = _t(est).requires_grad_(True)
    sum((lst[-1] ** 2).mean() for lst in msd(x)).backward()
    assert x.grad is not None and all(q.grad is None for q in msd.parameters())
    msd.differentiable = False
    msd.parameter_grad = True
    with pytest.raises(RuntimeError, match="inference-only"):
        msd(_t(est).requires_grad_(True))                        # x's gradient still needs `differentiable`
    out2 = msd(_t(est))
    assert all(m.requires_grad and torch.equal(m, p) for la, lb in zip(out2, out) for m, p in zip(la, lb))
    sum((lst[-1] ** 2).mean() for lst in out2).backward()
    assert all(q.grad is not None for q in msd.parameters())
    with torch.no_grad():
        assert not msd(_t(est))[0][0].requires_grad
    one = MelGANDiscriminator(**SMALL_MSD)
    one.apply_weight_norm()
    one = _load(one, {k[len("discriminators.1."):]: v for k, v in sd.items() if k.startswith("discriminators.1.")})
    _step(one, est, g["short_real"])                             # a single scale takes the same call
    want = wref.param_grad(est, g["short_real"], sd, scale=1, **SMALL_KW)[0]
    k, err = _worst({f"discriminators.1.{n}": v for n, v in _grads(one).items()}, want)
    print(f"small MelGANDiscriminator: {err:.2e} ({k})")
    assert err <= GRAD_RTOL, (k, err)


def test_input_and_parameter_gradient_together(golden_dir):
    """``differentiable`` and ``parameter_grad`` on an x that requires grad: x.grad holds the bits of the input
    gradient alone, the parameters' gradients the bits of the parameter gradient alone."""
    g, sd = _golden(golden_dir)
    est, real = g["long_est"], g["long_real"]
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    with torch.no_grad():
        p = msd(_t(real))

    def run(diff, params, x_grad):
        msd.zero_grad(set_to_none=True)
        msd.differentiable, msd.parameter_grad = diff, params
        x = _t(est).requires_grad_(x_grad)
        terms = discriminator_terms(msd(x), p, differentiable=True)
        (terms["fake"] + terms["adversarial"] + terms["feature_map"]).backward()
        return x.grad, _grads(msd)

    gx_only, none = run(True, False, True)
    assert all(v is None for v in none.values())
    _, gp_only = run(False, True, False)
    gx, gp = run(True, True, True)
    assert torch.equal(gx, gx_only)
    assert all(torch.equal(gp[k], gp_only[k]) for k in gp)


def test_a_module_without_weight_norm(golden_dir):
    g, sd = _golden(golden_dir)
    est, real = g["short_est"], g["short_real"]
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    msd.remove_weight_norm()
    plain_sd = {k: v.detach().cpu().numpy() for k, v in msd.state_dict().items()}
    assert all(not k.endswith(("weight_g", "weight_v")) for k in plain_sd)
    _step(msd, est, real)
    k, err = _worst(_grads(msd), wref.param_grad(est, real, plain_sd, **SMALL_KW)[0])
    print(f"small MSD without weight norm: {err:.2e} ({k})")
    assert err <= GRAD_RTOL, (k, err)


def test_full_size_msd_parameter_gradient_matches_the_oracle():
    sd = seeded_discriminator_state_dict("msd", 13)
    msd = _load(MelGANMultiScaleDiscriminator(), sd)
    n = msd.min_length() + 300
    rs = np.random.RandomState(21)
    real = (0.5 * rs.randn(1, 1, n)).astype(np.float32)
    est = (real + 0.2 * rs.randn(1, 1, n)).astype(np.float32)
    _step(msd, est, real)
    k, err = _worst(_grads(msd), wref.param_grad(est, real, sd)[0])
    print(f"full-size MSD n={n}: {err:.2e} ({k})")
    assert err <= GRAD_RTOL, (k, err)


def test_three_sgd_steps_follow_float64_and_the_caches_follow_the_optimizer(golden_dir):
    g, sd = _golden(golden_dir)
    est, real = g["short_est"], g["short_real"]
    lr = 0.05
    want_losses, _, _ = wref.sgd_steps(est, real, sd, 3, lr, **SMALL_KW)
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    opt = torch.optim.SGD(msd.parameters(), lr=lr)
    losses = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        losses.append(float(_step(msd, est, real, zero=False)["discriminator"].detach()))
        if step < 2:
            opt.step()
    errs = [abs(a - b) / abs(b) for a, b in zip(losses, want_losses)]
    print(f"three SGD steps: losses {losses} against {want_losses}: {max(errs):.2e}")
    assert max(errs) <= SGD_RTOL, errs
    fresh = MelGANMultiScaleDiscriminator(**SMALL_MSD)
    fresh.load_state_dict(msd.state_dict())
    fresh = fresh.to(_dev()).eval()
    _step(fresh, est, real)
    third, again = _grads(msd), _grads(fresh)
    assert all(torch.equal(third[k], again[k]) for k in third)
