"""GPU tests of the STFT and period discriminators' parameter gradient (csrc/mpd_wgrad.hip:
fv_period_conv_weight_grad, fv_mpd_first_weight_grad; fv_conv1d_weight_grad at the MFD's first-layer shapes;
loss.discriminator_step_terms with stft_grad / period_grad) against the float64 closed forms and the float64 autograd
of tests/mpd_wgrad_reference.py on the same fp32 inputs, and the reference's own gradient
(tests/golden/mpd_mfd_param_grad.npz).

Every bound is relative to the peak of the tensor compared and is 10 x the float32 eager-autograd error of the same
case family against float64 (mpd_wgrad_reference.YARDSTICK, measured on the CPU by tests/test_mpd_wgrad_host.py).
Worst errors measured on MI355X beside their bounds:
    period_conv  4.2e-7 (6.0e-6)      conv_post  1.4e-5 (5.4e-4)      first  1.9e-7 (1.2e-5)      mfd_first  2.4e-7 (2.0e-6)
    p            1.4e-6 (1.3e-5)      stft       2.1e-6 (8.3e-6)      full   7.3e-6 (2.2e-5; the MPD's conv_post.weight_g)"""
import ctypes
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANMultiScaleDiscriminator,
                                           MultiPeriodDiscriminator, MultiResolutionSTFTDiscriminator,
                                           STFTDiscriminator)
from fastvocoder_amd.loss import discriminator_step_terms, discriminator_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict
from tests import mpd_reference as ref
from tests import mpd_wgrad_reference as wref
from tests import msd_wgrad_reference as mw

pytestmark = pytest.mark.gpu

MARGIN = 10.0
MAP_RTOL = 2e-5          # tests/test_gpu_mpd_grad.py: the device's maps against float64, the condition of adopted sides
UNIT = _native.PERIOD_WGRAD_UNIT          # flat positions per unit of the matrix-core kernel
CHUNK = _native.PERIOD_WGRAD_CHUNK        # ... of the plain path and of the first layer's kernel


def _bound(family):
    return MARGIN * wref.YARDSTICK[family]


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


def kernel_heights(p, k, stride):
    """Input heights H of one kernel case: 1..5 (every H % 3, rows with missing taps, H' = 1) and the two whose
    H' p flat outputs end one row short of and one row past a unit boundary of the kernel that serves the layer."""
    unit = UNIT if k == 5 else CHUNK
    rows = unit // p                                   # H' = rows: the last row ends at or before the boundary
    return [1, 2, 3, 4, 5] + [stride * (h - 1) + 1 + (h % stride if stride > 1 else 0) for h in (rows, rows + 1)]


# ---- fv_period_conv_weight_grad ----
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", ref.PERIODS)
@pytest.mark.parametrize("cin,cout,k,stride", wref.KERNEL_LAYERS)
def test_period_conv_weight_grad_against_float64(cin, cout, k, stride, p, B):
    unit, family = (UNIT, "period_conv") if k == 5 else (CHUNK, "conv_post")
    heights = kernel_heights(p, k, stride)
    hs = [(H - 1) // stride + 1 for H in heights[-2:]]
    assert hs[0] * p <= unit < (hs[0] + 1) * p and hs[1] == hs[0] + 1      # short of and past the boundary
    worst = 0.0
    for H in heights:
        g, x = wref.kernel_inputs(cin, cout, k, stride, p, H, B)
        want_dw, want_db = wref.period_conv_weight_grad(g, x, k, stride)
        dw, db = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, True, True)
        assert dw.shape == (cout, cin, k) and db.shape == (cout,)
        err, berr = _rel(dw, want_dw), _rel(db, want_db)
        worst = max(worst, err, berr)
        print(f"period conv weight grad {(cin, cout, k, stride)} p={p} H={H} B={B}: dw {err:.2e} db {berr:.2e}")
        assert err <= _bound(family) and berr <= _bound(family), (H, err, berr)
        if H == 1 and k == 5:                                    # one row: only the centre tap meets it
            assert not dw[:, :, [0, 1, 3, 4]].any() and dw[:, :, 2].any()
        # without db, db alone, a second call and a call on a workspace full of NaN: equal bits
        only_dw = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, True, False)
        only_db = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, False, True)
        assert only_dw[1] is None and torch.equal(only_dw[0], dw)
        assert only_db[0] is None and torch.equal(only_db[1], db)
        n = _native.period_conv_weight_grad_workspace_floats(B, cin, cout, H, p, k, stride)
        nan = torch.full((n,), float("nan"), dtype=torch.float32, device=_dev())
        dw2, db2 = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, True, True)
        dw3, db3 = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, True, True, workspace=nan)
        assert torch.equal(dw, dw2) and torch.equal(dw, dw3) and torch.equal(db, db2) and torch.equal(db, db3)
    print(f"period conv weight grad {(cin, cout, k, stride)} p={p} B={B}: worst {worst:.2e} "
          f"(bound {_bound(family):.2e})")


def test_period_conv_weight_grad_over_many_units_and_splits():
    """More units than splits and more than one block along every grid axis: (128, 512) at a height of many units."""
    cin, cout, k, stride, p, H, B = 128, 512, 5, 3, 3, 400, 2
    g, x = wref.kernel_inputs(cin, cout, k, stride, p, H, B)
    want_dw, want_db = wref.period_conv_weight_grad(g, x, k, stride)
    dw, db = _native.period_conv_weight_grad(_t(g), _t(x), k, stride, True, True)
    err, berr = _rel(dw, want_dw), _rel(db, want_db)
    print(f"period conv weight grad, many units: dw {err:.2e} db {berr:.2e}")
    assert err <= _bound("period_conv") and berr <= _bound("period_conv")


def test_period_conv_weight_grad_workspace_and_error_codes():
    L = _native.lib()
    z = _t(np.zeros(1 << 16))
    p = z.data_ptr()
    B, cin, cout, H, period, k, stride = 1, 32, 128, 4, 2, 5, 3
    need = L.fv_period_conv_weight_grad_workspace_bytes(B, cin, cout, H, period, k, stride)
    assert need > 0 and need % 4 == 0
    ws = torch.empty(need // 4, dtype=torch.float32, device=_dev())
    dw = torch.empty(cout * cin * k, dtype=torch.float32, device=_dev())

    def call(g=p, x=p + 4096, out=None, db=None, size=need, wsp=None, **kw):
        a = dict(B=B, cin=cin, cout=cout, H=H, period=period, k=k, stride=stride)
        a.update(kw)
        return L.fv_period_conv_weight_grad(g, x, dw.data_ptr() if out is None else out, db, a["B"], a["cin"], a["cout"],
                                            a["H"], a["period"], a["k"], a["stride"],
                                            ws.data_ptr() if wsp is None else wsp, ctypes.c_size_t(size), None)
    assert call() == 0
    assert call(size=need - 1) == _native.ERR_INVALID_ARG                   # one byte less
    assert call(wsp=ws.data_ptr() + 1, size=need) == _native.ERR_INVALID_ARG   # misaligned
    assert call(period=4) == _native.ERR_UNSUPPORTED
    assert call(k=7) == _native.ERR_UNSUPPORTED
    assert call(k=4) == _native.ERR_UNSUPPORTED
    assert call(stride=0) == _native.ERR_UNSUPPORTED
    assert call(period=4, g=None) == _native.ERR_UNSUPPORTED                # UNSUPPORTED comes first
    assert call(g=None) == _native.ERR_INVALID_ARG
    assert call(x=None) == _native.ERR_INVALID_ARG
    assert call(out=p) == _native.ERR_INVALID_ARG                           # dw aliases g_pre
    assert call(out=p + 4096) == _native.ERR_INVALID_ARG                    # dw aliases x
    assert call(db=p) == _native.ERR_INVALID_ARG                            # db aliases g_pre
    assert L.fv_period_conv_weight_grad(p, p + 4096, None, None, B, cin, cout, H, period, k, stride, ws.data_ptr(),
                                        ctypes.c_size_t(need), None) == _native.ERR_INVALID_ARG   # nothing asked for
    assert call(B=0) == _native.ERR_INVALID_ARG
    assert call(H=0) == _native.ERR_INVALID_ARG
    assert L.fv_period_conv_weight_grad_workspace_bytes(B, cin, cout, H, 4, k, stride) == _native.ERR_UNSUPPORTED
    assert L.fv_period_conv_weight_grad_workspace_bytes(0, cin, cout, H, period, k, stride) == _native.ERR_INVALID_ARG
    need1 = L.fv_mpd_first_weight_grad_workspace_bytes(1, 100, 3)
    assert need1 > 0
    first = lambda g=p, size=need1, T=100, per=3: L.fv_mpd_first_weight_grad(  # noqa: E731
        g, p + 4096, dw.data_ptr(), None, 1, T, per, ws.data_ptr(), ctypes.c_size_t(size), None)
    assert need1 <= need and first() == 0
    assert first(size=need1 - 1) == _native.ERR_INVALID_ARG
    assert first(g=None) == _native.ERR_INVALID_ARG
    assert first(per=4) == _native.ERR_UNSUPPORTED
    assert first(T=1, per=3) == _native.ERR_INVALID_ARG                     # the reflect tail is not shorter than T
    assert L.fv_mpd_first_weight_grad_workspace_bytes(1, 1, 3) == _native.ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---- fv_mpd_first_weight_grad ----
def first_lengths(p):
    """T around multiples of p (tail 0, 1 and p - 1), the shortest legal T, and one T of several units."""
    shortest = next(T for T in range(1, 4 * p) if ref.reflect_tail(T, p) < T)
    return sorted({shortest, 6 * p, 6 * p - 1, 6 * p + 1, 3 * (CHUNK // p) * p + 2 * p + 1})


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", ref.PERIODS)
def test_mpd_first_weight_grad_against_float64(p, B):
    tails = set()
    for T in first_lengths(p):
        tails.add(ref.reflect_tail(T, p))
        g, x = wref.first_inputs(p, T, B)
        want_dw, want_db = wref.first_weight_grad(g, x, p)
        dw, db = _native.mpd_first_weight_grad(_t(g), _t(x), True, True)
        err, berr = _rel(dw, want_dw), _rel(db, want_db)
        print(f"mpd first weight grad p={p} T={T} B={B}: dw {err:.2e} db {berr:.2e}")
        assert err <= _bound("first") and berr <= _bound("first"), (T, err, berr)
        only_dw = _native.mpd_first_weight_grad(_t(g), _t(x), True, False)
        only_db = _native.mpd_first_weight_grad(_t(g), _t(x), False, True)
        assert only_dw[1] is None and torch.equal(only_dw[0], dw) and torch.equal(only_db[1], db)
        nan = torch.full((1 << 14,), float("nan"), dtype=torch.float32, device=_dev())
        dw3, db3 = _native.mpd_first_weight_grad(_t(g), _t(x), True, True, workspace=nan)
        assert torch.equal(dw, dw3) and torch.equal(db, db3)
    assert {0, 1, p - 1} <= tails


# ---- fv_conv1d_weight_grad at the MFD's first-layer shapes ----
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frames", [8, 33])
@pytest.mark.parametrize("cin", [257, 1025])
def test_dense_weight_grad_at_the_mfd_first_layer_shapes(cin, frames, B):
    cout, k, pad = 64, 15, 7
    g, x = wref.mfd_first_inputs(cin, frames, B)
    dw, db = _native.conv1d_weight_grad(_t(g), _t(x), k, pad, _native.PAD_REFLECT, True, True)
    err, berr = _rel(dw, mw.dense_weight_grad(g, x, k, pad, "reflect")), _rel(db, mw.bias_grad(g))
    print(f"dense weight grad at the MFD first layer Cin={cin} frames={frames} B={B}: dw {err:.2e} db {berr:.2e}")
    assert err <= _bound("mfd_first") and berr <= _bound("mfd_first"), (err, berr)
    dw2, db2 = _native.conv1d_weight_grad(_t(g), _t(x), k, pad, _native.PAD_REFLECT, True, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ---- the modules ----
TERM_RTOL = 7e-6         # tests/test_gpu_mpd_grad.py: the terms' values, relative
TINY = [f"p{p}" for p in ref.PERIODS] + ["stft"]
FULL = ["mfd", "mpd", "discriminator", "discriminator_mpd"]
KEYWORDS = {"p": dict(period_grad=True), "stft": dict(stft_grad=True), "mfd": dict(stft_grad=True),
            "mpd": dict(period_grad=True), "discriminator": dict(stft_grad=True),
            "discriminator_mpd": dict(stft_grad=True, period_grad=True)}
DIVISOR = {"p": 1, "stft": 1, "mfd": 3, "mpd": 5, "discriminator": 6, "discriminator_mpd": 11}


def _family(name):
    return "full" if name in FULL else ("stft" if name == "stft" else "p")


def _build(name):
    kind, kw = wref.case_kind(name)
    module = {"p": lambda: DiscriminatorP(kw["period"]), "stft": lambda: STFTDiscriminator(**wref.SMALL_STFT),
              "mfd": MultiResolutionSTFTDiscriminator, "mpd": MultiPeriodDiscriminator, "discriminator": Discriminator,
              "discriminator_mpd": lambda: Discriminator(use_mpd=True)}[kind]()
    sd = wref.case_state_dict(name)
    return _load(module, sd), sd, kind, kw


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mpd_mfd_param_grad.npz"))


def _step(module, kind, est, real, zero=True):
    if zero:
        module.zero_grad(set_to_none=True)
    terms = discriminator_step_terms(module, _t(est), _t(real), **KEYWORDS[kind])
    terms["discriminator"].backward()
    return terms


def _grads(module):
    return {k: None if q.grad is None else q.grad.clone() for k, q in module.named_parameters()}


def _lists(module, out):
    from fastvocoder_amd.loss.discriminator_loss import _as_lists
    return _as_lists(module, out)


def _np_lists(lists):
    return [[m.detach().cpu().numpy() for m in lst] for lst in lists]


@pytest.mark.parametrize("name", TINY + FULL)
def test_parameter_gradient_matches_the_oracle_and_the_golden(golden, name):
    module, sd, kind, kw = _build(name)
    est, real = wref.case_signals(name)
    bound = _bound(_family(name))
    with torch.no_grad():
        plain_est, plain_real = _lists(module, module(_t(est))), _lists(module, module(_t(real)))
        plain_terms = discriminator_terms(plain_est, plain_real)
        quiet = discriminator_step_terms(module, _t(est), _t(real), **KEYWORDS[kind])
    assert len(plain_est) == DIVISOR[kind]
    terms = _step(module, kind, est, real)
    grads = _grads(module)
    params = sorted(k for k in sd if wref.is_param(k))
    assert sorted(grads) == params and all(v is not None for v in grads.values())
    # the same launches: the maps and the three terms hold the bits of the plain path
    for x, plain in ((est, plain_est), (real, plain_real)):
        for la, lb in zip(_lists(module, module._param_forward(_t(x))), plain):
            assert len(la) == len(lb) and all(a.requires_grad and torch.equal(a, b) for a, b in zip(la, lb))
    for k in ("real", "fake", "discriminator"):
        assert terms[k].dtype == torch.float32 and terms[k].dim() == 0 and terms[k].requires_grad
        assert torch.equal(terms[k], plain_terms[k]) and torch.equal(quiet[k], plain_terms[k])
        assert not quiet[k].requires_grad
    # the oracle: its own float64 decisions for the tiny seeds; for the longer cases the device's leaky-ReLU sides,
    # every differing decision on a float64 value below the forward's error bound
    want, wterms, own_est, own_real = wref.param_grad(kind, est, real, sd, **kw)
    if name in FULL:
        e_maps, r_maps = _np_lists(plain_est), _np_lists(plain_real)
        slopes = wref.slopes_of(kind)
        differ = [wref.differing_sides(own, dev, slopes) for own, dev in ((own_est, e_maps), (own_real, r_maps))]
        print(f"{name}: decisions that differ from float64's own (count, largest |value| / peak): {differ}")
        assert all(d[1] <= MAP_RTOL for d in differ), differ
        plain_err = wref.worst_error({k: v.cpu().numpy() for k, v in grads.items()}, want)
        want, wterms, _, _ = wref.param_grad(kind, est, real, sd, est_maps=e_maps, real_maps=r_maps, **kw)
        print(f"{name}: against the plain oracle {plain_err[1]:.2e} ({plain_err[0]})")
    got = {k: v.cpu().double().numpy() for k, v in grads.items()}
    for k in params:
        assert got[k].shape == want[k].shape, k
    k1, err = wref.worst_error(got, want)
    print(f"{name}: oracle {err:.2e} ({k1}), bound {bound:.2e}")
    assert err <= bound, (k1, err)
    for k in ("real", "fake", "discriminator"):
        assert abs(float(terms[k]) - wterms[k]) <= TERM_RTOL * abs(wterms[k]), (k, float(terms[k]), wterms[k])
    if f"{name}_seed" in golden.files:
        gerr, nerr = 0.0, 0.0
        for k in params:
            smp, norm = wref.sample(got[k])
            gw = golden[f"{name}_grad/{k}"]
            gerr = max(gerr, float(np.abs(smp - gw).max() / max(np.abs(want[k]).max(), 1e-30)))
            nerr = max(nerr, abs(norm - float(golden[f"{name}_norm/{k}"])) / float(golden[f"{name}_norm/{k}"]))
        print(f"{name}: golden samples {gerr:.2e} norms {nerr:.2e}")
        assert gerr <= bound and nerr <= bound, (gerr, nerr)


@pytest.mark.parametrize("name", ["p3", "stft"])
def test_two_backward_passes_accumulate_and_identical_calls_give_identical_bits(name):
    module, sd, kind, kw = _build(name)
    est, real = wref.case_signals(name)
    _step(module, kind, est, real)
    grads = _grads(module)
    _step(module, kind, est, real)
    again = _grads(module)
    assert all(torch.equal(again[k], grads[k]) for k in grads)
    _step(module, kind, est, real, zero=False)
    assert all(torch.equal(q.grad, 2 * grads[k]) for k, q in module.named_parameters())


def test_a_frozen_layer_gets_none_and_the_walk_stops_at_the_lowest_flagged_layer(monkeypatch):
    module, sd, kind, kw = _build("p5")
    est, real = wref.case_signals("p5")
    _step(module, kind, est, real)
    full = _grads(module)
    named = dict(module.named_parameters())
    frozen = ["convs.0.weight_g", "convs.0.weight_v", "convs.0.bias", "convs.1.weight_g", "convs.1.weight_v",
              "convs.1.bias",                                    # the two lowest layers: the walk ends above them
              "convs.3.weight_v", "convs.4.bias", "conv_post.weight_g"]
    for k in frozen:
        named[k].requires_grad_(False)
    calls = {"first": 0, "period": [], "data": 0}
    first, period, data = _native.mpd_first_weight_grad, _native.period_conv_weight_grad, _native.period_conv_input_grad
    monkeypatch.setattr(_native, "mpd_first_weight_grad",
                        lambda *a, **k: calls.__setitem__("first", calls["first"] + 1) or first(*a, **k))
    monkeypatch.setattr(_native, "period_conv_weight_grad",
                        lambda g, x, *a, **k: calls["period"].append(x.shape[1]) or period(g, x, *a, **k))
    monkeypatch.setattr(_native, "period_conv_input_grad",
                        lambda *a, **k: calls.__setitem__("data", calls["data"] + 1) or data(*a, **k))
    _step(module, kind, est, real)
    for k, q in named.items():
        if k in frozen:
            assert q.grad is None, k
        else:
            assert torch.equal(q.grad, full[k]), k
    # two signals: conv_post, convs.4, convs.3, convs.2 each once per signal; nothing below layer 2, and one data
    # gradient of a strided layer (layer 3's, for layer 2) per signal
    assert calls["first"] == 0 and sorted(calls["period"]) == [128, 128, 512, 512, 1024, 1024, 1024, 1024]
    assert calls["data"] == 2
    for q in named.values():                                     # everything frozen: the values, no graph
        q.requires_grad_(False)
    terms = discriminator_step_terms(module, _t(est), _t(real), period_grad=True)
    assert not terms["discriminator"].requires_grad
    with pytest.raises(RuntimeError, match="requires grad"):      # an input that requires grad stays refused
        discriminator_step_terms(module, _t(est), _t(real).requires_grad_(True), period_grad=True)


@pytest.mark.parametrize("name", ["p2", "stft"])
def test_a_module_without_weight_norm(name):
    module, sd, kind, kw = _build(name)
    est, real = wref.case_signals(name)
    module.remove_weight_norm()
    plain_sd = {k: v.detach().cpu().numpy() for k, v in module.state_dict().items()}
    assert all(not k.endswith(("weight_g", "weight_v")) for k in plain_sd)
    _step(module, kind, est, real)
    got = {k: v.cpu().double().numpy() for k, v in _grads(module).items()}
    k, err = wref.worst_error(got, wref.param_grad(kind, est, real, plain_sd, **kw)[0])
    print(f"{name} without weight norm: {err:.2e} ({k})")
    assert err <= _bound(_family(name)), (k, err)


def test_three_sgd_steps_follow_float64_and_the_caches_follow_the_optimizer():
    module, sd, kind, kw = _build("discriminator")
    est, real = wref.case_signals("discriminator")
    lr = 2e-6                                                    # |grad|^2 is about 1e5: the loss falls by 2 % a step
    want_losses, _ = wref.sgd_steps(kind, est, real, sd, 3, lr)
    opt = torch.optim.SGD(module.parameters(), lr=lr)
    losses = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        losses.append(float(_step(module, kind, est, real, zero=False)["discriminator"].detach()))
        if step < 2:
            opt.step()
    errs = [abs(a - b) / abs(b) for a, b in zip(losses, want_losses)]
    print(f"three SGD steps on Discriminator(): losses {losses} against {want_losses}: {max(errs):.2e}")
    assert want_losses[2] < want_losses[0] and max(errs) <= TERM_RTOL, errs
    fresh = Discriminator()
    fresh.load_state_dict(module.state_dict())
    fresh = fresh.to(_dev()).eval()
    _step(fresh, kind, est, real)
    third, again = _grads(module), _grads(fresh)
    assert all(torch.equal(third[k], again[k]) for k in third)


def test_the_keywords_change_nothing_for_the_msd():
    sd = seeded_discriminator_state_dict("msd", 13)
    msd = _load(MelGANMultiScaleDiscriminator(), sd)
    est, real = wref.signals(3, msd.min_length() + 200)
    results = []
    for kw in ({}, dict(stft_grad=True, period_grad=True)):
        msd.zero_grad(set_to_none=True)
        terms = discriminator_step_terms(msd, _t(est), _t(real), **kw)
        terms["discriminator"].backward()
        results.append((terms, _grads(msd)))
    (t0, g0), (t1, g1) = results
    assert all(torch.equal(t0[k], t1[k]) for k in t0) and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_a_module_is_refused_without_its_keyword():
    module, sd, kind, kw = _build("stft")
    est, real = wref.case_signals("stft")
    with pytest.raises(NotImplementedError, match="stft_grad=True"):
        discriminator_step_terms(module, _t(est), _t(real))
    with pytest.raises(NotImplementedError, match="stft_grad=True"):
        discriminator_step_terms(module, _t(est), _t(real), period_grad=True)
    with pytest.raises(NotImplementedError, match="MelGANMultiScaleDiscriminator"):
        module.parameter_grad = True
