"""CPU tests of the oracle behind tests/test_gpu_generator_grad.py (tests/generator_grad_reference.py): its closed forms
meet float64 torch autograd, its restatement of the forward meets the reference's own parameter gradient
(tests/golden/hifigan_param_grad.npz), the golden keeps clear of the leaky-ReLU kinks, the float32 eager-autograd
yardsticks are printed, and the ``parameter_grad`` attribute, the header and the workspace queries behave."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fastvocoder_amd import _native
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.generator import (BasisMelGANGenerator, HiFiGANGenerator, MelGANGenerator,
                                       MultiBandHiFiGANGenerator)
from fastvocoder_amd.synthetic import seeded_state_dict
from tests import cases
from tests import generator_grad_reference as gref

GOLDEN_RTOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_conv1d_weight_grad_dilated", "fv_conv1d_weight_grad_dilated_workspace_bytes",
           "fv_conv_transpose1d_input_grad", "fv_conv_transpose1d_weight_grad",
           "fv_conv_transpose1d_weight_grad_workspace_bytes", "fv_tanh_grad", "fv_residual_merge_grad", "fv_grad_div")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "hifigan_param_grad.npz"))


def _sd():
    return seeded_state_dict("hifigan", gref.GOLDEN_CFG, gref.GOLDEN_WEIGHT_SEED)


def test_the_closed_forms_meet_float64_autograd():
    # the dilated conv: (Cin, Cout, k, dil, pad, Tin)
    for cin, cout, k, dil, pad, T in ((3, 5, 3, 1, 1, 9), (4, 2, 7, 3, 9, 11), (2, 3, 11, 5, 25, 4), (3, 1, 7, 1, 3, 1),
                                      (2, 2, 3, 2, 0, 8)):
        tout = T + 2 * pad - dil * (k - 1)
        g, x = gref.kernel_inputs((2, cout, tout), (2, cin, T), cin + cout + k)
        w = torch.zeros(cout, cin, k, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv1d(torch.from_numpy(x).double(), w, b, padding=pad, dilation=dil)
        (y * torch.from_numpy(g).double()).sum().backward()
        assert gref.rel_err(gref.dilated_weight_grad(g, x, k, dil, pad), w.grad.numpy()) <= 1e-13, (cin, cout, k, dil)
        assert gref.rel_err(gref.bias_grad(g), b.grad.numpy()) <= 1e-13
    # the transposed conv: (Cin, Cout, k, s, p, op, Tin): k % s != 0, k > 2 s, output padding
    for cin, cout, k, s, p, op, T in ((3, 2, 8, 4, 2, 0, 5), (2, 3, 7, 3, 2, 1, 6), (4, 2, 10, 5, 3, 1, 3),
                                      (2, 2, 9, 2, 1, 1, 4), (3, 1, 4, 2, 1, 0, 1), (2, 2, 3, 5, 0, 2, 4)):
        tout = gref.convt_out_len(T, k, s, p, op)
        g, x = gref.kernel_inputs((2, cout, tout), (2, cin, T), cin + cout + k + s)
        rs = np.random.RandomState(k)
        w = torch.from_numpy(rs.randn(cin, cout, k)).requires_grad_(True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        y = F.conv_transpose1d(xt, w, b, stride=s, padding=p, output_padding=op)
        assert y.shape[2] == tout
        (y * torch.from_numpy(g).double()).sum().backward()
        case = (cin, cout, k, s, p, op, T)
        assert gref.rel_err(gref.convt_weight_grad(g, x, k, s, p), w.grad.numpy()) <= 1e-13, case
        assert gref.rel_err(gref.convt_input_grad(g, w.detach().numpy(), T, s, p), xt.grad.numpy()) <= 1e-13, case
        assert gref.rel_err(gref.bias_grad(g), b.grad.numpy()) <= 1e-13, case


def test_the_restatement_meets_the_reference_gradient(golden):
    mel, c = gref.golden_inputs(int(golden["input_seed"]))
    assert np.array_equal(mel, golden["mel"]) and np.array_equal(c, golden["c"])
    assert int(golden["weight_seed"]) == gref.GOLDEN_WEIGHT_SEED
    sd = _sd()
    out, grads = gref.param_grad("hifigan", gref.GOLDEN_CFG, sd, mel, c)
    assert sorted(grads) == sorted(sd)
    assert gref.rel_err(out, golden["out"]) <= GOLDEN_RTOL
    worst = max(gref.rel_err(g, golden[f"grad/{k}"]) for k, g in grads.items())
    print(f"restatement against the reference's gradient: {worst:.2e}")
    assert worst <= GOLDEN_RTOL, worst


def test_the_golden_is_small_and_data_only(golden_dir):
    path = os.path.join(golden_dir, "hifigan_param_grad.npz")
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir)
                                        if f != "hifigan_param_grad.npz")
    with np.load(path, allow_pickle=False) as g:
        assert all(g[k].dtype.kind in "fi" for k in g.files)


def test_the_golden_keeps_clear_of_the_kinks(golden):
    margins = []
    gref.param_grad("hifigan", gref.GOLDEN_CFG, _sd(), golden["mel"], golden["c"], margins=margins)
    nk, n_up = 3, 2
    assert len(margins) == n_up * (1 + nk * 6) + 1               # every leaky ReLU of the forward
    print(f"golden: smallest kink margin {min(margins):.3e} (recorded {float(golden['margin']):.3e})")
    assert abs(min(margins) - float(golden["margin"])) <= 1e-9 * float(golden["margin"])
    assert min(margins) > gref.KINK


def test_float32_eager_autograd_error_of_the_chain_is_printed(golden):
    """The yardstick the GPU tolerances of tests/test_gpu_generator_grad.py are read against."""
    err, key = gref.float32_yardstick("hifigan", gref.GOLDEN_CFG, _sd(), golden["mel"], golden["c"])
    print(f"yardstick golden: float32 eager autograd against float64 {err:.3e} ({key})")
    assert 0.0 < err < 1e-4
    name, cfg, sd, mel, c = gref.chain_case("hifigan_s")
    err, key = gref.float32_yardstick(name, cfg, sd, mel, c)
    print(f"yardstick hifigan_s: float32 eager autograd against float64 {err:.3e} ({key})")
    assert 0.0 < err < 1e-4


@pytest.mark.parametrize("tag", sorted(gref.CHAIN_MEL_SEED))
def test_the_chain_cases_sit_at_their_recorded_kink_margin(tag):
    name, cfg, sd, mel, _ = gref.chain_case(tag)
    margins = []
    with torch.no_grad(), gref.recorded_margins(margins):
        gref.forward(name, cfg, sd, mel)
    want = gref.CHAIN_MEL_SEED[tag][1]
    print(f"{tag}: smallest kink margin {min(margins):.3e} (recorded {want:.2e})")
    assert abs(min(margins) - want) <= 0.01 * want
    a, b = (gref.kink_sides(name, cfg, sd, mel, dt) for dt in (torch.float64, torch.float32))
    assert sum(int((x != y).sum()) for x, y in zip(a, b)) == 0


def test_parameter_grad_defaults_setters_and_refusals():
    small = dict(upsample_rates=[4, 3], upsample_kernel_sizes=[8, 7], upsample_initial_channel=16)
    for gen in (HiFiGANGenerator(**small), MultiBandHiFiGANGenerator(**small)):
        assert gen.parameter_grad is False
        gen.parameter_grad = True
        assert gen.parameter_grad is True
        gen.parameter_grad = False
        assert gen.parameter_grad is False
    up = HiFiGANGenerator(transposedconv=False, **small)
    assert up.parameter_grad is False
    with pytest.raises(NotImplementedError, match="UpsampleLayer"):
        up.parameter_grad = True
    assert up.parameter_grad is False
    up.parameter_grad = False
    for name in ("melgan", "basis-melgan"):
        tag = "melgan_s" if name == "melgan" else "basis_s"
        gen = build_generator(name, next(c for c in cases.SMALL if c[0] == tag)[2])
        assert isinstance(gen, (MelGANGenerator, BasisMelGANGenerator))
        assert gen.parameter_grad is False
        with pytest.raises(NotImplementedError, match="ResidualStack"):
            gen.parameter_grad = True
        gen.parameter_grad = False
        assert gen.parameter_grad is False


def test_a_mel_that_requires_grad_is_refused():
    gen = HiFiGANGenerator(upsample_rates=[4, 3], upsample_kernel_sizes=[8, 7], upsample_initial_channel=16)
    gen.parameter_grad = True
    with pytest.raises(RuntimeError, match="mel requires grad"):
        gen(torch.zeros(1, 80, 4, requires_grad=True))
    with pytest.raises(_native.NativeError, match="ROCm device"):     # a plain mel reaches the device check
        gen(torch.zeros(1, 80, 4))


def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert "gen_grad.hip" in _native.SOURCES
    assert os.path.exists(os.path.join(ROOT, "fastvocoder_amd", "csrc", "gen_grad.hip"))


def test_the_workspace_queries_refuse_what_the_entries_refuse():
    ok = _native.conv1d_weight_grad_dilated_workspace_floats(2, 16, 16, 40, 11, 5, 25)
    assert ok > 0 and ok == _native.conv1d_weight_grad_dilated_workspace_floats(2, 16, 16, 40, 11, 5, 25)
    for bad in ((0, 16, 16, 40, 11, 5, 25), (2, 0, 16, 40, 11, 5, 25), (2, 16, 16, 40, 0, 5, 25),
                (2, 16, 16, 40, 11, 0, 25), (2, 16, 16, 40, 11, 5, -1), (2, 16, 16, 40, 11, 5, 4),
                (70000, 16, 16, 40, 11, 5, 25), (2, 16, 16, 0, 11, 5, 25)):
        with pytest.raises(_native.NativeError):
            _native.conv1d_weight_grad_dilated_workspace_floats(*bad)
    ok = _native.conv_transpose1d_weight_grad_workspace_floats(2, 32, 16, 13, 4, 2, 1, 0)
    assert ok > 0
    for bad in ((0, 32, 16, 13, 4, 2, 1, 0), (2, 0, 16, 13, 4, 2, 1, 0), (2, 32, 16, 13, 0, 2, 1, 0),
                (2, 32, 16, 13, 4, 0, 1, 0), (2, 32, 16, 13, 4, 2, -1, 0), (2, 32, 16, 1, 4, 2, 2, 0),
                (2, 32, 16, 0, 4, 2, 1, 0)):
        with pytest.raises(_native.NativeError):
            _native.conv_transpose1d_weight_grad_workspace_floats(*bad)
    # the entries themselves refuse the same arguments before they touch a pointer
    L = _native.lib()
    assert L.fv_conv1d_weight_grad_dilated(None, None, None, None, 2, 16, 16, 40, 11, 0, 25, None, 0, None) \
        == _native.ERR_UNSUPPORTED
    assert L.fv_conv1d_weight_grad_dilated(None, None, None, None, 2, 16, 16, 40, 11, 5, 4, None, 0, None) \
        == _native.ERR_INVALID_ARG
    assert L.fv_conv_transpose1d_weight_grad(None, None, None, None, 2, 32, 16, 13, 4, 0, 1, 0, None, 0, None) \
        == _native.ERR_UNSUPPORTED
    assert L.fv_conv_transpose1d_input_grad(None, None, None, 2, 32, 16, 1, 4, 2, 2, 0, None) == _native.ERR_INVALID_ARG
    assert L.fv_conv_transpose1d_input_grad(None, None, None, 2, 32, 16, 13, 4, 2, 1, 0, None) == _native.ERR_INVALID_ARG
