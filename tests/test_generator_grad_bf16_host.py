"""CPU tests behind tests/test_gpu_generator_grad_bf16.py: ``bf16_round`` of tests/generator_grad_bf16_reference.py
meets torch's bfloat16 conversion (ties of both parities, negatives, binade carries, representable values), the patched
chain oracle without its rounding is the exact gradient, the recorded yardstick and routing floor of every chain case
are recomputed, and the Python surface behaves with the native call stubbed: ``precision`` reaches ``_weight_grad_call``
from both backward walks, bad values raise, ``--grad_precision`` is absent unless given and ``--mixprecision 1`` still
exits."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native, optim
from fastvocoder_amd.bin import train as train_cli
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import Discriminator
from fastvocoder_amd.generator import MelGANGenerator
from fastvocoder_amd.generator import grad as hifi_walk
from fastvocoder_amd.generator import stack_grad as stack_walk
from fastvocoder_amd.generator.engine import conv_params
from fastvocoder_amd.train import Trainer
from tests import cases
from tests import generator_grad_bf16_reference as bref
from tests import generator_grad_reference as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_conv1d_weight_grad_dilated_bf16", "fv_conv1d_weight_grad_dilated_bf16_workspace_bytes",
           "fv_conv_transpose1d_weight_grad_bf16", "fv_conv_transpose1d_weight_grad_bf16_workspace_bytes")
TRAINER_KW = dict(lambda_stft=1.0, use_feature_map_loss=True, discriminator_train_start_steps=10, grad_clip_thresh=1.0)


def _torch_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


# ---- bf16_round ----
def test_bf16_round_meets_torch_on_random_normals():
    rs = np.random.RandomState(0)
    a = (rs.randn(100000) * np.exp(rs.uniform(-30.0, 30.0, 100000))).astype(np.float32)
    assert np.array_equal(bref.bf16_round(a), _torch_round(a))
    assert np.array_equal(bref.bf16_round(-a), -bref.bf16_round(a))


def test_bf16_round_ties_carries_and_representable_values():
    even_tie, odd_tie = _f32([0x3f808000, 0xbf808000]), _f32([0x3f818000, 0xbf818000])
    assert np.array_equal(bref.bf16_round(even_tie).view(np.uint32), [0x3f800000, 0xbf800000])   # kept bit 0: down
    assert np.array_equal(bref.bf16_round(odd_tie).view(np.uint32), [0x3f820000, 0xbf820000])    # kept bit 1: up
    just = _f32([0x3f808001, 0x3f807fff, 0xbf808001, 0xbf807fff])                                 # either side of a tie
    assert np.array_equal(bref.bf16_round(just).view(np.uint32), [0x3f810000, 0x3f800000, 0xbf810000, 0xbf800000])
    carry = _f32([0x3fffc000, 0x3fff8000, 0xbfffffff, 0x007f8000])           # up into the next binade / out of the subnormals
    assert np.array_equal(bref.bf16_round(carry).view(np.uint32), [0x40000000, 0x40000000, 0xc0000000, 0x00800000])
    same = _f32([0x3f810000, 0xc2ff0000, 0x00000000, 0x80000000, 0x00010000, 0x7f7f0000, 0x7f800000])
    assert np.array_equal(bref.bf16_round(same).view(np.uint32), same.view(np.uint32))
    every = np.concatenate([even_tie, odd_tie, just, carry, same])
    assert np.array_equal(bref.bf16_round(every).view(np.uint32), _torch_round(every).view(np.uint32))


def test_the_tie_inputs_are_ties_of_both_parities():
    t = bref.ties((3, 5, 7), 1).reshape(-1).view(np.uint32)
    assert np.all(t & 0xffff == 0x8000) and np.all((t >> 16) & 1 == np.arange(t.size) % 2)
    r = bref.bf16_round(t.view(np.float32)).view(np.uint32)
    up = (t >> 16) & 1 == 1
    assert np.array_equal(r[up], (t[up] + 0x8000) & 0xffff0000) and np.array_equal(r[~up], t[~up] & 0xffff0000)
    # half up and truncation each get half of them wrong
    assert np.mean(r != ((t + 0x8000) & 0xffff0000)) == pytest.approx(0.5, abs=0.02)
    assert np.mean(r != (t & 0xffff0000)) == pytest.approx(0.5, abs=0.02)


def test_the_closed_forms_round_their_operands():
    g, x = gref.kernel_inputs((2, 5, 20), (2, 6, 20), 3)
    want = gref.dilated_weight_grad(_torch_round(g), _torch_round(x), 3, 2, 2)
    assert np.array_equal(bref.dilated_weight_grad(g, x, 3, 2, 2), want)
    assert gref.rel_err(want, gref.dilated_weight_grad(g, x, 3, 2, 2)) > 1e-4


# ---- the chain oracle ----
@pytest.mark.parametrize("tag", ["hifigan_s", "melgan_s"])
def test_the_patched_oracle_without_rounding_is_the_exact_gradient(tag):
    name, cfg, sd, mel, c = bref.chain_case(tag)
    out, exact = bref.param_grad_exact(name, cfg, sd, mel, c)
    out2, plain = bref.param_grad_bf16(name, cfg, sd, mel, c, rounding=False)
    assert np.array_equal(out, out2) and sorted(exact) == sorted(plain)
    worst = max(gref.rel_err(plain[k], exact[k]) for k in exact)
    print(f"{tag}: patched oracle without rounding against autograd {worst:.2e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("tag", sorted(bref.CHAIN_FIGURES))
def test_the_recorded_yardstick_and_routing_floor(tag):
    yard, floor, far, bias = bref.chain_figures(tag)
    rec_yard, rec_floor = bref.CHAIN_FIGURES[tag]
    print(f"{tag}: yardstick (a) {yard:.3e} (recorded {rec_yard:.2e}), routing floor (b) {floor:.3e} "
          f"(recorded {rec_floor:.2e}), largest distance {far:.3e}, bias gradients {bias:.1e}")
    assert bias == 0.0                                            # the mode leaves the bias gradients exact
    assert abs(floor - rec_floor) <= bref.FLOOR_RTOL * rec_floor, (floor, rec_floor)
    assert rec_yard / bref.YARDSTICK_BAND <= yard <= rec_yard * bref.YARDSTICK_BAND, (yard, rec_yard)
    assert floor > 2 * yard and far >= floor                     # routing shows far above the evaluation noise


# ---- the Python surface, the native call stubbed ----
class _Reached(Exception):
    pass


@pytest.fixture
def calls(monkeypatch):
    """``_weight_grad_call`` replaced by a recorder that ends the walk: [(entry, args)]."""
    seen = []

    def record(name, entry, inputs, want_dw, want_db, dw_shape, db_shape, args, workspace, floats):
        seen.append((entry, tuple(args)))
        raise _Reached(entry)
    monkeypatch.setattr(_native, "_weight_grad_call", record)
    return seen


def _needs(gen, convs):
    params = [p for c in convs for p in conv_params(c)]
    return params, [True] * len(params)


@pytest.mark.parametrize("precision,entry", [("f32", "fv_conv1d_weight_grad_dilated"),
                                             ("bf16", "fv_conv1d_weight_grad_dilated_bf16")])
def test_precision_reaches_the_call_from_the_hifigan_walk(monkeypatch, calls, precision, entry):
    gen = build_generator("hifigan", gref.GOLDEN_CFG)
    assert gen.grad_precision == "f32"
    gen.grad_precision = precision
    monkeypatch.setattr(hifi_walk, "_layers", lambda g: {})
    monkeypatch.setattr(_native, "tanh_grad", lambda g, y: g)
    params, need = _needs(gen, hifi_walk.train_convs(gen))
    g = torch.zeros(2, 1, 24)
    tape = {"post_in": torch.zeros(2, gen.conv_post.in_channels, 24)}
    with pytest.raises(_Reached):
        hifi_walk.train_backward(gen, tape, g, params, need, g)
    assert calls == [(entry, (2, gen.conv_post.in_channels, 1, 24, 7, 1, 3) + ((_native.PAD_ZERO,) if precision == "bf16" else ()))]


@pytest.mark.parametrize("precision,entry", [("f32", "fv_conv1d_weight_grad_dilated_mode"),
                                             ("bf16", "fv_conv1d_weight_grad_dilated_bf16")])
def test_precision_reaches_the_call_from_the_melgan_walk(monkeypatch, calls, precision, entry):
    gen = MelGANGenerator(**next(c for t, _, c in cases.SMALL if t == "melgan_s"))
    gen.stack_grad = True
    gen.grad_precision = precision
    monkeypatch.setattr(stack_walk, "_layers", lambda g: {})
    monkeypatch.setattr(_native, "tanh_grad", lambda g, y: g)
    params, need = _needs(gen, stack_walk.train_convs(gen))
    last = stack_walk._graph(gen)[2]
    cin, k = last.conv.in_channels, last.conv.kernel_size[0]
    g = torch.zeros(2, last.conv.out_channels, 30)
    tape = {"stages": [{"ya": torch.zeros(2, cin, 30)}]}
    with pytest.raises(_Reached):
        stack_walk.train_backward(gen, tape, g, params, need, g)
    assert calls == [(entry, (2, cin, last.conv.out_channels, 30, k, 1, last._pad, _native.PAD_REFLECT))]


def test_precision_reaches_the_transposed_entry(calls):
    g, xa = torch.zeros(2, 4, 16), torch.zeros(2, 8, 4)
    for precision, entry in (("f32", "fv_conv_transpose1d_weight_grad"), ("bf16", "fv_conv_transpose1d_weight_grad_bf16")):
        with pytest.raises(_Reached):
            _native.conv_transpose1d_weight_grad(g, xa, 8, 4, 2, precision=precision)
        assert calls[-1] == (entry, (2, 8, 4, 4, 8, 4, 2, 0))


def test_bad_values_raise():
    g, xa = torch.zeros(2, 4, 16), torch.zeros(2, 4, 16)
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
            _native.conv1d_weight_grad_dilated(g, xa, 3, 1, 1, precision=bad)
        with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
            _native.conv_transpose1d_weight_grad(g, xa, 3, 1, 1, precision=bad)
        with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
            _native.conv1d_weight_grad_dilated_workspace_floats(2, 4, 4, 16, 3, 1, 1, precision=bad)
        with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
            _native.conv_transpose1d_weight_grad_workspace_floats(2, 4, 4, 16, 3, 1, 1, precision=bad)
    for tag in ("hifigan_s", "mb_s", "melgan_s", "basis_s"):
        gen = build_generator(*next((n, c) for t, n, c in cases.SMALL if t == tag))
        assert gen.grad_precision == "f32" and gen.precision == "split"          # two attributes, two policies
        for bad in ("fp16", "split", True, None):
            with pytest.raises(ValueError, match="'f32' or 'bf16'"):
                gen.grad_precision = bad
        assert gen.grad_precision == "f32"
        gen.grad_precision = "bf16"
        assert gen.grad_precision == "bf16" and gen.parameter_grad is False      # nothing else moves
        gen.grad_precision = "f32"


def test_the_trainer_takes_the_precision_as_its_last_keyword():
    import inspect
    assert list(inspect.signature(Trainer.__init__).parameters)[-1] == "grad_precision"
    assert inspect.signature(Trainer.__init__).parameters["grad_precision"].default == "f32"
    d = Discriminator()
    d_opt = optim.Adam(d.parameters(), lr=5e-5)
    gen = build_generator("hifigan", gref.GOLDEN_CFG)
    Trainer(gen, d, optim.Adam(gen.parameters()), d_opt, **TRAINER_KW)
    assert gen.grad_precision == "f32" and gen.parameter_grad is True
    Trainer(gen, d, optim.Adam(gen.parameters()), d_opt, grad_precision="bf16", **TRAINER_KW)
    assert gen.grad_precision == "bf16"
    with pytest.raises(ValueError, match="'f32' or 'bf16'"):
        Trainer(gen, d, optim.Adam(gen.parameters()), d_opt, grad_precision="fp16", **TRAINER_KW)
    mel = MelGANGenerator(**next(c for t, _, c in cases.SMALL if t == "melgan_s"))
    Trainer(mel, d, optim.Adam(mel.parameters()), d_opt, stack_grad=True, grad_precision="bf16", **TRAINER_KW)
    assert mel.grad_precision == "bf16"


def test_the_command_line_flag():
    parser = train_cli.build_parser()
    assert "grad_precision" not in vars(parser.parse_args([]))               # absent unless given
    assert parser.parse_args(["--grad_precision", "bf16"]).grad_precision == "bf16"
    base = ["--model_name", "hifigan", "--config", "c.yaml"]
    for value in ("bf16", "f32"):
        assert train_cli.check_args(parser.parse_args(base + ["--grad_precision", value])).grad_precision == value
    with pytest.raises(SystemExit) as e:
        train_cli.check_args(parser.parse_args(base + ["--grad_precision", "fp16"]))
    assert str(e.value).startswith("MODE=train: ") and "--grad_precision" in str(e.value)
    for extra in ([], ["--grad_precision", "bf16"]):                         # --mixprecision 1 keeps exiting
        with pytest.raises(SystemExit) as e:
            train_cli.run_train(base + ["--mixprecision", "1"] + extra)
        message = str(e.value)
        assert message.startswith("MODE=train: ") and "\n" not in message
        assert all(w in message for w in ("mixprecision", "mixed-precision", "--grad_precision bf16")), message


# ---- the entries ----
def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert "gen_grad_bf16.hip" in _native.SOURCES and "gen_grad_host.hpp" in _native.HEADERS


def test_the_entries_refuse_what_the_fp32_entries_refuse():
    Z, R = _native.PAD_ZERO, _native.PAD_REFLECT
    floats = _native.conv1d_weight_grad_dilated_workspace_floats
    tfloats = _native.conv_transpose1d_weight_grad_workspace_floats
    assert floats(2, 16, 16, 40, 3, 9, 9, R, "bf16") == floats(2, 16, 16, 40, 3, 9, 9, precision="bf16") > 0
    assert tfloats(2, 32, 16, 13, 4, 2, 1, 0, "bf16") > 0
    # the split count is a function of the shape alone, in units of 64 steps: 4099 steps are 65 units
    assert floats(1, 16, 16, 4099, 3, 1, 1, precision="bf16") == 65 * (16 * 48 + 16)
    L = _native.lib()
    tail = (None, 0, None)
    for args in ((2, 16, 16, 9, 3, 9, 9, R), (2, 16, 16, 3, 7, 1, 3, R), (2, 16, 16, 40, 3, 9, 9, 2),
                 (0, 16, 16, 40, 3, 9, 9, R), (2, 16, 16, 40, 3, 0, 9, R), (2, 0, 16, 40, 3, 9, 9, Z),
                 (2, 16, 16, 40, 3, 9, 9, R)):                                # the last: null tensors
        want = L.fv_conv1d_weight_grad_dilated_mode(None, None, None, None, *args, *tail)
        assert want < 0 and L.fv_conv1d_weight_grad_dilated_bf16(None, None, None, None, *args, *tail) == want, args
        if args[-1] in (Z, R) and args != (2, 16, 16, 40, 3, 9, 9, R):
            assert L.fv_conv1d_weight_grad_dilated_bf16_workspace_bytes(*args) == want, args
    for args in ((2, 32, 16, 13, 4, 0, 1, 0), (0, 32, 16, 13, 4, 2, 1, 0), (2, 32, 16, 1, 2, 2, 3, 0),
                 (2, 32, 16, 13, 4, 2, 1, 0)):
        want = L.fv_conv_transpose1d_weight_grad(None, None, None, None, *args, *tail)
        assert want < 0 and L.fv_conv_transpose1d_weight_grad_bf16(None, None, None, None, *args, *tail) == want, args
