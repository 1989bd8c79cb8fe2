"""CPU tests behind tests/test_gpu_mpd_wgrad_bf16.py: the entries exist and refuse what the fp32 entries refuse, the
workspace is a function of the shape in units of 64 flat positions, ``precision`` reaches the right entry, the
attribute, the Trainer keyword and the command-line flag behave, the flat-axis formula of the periodic kernel is the
period conv, every kernel-test shape rounds visibly (the floor the GPU test asserts can be met), the patched chain
oracle without its rounding is the exact gradient to 0.0, and the recorded chain figures are recomputed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native, optim
from fastvocoder_amd.bin import train as train_cli
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import Discriminator, DiscriminatorP, MultiPeriodDiscriminator
from fastvocoder_amd.train import Trainer
from tests import generator_grad_reference as gref
from tests import mpd_wgrad_bf16_reference as pb
from tests import mpd_wgrad_reference as wref
from tests.test_gpu_generator_grad import KERNEL_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_period_conv_weight_grad_bf16", "fv_period_conv_weight_grad_bf16_workspace_bytes")
TRAINER_KW = dict(lambda_stft=1.0, use_feature_map_loss=True, discriminator_train_start_steps=10, grad_clip_thresh=1.0)


# ---- the entries ----
def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert lib.fv_version() == 18
    fp32 = re.search(r"int fv_period_conv_weight_grad\(([^;]*)\);", header).group(1)
    bf16 = re.search(r"int fv_period_conv_weight_grad_bf16\(([^;]*)\);", header).group(1)
    assert " ".join(fp32.split()) == " ".join(bf16.split())        # the argument list of the fp32 entry


def test_the_entries_refuse_what_the_fp32_entries_refuse():
    L = _native.lib()
    good = dict(B=2, cin=32, cout=128, H=10, period=3, k=5, stride=3)
    order = ("B", "cin", "cout", "H", "period", "k", "stride")
    bad = [dict(period=4), dict(period=1), dict(k=7), dict(k=4), dict(k=0), dict(stride=0), dict(stride=4),
           dict(cin=0), dict(cout=0), dict(B=0), dict(B=65536), dict(H=0), dict(H=-3),
           dict(period=4, B=0),                                     # UNSUPPORTED comes first
           dict(stride=1, k=7), dict(stride=1, period=9), dict(stride=1, H=0), dict(stride=1, B=0)]
    for change in bad:
        args = [dict(good, **change)[n] for n in order]
        want = L.fv_period_conv_weight_grad(None, None, None, None, *args, None, 0, None)
        assert want in (_native.ERR_INVALID_ARG, _native.ERR_UNSUPPORTED), (change, want)
        assert L.fv_period_conv_weight_grad_bf16(None, None, None, None, *args, None, 0, None) == want, change
        assert L.fv_period_conv_weight_grad_workspace_bytes(*args) == want, change
        assert L.fv_period_conv_weight_grad_bf16_workspace_bytes(*args) == want, change
    for change in (dict(), dict(stride=1), dict(stride=1, cin=1024, cout=1, k=3)):
        args = [dict(good, **change)[n] for n in order]
        assert L.fv_period_conv_weight_grad_bf16_workspace_bytes(*args) > 0
        # null tensors; then tensors (never dereferenced: the workspace check comes before any launch) without a
        # workspace, and with one that is a byte short: no launch, the fp32 entry's code
        for tensors, ws, size in (((None,) * 4, None, 0), ((4096, 8192, 12288, None), None, 0),
                                  ((4096, 8192, 12288, None), 16384, L.fv_period_conv_weight_grad_bf16_workspace_bytes(*args) - 1),
                                  ((4096, 8192, 4096, None), None, 0), ((4096, 8192, None, None), None, 0)):
            want = L.fv_period_conv_weight_grad(*tensors, *args, ws, min(size, 1), None)
            assert want == _native.ERR_INVALID_ARG
            assert L.fv_period_conv_weight_grad_bf16(*tensors, *args, ws, size, None) == want, (change, tensors)


def test_a_strided_shape_outside_the_gemm_is_unsupported():
    L = _native.lib()
    for cin, cout, k in ((32, 32, 5), (1024, 1, 3), (8, 64, 5), (1, 32, 5)):      # Cout < 64, or Cin k < 64
        for stride in (2, 3):
            assert L.fv_period_conv_weight_grad_workspace_bytes(2, cin, cout, 10, 3, k, stride) > 0
            assert L.fv_period_conv_weight_grad_bf16_workspace_bytes(2, cin, cout, 10, 3, k, stride) == _native.ERR_UNSUPPORTED
            assert L.fv_period_conv_weight_grad_bf16(None, None, None, None, 2, cin, cout, 10, 3, k, stride, None, 0,
                                                     None) == _native.ERR_UNSUPPORTED
        assert L.fv_period_conv_weight_grad_bf16_workspace_bytes(2, cin, cout, 10, 3, k, 1) > 0   # stride 1: any shape
    with pytest.raises(_native.NativeError, match="Cout >= 64"):
        _native.period_conv_weight_grad_workspace_floats(2, 32, 32, 10, 3, 5, 3, "bf16")


def test_the_workspace_is_a_function_of_the_shape_in_units_of_64():
    floats = _native.period_conv_weight_grad_workspace_floats
    rec = 128 * 160 + 128
    # 32 -> 128: 2 column tiles x 1 row tile, up to 256 splits: one split per unit of 64 flat positions
    assert floats(1, 32, 128, pb.rows(64, 3), 2, 5, 3, "bf16") == 2 * rec           # 128 positions
    assert floats(1, 32, 128, pb.rows(65, 3), 2, 5, 3, "bf16") == 3 * rec           # 130
    assert floats(3, 32, 128, pb.rows(65, 3), 2, 5, 3, "bf16") == 9 * rec
    assert floats(1, 32, 128, pb.rows(65, 3), 2, 5, 3) == 5 * rec                   # the fp32 entry: units of 32
    assert floats(1, 32, 128, pb.rows(13, 3), 5, 5, 3, "bf16") == 2 * rec           # 65
    assert floats(64, 32, 128, pb.rows(13, 3), 11, 5, 3, "bf16") == 192 * rec       # 143 a row: 3 units
    assert floats(128, 32, 128, pb.rows(13, 3), 11, 5, 3, "bf16") == 256 * rec      # 384 units, 256 splits at most
    for shape in pb.SPLIT_SHAPES:                                                   # 160 tiles: 4 splits whatever B
        cin, cout, k, s, p, H, B = shape
        assert floats(B, cin, cout, H, p, k, s, "bf16") == 4 * (cout * cin * k + cout)
    # stride 1 is the dilated entry on the flat views
    for cin, cout, k, p, H, B in ((48, 40, 5, 2, 65, 1), (1024, 1, 3, 7, 20, 3), (1024, 1024, 5, 11, 6, 2)):
        assert floats(B, cin, cout, H, p, k, 1, "bf16") == _native.conv1d_weight_grad_dilated_workspace_floats(
            B, cin, cout, H * p, k, p, (k - 1) // 2 * p, precision="bf16")


# ---- the Python surface, the native call stubbed ----
class _Reached(Exception):
    pass


@pytest.fixture
def calls(monkeypatch):
    seen = []

    def record(name, entry, inputs, want_dw, want_db, dw_shape, db_shape, args, workspace, floats):
        seen.append((entry, tuple(args)))
        raise _Reached(entry)
    monkeypatch.setattr(_native, "_weight_grad_call", record)
    return seen


def test_precision_reaches_the_entry(calls):
    g, x = torch.zeros(2, 128, 4, 3), torch.zeros(2, 32, 10, 3)
    for kw, entry in (({}, "fv_period_conv_weight_grad"), ({"precision": "f32"}, "fv_period_conv_weight_grad"),
                      ({"precision": "bf16"}, "fv_period_conv_weight_grad_bf16")):
        with pytest.raises(_Reached):
            _native.period_conv_weight_grad(g, x, 5, 3, **kw)
        assert calls[-1] == (entry, (2, 32, 128, 10, 3, 5, 3))


@pytest.mark.parametrize("precision,entry", [("f32", "fv_period_conv_weight_grad"),
                                             ("bf16", "fv_period_conv_weight_grad_bf16")])
def test_precision_reaches_the_call_from_the_walk(monkeypatch, calls, precision, entry):
    d = DiscriminatorP(3)
    assert d.grad_precision == "f32"
    monkeypatch.setattr(d, "_native_grad_layers", lambda: [None] * 6)
    params = [q for ps in d._conv_params() for q in ps]
    outs = [torch.zeros(2, c, 4, 3) for c in (32, 128, 512, 1024, 1024, 1)]
    d.grad_precision = precision                                   # read at backward time: set after everything else
    with pytest.raises(_Reached):
        d._param_grad(torch.zeros(2, 1, 100), outs, params, [None] * 5 + [torch.zeros(2, 1, 4, 3)], False,
                      [True] * len(params))
    assert calls == [(entry, (2, 1024, 1, 4, 3, 3, 1))]


def test_bad_values_raise():
    g, x = torch.zeros(2, 128, 4, 3), torch.zeros(2, 32, 10, 3)
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
            _native.period_conv_weight_grad(g, x, 5, 3, precision=bad)
        with pytest.raises(_native.NativeError, match="'f32' or 'bf16'"):
            _native.period_conv_weight_grad_workspace_floats(2, 32, 128, 10, 3, 5, 3, precision=bad)
    for module in (DiscriminatorP(5), MultiPeriodDiscriminator(), Discriminator(use_mpd=True), Discriminator()):
        assert module.grad_precision == "f32"
        for bad in ("fp16", "split", True, None):
            with pytest.raises(ValueError, match="'f32' or 'bf16'"):
                module.grad_precision = bad
        assert module.grad_precision == "f32"


def test_the_attribute_sets_and_reads_the_children():
    mpd = MultiPeriodDiscriminator()
    mpd.grad_precision = "bf16"
    assert mpd.grad_precision == "bf16" and all(d.grad_precision == "bf16" for d in mpd.discriminators)
    mpd.discriminators[2].grad_precision = "f32"
    with pytest.raises(ValueError, match="disagree"):
        mpd.grad_precision
    mpd.grad_precision = "f32"
    assert all(d.grad_precision == "f32" for d in mpd.discriminators)
    d = Discriminator(use_mpd=True)
    d.grad_precision = "bf16"
    assert d.grad_precision == "bf16" and d.mpd.grad_precision == "bf16"
    assert "grad_precision" not in "".join(d.state_dict())         # an attribute, not state
    d.grad_precision = "f32"
    assert d.mpd.grad_precision == "f32"


def test_the_discriminator_without_the_mpd_refuses_bf16():
    d = Discriminator()
    d.grad_precision = "f32"
    with pytest.raises(NotImplementedError, match="MSD / MFD weight gradients have no bf16 kernels"):
        d.grad_precision = "bf16"
    assert d.grad_precision == "f32"


def test_the_trainer_keyword():
    names = list(inspect.signature(Trainer.__init__).parameters)
    assert names[-2:] == ["discriminator_grad_precision", "grad_precision"]
    assert inspect.signature(Trainer.__init__).parameters["discriminator_grad_precision"].default == "f32"
    gen = build_generator("hifigan", gref.GOLDEN_CFG)
    g_opt = optim.Adam(gen.parameters())
    d = Discriminator(use_mpd=True)
    d_opt = optim.Adam(d.parameters(), lr=5e-5)
    Trainer(gen, d, g_opt, d_opt, **TRAINER_KW)
    assert d.grad_precision == "f32" and gen.grad_precision == "f32"
    Trainer(gen, d, g_opt, d_opt, grad_precision="bf16", **TRAINER_KW)         # the generator's alone, as before
    assert d.grad_precision == "f32" and gen.grad_precision == "bf16"
    Trainer(gen, d, g_opt, d_opt, discriminator_grad_precision="bf16", **TRAINER_KW)
    assert d.grad_precision == "bf16" and gen.grad_precision == "f32"
    with pytest.raises(ValueError, match="'f32' or 'bf16'"):
        Trainer(gen, d, g_opt, d_opt, discriminator_grad_precision="fp16", **TRAINER_KW)
    plain = Discriminator()
    with pytest.raises(NotImplementedError, match="no bf16 kernels"):
        Trainer(gen, plain, g_opt, optim.Adam(plain.parameters()), discriminator_grad_precision="bf16", **TRAINER_KW)
    Trainer(gen, plain, g_opt, optim.Adam(plain.parameters()), **TRAINER_KW)


def test_the_command_line_flag():
    parser = train_cli.build_parser()
    assert "discriminator_grad_precision" not in vars(parser.parse_args([]))          # absent unless given
    base = ["--model_name", "hifigan", "--config", "c.yaml"]
    for value in ("bf16", "f32"):
        args = train_cli.check_args(parser.parse_args(base + ["--use_mpd", "1", "--discriminator_grad_precision", value]))
        assert args.discriminator_grad_precision == value
    assert train_cli.check_args(parser.parse_args(base + ["--discriminator_grad_precision", "f32"]))
    for extra, word in ((["--use_mpd", "1", "--discriminator_grad_precision", "fp16"], "f32 or bf16"),
                        (["--discriminator_grad_precision", "bf16"], "--use_mpd 1"),
                        (["--use_mpd", "0", "--discriminator_grad_precision", "bf16"], "--use_mpd 1")):
        with pytest.raises(SystemExit) as e:
            train_cli.check_args(parser.parse_args(base + extra))
        message = str(e.value)
        assert message.startswith("MODE=train: ") and "\n" not in message, message
        assert "--discriminator_grad_precision" in message and word in message, message


# ---- the arithmetic ----
def test_the_flat_axis_formula_is_the_period_conv():
    """Column (ci, j) at flat step q reads x_flat[stride (q - q mod p) + q mod p + (j - pad) p], zero unless inside
    [0, H p): what the periodic kernel stages, against the closed form."""
    rs = np.random.RandomState(0)
    worst = 0.0
    for p in pb.PERIODS:
        for stride in (1, 2, 3):
            for k in (3, 5):
                for H in (1, 3, 7, 9, 10, 13):
                    hout, pad = (H - 1) // stride + 1, (k - 1) // 2
                    g, x = rs.randn(2, 3, hout, p), rs.randn(2, 4, H, p)
                    q = np.arange(hout * p)
                    dw = np.zeros((3, 4, k))
                    for j in range(k):
                        pos = stride * (q - q % p) + q % p + (j - pad) * p
                        ok = (pos >= 0) & (pos < H * p)
                        col = np.where(ok, x.reshape(2, 4, H * p)[:, :, np.where(ok, pos, 0)], 0.0)
                        dw[:, :, j] = np.einsum("boq,biq->oi", g.reshape(2, 3, hout * p), col)
                    worst = max(worst, wref.rel_err(dw, wref.period_conv_weight_grad(g, x, k, stride)[0]))
    print(f"flat-axis formula against the closed form: {worst:.1e}")
    assert worst <= 1e-13


def test_every_kernel_shape_rounds_visibly():
    """The GPU test asserts a result more than 10 x KERNEL_RTOL away from the un-rounded closed form; on every one of
    its shapes the rounded closed form is."""
    floor = 10 * KERNEL_RTOL
    least, count = None, 0
    for shape in pb.KERNEL_SHAPES:
        cin, cout, k, stride, p, H, B = shape
        g, x = wref.kernel_inputs(*shape)
        away = wref.rel_err(pb.period_conv_weight_grad(g, x, k, stride)[0], wref.period_conv_weight_grad(g, x, k, stride)[0])
        assert away > floor, (shape, away)
        if least is None or away < least[1]:
            least = (shape, away)
        count += 1
    print(f"{count} kernel shapes: the rounded closed form sits at least {least[1]:.2e} from the un-rounded one "
          f"({least[0]}); the floor is {floor:.1e}")
    units = sorted({B * (-(-((H - 1) // s + 1) * p // pb.U)) // 4 for _, _, _, s, p, H, B in pb.SPLIT_SHAPES})
    assert units == [1, 2, 3]                                      # units per split of the three split shapes
    layers = {s[:4] for s in pb.KERNEL_SHAPES}
    assert set(wref.KERNEL_LAYERS) <= layers and any(s[3] == 2 for s in pb.KERNEL_SHAPES)
    cin, cout, k, stride = pb.REFUSED_SHAPE[:4]
    assert stride > 1 and cout < 64


@pytest.mark.parametrize("name", ["p3", "p11"])
def test_the_patched_oracle_without_rounding_is_the_exact_gradient(name):
    kind, kw, est, real, sd = pb.chain_case(name)
    exact, terms, _, _ = wref.param_grad(kind, est, real, sd, **kw)
    plain, terms2, _, _ = pb.param_grad_bf16(kind, est, real, sd, rounding=False, **kw)
    assert terms == terms2 and sorted(exact) == sorted(plain)
    worst = max(wref.rel_err(plain[k], exact[k]) for k in exact)
    print(f"{name}: patched oracle without rounding against autograd {worst:.1e}")
    assert worst == 0.0


@pytest.mark.parametrize("name", pb.CHAIN_CASES)
def test_the_recorded_yardstick_and_routing_floor(name):
    yard, floor, far, exact = pb.chain_figures(name)
    rec_yard, rec_floor = pb.CHAIN_FIGURES[name]
    print(f"{name}: yardstick (a) {yard:.3e} (recorded {rec_yard:.2e}), routing floor (b) {floor:.4e} "
          f"(recorded {rec_floor:.3e}), largest distance {far:.3e}, the exact tensors {exact:.1e}")
    assert exact == 0.0                                           # every bias and the first layer are left exact
    assert abs(floor - rec_floor) <= pb.FLOOR_RTOL * rec_floor, (floor, rec_floor)
    assert rec_yard / pb.YARDSTICK_BAND <= yard <= rec_yard * pb.YARDSTICK_BAND, (yard, rec_yard)
    assert far >= floor > 0
