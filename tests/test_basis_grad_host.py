"""CPU tests behind tests/test_gpu_basis_grad.py: the closed forms of tests/basis_grad_reference.py meet float64 torch
autograd, its restatement of the two-pass forward meets the reference's own parameter gradient
(tests/golden/basis_param_grad.npz), the B + 1-row formulation has the two-pass gradient, the chain case sits at its
recorded kink margin, the float32 eager-autograd yardsticks are printed, and the opt-in
(``BasisMelGANGenerator.basis_grad``, ``Trainer(basis_grad=True)``, ``MODE=train --basis_grad 1``), the header, the
entries' refusals, the launchers' index arithmetic under a host sanitizer and the data crop behave."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fastvocoder_amd import _native, data, optim
from fastvocoder_amd.bin import train as train_cli
from fastvocoder_amd.bin.synthesize import build_generator
from fastvocoder_amd.discriminator import Discriminator
from fastvocoder_amd.generator import BasisMelGANGenerator
from fastvocoder_amd.synthetic import seeded_state_dict
from fastvocoder_amd.train import KEYS, Trainer, samples_per_frame
from oracle import torch_port
from tests import basis_grad_reference as bref
from tests import cases

CLOSED_FORM_RTOL = 1e-12
GOLDEN_RTOL = 1e-9                 # the fixture's gradients keep 32 bits of mantissa (2.3e-10)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_basis_head_forward", "fv_basis_head_grad", "fv_basis_weight_l1_workspace_bytes", "fv_basis_weight_l1",
           "fv_basis_weight_l1_grad")
TRAINER_KW = dict(lambda_stft=1.0, use_feature_map_loss=True, discriminator_train_start_steps=10, grad_clip_thresh=1.0)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "basis_param_grad.npz"))


def _cfg(tag):
    return next(c for t, _, c in cases.SMALL if t == tag)


def _golden_sd():
    return seeded_state_dict("basis-melgan", bref.GOLDEN_CFG, bref.GOLDEN_WEIGHT_SEED)


def _golden_cw(golden):
    """The cotangent the L1 term hands to weight [B, F, C]."""
    return bref.weight_l1_grad(golden["weight"].transpose(0, 2, 1), golden["target"]).transpose(0, 2, 1)


# ---- the oracles ----
def test_the_closed_forms_meet_float64_autograd():
    # (B, C, F, L): L = 2, F = 1 and C = 1 included; F = 2: the cropped tail
    for B, C, Fr, L in ((1, 1, 1, 2), (3, 1, 2, 2), (2, 5, 2, 8), (1, 3, 7, 30), (3, 4, 1, 30), (2, 6, 9, 6)):
        rs = np.random.RandomState(B + C + Fr + L)
        hop = L // 2
        Y = rs.randn(B + 1, C, Fr)
        Y.reshape(-1)[::4] = 0.0
        basis, target = rs.randn(L, C), rs.randn(B, Fr, C)
        g_est, g_w = rs.randn(B, Fr * hop), rs.randn(B, C, Fr)
        Yt = torch.from_numpy(Y).requires_grad_(True)
        r = torch.relu(Yt)
        D = r[:-1] - r[-1:]
        w = D.transpose(1, 2)
        est = torch_port.overlap_and_add(F.linear(w, torch.from_numpy(basis)), hop)[:, : Fr * hop]
        case = (B, C, Fr, L)
        assert bref.rel_err(bref.head_forward(Y), D.detach().numpy()) <= CLOSED_FORM_RTOL, case
        for ge, gw in ((g_est, g_w), (g_est, None), (None, g_w)):
            Yt.grad = None
            total = 0.0
            if ge is not None:
                total = total + (est * torch.from_numpy(ge)).sum()
            if gw is not None:
                total = total + (D * torch.from_numpy(gw)).sum()
            total.backward(retain_graph=True)
            # torch's relu passes nothing at an exact zero either: the mask is > 0
            assert bref.rel_err(bref.head_grad(ge, gw, Y, basis), Yt.grad.numpy()) <= CLOSED_FORM_RTOL, case
        Dl = D.detach().clone().requires_grad_(True)
        target[0, 0, 0] = float(Dl.detach()[0, 0, 0])                      # sign(0) = 0
        loss = torch.nn.L1Loss()(Dl.transpose(1, 2), torch.from_numpy(target))
        (-1.75 * loss).backward()
        mean_abs, mean_d = bref.weight_l1(Dl.detach().numpy(), target)
        assert abs(mean_abs - float(loss.detach())) <= CLOSED_FORM_RTOL * max(float(loss.detach()), 1.0), case
        assert abs(mean_d - float(Dl.detach().mean())) <= CLOSED_FORM_RTOL, case
        got = bref.weight_l1_grad(Dl.detach().numpy(), target, -1.75)
        assert got[0, 0, 0] == 0.0 and float(np.abs(got - Dl.grad.numpy()).max()) <= 1e-12 / got.size, case


def test_the_restatement_meets_the_reference_gradient(golden):
    mel, c, target = bref.golden_inputs(int(golden["input_seed"]))
    assert np.array_equal(mel, golden["mel"]) and np.array_equal(c, golden["c"])
    assert np.array_equal(target, golden["target"]) and int(golden["weight_seed"]) == bref.GOLDEN_WEIGHT_SEED
    sd = _golden_sd()
    est, weight, grads = bref.param_grad(bref.GOLDEN_CFG, sd, mel, c, _golden_cw(golden))
    assert sorted(grads) == sorted(k for k in sd if k != bref.BASIS_KEY)
    assert f"grad/{bref.BASIS_KEY}" in golden.files               # the reference gives the basis one; nothing reads it
    assert bref.rel_err(est, golden["est"]) <= GOLDEN_RTOL and bref.rel_err(weight, golden["weight"]) <= GOLDEN_RTOL
    worst = max(bref.rel_err(g, golden[f"grad/{k}"]) for k, g in grads.items())
    print(f"restatement against the reference's gradient: {worst:.2e}")
    assert worst <= GOLDEN_RTOL, worst


def test_the_golden_is_small_data_only_and_clear_of_the_kinks(golden, golden_dir):
    path = os.path.join(golden_dir, "basis_param_grad.npz")
    assert os.path.getsize(path) < 100 * 1024
    with np.load(path, allow_pickle=False) as g:
        assert all(g[k].dtype.kind in "fi" for k in g.files)
    margins = []
    _, weight, _ = bref.param_grad(bref.GOLDEN_CFG, _golden_sd(), golden["mel"], golden["c"], None, margins=margins)
    margins.append(float(np.abs(weight - golden["target"]).min() / np.abs(weight - golden["target"]).max()))
    n_up, stacks = len(bref.GOLDEN_CFG["upsample_scales"]), bref.GOLDEN_CFG["stacks"]
    assert len(margins) == 2 * n_up * (1 + 2 * stacks) + 2 + 1    # every leaky ReLU and the final ReLU of both passes, L1
    print(f"golden: smallest kink margin {min(margins):.3e} (recorded {float(golden['margin']):.3e})")
    assert abs(min(margins) - float(golden["margin"])) <= 1e-9 * float(golden["margin"])
    assert min(margins) > bref.KINK


def test_the_one_pass_form_has_the_two_pass_gradient(golden):
    """B + 1 rows, the zero mel last, against the reference's two passes: float64 on the CPU oracle, to rounding."""
    runs = [("golden", (bref.GOLDEN_CFG, _golden_sd(), golden["mel"], golden["c"], _golden_cw(golden)))]
    runs.append(("basis_s", bref.chain_case("basis_s")[:5]))
    for tag, (cfg, sd, mel, c_est, c_w) in runs:
        for ce, cw in ((c_est, c_w), (c_est, None), (None, c_w)):
            e2, w2, g2 = bref.param_grad(cfg, sd, mel, ce, cw)
            e1, w1, g1 = bref.param_grad(cfg, sd, mel, ce, cw, one_pass=True)
            worst = max(bref.rel_err(g1[k], g2[k]) for k in g2)
            # est: overlap_add(a) - overlap_add(b) against overlap_add(a - b), equal by linearity, not bit for bit
            outs = bref.rel_err(e1, e2), bref.rel_err(w1, w2)
            print(f"{tag}: one pass against two passes: gradient {worst:.2e}, est {outs[0]:.2e}, weight {outs[1]:.2e}")
            assert worst <= CLOSED_FORM_RTOL and max(outs) <= CLOSED_FORM_RTOL, (tag, worst, outs)


def test_float32_eager_autograd_error_of_the_chain_is_printed(golden):
    """The yardstick the GPU tolerances of tests/test_gpu_basis_grad.py are read against."""
    err, key, one = bref.float32_yardstick(bref.GOLDEN_CFG, _golden_sd(), golden["mel"], golden["c"], _golden_cw(golden))
    print(f"yardstick golden: float32 eager autograd against float64 {err:.3e} ({key}), one-element tensors {one:.3e}")
    assert 0.0 < err < 1e-4 and one == 0.0
    cfg, sd, mel, c_est, c_w, _ = bref.chain_case("basis_s")
    for name, ce, cw in (("both", c_est, c_w), ("est", c_est, None), ("weight", None, c_w)):
        err, key, one = bref.float32_yardstick(cfg, sd, mel, ce, cw)
        print(f"yardstick basis_s ({name}): float32 eager autograd against float64 {err:.3e} ({key}), one-element "
              f"tensors {one:.3e}")
        assert 0.0 < err < 1e-4 and one == 0.0


@pytest.mark.parametrize("tag", sorted(bref.CHAIN_MEL_SEED))
def test_the_chain_case_sits_at_its_recorded_kink_margin(tag):
    cfg, sd, mel = bref.chain_case(tag)[:3]
    want = bref.CHAIN_MEL_SEED[tag][1]
    got = bref.chain_margin(tag)
    print(f"{tag}: smallest kink margin {got:.3e} (recorded {want:.2e})")
    assert abs(got - want) <= 0.01 * want
    a, b = (bref.kink_sides(cfg, sd, mel, dt) for dt in (torch.float64, torch.float32))
    assert len(a) == 2 * (len(cfg["upsample_scales"]) * (1 + 2 * cfg["stacks"]) + 1)     # both passes, final ReLU too
    assert sum(int((x != y).sum()) for x, y in zip(a, b)) == 0


@pytest.mark.parametrize("tag", sorted(bref.CHAIN_MEL_SEED))
def test_the_chain_seed_is_the_best_of_its_search(tag):
    best = max(bref.CHAIN_SEARCH, key=lambda s: bref.chain_margin(tag, s))
    assert best == bref.CHAIN_MEL_SEED[tag][0]


# ---- the opt-in ----
def test_basis_grad_defaults_setters_and_refusals():
    gen = build_generator("basis-melgan", _cfg("basis_s"))
    assert isinstance(gen, BasisMelGANGenerator) and not hasattr(gen, "stack_grad")
    assert gen.basis_grad is False and gen.parameter_grad is False
    with pytest.raises(NotImplementedError, match="ResidualStack"):
        gen.parameter_grad = True
    assert gen.parameter_grad is False
    gen.parameter_grad = False
    gen.basis_grad = True
    assert gen.basis_grad is True and gen.parameter_grad is False
    gen.parameter_grad = True
    assert gen.parameter_grad is True
    gen.basis_grad = False                                         # switching the opt-in off takes parameter_grad along
    assert gen.basis_grad is False and gen.parameter_grad is False
    with pytest.raises(NotImplementedError, match="ResidualStack"):
        gen.parameter_grad = True
    for tag, word in (("basis_causal_ll", "use_causal_conv"), ("basis_up", "transposedconv=False")):
        other = build_generator("basis-melgan", _cfg(tag))
        with pytest.raises(NotImplementedError) as e:
            other.basis_grad = True
        message = str(e.value)
        assert word in message and "\n" not in message and message.count(". ") == 0, message
        assert other.basis_grad is False
    lastlinear = build_generator("basis-melgan", dict(_cfg("basis_s"), lastlinear=True))
    with pytest.raises(NotImplementedError, match="lastlinear=True") as e:
        lastlinear.basis_grad = True
    assert str(e.value).count(". ") == 0
    basis = torch.zeros(30, 32)
    keys = {k: v for k, v in _cfg("basis_s").items() if k not in ("L", "transposedconv")}
    raw = BasisMelGANGenerator(basis_signal_weight=basis, L=30, use_final_nonlinear_activation=False, **keys)
    with pytest.raises(NotImplementedError, match="use_final_nonlinear_activation=False") as e:
        raw.basis_grad = True
    assert str(e.value).count(". ") == 0


def test_the_trainer_takes_the_opt_in_as_a_keyword():
    d = Discriminator()
    d_opt = optim.Adam(d.parameters(), lr=5e-5)
    gen = build_generator("basis-melgan", _cfg("basis_s"))
    for kw in ({}, {"stack_grad": True}):
        with pytest.raises(NotImplementedError, match="ResidualStack"):
            Trainer(gen, d, optim.Adam(gen.melgan.parameters()), d_opt, **kw, **TRAINER_KW)
        assert gen.basis_grad is False and gen.parameter_grad is False and not hasattr(gen, "stack_grad")
    with pytest.raises(TypeError):                                          # keyword-only
        Trainer(gen, d, optim.Adam(gen.melgan.parameters()), d_opt, None, None, None, False, True, **TRAINER_KW)
    t = Trainer(gen, d, optim.Adam(gen.melgan.parameters()), d_opt, basis_grad=True, **TRAINER_KW)
    assert gen.basis_grad is True and gen.parameter_grad is True and t.basis is True
    assert t.samples_per_frame == 4 * 4 * 15 == samples_per_frame(gen)
    full = build_generator("basis-melgan", cases.load_conf("conf/basis-melgan/light.yaml"))
    assert samples_per_frame(full) == 240
    assert KEYS == ("stft", "total", "adversarial", "feature_map", "discriminator", "grad_norm", "discriminator_grad_norm")
    up = build_generator("basis-melgan", _cfg("basis_up"))
    with pytest.raises(NotImplementedError, match="transposedconv=False"):
        Trainer(up, d, optim.Adam(up.melgan.parameters()), d_opt, basis_grad=True, **TRAINER_KW)


def test_the_command_line_opt_in(tmp_path):
    parser = train_cli.build_parser()
    assert "basis_grad" not in vars(parser.parse_args([])) and "basis_dataset_path" not in vars(parser.parse_args([]))
    assert parser.parse_args(["--basis_grad", "1"]).basis_grad == 1
    assert parser.parse_args(["--basis_dataset_path", "d"]).basis_dataset_path == "d"
    base = ["--model_name", "basis-melgan", "--config", "c.yaml"]
    args = train_cli.check_args(parser.parse_args(base + ["--basis_grad", "1"]))
    assert args.model_name == "basis-melgan" and args.basis_grad == 1
    for argv in (base, base + ["--basis_grad", "0"], base + ["--stack_grad", "1"]):
        with pytest.raises(SystemExit) as e:
            train_cli.run_train(argv)
        message = str(e.value)
        assert message.startswith("MODE=train: ") and "\n" not in message
        assert "basis-melgan" in message and "no parameter gradient" in message, message
    assert train_cli.SUPPORTED == ("hifigan", "multiband-hifigan")
    # a missing basis file ends the run with one sentence that names the path (run() loads it right after the model)
    gen = build_generator("basis-melgan", bref.GOLDEN_CFG)
    missing = tmp_path / "nowhere" / "basis_signal_weight.npy"
    with pytest.raises(SystemExit) as e:
        train_cli.load_basis(gen, str(missing))
    message = str(e.value)
    assert message.startswith("MODE=train: ") and "\n" not in message and str(missing) in message, message
    np.save(tmp_path / "wrong.npy", np.zeros((4, 8), np.float32))
    with pytest.raises(SystemExit, match="wrong.npy"):
        train_cli.load_basis(gen, str(tmp_path / "wrong.npy"))
    value = np.random.RandomState(0).randn(bref.GOLDEN_CFG["L"], bref.GOLDEN_CFG["out_channels"]).astype(np.float32)
    np.save(tmp_path / "basis_signal_weight.npy", value)
    train_cli.load_basis(gen, str(tmp_path / "basis_signal_weight.npy"))
    assert np.array_equal(gen.basis_signal.layer.weight.detach().numpy(), value)


# ---- the entries ----
def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert "additions of ABI 18" in header[header.index("The head of Basis-MelGAN"):header.index("fv_basis_head_forward:")]


def test_the_entries_refuse_before_they_touch_a_pointer():
    L = _native.lib()
    INV, UNS = _native.ERR_INVALID_ARG, _native.ERR_UNSUPPORTED
    wild = ctypes.c_void_p(0x10)                                   # never dereferenced: every call below is refused first
    for B, C, Fr, code in ((0, 4, 4, INV), (2, 0, 4, INV), (2, 4, 0, INV), (-1, 4, 4, INV), (65536, 4, 4, UNS)):
        assert L.fv_basis_head_forward(wild, wild, B, C, Fr, None) == code, (B, C, Fr)
        assert L.fv_basis_head_grad(wild, wild, wild, wild, wild, B, C, Fr, 30, None) == code, (B, C, Fr)
        assert L.fv_basis_weight_l1_workspace_bytes(B, C, Fr) == code, (B, C, Fr)
        assert L.fv_basis_weight_l1(wild, wild, wild, B, C, Fr, wild, 1 << 20, None) == code, (B, C, Fr)
        assert L.fv_basis_weight_l1_grad(wild, wild, wild, wild, B, C, Fr, None) == code, (B, C, Fr)
    for bad_L, code in ((1, INV), (0, INV), (3, INV), (31, INV), (-2, INV), (258, UNS)):
        assert L.fv_basis_head_grad(wild, wild, wild, wild, wild, 2, 4, 4, bad_L, None) == code, bad_L
    # null tensors, with arguments that are fine
    assert L.fv_basis_head_forward(None, None, 2, 4, 4, None) == INV
    assert L.fv_basis_head_grad(None, None, None, None, None, 2, 4, 4, 30, None) == INV
    assert L.fv_basis_weight_l1(None, None, None, 2, 4, 4, None, 0, None) == INV
    assert L.fv_basis_weight_l1_grad(None, None, None, None, 2, 4, 4, None) == INV
    assert L.fv_basis_weight_l1_workspace_bytes(3, 256, 70) == 2 * 8 * 2 * 4 * 3
    assert b"basis_head_grad" in L.fv_last_error() or b"basis" in L.fv_last_error()


def test_the_launchers_index_arithmetic_under_a_host_sanitizer(tmp_path):
    """tests/native/basis_grad_host_main.cpp walks csrc/basis_grad_host.hpp's geometry over buffers of the tensors' exact
    sizes (L = 2, F = 1, C = 1 included), built with -fsanitize=address,undefined as a stand-alone program."""
    cxx = next((c for c in (shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "basis_grad_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "basis_grad_host_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "basis_grad_host ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "L=2" in r.stdout and "C=1 F=1" in r.stdout


# ---- the data ----
def _utterance(tmp_path, name, frames, hop, rate, C, weights=True):
    rs = np.random.RandomState(frames)
    np.save(tmp_path / f"{name}.npy", rs.randn(frames * hop).astype(np.float32))
    np.save(tmp_path / f"{name}.mel.npy", rs.randn(80, frames).astype(np.float32))
    if weights:
        (tmp_path / "weight").mkdir(exist_ok=True)
        np.save(tmp_path / "weight" / f"{name}.npy", rs.randn(C, frames * rate).astype(np.float32))
    return str(tmp_path / f"{name}.npy"), str(tmp_path / f"{name}.mel.npy")


def test_the_data_crop_follows_weight_dataset(tmp_path):
    hop, L, C, fixed = 240, 30, 8, 5
    rate = hop // (L // 2)
    assert rate == 16
    pairs = [_utterance(tmp_path, f"u{i}", 9 + i, hop, rate, C) for i in range(3)]
    (tmp_path / "audio.txt").write_text("".join(a + "\n" for a, _ in pairs))
    (tmp_path / "mel.txt").write_text("".join(m + "\n" for _, m in pairs))
    buffer = data.load_data_to_buffer(str(tmp_path / "audio.txt"), str(tmp_path / "mel.txt"), size=0,
                                      weight_dir=str(tmp_path / "weight"))
    item = buffer[1]
    stored = np.load(tmp_path / "weight" / "u1.npy")
    assert item["weight"].shape == (10 * rate, C) and np.array_equal(item["weight"].numpy(), stored.T)
    for start in (0, 3, 4):
        mel, wav, weight = data.crop(item, start, fixed, hop, rate)
        end = start + fixed
        # WeightDataset.__getitem__ (dataset.py:96-106): hparams.hop_size // (L // 2) weight frames per mel frame
        assert torch.equal(weight, item["weight"][start * (hop // (L // 2)):end * (hop // (L // 2)), :])
        assert weight.shape == (fixed * 16, C) and wav.shape == (fixed * hop,) and mel.shape == (fixed, 80)
        assert torch.equal(wav, item["wav"][start * hop:end * hop]) and torch.equal(mel, item["mel"][start:end])
    batches = data.BatchIterator(buffer, 2, fixed, hop, seed=1, basis_L=L)
    got = next(iter(batches.epoch()))
    assert len(got) == 3 and got[0].shape == (2, fixed, 80) and got[1].shape == (2, fixed * hop)
    assert got[2].shape == (2, fixed * rate, C)
    with pytest.raises(ValueError, match="basis_L"):
        data.BatchIterator(buffer, 2, fixed, hop, seed=1)
    some = [dict(buffer[0]), {k: v for k, v in buffer[1].items() if k != "weight"}]
    with pytest.raises(ValueError, match="all of them or none"):           # no batch of mixed tuples
        data.BatchIterator(some, 2, fixed, hop, seed=1, basis_L=L)
    # a buffer without weights still yields pairs, and the same ones as before
    plain = data.load_data_to_buffer(str(tmp_path / "audio.txt"), str(tmp_path / "mel.txt"), size=0)
    assert all("weight" not in it for it in plain)
    pair = next(iter(data.BatchIterator(plain, 2, fixed, hop, seed=1).epoch()))
    assert len(pair) == 2 and torch.equal(pair[0], got[0]) and torch.equal(pair[1], got[1])
    assert len(data.crop(plain[0], 0, fixed, hop)) == 2
    # a missing weight file names its path
    os.remove(tmp_path / "weight" / "u2.npy")
    with pytest.raises(data.MissingWeightFile, match=re.escape(str(tmp_path / "weight" / "u2.npy"))):
        data.load_data_to_buffer(str(tmp_path / "audio.txt"), str(tmp_path / "mel.txt"), size=0,
                                 weight_dir=str(tmp_path / "weight"))
    assert issubclass(data.MissingWeightFile, FileNotFoundError)
    # a missing mel or waveform is not that error: MODE=train lets it raise as it always did
    os.remove(tmp_path / "u1.mel.npy")
    with pytest.raises(FileNotFoundError) as e:
        data.load_data_to_buffer(str(tmp_path / "audio.txt"), str(tmp_path / "mel.txt"), size=0)
    assert not isinstance(e.value, data.MissingWeightFile)
