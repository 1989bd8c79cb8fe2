"""CPU tests behind tests/test_gpu_basis_learn.py: the header and the entries' refusals, the framing of
tests/basis_learn_reference.py against the oracle's basis overlap-add, its closed-form backward against float64
autograd, the export helper against ``data.load_data_to_buffer(weight_dir=)`` and ``BatchIterator(basis_L=)``,
``MODE=basis``'s parser and exits, the launcher's mode list, and the seeded cases of the GPU tests: no ReLU takes
another side in float32 than in float64, and the float32 eager error that is the GPU constants' yardstick."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native, basis, data
from fastvocoder_amd import hparams as hp
from fastvocoder_amd.bin import basis as basis_cli
from oracle import ops as oracle_ops
from tests import basis_learn_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fv_basis_encode", "fv_basis_learn_grad_workspace_bytes", "fv_basis_learn_grad")
YARDSTICK_THREADS = 1


def test_the_header_declares_the_entries_and_the_abi_stays():
    with open(os.path.join(ROOT, "include", "fastvocoder_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b(int|int64_t) {name}\(", header), name
        assert hasattr(lib, name), name
    assert re.search(r"#define FV_ABI_VERSION 18\b", header) and _native.ABI_VERSION == 18
    assert "additions of ABI 18" in header[header.index("Learning the basis itself"):header.index("fv_basis_encode:")]
    assert "basis_learn.hip" in _native.SOURCES


def test_the_entries_refuse_before_they_touch_a_pointer():
    L = _native.lib()
    INV, UNS = _native.ERR_INVALID_ARG, _native.ERR_UNSUPPORTED
    wild = ctypes.c_void_p(0x10)                                   # never dereferenced: every call below is refused first

    def grad(B, n, C, Lb, ptrs=(wild,) * 6, ws=wild):
        return L.fv_basis_learn_grad(*ptrs, B, n, C, Lb, ws, 1 << 20, None)
    for B, n, C, code in ((0, 40, 4, INV), (2, 0, 4, INV), (2, 40, 0, INV), (-1, 40, 4, INV), (2, -5, 4, INV),
                          (65536, 40, 4, UNS), (2, 1 << 40, 4, UNS)):
        assert L.fv_basis_encode(wild, wild, wild, B, n, C, 30, None) == code, (B, n, C)
        assert L.fv_basis_learn_grad_workspace_bytes(B, n, C, 30) == code, (B, n, C)
        assert grad(B, n, C, 30) == code, (B, n, C)
    for bad_L, code in ((1, INV), (0, INV), (3, INV), (31, INV), (-2, INV), (258, UNS)):
        assert L.fv_basis_encode(wild, wild, wild, 2, 40, 4, bad_L, None) == code, bad_L
        assert L.fv_basis_learn_grad_workspace_bytes(2, 40, 4, bad_L) == code, bad_L
        assert grad(2, 40, 4, bad_L) == code, bad_L
    # null tensors and aliases, with arguments that are fine
    a, b, c, d, e, f = (ctypes.c_void_p(0x10 * (i + 1)) for i in range(6))
    assert L.fv_basis_encode(None, b, c, 2, 40, 4, 30, None) == INV
    assert L.fv_basis_encode(a, b, None, 2, 40, 4, 30, None) == INV
    assert L.fv_basis_encode(a, b, a, 2, 40, 4, 30, None) == INV and L.fv_basis_encode(a, b, b, 2, 40, 4, 30, None) == INV
    for at in range(4):
        assert grad(2, 40, 4, 30, tuple(None if i == at else p for i, p in enumerate((a, b, c, d, e, f)))) == INV, at
    assert grad(2, 40, 4, 30, (a, b, c, d, None, None)) == INV     # both results frozen: nothing to compute
    assert grad(2, 40, 4, 30, (a, b, c, d, e, e)) == INV
    for at in range(4):
        for res in (4, 5):
            ptrs = [a, b, c, d, e, f]
            ptrs[res] = ptrs[at]
            assert grad(2, 40, 4, 30, tuple(ptrs)) == INV, (at, res)
    assert grad(2, 40, 4, 30, (a, b, c, d, e, f), ws=None) == INV
    assert L.fv_basis_learn_grad(a, b, c, d, e, f, 2, 40, 4, 30, wild, 4, None) == INV          # a workspace too small
    assert b"basis_learn_grad" in L.fv_last_error()
    # the split count is a function of the shape alone: 32 crops x 140 frames, L 30, C 256
    nbytes = L.fv_basis_learn_grad_workspace_bytes(32, 140 * 240, 256, 30)
    assert nbytes == 4 * 2 * 256 * 30 * 128 and nbytes == L.fv_basis_learn_grad_workspace_bytes(32, 140 * 240, 256, 30)
    assert L.fv_basis_learn_grad_workspace_bytes(1, 1, 1, 2) == 4 * 2 * 1 * 2


def test_the_restatements_decode_is_the_oracles_overlap_add():
    """The encoder's framing is pinned to the project's own decoder: same weights, same samples, the cut included."""
    for L, C, B, Fr in ((2, 1, 1, 1), (6, 8, 3, 17), (30, 33, 2, 5), (30, 256, 1, 33)):
        rs = np.random.RandomState(L + C + Fr)
        W = np.maximum(rs.randn(B, C, Fr), 0.0).astype(np.float32)
        basis_w = rs.randn(L, C).astype(np.float32)
        hop = L // 2
        want = oracle_ops.basis_ola(W, basis_w, hop)[:, : Fr * hop]
        got = ref.decode(torch.from_numpy(W).double(), torch.from_numpy(basis_w).double()).numpy()
        assert got.shape == want.shape and ref.rel_err(got, want) <= 2e-6, (L, C, B, Fr)
    # and a crop of a whole number of hops comes back at its own length, frame f starting at sample f hop
    wav = torch.arange(1.0, 13.0, dtype=torch.float64)[None]
    pre = ref.pre_activation(wav, torch.eye(6, dtype=torch.float64))          # "encoder" = the frame itself
    assert pre.shape == (1, 6, 4) and torch.equal(pre[0, :, 1], torch.arange(4.0, 10.0, dtype=torch.float64))
    assert torch.equal(pre[0, :, 3], torch.tensor([10.0, 11.0, 12.0, 0.0, 0.0, 0.0], dtype=torch.float64))
    assert ref.frames(12, 6) == 4 and ref.frames(10, 6) == 4 and ref.frames(9, 6) == 3


def test_the_closed_form_of_the_backward_is_autograds():
    """grad_from_weights, the reference of the gradient launch's GPU test, against float64 autograd through the whole
    restatement."""
    for L, C, B, n in ((6, 8, 3, 100), (30, 33, 2, 15 * 17 - 14), (2, 1, 1, 1), (66, 8, 1, 17 * 33 - 5)):
        wav, enc, basis_w, g_est = ref.seeded_case(L, C, B, n, sines=False)
        W, _, d_enc, d_basis = ref.kernel_reference(wav, enc, basis_w, g_est)
        got = ref.grad_from_weights(wav, W, basis_w, g_est)
        assert ref.rel_err(got[0], d_enc) <= 1e-12 and ref.rel_err(got[1], d_basis) <= 1e-12, (L, C, B, n)


def test_the_exported_directory_is_what_the_training_data_path_reads(tmp_path):
    hop, L, C, fixed = 240, 30, 8, 5
    rate = hop // (L // 2)
    rs = np.random.RandomState(3)
    audio, mel, weights = [], [], {}
    for i in range(3):
        frames = 9 + i
        n = frames * hop - 7 * (i == 1)                             # one utterance ends inside a weight frame
        np.save(tmp_path / f"u{i}.npy", rs.randn(n).astype(np.float32))
        np.save(tmp_path / f"u{i}.mel.npy", rs.randn(80, frames).astype(np.float32))
        audio.append(str(tmp_path / f"u{i}.npy"))
        mel.append(str(tmp_path / f"u{i}.mel.npy"))
        weights[f"u{i}.npy"] = rs.rand(C, ref.frames(n, L)).astype(np.float32)
    (tmp_path / "audio.txt").write_text("".join(a + "\n" for a in audio))
    (tmp_path / "mel.txt").write_text("".join(m + "\n" for m in mel))
    basis_w, enc = rs.randn(L, C).astype(np.float32), rs.randn(C, L).astype(np.float32)
    out = tmp_path / "Basis-MelGAN-dataset"
    assert basis.export_dataset(str(out), basis_w, enc, weights.items()) == 3
    assert np.array_equal(np.load(out / "basis_signal_weight.npy"), basis_w)
    assert np.array_equal(np.load(out / "encoder_weight.npy"), enc)
    assert sorted(os.listdir(out / "weight")) == ["u0.npy", "u1.npy", "u2.npy"]
    buffer = data.load_data_to_buffer(str(tmp_path / "audio.txt"), str(tmp_path / "mel.txt"), size=0,
                                      weight_dir=str(out / "weight"))
    for i, item in enumerate(buffer):
        assert np.array_equal(item["weight"].numpy(), weights[f"u{i}.npy"].T)
    batches = data.BatchIterator(buffer, 3, fixed, hop, seed=1, basis_L=L)
    assert len(batches.items) == 3 and batches.weight_rate == rate
    got_mel, got_wav, got_weight = next(iter(batches.epoch()))
    assert got_weight.shape == (3, fixed * rate, C)
    for row in range(3):                                            # each crop is the right rows of its own utterance
        hits = [(i, s) for i, item in enumerate(buffer) for s in range(item["mel"].shape[0] - fixed)
                if torch.equal(item["mel"][s:s + fixed], got_mel[row])]
        assert len(hits) == 1
        i, s = hits[0]
        assert torch.equal(got_weight[row], torch.from_numpy(weights[f"u{i}.npy"].T[s * rate:(s + fixed) * rate]))
        assert torch.equal(got_wav[row], buffer[i]["wav"][s * hop:(s + fixed) * hop])
    with pytest.raises(ValueError, match="encoder"):
        basis.export_dataset(str(out), basis_w, enc.T, [])
    with pytest.raises(ValueError, match="u9"):
        basis.export_dataset(str(out), basis_w, enc, [("u9.npy", np.zeros((C + 1, 4), np.float32))])


def _index_files(tmp_path):
    flags = []
    for name in ("audio_index_path", "mel_index_path", "audio_index_valid_path", "mel_index_valid_path"):
        (tmp_path / name).write_text("")
        flags += [f"--{name}", str(tmp_path / name)]
    return flags


def test_the_parser_and_the_exits(tmp_path):
    args = basis_cli.build_parser().parse_args([])
    assert args.basis_dataset_path == "Basis-MelGAN-dataset" and args.stage == "all" and args.lambda_wave == 0.0
    assert args.learning_rate == hp.learning_rate and args.batch_size == hp.batch_size
    assert args.fixed_length == hp.fixed_length and args.log_step == hp.log_step and args.save_step == hp.save_step
    assert args.max_steps == 0 and args.seed == 0 and args.restore_step == 0 and args.checkpoint_path == ""
    assert not hasattr(args, "gpus")
    with pytest.raises(SystemExit):
        basis_cli.build_parser().parse_args(["--stage", "train"])
    flags = _index_files(tmp_path)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("L: 30\nout_channels: 256\nupsample_scales: [4, 4]\n")
    ok = basis_cli.check_args(basis_cli.build_parser().parse_args(["--config", str(cfg), *flags]))
    assert ok.stage == "all" and basis_cli.read_geometry(str(cfg)) == (30, 256, 240)

    def exits(argv, *words):
        with pytest.raises(SystemExit) as e:
            a = basis_cli.check_args(basis_cli.build_parser().parse_args(argv))
            basis_cli.read_geometry(a.config)
        message = str(e.value)
        assert message.startswith("MODE=basis: ") and "\n" not in message and message.count(". ") == 0, message
        assert all(w in message for w in words), message
    exits([*flags], "--config")
    exits(["--config", str(cfg), *flags, "--gpus", "2"], "--gpus")
    exits(["--config", str(cfg), *flags, "--mixprecision", "1"], "--mixprecision")
    exits(["--config", str(cfg), *flags, "--batch_size", "0"], "--batch_size")
    exits(["--config", str(cfg), *flags, "--stage", "encode"], "--checkpoint_path")
    gone = str(tmp_path / "nowhere.txt")
    exits(["--config", str(cfg), *flags[:-1], gone], gone, "--mel_index_valid_path")
    exits(["--config", str(cfg), "--audio_index_path", gone, *flags[2:]], gone, "--audio_index_path")
    odd = tmp_path / "odd.yaml"
    odd.write_text("L: 31\nout_channels: 8\n")
    exits(["--config", str(odd), *flags], "L = 31", "even")
    wide = tmp_path / "wide.yaml"
    wide.write_text("L: 14\nout_channels: 8\n")                     # 240 % 7 != 0
    exits(["--config", str(wide), *flags], "hop_size 240", "L // 2 = 7")
    assert basis_cli.read_geometry(str(tmp_path / "cfg.yaml"))[2] == 240
    plain = tmp_path / "plain.yaml"
    plain.write_text("L: 6\nout_channels: 8\n")
    assert basis_cli.read_geometry(str(plain)) == (6, 8, hp.hop_size)


def test_the_launcher_names_the_mode():
    from fastvocoder_amd.bin import launcher
    assert "basis" in launcher.__doc__.splitlines()[0]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "launcher.py")], env=dict(os.environ, MODE="nothing"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "MODE=train | basis | synthesize" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "launcher.py")], env=dict(os.environ, MODE="basis"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stderr.strip().splitlines()[-1].startswith("MODE=basis: ")


def test_the_module_has_the_stated_keys_and_no_cpu_path():
    model = basis.BasisAutoencoder()
    sd = model.state_dict()
    assert sorted(sd) == ["basis_signal.layer.weight", "encoder.weight"]
    assert tuple(sd["encoder.weight"].shape) == (256, 1, 30) and tuple(sd["basis_signal.layer.weight"].shape) == (30, 256)
    assert isinstance(model.encoder, torch.nn.Conv1d) and model.encoder.stride == (15,) and model.encoder.bias is None
    for bad in (dict(L=31), dict(L=0), dict(channels=0)):
        with pytest.raises(ValueError):
            basis.BasisAutoencoder(**bad)
    wav = np.zeros((1, 64), np.float32)
    for call in (model, model.encode):
        with pytest.raises(_native.NativeError):
            call(wav)
    with pytest.raises(_native.NativeError):
        model.decode(np.zeros((1, 4, 256), np.float32))
    # the learnt basis drops into the generator under the same key
    from fastvocoder_amd.bin.synthesize import build_generator
    from tests import cases
    gen = build_generator("basis-melgan", next(c for t, _, c in cases.SMALL if t == "basis_s"))
    assert "basis_signal.layer.weight" in gen.state_dict()


def test_no_relu_flips_and_the_float32_yardstick_of_the_seeded_cases():
    """Float32 and float64 take the same side of every ReLU on the seeded cases of the GPU tests, so no element is ever
    left out of a comparison; and the float32 eager error against float64, per tensor peak: the yardstick of
    KERNEL_RTOL and CHAIN_RTOL in tests/test_gpu_basis_learn.py."""
    threads = torch.get_num_threads()
    torch.set_num_threads(YARDSTICK_THREADS)
    try:
        for L, C, B, n in ref.FLIP_CASES:
            wav, enc, basis_w, g_est = ref.seeded_case(L, C, B, n)
            assert ref.relu_flips(wav, enc) == 0, (L, C, B, n)
            want = ref.kernel_reference(wav, enc, basis_w, g_est)
            got = ref.kernel_reference(wav, enc, basis_w, g_est, dtype=torch.float32)
            errs = [ref.rel_err(g, w) for g, w in zip(got[1:], want[1:])]
            print(f"kernel yardstick (L, C, B, n) = {(L, C, B, n)}: float32 eager against float64: est {errs[0]:.2e}, "
                  f"d_enc {errs[1]:.2e}, d_basis {errs[2]:.2e}")
            assert max(errs) <= 2e-6, errs
            if (L, C, B, n) not in ref.CHAIN_CASES:
                continue
            want = ref.chain_reference(wav, enc, basis_w)
            got = ref.chain_reference(wav, enc, basis_w, dtype=torch.float32)
            errs = [abs(got[0] - want[0]) / want[0]] + [ref.rel_err(g, w) for g, w in zip(got[1:], want[1:])]
            print(f"chain yardstick (L, C, B, n) = {(L, C, B, n)}: float32 eager against float64: loss {errs[0]:.2e}, "
                  f"est {errs[1]:.2e}, d_enc {errs[2]:.2e}, d_basis {errs[3]:.2e}; loss {want[0]:.5f}")
            assert max(errs) <= 1e-3, errs
        L, C, B, n = ref.LEARN_CASE
        wav, enc, basis_w, _ = ref.seeded_case(L, C, B, n)
        assert ref.relu_flips(wav, enc) == 0
        # the learning test's reference against itself in float64: the margin LEARN_RTOL is read against
        f32 = ref.eager_learning(wav, enc, basis_w, steps=10, lr=1e-3, clip=1.0)
        f64 = ref.eager_learning(wav, enc, basis_w, steps=10, lr=1e-3, clip=1.0, dtype=torch.float64)
        worst = max(abs(a - b) / b for a, b in zip(f32, f64))
        print(f"learning yardstick: float32 eager {f32[0]:.5f} -> {f32[-1]:.5f}, float64 eager {f64[0]:.5f} -> "
              f"{f64[-1]:.5f}, worst relative difference of the ten losses {worst:.2e}")
        assert f32[-1] < f32[0] and f64[-1] < f64[0] and worst <= 5e-2
    finally:
        torch.set_num_threads(threads)
