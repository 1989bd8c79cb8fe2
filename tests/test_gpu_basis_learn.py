"""GPU tests of learning Basis-MelGAN's basis: fv_basis_encode and fv_basis_learn_grad alone against float64 on the
same fp32 inputs, ``BasisAutoencoder.forward`` + the STFT loss against the float64 restatement
(tests/basis_learn_reference.py), ten Adam steps against float32 eager torch on the CPU, and ``MODE=basis`` through
bin/launcher.py up to the ``MODE=train --model_name basis-melgan`` run that reads what it wrote.

Every error is relative to the reference tensor's largest magnitude; no element is left out of a comparison.  The
constants are about ten times the worst figure measured on the MI355X; DESIGN.md section 6.25 lists each beside the
float32 CPU eager yardstick that tests/test_basis_learn_host.py prints.  Each subprocess runs under a time limit."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastvocoder_amd import _native, optim
from fastvocoder_amd.basis import BasisAutoencoder
from fastvocoder_amd.loss import MultiResolutionSTFTLoss
from tests import basis_grad_reference as bgref
from tests import basis_learn_reference as ref
from tests import cases

pytestmark = pytest.mark.gpu

# The kernels alone: measured worst 4.6e-7 (d_enc, L 2 C 1), float32 eager on the CPU 1.5e-7 .. 1.7e-6.
KERNEL_RTOL = 5e-6
# The chain through the STFT loss against float64, per case: measured worst 2.6e-5 (L 6 / C 8) and 3.9e-4 (L 30 /
# C 256), float32 eager 2.2e-5 and 1.0e-4.  The figure above its yardstick is the cotangent's: the STFT loss'
# gradient kernels (an earlier feature, tests/test_gpu_stft_loss_grad.py) err by 3e-4 .. 7e-3 of the peak on their
# own cases, because the mag term jumps where a bin of X crosses Y; the autoencoder's backward is linear in that
# cotangent.  The same test therefore also feeds the device's own cotangent to the float64 closed form, and holds the
# new kernels to KERNEL_RTOL there (measured 2.4e-7).
CHAIN_RTOL = {(6, 8, 2, 2520): 3e-4, (30, 256, 2, 2520): 4e-3}
# The loss sequence of ten Adam steps against float32 eager torch on the CPU (one thread): measured worst 2.2e-3.
# The trajectory crosses those jumps, so the reference does not pin it tighter itself: float32 eager differs from
# float64 eager by 4.1e-3 on this case (tests/test_basis_learn_host.py prints it), and from itself at another thread
# count by 9.8e-4.
LEARN_RTOL = 2e-2
LIMIT = 300                # seconds per subprocess
ENC_KEY, BASIS_KEY = "encoder.weight", "basis_signal.layer.weight"


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def kernel_shapes(C):
    """(L, C, B, n) of the kernel tests: F in {1, 2, 17, a gradient unit + 1, an encode tile + 1}, B in {1, 3}, n a
    whole number of hops and hop - 1 short of it; then the shapes that take the other paths: more units than splits
    (one and two channel tiles), and two tap tiles."""
    out = []
    for L in (2, 6, 30):
        hop = L // 2
        for Fr in (1, 2, 17, 33, 65):
            for B in (1, 3):
                for n in sorted({Fr * hop, Fr * hop - (hop - 1)}):
                    out.append((L, C, B, n))
    if C == 8:
        out += [(6, 8, 3, 9000), (66, 8, 1, 17 * 33 - 5)]
    if C == 33:
        out.append((66, 33, 1, 17 * 33))
    if C == 256:
        out.append((30, 256, 3, 1409 * 15 - 14))
    return out


@pytest.mark.parametrize("C", [1, 8, 33, 256])
def test_the_encoder_against_float64(C):
    worst = (0.0, None)
    for L, _, B, n in kernel_shapes(C):
        wav, enc, _, _ = ref.seeded_case(L, C, B, n, sines=False)
        want = ref.encode(torch.from_numpy(wav).double(), torch.from_numpy(enc).double()).numpy()
        got = _native.basis_encode(_t(wav), _t(enc)).cpu().numpy()
        assert got.shape == want.shape == (B, C, ref.frames(n, L)) and np.isfinite(got).all() and (got >= 0).all()
        worst = max(worst, (ref.rel_err(got, want), (L, C, B, n)))
    print(f"encode C={C}: worst {worst[0]:.2e} at (L, C, B, n) = {worst[1]}")
    assert worst[0] <= KERNEL_RTOL, worst


@pytest.mark.parametrize("C", [1, 8, 33, 256])
def test_the_gradient_launch_against_float64(C):
    worst = {"d_enc": (0.0, None), "d_basis": (0.0, None)}
    for L, _, B, n in kernel_shapes(C):
        wav, enc, basis, g_est = ref.seeded_case(L, C, B, n, sines=False)
        # the forward's W as float32 data: the mask the kernel and the reference apply is that of the same numbers
        W = ref.encode(torch.from_numpy(wav).double(), torch.from_numpy(enc).double()).float().numpy()
        want = dict(zip(("d_enc", "d_basis"), ref.grad_from_weights(wav, W, basis, g_est)))
        got = dict(zip(("d_enc", "d_basis"), _native.basis_learn_grad(_t(wav), _t(g_est), _t(W), _t(basis))))
        for k in want:
            assert tuple(got[k].shape) == want[k].shape
            worst[k] = max(worst[k], (ref.rel_err(got[k].cpu().numpy(), want[k]), (L, C, B, n)))
    for k, (err, case) in worst.items():
        print(f"learn_grad C={C} {k}: worst {err:.2e} at (L, C, B, n) = {case}")
    assert max(v[0] for v in worst.values()) <= KERNEL_RTOL, worst


@pytest.mark.parametrize("case", [(30, 256, 3, 1409 * 15 - 14), (6, 8, 3, 9000), (66, 33, 1, 17 * 33), (2, 1, 1, 1)])
def test_identical_calls_identical_bits_and_the_workspace_does_not_matter(case):
    L, C, B, n = case
    wav, enc, basis, g_est = (_t(a) for a in ref.seeded_case(L, C, B, n, sines=False))
    W = _native.basis_encode(wav, enc)
    assert torch.equal(W, _native.basis_encode(wav, enc))
    first = _native.basis_learn_grad(wav, g_est, W, basis)
    again = _native.basis_learn_grad(wav, g_est, W, basis)
    floats = (_native.lib().fv_basis_learn_grad_workspace_bytes(B, n, C, L) + 3) // 4
    poisoned = torch.full((floats,), float("nan"), dtype=torch.float32, device=_dev())
    nan = _native.basis_learn_grad(wav, g_est, W, basis, workspace=poisoned)
    for a, b, c in zip(first, again, nan):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    # a frozen parameter: its result is None and the other one keeps its bits
    only_enc = _native.basis_learn_grad(wav, g_est, W, basis, want_basis=False)
    only_basis = _native.basis_learn_grad(wav, g_est, W, basis, want_enc=False)
    assert only_enc[1] is None and only_basis[0] is None
    assert torch.equal(only_enc[0], first[0]) and torch.equal(only_basis[1], first[1])


def _model(L, C, enc, basis):
    model = BasisAutoencoder(L=L, channels=C)
    model.load_state_dict({ENC_KEY: torch.from_numpy(np.array(enc)).reshape(C, 1, L),
                           BASIS_KEY: torch.from_numpy(np.array(basis))})
    return model.to(_dev())


def _stft_loss():
    loss = MultiResolutionSTFTLoss().to(_dev())
    loss.differentiable = True
    return loss


@pytest.mark.parametrize("case", ref.CHAIN_CASES)
def test_the_chain_against_the_float64_restatement(case):
    L, C, B, n = case
    wav, enc, basis, _ = ref.seeded_case(L, C, B, n)
    want_loss, want_est, want_enc, want_basis = ref.chain_reference(wav, enc, basis)
    model = _model(L, C, enc, basis)
    assert sorted(model.state_dict()) == sorted([ENC_KEY, BASIS_KEY])
    x = _t(wav)
    est, weight = model(x)
    assert tuple(est.shape) == (B, n) and tuple(weight.shape) == (B, ref.frames(n, L), C) and not weight.requires_grad
    est.retain_grad()
    sc, mag = _stft_loss()(est, x)
    (sc + mag).backward()
    errs = {"loss": abs(float((sc + mag).detach()) - want_loss) / want_loss, "est": ref.rel_err(est.detach().cpu().numpy(), want_est),
            "d_enc": ref.rel_err(model.encoder.weight.grad.reshape(C, L).cpu().numpy(), want_enc),
            "d_basis": ref.rel_err(model.basis_signal.layer.weight.grad.cpu().numpy(), want_basis)}
    # the new kernels' share: the float64 closed form of the backward on the device's own cotangent and weights
    own = ref.grad_from_weights(wav, weight.transpose(1, 2).cpu().numpy(), basis, est.grad.cpu().numpy())
    split = {"d_enc": ref.rel_err(model.encoder.weight.grad.reshape(C, L).cpu().numpy(), own[0]),
             "d_basis": ref.rel_err(model.basis_signal.layer.weight.grad.cpu().numpy(), own[1])}
    print(f"chain {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + "; on the device's own cotangent: "
          + ", ".join(f"{k} {v:.2e}" for k, v in split.items()))
    assert max(errs["loss"], errs["est"], *split.values()) <= KERNEL_RTOL, (errs, split)
    assert max(errs.values()) <= CHAIN_RTOL[case], errs
    # the methods: encode is forward's weight, decode its est, bit for bit
    assert torch.equal(model.encode(x), weight) and torch.equal(model.decode(weight), est.detach())
    # a frozen parameter gets None; the other one its bits
    p_enc, p_basis = model.encoder.weight, model.basis_signal.layer.weight
    kept = {p_enc: p_enc.grad.clone(), p_basis: p_basis.grad.clone()}
    for frozen, live in ((p_enc, p_basis), (p_basis, p_enc)):
        model.zero_grad(set_to_none=True)
        frozen.requires_grad_(False)
        sc, mag = _stft_loss()(model(x)[0], x)
        (sc + mag).backward()
        assert frozen.grad is None and torch.equal(live.grad, kept[live])
        frozen.requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        model(x.clone().requires_grad_(True))
    with pytest.raises(_native.NativeError):
        BasisAutoencoder(L=L, channels=C)(wav)                     # a module on the CPU: there is no CPU path


def test_ten_adam_steps_follow_float32_eager_torch():
    L, C, B, n = ref.LEARN_CASE
    wav, enc, basis, _ = ref.seeded_case(L, C, B, n)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                       # the reference's own sums depend on it
    try:
        want = ref.eager_learning(wav, enc, basis, steps=10, lr=1e-3, clip=1.0)
    finally:
        torch.set_num_threads(threads)
    model, loss_fn, x = _model(L, C, enc, basis), _stft_loss(), _t(wav)
    opt = optim.Adam(model.parameters(), lr=1e-3, eps=1e-6)
    got = []
    for _ in range(10):
        sc, mag = loss_fn(model(x)[0], x)
        opt.zero_grad(set_to_none=True)
        (sc + mag).backward()
        opt.step(max_norm=1.0)
        got.append(float((sc + mag).detach()))
    worst = max(abs(g - w) / w for g, w in zip(got, want))
    print("learning: GPU " + " ".join(f"{v:.5f}" for v in got))
    print("learning: CPU " + " ".join(f"{v:.5f}" for v in want) + f"; worst relative difference {worst:.2e}")
    assert worst <= LEARN_RTOL, (got, want)
    assert got[-1] < got[0] and want[-1] < want[0]


# ---- the flow ----
CLI_CFG = dict(bgref.GOLDEN_CFG, lamda_stft=1.0, multiband=False, use_feature_map_loss=True)
FL, FC = CLI_CFG["L"], CLI_CFG["out_channels"]
RATE = 6                                  # weight frames per mel frame: prod(upsample_scales)
SPF, FIXED = RATE * (FL // 2), 140        # 140 frames x 18 = 2520 samples


def _dataset(tmp_path, split, count, seed):
    rs = np.random.RandomState(seed)
    audio, mel = [], []
    for i in range(count):
        t = np.arange((FIXED + 1) * SPF) / 24000.0
        wav = (0.3 * np.sin(2 * np.pi * (150.0 + 40 * i) * t) + 0.02 * rs.randn(t.size)).astype(np.float32)
        np.save(tmp_path / f"{split}{i}.npy", wav)
        np.save(tmp_path / f"{split}{i}.mel.npy", rs.uniform(-4.0, 1.0, (80, FIXED + 1)).astype(np.float32))
        audio.append(str(tmp_path / f"{split}{i}.npy"))
        mel.append(str(tmp_path / f"{split}{i}.mel.npy"))
    for kind, paths in (("audio", audio), ("mel", mel)):
        (tmp_path / f"{kind}_{split}.txt").write_text("".join(p + "\n" for p in paths))


def _launch(tmp_path, mode, *extra):
    args = ["--config", str(tmp_path / "cfg.yaml"),
            "--audio_index_path", str(tmp_path / "audio_train.txt"), "--mel_index_path", str(tmp_path / "mel_train.txt"),
            "--audio_index_valid_path", str(tmp_path / "audio_valid.txt"),
            "--mel_index_valid_path", str(tmp_path / "mel_valid.txt"), "--basis_dataset_path", str(tmp_path / "basis"),
            "--batch_size", "2", "--fixed_length", str(FIXED), "--log_step", "1", "--save_step", "3", *extra]
    return subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), *args],
                          env=dict(os.environ, MODE=mode), cwd=str(tmp_path), capture_output=True, text=True,
                          timeout=LIMIT)


def _checkpoint(tmp_path, step, which=0):
    found = sorted(glob.glob(str(tmp_path / "checkpoint" / "*" / f"basis_{step}.pth.tar")), key=os.path.getmtime)
    assert len(found) > which, (step, found)
    return found[which]


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("basis_learn")
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(CLI_CFG))
    _dataset(tmp_path, "train", 2, seed=0)
    _dataset(tmp_path, "valid", 2, seed=1)
    r = _launch(tmp_path, "basis", "--max_steps", "6", "--learning_rate", "0.001")
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp_path, r.stdout


def test_the_run_logs_saves_and_writes_the_three_kinds_of_files(first_run):
    import re
    from fastvocoder_amd.bin.synthesize import load_checkpoint
    tmp_path, out = first_run
    assert len(re.findall(r"^basis [1-6] stft=\d\.\d{8}e[+-]\d\d grad_norm=\d\.\d{8}e[+-]\d\d$", out, flags=re.M)) == 6
    assert re.search(r"^valid stft=\d\.\d{8}e[+-]\d\d snr=-?\d+\.\d\d dB$", out, flags=re.M), out
    basis = np.load(tmp_path / "basis" / "basis_signal_weight.npy")
    encoder = np.load(tmp_path / "basis" / "encoder_weight.npy")
    assert basis.shape == (FL, FC) and encoder.shape == (FC, FL) and basis.dtype == encoder.dtype == np.float32
    ckpt = load_checkpoint(_checkpoint(tmp_path, 6), "cpu")
    assert sorted(ckpt) == ["model", "optimizer"] and sorted(ckpt["model"]) == sorted([ENC_KEY, BASIS_KEY])
    assert np.array_equal(ckpt["model"][BASIS_KEY].numpy(), basis)
    assert np.array_equal(ckpt["model"][ENC_KEY].numpy().reshape(FC, FL), encoder)
    model = _model(FL, FC, encoder, basis)
    names = sorted(os.listdir(tmp_path / "basis" / "weight"))
    assert names == ["train0.npy", "train1.npy", "valid0.npy", "valid1.npy"]
    for name in names:
        wav, w = np.load(tmp_path / name), np.load(tmp_path / "basis" / "weight" / name)
        assert w.dtype == np.float32 and w.shape == (FC, ref.frames(wav.size, FL)) == (FC, (FIXED + 1) * RATE)
        assert np.array_equal(model.encode(_t(wav[None]))[0].cpu().numpy().T, w), name


def test_a_run_resumed_from_the_first_checkpoint_reaches_the_second(first_run):
    from fastvocoder_amd.bin.synthesize import load_checkpoint
    tmp_path, _ = first_run
    want = load_checkpoint(_checkpoint(tmp_path, 6), "cpu")["model"]
    start = load_checkpoint(_checkpoint(tmp_path, 3), "cpu")["model"]
    r = _launch(tmp_path, "basis", "--stage", "learn", "--checkpoint_path", _checkpoint(tmp_path, 3), "--restore_step", "3",
                "--max_steps", "3", "--learning_rate", "0.001")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "---Model Restored at Step 3---" in r.stdout and "basis 6 stft=" in r.stdout and "basis 3 stft=" not in r.stdout
    got = load_checkpoint(_checkpoint(tmp_path, 6, which=1), "cpu")["model"]
    worst = max(ref.rel_err(got[k].numpy(), want[k].numpy()) for k in want)
    moved = max(ref.rel_err(start[k].numpy(), want[k].numpy()) for k in want)
    print(f"resumed run against the first: parameters {worst:.2e} (steps 4 .. 6 moved them by {moved:.2e})")
    # the two rows of the batch may come in the other order: the same sums in another order, not the same bits
    assert worst <= KERNEL_RTOL < moved, (worst, moved)


def test_the_generator_trains_on_the_directory_that_was_written(first_run):
    """The point of the feature: MODE=train --model_name basis-melgan reads what MODE=basis wrote."""
    import re
    tmp_path, _ = first_run
    args = ["--model_name", "basis-melgan", "--config", str(tmp_path / "cfg.yaml"),
            "--audio_index_path", str(tmp_path / "audio_train.txt"), "--mel_index_path", str(tmp_path / "mel_train.txt"),
            "--audio_index_valid_path", str(tmp_path / "audio_valid.txt"),
            "--mel_index_valid_path", str(tmp_path / "mel_valid.txt"), "--basis_dataset_path", str(tmp_path / "basis"),
            "--batch_size", "2", "--fixed_length", str(FIXED), "--log_step", "1", "--basis_grad", "1", "--max_steps", "2"]
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "bin", "launcher.py"), *args],
                       env=dict(os.environ, MODE="train"), cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=LIMIT)
    assert r.returncode == 0, r.stdout + r.stderr
    found = re.findall(r"Weight Loss: (\d+\.\d{6}),", r.stdout)
    assert len(found) == 2 and all(float(v) > 0.0 for v in found), r.stdout
