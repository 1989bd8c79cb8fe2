"""GPU tests of the discriminators (csrc/disc.hip: fv_grouped_conv1d, fv_avg_pool1d, fv_disc_score_sums;
fv_stft_magnitude_bins; fastvocoder_amd.discriminator; loss.discriminator_terms) against the float64 oracle
tests/discriminator_reference.py and the reference's values (tests/golden/discriminator.npz), and of
MODE=evaluation --discriminator."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import torch
import torch.nn.functional as F

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, MelGANDiscriminator, MelGANMultiScaleDiscriminator,
                                           MultiResolutionSTFTDiscriminator, STFTDiscriminator)
from fastvocoder_amd.loss import discriminator_terms, stft, stft_tables
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_state_dict
from tests import cases
from tests import discriminator_reference as ref

pytestmark = pytest.mark.gpu

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_STFT = dict(fft_size=512, shift_size=50, win_length=240, channels=8, max_downsample_channels=64)
SEEDS = {"small_msd": 11, "small_stft": 12, "full": 13}

# against the float64 oracle, relative to the largest magnitude of the tensor compared (a feature map: also of its
# input): the worst errors measured on MI355X times about 10
CONV_RTOL = 6e-6         # grouped conv alone (worst 5.8e-7)
DENSE_RTOL = 2e-5        # the discriminators' dense shapes through fv_conv1d_fused (worst 1.6e-6)
POOL_RTOL = 1e-6         # average pool: an fp32 sum of at most 5 samples and one division
MAP_RTOL = 2e-5          # every feature map of a forward (worst 2.1e-6)
SCORE_RTOL = 7e-6        # the five scores, relative (worst 7.0e-7)
# against the reference's float32 CPU values (the oracle meets them within 2e-5: tests/test_discriminator_host.py)
GOLDEN_RTOL = 5e-5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _rel(got, want):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _load(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.to(_dev()).eval()


# (Cin, Cout, k, stride, Tin): every discriminator shape (MSD 16->64->256->1024->1024 k41 s4, MFD 64->256->1024 k25
# s4, the small configs' 4->16 k41 s4 and 16->16 k21 s2), stride 1 and 2, Cout/groups 1, 2, 4, 8 and 16, odd lengths
GROUPED_GRID = [
    (16, 64, 41, 4, 24001), (64, 256, 41, 4, 6001), (256, 1024, 41, 4, 1501), (1024, 1024, 41, 4, 377),
    (64, 256, 25, 4, 1001), (256, 1024, 25, 4, 251), (4, 16, 41, 4, 2001), (16, 16, 21, 2, 501),
    (8, 8, 7, 1, 1033), (4, 1, 11, 1, 999), (8, 4, 13, 2, 1000), (4, 8, 31, 3, 777), (12, 48, 51, 5, 4097),
    (8, 32, 13, 2, 3),
]


def test_grouped_conv_against_float64():
    rs = np.random.RandomState(1)
    worst = 0.0
    for cin, cout, k, s, T in GROUPED_GRID:
        for bias in (True, False):
            x = rs.randn(2, cin, T).astype(np.float32)
            w = (rs.randn(cout, 4, k) / np.sqrt(4 * k)).astype(np.float32)
            b = rs.randn(cout).astype(np.float32) if bias else None
            got = _native.grouped_conv1d(_t(x), _t(w), _t(b) if bias else None, k, s, (k - 1) // 2, 0.2)
            want = F.leaky_relu(F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                                         torch.from_numpy(b).double() if bias else None, stride=s,
                                         padding=(k - 1) // 2, groups=cin // 4), 0.2)
            err = _rel(got, want)
            worst = max(worst, err)
            assert err <= CONV_RTOL, (cin, cout, k, s, T, bias, err)
    # other paddings and the raw conv (slope 1)
    x = rs.randn(1, 16, 777).astype(np.float32)
    w = rs.randn(32, 4, 9).astype(np.float32)
    for pad in (0, 1, 9):
        got = _native.grouped_conv1d(_t(x), _t(w), None, 9, 2, pad, 1.0)
        want = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), stride=2, padding=pad, groups=4)
        assert _rel(got, want) <= CONV_RTOL, pad
    print(f"grouped conv: worst error relative to the output's peak {worst:.2e}")


def test_grouped_conv_refuses_what_it_does_not_cover():
    x = _t(np.zeros((1, 6, 100)))
    with pytest.raises(_native.NativeError, match="grouped_conv1d"):
        _native.grouped_conv1d(x, _t(np.zeros((3, 4, 5))), None, 5, 1, 2)     # Cin = 6: not 4 channels per group
    x = _t(np.zeros((1, 8, 100)))
    with pytest.raises(_native.NativeError, match="grouped_conv1d"):
        _native.grouped_conv1d(x, _t(np.zeros((3, 4, 5))), None, 5, 1, 2)     # Cout = 3: not a multiple of 2 groups
    with pytest.raises(_native.NativeError, match="grouped_conv1d"):
        _native.grouped_conv1d(x, _t(np.zeros((4, 4, 161))), None, 161, 16, 80)   # beyond a block's shared memory
    with pytest.raises(_native.NativeError):
        _native.grouped_conv1d(x, _t(np.zeros((4, 4, 301))), None, 301, 1, 0)    # empty output


def test_dense_discriminator_shapes_through_conv1d_fused():
    """Cin 1 -> 16 k15 reflect, 1025 / 513 / 257 -> 64 k15 reflect, 1024 -> 1024 k5, 1024 -> 1 k3."""
    rs = np.random.RandomState(2)
    worst = 0.0
    for cin, cout, k, mode, T, slope in [(1, 16, 15, _native.PAD_REFLECT, 24001, 0.2),
                                         (1025, 64, 15, _native.PAD_REFLECT, 1001, 0.2),
                                         (513, 64, 15, _native.PAD_REFLECT, 2001, 0.2),
                                         (257, 64, 15, _native.PAD_REFLECT, 4801, 0.2),
                                         (1025, 64, 15, _native.PAD_REFLECT, 8, 0.2),
                                         (1024, 1024, 5, _native.PAD_ZERO, 939, 0.2),
                                         (1024, 1024, 5, _native.PAD_ZERO, 17, 0.2),
                                         (1024, 1, 3, _native.PAD_ZERO, 939, 1.0)]:
        x = np.abs(rs.randn(2, cin, T)).astype(np.float32) if cin > 1 else rs.randn(2, 1, T).astype(np.float32)
        w = (rs.randn(cout, cin, k) / np.sqrt(cin * k)).astype(np.float32)
        b = rs.randn(cout).astype(np.float32)
        pad = (k - 1) // 2
        got = _native.conv1d_fused(_t(x), _native.pack_conv1d(_t(w)), _t(b), cout, k, pad=pad, pad_mode=mode,
                                   act_slope=slope)
        xd = torch.from_numpy(x).double()
        xd = F.pad(xd, (pad, pad), mode="reflect") if mode == _native.PAD_REFLECT else F.pad(xd, (pad, pad))
        want = F.leaky_relu(F.conv1d(xd, torch.from_numpy(w).double(), torch.from_numpy(b).double()), slope)
        err = _rel(got, want)
        worst = max(worst, err)
        assert err <= DENSE_RTOL, (cin, cout, k, T, err)
    print(f"dense shapes: worst error relative to the output's peak {worst:.2e}")


def test_avg_pool_against_the_oracle():
    rs = np.random.RandomState(3)
    for T in (1, 2, 3, 4, 5, 8, 1000, 1001, 24001, 24000):
        for k, s, p in ((4, 2, 1), (4, 2, 2), (3, 1, 1), (5, 3, 0), (1, 1, 0)):
            if T + 2 * p < k:
                continue
            x = rs.randn(3, 1, T).astype(np.float32)
            got = _native.avg_pool1d(_t(x), k, s, p)
            want = ref.avg_pool(torch.from_numpy(x).double(), k, s, p)
            assert _rel(got, want) <= POOL_RTOL, (T, k, s, p)
            tw = F.avg_pool1d(_t(x), k, s, p, count_include_pad=False)
            assert got.shape == tw.shape


def test_bins_major_magnitude_is_the_transpose_bit_for_bit():
    rs = np.random.RandomState(4)
    for nf, hop, wl in ref.MFD_RESOLUTIONS + ((512, 1, 7), (1024, 77, 1024)):
        for n in (nf // 2 + 1, 1680, 6007, 24000):
            x = _t(rs.uniform(-1, 1, (3, n)))
            tab = stft_tables(_dev(), nf, wl)
            bins = _native.stft_magnitude_bins(x, tab, nf, hop, wl)
            frames = stft(x, nf, hop, wl, "hann_window")
            assert bins.shape == (3, nf // 2 + 1, 1 + n // hop)
            assert torch.equal(bins, frames.transpose(1, 2)), (nf, hop, n)


def _flat(outs):
    return [m for lst in outs for m in lst]


def _check_maps(got_lists, want_lists, what):
    """Every map's worst error relative to the larger of its own peak and its input's (the previous map's) peak: a
    score map of one or two values can sit near zero while its inputs are O(1)."""
    assert [len(a) for a in got_lists] == [len(b) for b in want_lists], what
    worst = 0.0
    for i, (gl, wl) in enumerate(zip(got_lists, want_lists)):
        for j, (g, w) in enumerate(zip(gl, wl)):
            scale = max(float(w.abs().max()), float(wl[j - 1].abs().max()) if j else 0.0)
            err = float((g.detach().cpu().double() - w).abs().max()) / scale
            worst = max(worst, err)
            assert err <= MAP_RTOL, (what, i, j, tuple(g.shape), err)
    return worst


def test_small_configs_match_the_oracle_and_the_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "discriminator.npz"))
    sd = seeded_discriminator_state_dict("msd", SEEDS["small_msd"], **SMALL_MSD)
    msd = _load(MelGANMultiScaleDiscriminator(**SMALL_MSD), sd)
    kw = dict(SMALL_MSD, downsample_scales=tuple(SMALL_MSD["downsample_scales"]))
    worst = 0.0
    with torch.no_grad():
        out = msd(_t(g["small_x"]))
        for i, lst in enumerate(out):
            for j, m in enumerate(lst):
                assert _rel(m, g[f"msd_{i}_{j}"]) <= GOLDEN_RTOL, (i, j)
        for n in (32, 33, 101, 2001):
            x = np.random.RandomState(n).uniform(-1, 1, (3, 1, n)).astype(np.float32)
            worst = max(worst, _check_maps(msd(_t(x)), ref.msd(torch.from_numpy(x).double(), sd, **kw), ("msd", n)))
            one = MelGANDiscriminator(**SMALL_MSD)
            one.apply_weight_norm()
            one = _load(one, {k[len("discriminators.1."):]: v for k, v in sd.items()
                              if k.startswith("discriminators.1.")})
            want = ref.melgan(torch.from_numpy(x).double(), sd, "discriminators.1", **kw)
            worst = max(worst, _check_maps([one(_t(x))], [want], ("melgan", n)))
        sd = seeded_discriminator_state_dict("stft", SEEDS["small_stft"], **SMALL_STFT)
        sdisc = _load(STFTDiscriminator(**SMALL_STFT), sd)
        for j, m in enumerate(sdisc(_t(g["small_x"][:, 0]))):
            assert _rel(m, g[f"stft_{j}"]) <= GOLDEN_RTOL, j
        for n in (350, 351, 2001, 9999):
            x = np.random.RandomState(n).uniform(-1, 1, (3, n)).astype(np.float32)
            worst = max(worst, _check_maps([sdisc(_t(x))], [ref.stft_disc(x.astype(np.float64), sd, "", **SMALL_STFT)],
                                           ("stft", n)))
    print(f"small configurations: worst map error {worst:.2e}")


@pytest.mark.parametrize("B,n", [(1, 1680), (3, 1680), (1, 6007), (3, 4001), (2, 24000)])
def test_every_feature_map_matches_the_oracle(B, n):
    sd = seeded_discriminator_state_dict("discriminator", SEEDS["full"])
    d = _load(Discriminator(), sd)
    x = (0.5 * np.random.RandomState(B * n).randn(B, 1, n)).astype(np.float32)
    with torch.no_grad():
        got = d(_t(x))
        want = ref.discriminator(x.astype(np.float64), sd)
        worst = _check_maps(got, want, ("Discriminator", B, n))
        # the weight-norm-free module computes the same
        d.remove_weight_norm()
        assert not any(k.endswith("weight_g") for k in d.state_dict())
        worst = max(worst, _check_maps(d(_t(x)), want, ("removed weight norm", B, n)))
        # the sub-modules alone
        worst = max(worst, _check_maps(d.msd(_t(x)), want[:3], "msd"))
        worst = max(worst, _check_maps(d.mfd(_t(x)), want[3:], "mfd"))
    print(f"Discriminator B={B} n={n}: worst map error {worst:.2e}")


def test_the_full_discriminator_meets_the_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "discriminator.npz"))
    d = _load(Discriminator(), seeded_discriminator_state_dict("discriminator", SEEDS["full"]))
    with torch.no_grad():
        maps = _flat(d(_t(g["full_x"])))
        assert len(maps) == 36
        for i, m in enumerate(maps):
            v = m.double()
            assert abs(float(v.sum()) - g["full_sum"][i]) <= 1e-5 * g["full_abs"][i], i
            flat = m.flatten().cpu().numpy()
            idx = np.unique(np.linspace(0, flat.size - 1, 64).astype(np.int64))
            assert _rel(flat[idx], g["full_samples"][i][:idx.size]) <= GOLDEN_RTOL, i
        est_p, p = d(_t(g["est"])), d(_t(g["real"]))
        terms = discriminator_terms(est_p, p)
    names = ("adversarial", "feature_map", "real", "fake", "discriminator")
    for k, want in zip(names, g["scores"]):
        assert abs(float(terms[k]) - want) <= GOLDEN_RTOL * abs(want), (k, float(terms[k]), want)


def test_scores_match_the_oracle_per_batch_and_per_utterance():
    sd = seeded_discriminator_state_dict("discriminator", SEEDS["full"])
    d = _load(Discriminator(), sd)
    rs = np.random.RandomState(9)
    real = (0.3 * rs.randn(3, 1, 5003)).astype(np.float32)
    est = (real + 0.05 * rs.randn(*real.shape)).astype(np.float32)
    with torch.no_grad():
        est_p, p = d(_t(est)), d(_t(real))
        terms = discriminator_terms(est_p, p)
        per = discriminator_terms(est_p, p, per_utterance=True)
        again = discriminator_terms(est_p, p)
    want_e, want_r = ref.discriminator(est.astype(np.float64), sd), ref.discriminator(real.astype(np.float64), sd)
    want = ref.scores(want_e, want_r)
    worst = 0.0
    for k, v in want.items():
        err = abs(float(terms[k]) - v) / abs(v)
        worst = max(worst, err)
        assert err <= SCORE_RTOL, (k, float(terms[k]), v)
        assert torch.equal(terms[k], again[k])
        assert per[k].shape == (3,)
    for b in range(3):
        one = ref.scores([[m[b:b + 1] for m in lst] for lst in want_e], [[m[b:b + 1] for m in lst] for lst in want_r])
        for k, v in one.items():
            assert abs(float(per[k][b]) - v) <= SCORE_RTOL * abs(v), (k, b)
    print(f"scores: worst relative error {worst:.2e}")


def test_repeated_calls_are_bit_identical_and_rows_are_batch_invariant():
    d = _load(Discriminator(), seeded_discriminator_state_dict("discriminator", 5))
    rs = np.random.RandomState(10)
    x = _t(0.4 * rs.randn(3, 1, 7001))
    y = _t(0.4 * rs.randn(3, 1, 7001))
    with torch.no_grad():
        a, b = _flat(d(x)), _flat(d(x))
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        for r in range(3):
            one = _flat(d(x[r:r + 1].contiguous()))
            assert all(torch.equal(u[r:r + 1], v) for u, v in zip(a, one)), r
        ep, p = d(x), d(y)
        s3 = _native.disc_score_sums(_flat(ep), _flat(p))
        assert torch.equal(s3, _native.disc_score_sums(_flat(ep), _flat(p)))
        for r in range(3):
            s1 = _native.disc_score_sums([m[r:r + 1].contiguous() for m in _flat(ep)],
                                         [m[r:r + 1].contiguous() for m in _flat(p)])
            assert torch.equal(s1[:, 0], s3[:, r]), r
        pooled = _native.avg_pool1d(x, 4, 2, 1)
        assert torch.equal(pooled[1:2], _native.avg_pool1d(x[1:2].contiguous(), 4, 2, 1))


def test_score_sums_against_float64():
    rs = np.random.RandomState(12)
    es = [rs.randn(2, c, t).astype(np.float32) for c, t in ((1, 1), (3, 4097), (16, 5000), (1, 70000))]
    rs_ = [rs.randn(*e.shape).astype(np.float32) for e in es]
    got = _native.disc_score_sums([_t(e) for e in es], [_t(r) for r in rs_]).cpu().numpy()
    for m, (e, r) in enumerate(zip(es, rs_)):
        e, r = e.astype(np.float64).reshape(2, -1), r.astype(np.float64).reshape(2, -1)
        want = np.stack([np.abs(e - r).sum(1), ((e - 1) ** 2).sum(1), (e ** 2).sum(1), ((r - 1) ** 2).sum(1)], 1)
        assert np.allclose(got[m], want, rtol=1e-6, atol=0), m


def test_bad_input_raises():
    d = _load(Discriminator(), seeded_discriminator_state_dict("discriminator", 6))
    with pytest.raises(ValueError, match="too short"):
        d(_t(np.zeros((1, 1, 1679))))
    with pytest.raises(ValueError, match="too short"):
        d.msd(_t(np.zeros((1, 1, 31))))
    with pytest.raises(ValueError):
        d(_t(np.zeros((1, 4000))))                      # rank 2
    with pytest.raises(ValueError):
        d(_t(np.zeros((1, 2, 4000))))                   # two channels
    x = _t(np.zeros((1, 1, 4000))).requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        d(x)
    with torch.no_grad():
        out = d(x)                                      # allowed under no_grad
        with pytest.raises(ValueError):
            discriminator_terms(out, out[:-1])
        with pytest.raises(_native.NativeError):
            discriminator_terms([[m.cpu() for m in lst] for lst in out], out)
    with pytest.raises(_native.NativeError):
        MultiResolutionSTFTDiscriminator()(_t(np.zeros((1, 1, 4000))))    # the module is still on the CPU


def test_mode_evaluation_with_discriminator(tmp_path):
    """MODE=evaluation --discriminator through the launcher on a seeded HiFi-GAN light checkpoint that carries a
    seeded 'discriminator': every eval-d number equals the library call on the same data; without the flag no eval-d
    line appears, and a checkpoint without a discriminator is refused with a clear message."""
    from fastvocoder_amd.bin.synthesize import Synthesizer
    rs = np.random.RandomState(29)
    save = str(tmp_path / "out")
    os.makedirs(save)
    names = []
    for i in range(2):
        n = 8000 + 3001 * i
        s = (0.5 * np.sin(2 * np.pi * (200 + 70 * i) * np.arange(n) / 24000) * 32767
             + rs.uniform(-2000, 2000, n)).astype(np.int16)
        p = str(tmp_path / f"utt{i}.wav")
        scipy.io.wavfile.write(p, 24000, s)
        names.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(p + "\n" for p in names))
    env = dict(os.environ)
    launcher = os.path.join(cases.ROOT, "bin", "launcher.py")
    r = subprocess.run([sys.executable, launcher, "--data_path", str(lst), "--save_path", save, "--audio_index_path",
                        str(tmp_path / "audio"), "--mel_index_path", str(tmp_path / "mel")],
                       env=dict(env, MODE="preprocess"), cwd=cases.ROOT, capture_output=True, text=True, timeout=600)
    assert "min length of mel spectrogram" in r.stdout, r.stdout + r.stderr
    audio_idx, mel_idx = tmp_path / "eval_audio", tmp_path / "eval_mel"
    audio_idx.write_text("".join(os.path.join(save, os.path.basename(p) + ".npy\n") for p in names))
    mel_idx.write_text("".join(os.path.join(save, os.path.basename(p) + ".mel.npy\n") for p in names))
    conf = os.path.join(cases.ROOT, "conf", "hifigan", "light.yaml")
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    model = {k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=3).items()}
    disc = {k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("discriminator", 8).items()}
    ck, ck_bare = str(tmp_path / "ck.pth.tar"), str(tmp_path / "bare.pth.tar")
    torch.save({"model": model, "discriminator": disc}, ck)
    torch.save({"model": model}, ck_bare)
    args = ["--audio_index_path", str(audio_idx), "--mel_index_path", str(mel_idx), "--config", conf,
            "--model_name", "hifigan", "--num", "2"]

    def run(*extra):
        return subprocess.run([sys.executable, launcher, *extra, *args], env=dict(env, MODE="evaluation"),
                              cwd=cases.ROOT, capture_output=True, text=True, timeout=600)

    r = run("--checkpoint_path", ck, "--discriminator")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^eval-d (\d+) adv=(\S+) fm=(\S+) real=(\S+) fake=(\S+) d=(\S+)$", r.stdout, re.M)
    mean = re.findall(r"^eval-d mean utterances=2 adv=(\S+) fm=(\S+) d=(\S+)$", r.stdout, re.M)
    assert len(lines) == 2 and len(mean) == 1, r.stdout
    assert len(re.findall(r"^eval \d+ ", r.stdout, re.M)) == 2

    plain = run("--checkpoint_path", ck)
    assert plain.returncode == 0 and "eval-d" not in plain.stdout, plain.stdout + plain.stderr
    assert [ln for ln in r.stdout.splitlines() if not ln.startswith("eval-d")] == plain.stdout.splitlines()

    bare = run("--checkpoint_path", ck_bare, "--discriminator")
    assert bare.returncode != 0 and "'discriminator' entry" in bare.stdout + bare.stderr

    synth = Synthesizer(ck, conf, "hifigan")
    d = _load(Discriminator(), {k: v.numpy() for k, v in disc.items()})
    rows = []
    for i, p in enumerate(names):
        wav = np.load(os.path.join(save, os.path.basename(p) + ".npy"))
        mel = np.load(os.path.join(save, os.path.basename(p) + ".mel.npy"))
        est = synth.synthesize(mel.T)[0]
        m = min(est.shape[0], wav.shape[0])
        with torch.no_grad():
            t = discriminator_terms(d(est[None, None, :m].contiguous()), d(_t(wav[None, None, :m])))
        want = [f"{float(t[k]):.8e}" for k in ("adversarial", "feature_map", "real", "fake", "discriminator")]
        assert list(lines[i][1:]) == want and int(lines[i][0]) == i, (i, lines[i], want)
        rows.append([float(t[k]) for k in ("adversarial", "feature_map", "discriminator")])
    rows = np.array(rows)
    assert mean[0] == tuple(f"{v:.8e}" for v in rows.mean(axis=0))
