"""GPU tests of the multi-period discriminator (csrc/mpd.hip: fv_mpd_conv_first, fv_period_conv,
fv_pack_period_conv; fastvocoder_amd.discriminator.mpd; Discriminator(use_mpd=True)) against the float64 oracle
tests/mpd_reference.py and the reference's values (tests/golden/mpd.npz), and of MODE=evaluation --discriminator on
a checkpoint with ``mpd.`` keys.

Worst errors on MI355X, relative to the peak of the map compared: not recorded yet; the
tests print them (run with -s)."""
import os
import re

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.evaluation import run_evaluation
from fastvocoder_amd.discriminator import Discriminator, DiscriminatorP, MultiPeriodDiscriminator
from fastvocoder_amd.loss import discriminator_terms
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict, seeded_mel, seeded_state_dict
from tests import cases
from tests import discriminator_reference as dref
from tests import mpd_reference as ref

pytestmark = pytest.mark.gpu

SEEDS = {"mpd": 21, "discriminator": 22}
# against the float64 oracle, relative to the largest magnitude of the map compared
DENSE_RTOL = 2e-5        # one period conv alone: the project's bound for dense fp32-MFMA convs of K = 5120
MAP_RTOL = 2e-5          # every feature map of a forward
SCORE_RTOL = 7e-6        # the five scores, relative
# against the reference's float32 CPU values (the oracle meets them within 1e-6: tests/test_mpd_host.py)
GOLDEN_RTOL = 5e-5

TILE_N = 128             # flattened outputs per block of period_conv_kernel (csrc/mpd.hip kPN)


def _h_near_tile(p, past):
    """The smallest H' > TILE_N / p whose H' p flattened outputs end as little as possible past (or short of) a
    column-tile boundary: one output for the odd periods, one row of two for p = 2."""
    want = (1 if past else TILE_N - 1) if p % 2 else (2 if past else TILE_N - 2)
    return next(h for h in range(TILE_N // p + 1, 8 * TILE_N) if (h * p) % TILE_N == want)


def _lengths(p):
    """2310 (a multiple of every period: no tail), 2311 (the longest tails p - 1), a prime, and per period two T
    whose 32 -> 128 layer ends one output past / one short of a tile (H = 3 (3 H_2 - 2) - 2 rows, a tail of p - 1)."""
    out = [2310, 2311, 4099]
    for past in (True, False):
        h2 = _h_near_tile(p, past)
        out.append((3 * (3 * h2 - 2) - 2) * p - (p - 1))
    return out


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


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mpd.npz"))


@pytest.fixture(scope="module")
def mpd_sd():
    return seeded_discriminator_state_dict("mpd", SEEDS["mpd"])


@pytest.fixture(scope="module")
def mpd_module(mpd_sd):
    return _load(MultiPeriodDiscriminator(), mpd_sd)


@pytest.fixture(scope="module")
def full_sd():
    return seeded_discriminator_state_dict("discriminator", SEEDS["discriminator"], use_mpd=True)


@pytest.fixture(scope="module")
def full_module(full_sd):
    return _load(Discriminator(use_mpd=True), full_sd)


def test_tile_lengths_hit_the_boundary():
    for p in ref.PERIODS:
        past, short = _lengths(p)[3:]
        assert (ref.heights(past, p)[2] * p) % TILE_N == (1 if p % 2 else 2)
        assert (ref.heights(short, p)[2] * p) % TILE_N == TILE_N - (1 if p % 2 else 2)
        assert ref.reflect_tail(past, p) == p - 1 and ref.heights(past, p)[2] * p > TILE_N


@pytest.mark.parametrize("pi", range(5))
def test_each_new_kernel_alone_against_float64(pi, mpd_sd):
    """fv_mpd_conv_first and fv_period_conv (32 -> 128, 128 -> 512, 512 -> 1024), each fed the float32 rounding of the
    oracle's previous map and compared with the oracle's conv of that same input."""
    p = ref.PERIODS[pi]
    prefix = f"discriminators.{pi}"
    rs = np.random.RandomState(50 + p)
    folded = [ref.folded(mpd_sd, f"{prefix}.convs.{j}") for j in range(4)]
    packed = [_native.pack_period_conv(_t(w)) for w, _ in folded[1:]]
    worst = [0.0] * 4
    for T in _lengths(p):
        for B in (1, 3):
            x = (0.5 * rs.randn(B, 1, T)).astype(np.float32)
            w, b = folded[0]
            got = _native.mpd_conv_first(_t(x), _t(w.reshape(32, 5)), _t(b), p, 0.1)
            want = ref.conv_h(ref.view(x, p), w, b, 3, 0.1)
            err = _rel(got, want)
            worst[0] = max(worst[0], err)
            assert err <= DENSE_RTOL, ("first", p, T, B, err)
            for j in (1, 2, 3):
                xin = want.astype(np.float32)
                w, b = folded[j]
                got = _native.period_conv(_t(xin), packed[j - 1], _t(b), w.shape[0], 0.1)
                want = ref.conv_h(xin.astype(np.float64), w, b, 3, 0.1)
                err = _rel(got, want)
                worst[j] = max(worst[j], err)
                assert err <= DENSE_RTOL, (j, p, T, B, err)
    print(f"period {p}: worst error relative to the map's peak, layers 0-3: " + " ".join(f"{e:.2e}" for e in worst))


def test_period_conv_without_bias_and_raw(mpd_sd):
    rs = np.random.RandomState(7)
    w = (rs.randn(128, 32, 5) / np.sqrt(160)).astype(np.float32)
    x = rs.randn(2, 32, 130, 3).astype(np.float32)
    got = _native.period_conv(_t(x), _native.pack_period_conv(_t(w)), None, 128, 1.0)
    want = ref.conv_h(x.astype(np.float64), w.astype(np.float64), np.zeros(128), 3, None)
    assert _rel(got, want) <= DENSE_RTOL


def test_whole_forward_against_oracle_and_golden(golden, mpd_sd, mpd_module):
    x = golden["x"]
    with torch.no_grad():
        outs = mpd_module(_t(x))
    want = ref.mpd(x.astype(np.float64), mpd_sd)
    assert len(outs) == 5 and [len(lst) for lst in outs] == [7] * 5
    worst_o = worst_g = 0.0
    i = 0
    for lst, wlst in zip(outs, want):
        for m, wm in zip(lst, wlst):
            assert tuple(m.shape) == wm.shape == tuple(int(d) for d in golden["map_shapes"][i] if d >= 0), i
            assert m.is_cuda and m.dtype == torch.float32
            err = _rel(m, wm)
            worst_o = max(worst_o, err)
            assert err <= MAP_RTOL, (i, err)
            flat = m.flatten().double().cpu().numpy()
            idx = np.unique(np.linspace(0, flat.size - 1, 64).astype(np.int64))
            g = golden["map_samples"][i][:idx.size].astype(np.float64)
            gerr = float(np.abs(flat[idx] - g).max() / np.abs(g).max())
            worst_g = max(worst_g, gerr)
            assert gerr <= GOLDEN_RTOL, (i, gerr)
            assert abs(flat.sum() - golden["map_sum"][i]) <= 1e-5 * golden["map_abs"][i], i
            i += 1
        assert torch.equal(lst[6], lst[5].flatten(1).unsqueeze(1))
    assert i == 35
    print(f"MPD forward: worst error against the oracle {worst_o:.2e}, against the reference's values {worst_g:.2e}")


def test_scores_with_mpd(golden, full_sd, full_module):
    est, real = golden["est"], golden["real"]
    with torch.no_grad():
        est_p, p = full_module(_t(est)), full_module(_t(real))
        assert len(est_p) == 11 and sum(len(lst) for lst in est_p) == 71
        got = {k: float(v) for k, v in discriminator_terms(est_p, p).items()}
        per = {k: v.double().cpu().numpy() for k, v in discriminator_terms(est_p, p, per_utterance=True).items()}
    want = dict(zip(("adversarial", "feature_map", "real", "fake", "discriminator"), golden["scores"]))
    for k, v in got.items():
        assert abs(v - want[k]) <= GOLDEN_RTOL * abs(want[k]), (k, v, want[k])
    worst = 0.0
    for b in range(est.shape[0]):
        o = dref.scores(ref.discriminator_with_mpd(est[b:b + 1].astype(np.float64), full_sd),
                        ref.discriminator_with_mpd(real[b:b + 1].astype(np.float64), full_sd))
        for k, v in o.items():
            err = abs(per[k][b] - v) / abs(v)
            worst = max(worst, err)
            assert err <= SCORE_RTOL, (k, b, per[k][b], v)
    print(f"scores with the MPD: worst relative error of a per-utterance score {worst:.2e}")


def test_default_discriminator_outputs_do_not_depend_on_the_mpd(full_module, full_sd):
    """Discriminator() on the msd / mfd weights gives the last 6 lists of Discriminator(use_mpd=True), bit for bit."""
    plain = _load(Discriminator(), {k: v for k, v in full_sd.items() if not k.startswith("mpd.")})
    x = _t(0.3 * np.random.RandomState(3).randn(2, 1, 2311))
    with torch.no_grad():
        a, b = plain(x), full_module(x)
    assert len(a) == 6 and len(b) == 11
    for la, lb in zip(a, b[5:]):
        assert len(la) == len(lb) and all(torch.equal(u, v) for u, v in zip(la, lb))


def test_rows_do_not_depend_on_the_batch(mpd_module):
    x = _t(0.5 * np.random.RandomState(5).randn(3, 1, 2311))
    with torch.no_grad():
        three, one = mpd_module(x), mpd_module(x[:1].contiguous())
    for l3, l1 in zip(three, one):
        for m3, m1 in zip(l3, l1):
            assert torch.equal(m3[:1], m1)


def test_refusals(mpd_module):
    need = mpd_module.min_length()
    with pytest.raises(ValueError, match=f"at least {need} samples"):
        mpd_module(_t(np.zeros((1, 1, need - 1))))
    with torch.no_grad():
        assert [tuple(lst[-1].shape) for lst in mpd_module(_t(np.ones((1, 1, need))))] == \
            [(1, 1, ref.heights(need, p)[6] * p) for p in ref.PERIODS]
    with pytest.raises(_native.NativeError):
        mpd_module(torch.zeros(1, 1, 4000))                             # a CPU tensor
    with pytest.raises(NotImplementedError, match="spectral"):
        DiscriminatorP(2, use_spectral_norm=True)
    # unsupported shapes at the ABI: a return code, checked before anything else (nothing is launched)
    L = _native.lib()
    assert L.fv_period_conv(None, None, None, None, 1, 32, 128, 10, 4, 0.1, None) == _native.ERR_UNSUPPORTED
    assert L.fv_period_conv(None, None, None, None, 1, 64, 128, 10, 3, 0.1, None) == _native.ERR_UNSUPPORTED
    assert L.fv_period_conv(None, None, None, None, 1, 32, 96, 10, 3, 0.1, None) == _native.ERR_UNSUPPORTED
    assert L.fv_mpd_conv_first(None, None, None, None, 1, 100, 13, 0.1, None) == _native.ERR_UNSUPPORTED
    assert L.fv_pack_period_conv(None, None, 128, 48, None) == _native.ERR_UNSUPPORTED
    assert L.fv_packed_period_conv_floats(128, 48) == 0 and L.fv_packed_period_conv_floats(1024, 512) == 1024 * 512 * 5
    assert L.fv_period_conv(None, None, None, None, 1, 32, 128, 10, 3, 0.1, None) == _native.ERR_INVALID_ARG
    assert L.fv_version() == 18


def test_mode_evaluation_with_mpd_keys(tmp_path, capsys, full_sd, full_module):
    """MODE=evaluation --discriminator on a checkpoint whose 'discriminator' carries mpd.* keys prints eval-d lines
    equal to discriminator_terms through Discriminator(use_mpd=True); on one without them, through Discriminator()."""
    from fastvocoder_amd.bin.synthesize import Synthesizer
    rs = np.random.RandomState(9)
    conf = os.path.join(cases.ROOT, "conf", "hifigan", "light.yaml")
    cfg = cases.load_conf("conf/hifigan/light.yaml")
    model = {k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", cfg, seed=3).items()}
    audio, mels = [], []
    for i in range(2):
        mel = seeded_mel(20 + 3 * i, seed=i)                            # [T, 80]
        np.save(str(tmp_path / f"u{i}.mel.npy"), np.ascontiguousarray(mel.T))
        np.save(str(tmp_path / f"u{i}.npy"), (0.3 * rs.randn(mel.shape[0] * 240 - 37)).astype(np.float32))
        audio.append(str(tmp_path / f"u{i}.npy"))
        mels.append(str(tmp_path / f"u{i}.mel.npy"))
    (tmp_path / "audio").write_text("".join(a + "\n" for a in audio))
    (tmp_path / "mel").write_text("".join(m + "\n" for m in mels))
    plain_sd = {k: v for k, v in full_sd.items() if not k.startswith("mpd.")}
    plain_module = _load(Discriminator(), plain_sd)
    for name, sd, module in (("mpd", full_sd, full_module), ("plain", plain_sd, plain_module)):
        ck = str(tmp_path / f"{name}.pth.tar")
        torch.save({"model": model, "discriminator": {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
        capsys.readouterr()
        run_evaluation(["--checkpoint_path", ck, "--audio_index_path", str(tmp_path / "audio"), "--mel_index_path",
                        str(tmp_path / "mel"), "--config", conf, "--model_name", "hifigan", "--num", "2",
                        "--discriminator"])
        out = capsys.readouterr().out
        lines = re.findall(r"^eval-d (\d+) adv=(\S+) fm=(\S+) real=(\S+) fake=(\S+) d=(\S+)$", out, re.M)
        mean = re.findall(r"^eval-d mean utterances=2 adv=(\S+) fm=(\S+) d=(\S+)$", out, re.M)
        assert len(lines) == 2 and len(mean) == 1, out
        synth = Synthesizer(ck, conf, "hifigan")
        rows = []
        for i in range(2):
            wav = np.load(audio[i])
            est = synth.synthesize(np.load(mels[i]).T)[0]
            m = min(est.shape[0], wav.shape[0])
            with torch.no_grad():
                t = discriminator_terms(module(est[None, None, :m].contiguous()), module(_t(wav[None, None, :m])))
            want = [f"{float(t[k]):.8e}" for k in ("adversarial", "feature_map", "real", "fake", "discriminator")]
            assert list(lines[i][1:]) == want and int(lines[i][0]) == i, (name, i, lines[i], want)
            rows.append([float(t[k]) for k in ("adversarial", "feature_map", "discriminator")])
        assert mean[0] == tuple(f"{v:.8e}" for v in np.array(rows).mean(axis=0)), name
