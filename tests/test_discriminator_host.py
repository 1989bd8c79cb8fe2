"""Host tests of the discriminators (fastvocoder_amd.discriminator, loss.discriminator_terms): the float64 oracle
tests/discriminator_reference.py against the reference's values (tests/golden/discriminator.npz), the modules' keys
and shapes, refused configurations and inputs, and the composition of the scores from their sums."""
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANDiscriminator,
                                           MelGANMultiScaleDiscriminator, MultiPeriodDiscriminator,
                                           MultiResolutionSTFTDiscriminator, STFTDiscriminator)
from fastvocoder_amd.discriminator.common import DiscriminatorModule, cached
from fastvocoder_amd.loss.discriminator_loss import compose_terms
from fastvocoder_amd.synthetic import discriminator_spec, seeded_discriminator_state_dict
from tests import discriminator_reference as ref

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_STFT = dict(fft_size=512, shift_size=50, win_length=240, channels=8, max_downsample_channels=64)
SEEDS = {"small_msd": 11, "small_stft": 12, "full": 13}
# the oracle (float64) against the reference's float32 CPU values, relative to each map's largest magnitude
GOLDEN_RTOL = 2e-5


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "discriminator.npz"))


def _strided(n, count=64):
    return np.unique(np.linspace(0, n - 1, count).astype(np.int64))


def _close(got, want, rtol=GOLDEN_RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
    assert err <= rtol, err


def test_oracle_meets_the_reference_small_configs(golden_dir):
    g = _golden(golden_dir)
    x = torch.from_numpy(g["small_x"]).double()
    sd = seeded_discriminator_state_dict("msd", SEEDS["small_msd"], **SMALL_MSD)
    kw = dict(SMALL_MSD, downsample_scales=tuple(SMALL_MSD["downsample_scales"]))
    for i, lst in enumerate(ref.msd(x, sd, **kw)):
        assert len(lst) == 5
        for j, m in enumerate(lst):
            _close(m.numpy(), g[f"msd_{i}_{j}"])
    sd = seeded_discriminator_state_dict("stft", SEEDS["small_stft"], **SMALL_STFT)
    outs = ref.stft_disc(x[:, 0], sd, "", **SMALL_STFT)
    assert len(outs) == 5
    for j, m in enumerate(outs):
        _close(m.numpy(), g[f"stft_{j}"])


def test_oracle_meets_the_reference_full_discriminator(golden_dir):
    g = _golden(golden_dir)
    sd = seeded_discriminator_state_dict("discriminator", SEEDS["full"])
    maps = [m for lst in ref.discriminator(g["full_x"].astype(np.float64), sd) for m in lst]
    assert len(maps) == 36
    for i, m in enumerate(maps):
        flat = m.flatten().numpy()
        assert abs(flat.sum() - g["full_sum"][i]) <= 1e-5 * g["full_abs"][i], i
        idx = _strided(flat.size)
        _close(flat[idx], g["full_samples"][i][:idx.size])
    est_p = ref.discriminator(g["est"].astype(np.float64), sd)
    p = ref.discriminator(g["real"].astype(np.float64), sd)
    s = ref.scores(est_p, p)
    want = dict(zip(("adversarial", "feature_map", "real", "fake", "discriminator"), g["scores"]))
    for k, v in s.items():
        assert abs(v - want[k]) <= 1e-5 * abs(want[k]), (k, v, want[k])


def test_module_keys_and_shapes_match_the_reference(golden_dir):
    g = _golden(golden_dir)
    want = {k: tuple(int(d) for d in s if d >= 0) for k, s in zip(g["keys"], g["shapes"])}
    got = {k: tuple(v.shape) for k, v in Discriminator().state_dict().items()}
    assert got == want
    assert {k: s for k, s, _ in discriminator_spec()} == want
    assert {k: tuple(v.shape) for k, v in MelGANMultiScaleDiscriminator(**SMALL_MSD).state_dict().items()} == \
        {k: s for k, s, _ in discriminator_spec("msd", **SMALL_MSD)}
    assert {k: tuple(v.shape) for k, v in STFTDiscriminator(**SMALL_STFT).state_dict().items()} == \
        {k: s for k, s, _ in discriminator_spec("stft", **SMALL_STFT)}
    bare = MelGANDiscriminator()
    assert {k: tuple(v.shape) for k, v in bare.state_dict().items()} == \
        {k: s for k, s, _ in discriminator_spec("melgan", weight_norm=False)}
    d = Discriminator()
    d.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict(seed=1).items()})
    w = d.mfd.stft_discriminator[0].window
    assert w.shape == (1200,) and torch.allclose(w, torch.hann_window(1200), rtol=0, atol=1e-6)


def test_minimum_lengths():
    assert Discriminator().min_length() == 1680           # the 2048/240 resolution: 8 frames
    assert MelGANMultiScaleDiscriminator().min_length() == 32   # the third scale: 8 samples after two pools
    assert MultiResolutionSTFTDiscriminator().min_length() == 1680
    assert STFTDiscriminator(fft_size=2048, shift_size=100, win_length=1200).min_length() == 1025
    assert MelGANDiscriminator().min_length() == 8


@pytest.mark.parametrize("ctor,kw", [
    (MelGANDiscriminator, dict(in_channels=2)),
    (MelGANDiscriminator, dict(out_channels=2)),
    (MelGANDiscriminator, dict(pad="ReplicationPad1d")),
    (MelGANDiscriminator, dict(nonlinear_activation="ReLU", nonlinear_activation_params={})),
    (MelGANDiscriminator, dict(channels=6)),
    (MelGANMultiScaleDiscriminator, dict(downsample_pooling="MaxPool1d",
                                         downsample_pooling_params={"kernel_size": 4})),
    (MelGANMultiScaleDiscriminator, dict(downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 1,
                                                                    "count_include_pad": True})),
    (STFTDiscriminator, dict(fft_size=4096, win_length=1200)),
    (STFTDiscriminator, dict(out_channels=3)),
    (STFTDiscriminator, dict(nonlinear_activation="PReLU", nonlinear_activation_params={})),
])
def test_unsupported_configurations_are_refused(ctor, kw):
    with pytest.raises(NotImplementedError):
        ctor(**kw)


def test_a_cpu_forward_raises():
    x = torch.zeros(1, 1, 4000)
    for m in (Discriminator(), MelGANMultiScaleDiscriminator(), MultiResolutionSTFTDiscriminator()):
        with pytest.raises(_native.NativeError):
            m(x)
    with pytest.raises(_native.NativeError):
        STFTDiscriminator()(torch.zeros(1, 4000))


def test_score_composition_matches_the_training_loop():
    """compose_terms on the sums of random maps == bin/train.py's formulas in numpy (the /36 divisor included:
    6 lists, the first with 7 maps, the MFD lists adding 4 feature-map terms each)."""
    rs = np.random.RandomState(3)
    B = 3
    lengths = [7, 7, 7, 5, 5, 5]
    est_p = [[rs.randn(B, rs.randint(1, 4), rs.randint(2, 9)) for _ in range(n)] for n in lengths]
    p = [[rs.randn(*m.shape) for m in lst] for lst in est_p]
    es, rs_ = [m for lst in est_p for m in lst], [m for lst in p for m in lst]
    sums = np.stack([np.stack([np.abs(e - r).reshape(B, -1).sum(1), ((e - 1) ** 2).reshape(B, -1).sum(1),
                               (e ** 2).reshape(B, -1).sum(1), ((r - 1) ** 2).reshape(B, -1).sum(1)], 1)
                     for e, r in zip(es, rs_)])
    counts = [e[0].size for e in es]

    def train_py(est_p, p):
        adv = sum(((e[-1] - 1) ** 2).mean() for e in est_p) / len(est_p)
        fm = sum(np.abs(est_p[i][j] - p[i][j]).mean() for i in range(len(est_p)) for j in range(len(est_p[i]) - 1))
        fm /= float(len(est_p)) * float(len(est_p[0]) - 1)
        real = sum(((r[-1] - 1) ** 2).mean() for r in p) / len(p)
        fake = sum((e[-1] ** 2).mean() for e in est_p) / len(p)
        return {"adversarial": adv, "feature_map": fm, "real": real, "fake": fake, "discriminator": real + fake}

    assert len(est_p) * (len(est_p[0]) - 1) == 36
    got = compose_terms(torch.from_numpy(sums), counts, lengths)
    for k, v in train_py(est_p, p).items():
        assert abs(float(got[k]) - v) <= 1e-12 * max(1.0, abs(v)), k
    per = compose_terms(torch.from_numpy(sums), counts, lengths, per_utterance=True)
    for b in range(B):
        one = train_py([[m[b:b + 1] for m in lst] for lst in est_p], [[m[b:b + 1] for m in lst] for lst in p])
        for k, v in one.items():
            assert abs(float(per[k][b]) - v) <= 1e-12 * max(1.0, abs(v)), (k, b)


def test_cached_follows_the_module_state():
    """common.cached: one build for calls in a row, a new one after an in-place update of a parameter and after
    load_state_dict, one entry per key; the build runs under torch.no_grad()."""
    m = MelGANDiscriminator(**SMALL_MSD)
    m._device = lambda: torch.device("cpu")              # the builds below launch nothing
    builds = []

    def build():
        builds.append(torch.is_grad_enabled())
        return len(builds)

    assert cached(m, "a", build) == 1 and cached(m, "a", build) == 1 and builds == [False]
    with torch.no_grad():
        next(m.parameters()).mul_(1.5)
    assert cached(m, "a", build) == 2 and cached(m, "a", build) == 2
    m.load_state_dict(m.state_dict())
    assert cached(m, "a", build) == 3 and cached(m, "a", build) == 3
    assert cached(m, "b", build) == 4
    assert cached(m, "a", build) == 3 and cached(m, "b", build) == 4 and len(builds) == 4


def test_every_discriminator_takes_the_shared_forward_and_graph_forward():
    """One ``_forward(x, graph)`` per module: ``forward`` and ``_graph_forward`` are DiscriminatorModule's."""
    for cls in (MelGANDiscriminator, MelGANMultiScaleDiscriminator, STFTDiscriminator,
                MultiResolutionSTFTDiscriminator, DiscriminatorP, MultiPeriodDiscriminator, Discriminator):
        assert cls.forward is DiscriminatorModule.forward, cls
        assert cls._graph_forward is DiscriminatorModule._graph_forward, cls
        assert "_forward" in vars(cls), cls
