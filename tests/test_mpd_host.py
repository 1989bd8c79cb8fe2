"""Host tests of the multi-period discriminator (fastvocoder_amd.discriminator.mpd): the float64 oracle
tests/mpd_reference.py against the reference's values (tests/golden/mpd.npz), the pad / height / minimum-length
arithmetic, the modules' keys and shapes, the evaluation flow's choice of class, and the health of the fixture."""
import os

import numpy as np
import pytest
import torch

from fastvocoder_amd import _native
from fastvocoder_amd.bin.evaluation import discriminator_uses_mpd
from fastvocoder_amd.discriminator import Discriminator, DiscriminatorP, MultiPeriodDiscriminator
from fastvocoder_amd.discriminator.mpd import period_heights
from fastvocoder_amd.synthetic import discriminator_spec, seeded_discriminator_state_dict
from tests import discriminator_reference as dref
from tests import mpd_reference as ref

SEEDS = {"mpd": 21, "discriminator": 22}
GOLDEN_RTOL = 1e-6       # the oracle (float64) against the reference's float32 CPU values, relative to the peak compared


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mpd.npz"))


def _strided(n, count=64):
    return np.unique(np.linspace(0, n - 1, count).astype(np.int64))


def _shapes(keys, shapes):
    return {str(k): tuple(int(d) for d in s if d >= 0) for k, s in zip(keys, shapes)}


def test_oracle_meets_the_reference(golden):
    sd = seeded_discriminator_state_dict("mpd", SEEDS["mpd"])
    outs = ref.mpd(golden["x"], sd)
    assert [len(lst) for lst in outs] == [7] * 5
    maps = [m for lst in outs for m in lst]
    assert len(maps) == 35
    for i, m in enumerate(maps):
        assert m.shape == tuple(int(d) for d in golden["map_shapes"][i] if d >= 0), i
        flat = m.reshape(-1)
        assert abs(flat.sum() - golden["map_sum"][i]) <= 1e-6 * golden["map_abs"][i], i
        assert abs(np.abs(flat).sum() - golden["map_abs"][i]) <= 1e-6 * golden["map_abs"][i], i
        idx = _strided(flat.size)
        want = golden["map_samples"][i][:idx.size].astype(np.float64)
        err = np.abs(flat[idx] - want).max() / np.abs(want).max()
        assert err <= GOLDEN_RTOL, (i, err)


def test_oracle_scores_meet_the_reference(golden):
    sd = seeded_discriminator_state_dict("discriminator", SEEDS["discriminator"], use_mpd=True)
    est_p = ref.discriminator_with_mpd(golden["est"].astype(np.float64), sd)
    p = ref.discriminator_with_mpd(golden["real"].astype(np.float64), sd)
    assert [len(lst) for lst in est_p] == [7] * 8 + [5] * 3 and sum(len(lst) for lst in est_p) == 71
    got = dref.scores(est_p, p)
    want = dict(zip(("adversarial", "feature_map", "real", "fake", "discriminator"), golden["scores"]))
    for k, v in got.items():
        assert abs(v - want[k]) <= GOLDEN_RTOL * abs(want[k]), (k, v, want[k])


def test_fixture_maps_are_alive(golden):
    """Every golden map's standard deviation within [1e-2, 1e2] times the input's: no map of the compared network is
    dead or exploding."""
    x_std = float(golden["x"].astype(np.float64).std())
    ratio = golden["map_std"] / x_std
    assert ratio.shape == (35,)
    assert (ratio >= 1e-2).all() and (ratio <= 1e2).all(), ratio


def test_pad_height_and_minimum_length_arithmetic():
    need = ref.min_length()
    assert need == 6                                       # period 11: the tail 11 - T must be shorter than T
    assert MultiPeriodDiscriminator().min_length() == need
    assert [DiscriminatorP(p).min_length() for p in ref.PERIODS] == [ref.min_length((p,)) for p in ref.PERIODS] \
        == [2, 2, 3, 4, 6]
    assert Discriminator(use_mpd=True).min_length() == Discriminator().min_length() == 1680
    for T in (need, need - 1, 2310, 2311):
        for p in ref.PERIODS:
            n_pad = ref.reflect_tail(T, p)
            assert n_pad == (-T) % p and _native.mpd_reflect_tail(T, p) == n_pad
            if T == need - 1 and p == 11:
                assert n_pad >= T
                with pytest.raises(ValueError):
                    ref.view(np.zeros((1, 1, T)), p)
                continue
            assert n_pad < T
            x = np.arange(T, dtype=np.float64).reshape(1, 1, T)
            v = ref.view(x, p)
            hs = ref.heights(T, p)
            assert v.shape == (1, 1, hs[0], p) and hs[0] * p == T + n_pad
            flat = v.reshape(-1)
            assert (flat[:T] == x.reshape(-1)).all()
            assert (flat[T:] == T - 2 - np.arange(n_pad)).all()     # index T + i reads x[T - 2 - i]
            for a, b in zip(hs[:4], hs[1:5]):
                assert b == (a - 1) // 3 + 1
            assert hs[5] == hs[4] and hs[6] == hs[4]
            assert period_heights(T, p) == (n_pad, hs[:5])
    assert [ref.reflect_tail(2310, p) for p in ref.PERIODS] == [0] * 5
    assert [ref.reflect_tail(2311, p) for p in ref.PERIODS] == [p - 1 for p in ref.PERIODS]


def test_module_keys_and_shapes_match_the_reference(golden):
    want = _shapes(golden["keys"], golden["shapes"])
    got = {k: tuple(v.shape) for k, v in MultiPeriodDiscriminator().state_dict().items()}
    assert got == want and list(got) == [str(k) for k in golden["keys"]]
    assert {k: s for k, s, _ in discriminator_spec("mpd")} == want
    assert want["discriminators.4.convs.3.weight_v"] == (1024, 512, 5, 1)
    assert want["discriminators.0.conv_post.weight_g"] == (1, 1, 1, 1)
    d_want = _shapes(golden["d_keys"], golden["d_shapes"])
    d_got = {k: tuple(v.shape) for k, v in Discriminator(use_mpd=True).state_dict().items()}
    assert d_got == d_want and list(d_got) == [str(k) for k in golden["d_keys"]]
    assert {k: s for k, s, _ in discriminator_spec("discriminator", use_mpd=True)} == d_want
    sd = seeded_discriminator_state_dict("discriminator", 3, use_mpd=True)
    Discriminator(use_mpd=True).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


def test_default_discriminator_is_unchanged(golden_dir):
    g = np.load(os.path.join(golden_dir, "discriminator.npz"))
    want = {str(k): tuple(int(d) for d in s if d >= 0) for k, s in zip(g["keys"], g["shapes"])}
    d = Discriminator()
    got = {k: tuple(v.shape) for k, v in d.state_dict().items()}
    assert got == want and list(got) == [str(k) for k in g["keys"]]
    assert not hasattr(d, "mpd") and not any(k.startswith("mpd.") for k in got)
    assert [k for k, _, _ in discriminator_spec()] == list(got)
    with_mpd = Discriminator(use_mpd=True).state_dict()
    assert [k for k in with_mpd if not k.startswith("mpd.")] == list(got)


def test_evaluation_picks_the_class_from_the_keys():
    plain = [k for k, _, _ in discriminator_spec()]
    full = [k for k, _, _ in discriminator_spec("discriminator", use_mpd=True)]
    assert not discriminator_uses_mpd(dict.fromkeys(plain))
    assert discriminator_uses_mpd(dict.fromkeys(full))
    assert not discriminator_uses_mpd({"msd.mpd.x": 0, "mfd.stft_discriminator.0.window": 0})


def test_refusals_on_the_host():
    with pytest.raises(NotImplementedError, match="spectral"):
        DiscriminatorP(3, use_spectral_norm=True)
    with pytest.raises(NotImplementedError):
        DiscriminatorP(4)
    with pytest.raises(NotImplementedError):
        DiscriminatorP(3, kernel_size=7)
    with pytest.raises(_native.NativeError):
        MultiPeriodDiscriminator()(torch.zeros(1, 1, 4000))            # a CPU tensor
    assert "mpd.hip" in _native.SOURCES and _native.ABI_VERSION == 18
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "fastvocoder_hip.h")).read()
    for name in ("fv_mpd_conv_first", "fv_period_conv", "fv_pack_period_conv", "fv_packed_period_conv_floats"):
        assert f"{name}(" in header
