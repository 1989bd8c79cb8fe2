"""Writes tests/golden/mpd.npz: the reference's multi-period discriminator (model/discriminator/mpd.py, the second
MultiPeriodDiscriminator, :288) run by torch on the CPU in float32, on the seeded weights of fastvocoder_amd.synthetic
(seeded_discriminator_state_dict("mpd") and ("discriminator", use_mpd=True): 41 M parameters, regenerated on any
box, never stored).  Run once against a checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_mpd_golden.py /path/to/FastVocoder

Contents:
  keys, shapes          MultiPeriodDiscriminator().state_dict(): key names and shapes (padded with -1 to rank 4)
  d_keys, d_shapes      the same for Discriminator with the reference's two mpd lines enabled (discriminator.py:11, 16)
  x                     [2, 1, 4099] float32 input
  map_shapes            [35, 4] the shape of every map of mpd(x) in flattened list order (scores padded with -1)
  map_sum, map_abs      [35] float64 sum and sum of |v| of every map
  map_std               [35] float64 standard deviation of every map
  map_samples           [35, 64] float32 every map's flattened values at strided_samples(n) positions
  est, real             [2, 1, 3001] float32 the scored pair
  scores                [5] float64 adversarial, feature_map, real, fake, discriminator of D(est), D(real) with
                        D = mpd + msd + mfd (11 lists, feature-map divisor 11 * 6)
The fixture is data only; no test reads the reference tree."""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True

import numpy as np
import scipy.signal
import scipy.signal.windows
import torch

scipy.signal.kaiser = scipy.signal.windows.kaiser

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402

SEEDS = {"mpd": 21, "discriminator": 22}


def strided_samples(n, count=64):
    """count positions spread over a flattened map of n values (all of them when n <= count)."""
    return np.unique(np.linspace(0, n - 1, count).astype(np.int64))


def inputs():
    rs = np.random.RandomState(41)
    x = 0.5 * rs.randn(2, 1, 4099)
    t = np.arange(3001) / 24000.0
    real = np.stack([0.4 * np.sin(2 * np.pi * 210 * t) + 0.05 * rs.randn(t.size), 0.3 * rs.randn(t.size)])
    est = real + 0.05 * rs.randn(*real.shape)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    return f32(x), f32(est[:, None]), f32(real[:, None])


def keys_and_shapes(module):
    sd = module.state_dict()
    return np.array(list(sd)), np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)


def main(reference):
    sys.path.insert(0, reference)
    from model.discriminator.mfd import MultiResolutionSTFTDiscriminator
    from model.discriminator.mpd import MultiPeriodDiscriminator
    from model.discriminator.msd import MelGANMultiScaleDiscriminator

    class Discriminator(torch.nn.Module):
        """discriminator.py with its two mpd lines enabled."""

        def __init__(self):
            super().__init__()
            self.mpd = MultiPeriodDiscriminator()
            self.msd = MelGANMultiScaleDiscriminator()
            self.mfd = MultiResolutionSTFTDiscriminator()

        def forward(self, x):
            return self.mpd(x) + self.msd(x) + self.mfd(x)

    def load(module, sd):
        module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return module.eval()

    torch.manual_seed(0)
    x, est, real = inputs()
    out = {"x": x, "est": est, "real": real}
    M = MultiPeriodDiscriminator()
    out["keys"], out["shapes"] = keys_and_shapes(M)
    D = Discriminator()
    out["d_keys"], out["d_shapes"] = keys_and_shapes(D)
    with torch.no_grad():
        M = load(M, seeded_discriminator_state_dict("mpd", SEEDS["mpd"]))
        maps = [m for lst in M(torch.from_numpy(x)) for m in lst]
        out["map_shapes"] = np.array([list(m.shape) + [-1] * (4 - m.dim()) for m in maps], dtype=np.int64)
        out["map_sum"] = np.array([m.double().sum().item() for m in maps])
        out["map_abs"] = np.array([m.double().abs().sum().item() for m in maps])
        out["map_std"] = np.array([m.double().std().item() for m in maps])
        out["map_samples"] = np.stack([np.pad(m.flatten().numpy()[strided_samples(m.numel())],
                                              (0, 64 - strided_samples(m.numel()).size)) for m in maps])
        for m, s in zip(maps, out["map_std"]):
            print(f"map {tuple(m.shape)} std {s:.3e} (input {x.std():.3e})")
        D = load(D, seeded_discriminator_state_dict("discriminator", SEEDS["discriminator"], use_mpd=True))
        est_p, p = D(torch.from_numpy(est)), D(torch.from_numpy(real))
        mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()
        adv = sum(mse(e[-1], torch.ones_like(e[-1])) for e in est_p) / len(est_p)
        fm = 0.0
        for i in range(len(est_p)):
            for j in range(len(est_p[i]) - 1):
                fm += l1(est_p[i][j], p[i][j])
        fm /= float(len(est_p)) * float(len(est_p[0]) - 1)
        real_l = sum(mse(r[-1], torch.ones_like(r[-1])) for r in p) / len(p)
        fake_l = sum(mse(e[-1], torch.zeros_like(e[-1])) for e in est_p) / len(p)
        out["scores"] = np.array([float(adv), float(fm), float(real_l), float(fake_l), float(real_l + fake_l)])
    path = os.path.join(HERE, "mpd.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, scores {out['scores']}")


if __name__ == "__main__":
    main(sys.argv[1])
