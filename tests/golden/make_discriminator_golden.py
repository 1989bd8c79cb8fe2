"""Writes tests/golden/discriminator.npz: the reference's discriminators (model/discriminator/msd.py, mfd.py,
discriminator.py) and training-loop scores (bin/train.py:97-117, 157-169) run by torch on the CPU in float32, on the
seeded weights of fastvocoder_amd.synthetic (seeded_discriminator_state_dict, regenerated on any box, not stored).
Run once against a checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_discriminator_golden.py /path/to/FastVocoder

Contents:
  keys, shapes          the full Discriminator() state_dict: key names and shapes (shapes padded with -1 to rank 3)
  small_x               [2, 1, 2001] float32 input of the small configurations
  msd_<i>_<j>           MelGANMultiScaleDiscriminator(**SMALL_MSD) scale i, layer j output, in full
  stft_<j>              STFTDiscriminator(**SMALL_STFT) layer j output on small_x[:, 0], in full
  full_x                [2, 1, 4001] float32 input of the default Discriminator()
  full_sum, full_abs    [36] float64 sum and sum of |v| of every feature map (flattened list order)
  full_samples          [36, 64] float32 every map's flattened values at STRIDED_SAMPLES(n) positions
  est, real             [2, 1, 6007] float32 the scored pair
  scores                [5] float64 adversarial, feature_map, real, fake, discriminator of D(est), D(real)
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

SMALL_MSD = dict(channels=4, max_downsample_channels=16, downsample_scales=[4, 2])
SMALL_STFT = dict(fft_size=512, shift_size=50, win_length=240, channels=8, max_downsample_channels=64)
SEEDS = {"small_msd": 11, "small_stft": 12, "full": 13}


def strided_samples(n, count=64):
    """count positions spread over a flattened map of n values (all of them when n <= count)."""
    return np.unique(np.linspace(0, n - 1, count).astype(np.int64))


def inputs():
    rs = np.random.RandomState(31)
    t = np.arange(6007) / 24000.0
    real = np.stack([0.4 * np.sin(2 * np.pi * 210 * t) + 0.05 * rs.randn(t.size), 0.3 * rs.randn(t.size)])
    est = real + 0.05 * rs.randn(*real.shape)
    small = rs.uniform(-0.8, 0.8, (2, 1, 2001))
    full = 0.5 * rs.randn(2, 1, 4001)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    return f32(small), f32(full), f32(est[:, None]), f32(real[:, None])


def flat(outs):
    return [m for lst in outs for m in lst]


def main(reference):
    sys.path.insert(0, reference)
    from model.discriminator.discriminator import Discriminator
    from model.discriminator.mfd import STFTDiscriminator
    from model.discriminator.msd import MelGANMultiScaleDiscriminator

    def load(module, sd):
        module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return module.eval()

    torch.manual_seed(0)
    small, full, est, real = inputs()
    out = {"small_x": small, "full_x": full, "est": est, "real": real}
    D = Discriminator()
    sd = D.state_dict()
    out["keys"] = np.array(list(sd))
    out["shapes"] = np.array([list(v.shape) + [-1] * (3 - v.dim()) for v in sd.values()], dtype=np.int64)
    with torch.no_grad():
        msd = load(MelGANMultiScaleDiscriminator(**SMALL_MSD),
                   seeded_discriminator_state_dict("msd", SEEDS["small_msd"], **SMALL_MSD))
        for i, lst in enumerate(msd(torch.from_numpy(small))):
            for j, m in enumerate(lst):
                out[f"msd_{i}_{j}"] = m.numpy()
        sdisc = load(STFTDiscriminator(**SMALL_STFT),
                     seeded_discriminator_state_dict("stft", SEEDS["small_stft"], **SMALL_STFT))
        for j, m in enumerate(sdisc(torch.from_numpy(small[:, 0]))):
            out[f"stft_{j}"] = m.numpy()
        D = load(D, seeded_discriminator_state_dict("discriminator", SEEDS["full"]))
        maps = flat(D(torch.from_numpy(full)))
        out["full_sum"] = np.array([m.double().sum().item() for m in maps])
        out["full_abs"] = np.array([m.double().abs().sum().item() for m in maps])
        out["full_samples"] = np.stack([np.pad(m.flatten().numpy()[strided_samples(m.numel())],
                                               (0, 64 - strided_samples(m.numel()).size)) for m in maps])
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
        for m in maps:
            print(f"map {tuple(m.shape)} std {m.std().item():.3e}")
    path = os.path.join(HERE, "discriminator.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, scores {out['scores']}")


if __name__ == "__main__":
    main(sys.argv[1])
