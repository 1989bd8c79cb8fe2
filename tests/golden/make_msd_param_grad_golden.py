"""Writes tests/golden/msd_param_grad.npz: seeded signals and the reference's own autograd gradient of its
discriminator loss real_loss + fake_loss (bin/train.py:157-169) with respect to every parameter of
model/discriminator/msd.py, torch on the CPU with the module and the signals in float64, on the seeded weights of
fastvocoder_amd.synthetic (seeded_discriminator_state_dict("msd", seed, **SMALL_MSD), regenerated on any box, not
stored).  Run once against a checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_msd_param_grad_golden.py /path/to/FastVocoder

Contents, for the two cases c in ("short", "long"):
  <c>_est, <c>_real         [2, 1, n] float32   estimate and real signal (n = 45, RandomState(113): no pre-activation
                                                of either signal's float64 forward within 1e-4 of its map's peak,
                                                tests/test_msd_wgrad_host.py; n = 2001, RandomState(38))
  <c>_grad/<state key>      float64             d(real_loss + fake_loss)/d parameter, one entry per state-dict key
  <c>_real_loss, <c>_fake_loss   float64        the two terms
  seed                      the state dict's seed
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
SEED = 11
CASES = {"short": (113, 45), "long": (38, 2001)}       # name -> (RandomState seed, samples)


def signals(name):
    seed, n = CASES[name]
    rs = np.random.RandomState(seed)
    real = rs.uniform(-0.8, 0.8, (2, 1, n)).astype(np.float32)
    est = (real + 0.3 * rs.randn(2, 1, n)).astype(np.float32)
    return est, real


def main(reference):
    sys.path.insert(0, reference)
    from model.discriminator.msd import MelGANMultiScaleDiscriminator

    sd = seeded_discriminator_state_dict("msd", SEED, **SMALL_MSD)
    msd = MelGANMultiScaleDiscriminator(**SMALL_MSD)
    msd.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    msd = msd.double().train()
    mse = torch.nn.MSELoss()

    out = {"seed": np.int64(SEED)}
    for name in CASES:
        est, real = signals(name)
        out[f"{name}_est"], out[f"{name}_real"] = est, real
        msd.zero_grad()
        # bin/train.py:157-169
        p = msd(torch.from_numpy(real).double())
        est_p = msd(torch.from_numpy(est).double().detach())
        real_loss, fake_loss = 0.0, 0.0
        for ii in range(len(p)):
            real_loss = real_loss + mse(p[ii][-1], p[ii][-1].new_ones(p[ii][-1].size()))
            fake_loss = fake_loss + mse(est_p[ii][-1], est_p[ii][-1].new_zeros(est_p[ii][-1].size()))
        real_loss = real_loss / float(len(p))
        fake_loss = fake_loss / float(len(p))
        (real_loss + fake_loss).backward()
        named = dict(msd.named_parameters())
        assert sorted(named) == sorted(sd), "every state-dict entry is a parameter"
        for k in sd:
            out[f"{name}_grad/{k}"] = named[k].grad.numpy().copy()
        out[f"{name}_real_loss"] = np.float64(real_loss.item())
        out[f"{name}_fake_loss"] = np.float64(fake_loss.item())
    path = os.path.join(HERE, "msd_param_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; " +
          " ".join(f"{c} |grad| {np.sqrt(sum(np.sum(v ** 2) for k, v in out.items() if k.startswith(c + '_grad/'))):.6e}"
                   for c in CASES))


if __name__ == "__main__":
    main(sys.argv[1])
