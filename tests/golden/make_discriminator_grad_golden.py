"""Writes tests/golden/discriminator_grad.npz: seeded inputs and the reference's own autograd gradient of its
adversarial + feature-map generator terms (bin/train.py:97-117) through model/discriminator/msd.py, torch on the CPU
with the module and the signals in float64, on the seeded weights of fastvocoder_amd.synthetic
(seeded_discriminator_state_dict("msd", seed, **SMALL_MSD), regenerated on any box, not stored).  Run once against a
checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_discriminator_grad_golden.py /path/to/FastVocoder

Contents, for the two cases c in ("short", "long"):
  <c>_est, <c>_real    [2, 1, n] float32   estimate and real signal (n = 45: no value of the float64 forward within
                                           1e-4 of a kink, tests/test_disc_grad_host.py; n = 2001)
  <c>_grad             [2, 1, n] float64   d(adversarial + feature_map)/d est
  <c>_grad_fake        [2, 1, n] float64   d fake / d est
  <c>_grad_scale1      [2, 1, n] float64   d(adversarial + feature_map)/d est of discriminators.1 alone
  seed                 the state dict's seed
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
CASES = {"short": (37, 45), "long": (38, 2001)}        # name -> (RandomState seed, samples)


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
    msd = msd.double().eval()
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()

    def grad(est, real, which, run):
        x = torch.from_numpy(est).double().requires_grad_(True)
        est_p = run(x)
        with torch.no_grad():
            p = run(torch.from_numpy(real).double())
        loss = 0.0
        if "adversarial" in which:
            for ii in range(len(est_p)):
                loss = loss + mse(est_p[ii][-1], est_p[ii][-1].new_ones(est_p[ii][-1].size())) / float(len(est_p))
        if "feature_map" in which:
            fm = 0.0
            for ii in range(len(est_p)):
                for jj in range(len(est_p[ii]) - 1):
                    fm = fm + l1(est_p[ii][jj], p[ii][jj].detach())
            loss = loss + fm / (float(len(est_p)) * float(len(est_p[0]) - 1))
        if "fake" in which:
            for ii in range(len(est_p)):
                loss = loss + mse(est_p[ii][-1], est_p[ii][-1].new_zeros(est_p[ii][-1].size())) / float(len(est_p))
        loss.backward()
        return x.grad.numpy().copy()

    out = {"seed": np.int64(SEED)}
    for name in CASES:
        est, real = signals(name)
        out[f"{name}_est"], out[f"{name}_real"] = est, real
        out[f"{name}_grad"] = grad(est, real, ("adversarial", "feature_map"), msd)
        out[f"{name}_grad_fake"] = grad(est, real, ("fake",), msd)
        out[f"{name}_grad_scale1"] = grad(est, real, ("adversarial", "feature_map"),
                                          lambda v: [msd.discriminators[1](v)])
    path = os.path.join(HERE, "discriminator_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; " +
          " ".join(f"|{k}| {np.linalg.norm(v):.6e}" for k, v in out.items() if "grad" in k))


if __name__ == "__main__":
    main(sys.argv[1])
