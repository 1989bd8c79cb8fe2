"""Writes tests/golden/mfd_grad.npz: seeded inputs and the reference's own autograd gradient of its adversarial +
feature-map generator terms (bin/train.py:97-117) through model/discriminator/mfd.py's STFTDiscriminator, torch on the
CPU with the module and the signals in float64, on the seeded weights of fastvocoder_amd.synthetic
(seeded_discriminator_state_dict("stft", seed, **SMALL_STFT), regenerated on any box, not stored).  Run once against a
checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_mfd_grad_golden.py /path/to/FastVocoder

Contents, for the two cases c in ("n400", "n1999"):
  <c>_est, <c>_real    [2, n] float32   estimate and real signal (n = 400: no value of the float64 forward within
                                        1e-4 of a kink and no bin power within a factor 4 of the clamp,
                                        tests/test_mfd_grad_host.py; n = 1999)
  <c>_grad             [2, n] float64   d(adversarial + feature_map)/d est
  <c>_grad_adv         [2, n] float64   d adversarial / d est (the real=None form)
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

SMALL_STFT = dict(fft_size=512, shift_size=50, win_length=240, channels=8, max_downsample_channels=32,
                  downsample_scales=[4, 2])
SEED = 17
CASES = {"n400": (41, 400), "n1999": (42, 1999)}        # name -> (RandomState seed, samples)


def signals(name):
    seed, n = CASES[name]
    rs = np.random.RandomState(seed)
    real = rs.uniform(-0.8, 0.8, (2, n)).astype(np.float32)
    est = (real + 0.3 * rs.randn(2, n)).astype(np.float32)
    return est, real


def main(reference):
    sys.path.insert(0, reference)
    from model.discriminator.mfd import STFTDiscriminator

    sd = seeded_discriminator_state_dict("stft", SEED, **SMALL_STFT)
    disc = STFTDiscriminator(**SMALL_STFT)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    disc = disc.double().eval()
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()

    def grad(est, real, which):
        x = torch.from_numpy(est).double().requires_grad_(True)
        est_p = [disc(x)]
        with torch.no_grad():
            p = [disc(torch.from_numpy(real).double())]
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
        loss.backward()
        return x.grad.numpy().copy()

    out = {"seed": np.int64(SEED)}
    for name in CASES:
        est, real = signals(name)
        out[f"{name}_est"], out[f"{name}_real"] = est, real
        out[f"{name}_grad"] = grad(est, real, ("adversarial", "feature_map"))
        out[f"{name}_grad_adv"] = grad(est, real, ("adversarial",))
    path = os.path.join(HERE, "mfd_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; " +
          " ".join(f"|{k}| {np.linalg.norm(v):.6e}" for k, v in out.items() if "grad" in k))


if __name__ == "__main__":
    main(sys.argv[1])
