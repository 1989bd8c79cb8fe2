"""Writes tests/golden/mpd_grad.npz: seeded inputs and the reference's own autograd gradient of its adversarial +
feature-map generator terms (bin/train.py:97-117) through model/discriminator/mpd.py, torch on the CPU with the module
and the signals in float64, on the seeded weights of fastvocoder_amd.synthetic
(seeded_discriminator_state_dict("mpd", seed), regenerated on any box, not stored).  Run once against a checkout of
the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_mpd_grad_golden.py /path/to/FastVocoder

Contents:
  tiny<p>_est, tiny<p>_real        [2, 1, T] float32   one case per period p on DiscriminatorP(p) (the MPD's own
                                                       sub-discriminator of that period), T % p != 0 (a reflect tail)
  tiny<p>_grad, tiny<p>_grad_adv   [2, 1, T] float64   d(adversarial + feature_map)/d est; d adversarial / d est
  tiny_seeds                       [5] the RandomState seed of each tiny case (the first whose float64 forward keeps
                                   every kink further than tests/mpd_grad_reference.py UNRESOLVED from zero)
  n2311_est, n2311_real            [2, 1, 2311] float32 the whole MultiPeriodDiscriminator
  n2311_grad, n2311_grad_adv       [2, 1, 2311] float64
  seed                             the state dict's seed
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
from tests import mpd_grad_reference as mref  # noqa: E402


def main(reference):
    sys.path.insert(0, reference)
    from model.discriminator.mpd import MultiPeriodDiscriminator

    seed = mref.SEEDS["mpd"]
    sd = seeded_discriminator_state_dict("mpd", seed)
    mpd = MultiPeriodDiscriminator()
    mpd.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    mpd = mpd.double().eval()
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()

    def grad(run, est, real, which):
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
        loss.backward()
        return x.grad.numpy().copy()

    out = {"seed": np.int64(seed)}
    seeds = []
    for i, period in enumerate(mref.PERIODS):
        d = mpd.discriminators[i]

        def one(x, d=d):
            score, fmap = d(x)
            return [fmap + [score.unsqueeze(1)]]
        psd = mref.sub_state_dict(sd, i)
        T = mref.TINY_T[period]
        s = next(s for s in range(1000)
                 if mref.kink_count("p", *mref.signals(s, T), psd, period=period, rel=mref.UNRESOLVED) == 0)
        seeds.append(s)
        est, real = mref.signals(s, T)
        print(f"period {period}: T {T} seed {s}, {mref.kink_count('p', est, real, psd, period=period)} values within "
              f"{mref.KINK_BAND:g} of a kink")
        out[f"tiny{period}_est"], out[f"tiny{period}_real"] = est, real
        out[f"tiny{period}_grad"] = grad(one, est, real, ("adversarial", "feature_map"))
        out[f"tiny{period}_grad_adv"] = grad(one, est, real, ("adversarial",))
    out["tiny_seeds"] = np.asarray(seeds, np.int64)
    est, real = mref.signals(mref.N2311[1], mref.N2311[0])
    out["n2311_est"], out["n2311_real"] = est, real
    out["n2311_grad"] = grad(mpd, est, real, ("adversarial", "feature_map"))
    out["n2311_grad_adv"] = grad(mpd, est, real, ("adversarial",))
    path = os.path.join(HERE, "mpd_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; " +
          " ".join(f"|{k}| {np.linalg.norm(v):.6e}" for k, v in out.items() if "grad" in k))


if __name__ == "__main__":
    main(sys.argv[1])
