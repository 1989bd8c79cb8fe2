"""Writes tests/golden/mpd_mfd_param_grad.npz: seeded signals and the reference's own autograd gradient of its
discriminator loss real_loss + fake_loss (bin/train.py:157-169) with respect to every parameter of
model/discriminator/mpd.py and mfd.py (and msd.py inside the whole Discriminator), torch on the CPU with the modules
and the signals in float64, on the seeded weights of fastvocoder_amd.synthetic (regenerated on any box, not stored).
Run once against a checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_mpd_mfd_param_grad_golden.py /path/to/FastVocoder

Cases (tests/mpd_wgrad_reference.py holds their sizes and seeds):
  p<period>           DiscriminatorP(period), the sub-discriminator of that period of the seeded MPD, B = 2
  stft                the small STFTDiscriminator(**SMALL_STFT), signals (2, T)
  mfd                 the default MultiResolutionSTFTDiscriminator just above min_length(), B = 2
  discriminator_mpd   Discriminator(use_mpd=True): the reference's mpd(x) + msd(x) + mfd(x) (discriminator.py:11-16
                      with its commented line restored), same length
Contents per case c:
  <c>_est, <c>_real               float32   estimate and real signal
  <c>_grad/<state key>            float64   d(real_loss + fake_loss)/d parameter: the whole tensor up to SAMPLE
                                            entries, else SAMPLE entries of the flat tensor at the fixed stride
                                            size // SAMPLE (mpd_wgrad_reference.sample)
  <c>_norm/<state key>            float64   the L2 norm of the whole tensor
  <c>_real_loss, <c>_fake_loss    float64   the two terms
  <c>_seed                        the signals' RandomState seed
The fixture is data only; no test reads the reference tree.  SAMPLE is 160: the 41 M entries of the MPD's gradient, the
MFD's and the MSD's add up to 230 tensors above 160 entries, and 4096 float64 samples of each would take 3.9 MB where
the largest fixture of tests/golden/ has 676 KB."""
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
from tests import mpd_wgrad_reference as wref  # noqa: E402


def main(reference):
    sys.path.insert(0, reference)
    from model.discriminator.mfd import MultiResolutionSTFTDiscriminator, STFTDiscriminator
    from model.discriminator.mpd import MultiPeriodDiscriminator
    from model.discriminator.msd import MelGANMultiScaleDiscriminator

    mse = torch.nn.MSELoss()
    out = {}

    def load(module, sd, prefix=""):
        module.load_state_dict({k[len(prefix):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()
                                if k.startswith(prefix)})
        return module.double().train()

    def case(name, modules, run, sd, est, real, seed):
        """modules: [(prefix, module)]; run(x) -> the lists, the score last in each"""
        for _, m in modules:
            m.zero_grad()
        # bin/train.py:157-169
        p = run(torch.from_numpy(real).double())
        est_p = run(torch.from_numpy(est).double().detach())
        real_loss, fake_loss = 0.0, 0.0
        for ii in range(len(p)):
            real_loss = real_loss + mse(p[ii][-1], p[ii][-1].new_ones(p[ii][-1].size()))
            fake_loss = fake_loss + mse(est_p[ii][-1], est_p[ii][-1].new_zeros(est_p[ii][-1].size()))
        real_loss = real_loss / float(len(p))
        fake_loss = fake_loss / float(len(p))
        (real_loss + fake_loss).backward()
        named = {prefix + k: q for prefix, m in modules for k, q in m.named_parameters()}
        assert sorted(named) == sorted(k for k in sd if wref.is_param(k)), "every parameter has a state-dict entry"
        out[f"{name}_est"], out[f"{name}_real"], out[f"{name}_seed"] = est, real, np.int64(seed)
        total = 0.0
        for k, q in named.items():
            out[f"{name}_grad/{k}"], out[f"{name}_norm/{k}"] = wref.sample(q.grad.numpy())
            total += out[f"{name}_norm/{k}"] ** 2
        out[f"{name}_real_loss"] = np.float64(real_loss.item())
        out[f"{name}_fake_loss"] = np.float64(fake_loss.item())
        print(f"{name}: seed {seed}, real {real_loss.item():.6e} fake {fake_loss.item():.6e} |grad| {total ** 0.5:.6e}")

    for i, period in enumerate(wref.PERIODS):
        sd = wref.case_state_dict(f"p{period}")
        mpd = MultiPeriodDiscriminator()
        d = load(mpd.discriminators[i], sd)

        def one(x, d=d):
            score, fmap = d(x)
            return [fmap + [score.unsqueeze(1)]]
        seed = wref.SIGNAL_SEEDS[f"p{period}"]
        est, real = wref.case_signals(f"p{period}")
        case(f"p{period}", [("", d)], one, sd, est, real, seed)

    sd = wref.case_state_dict("stft")
    stft = load(STFTDiscriminator(**wref.SMALL_STFT), sd)
    est, real = wref.case_signals("stft")
    case("stft", [("", stft)], lambda x: [stft(x)], sd, est, real, wref.SIGNAL_SEEDS["stft"])

    sd = wref.case_state_dict("mfd")
    mfd = load(MultiResolutionSTFTDiscriminator(), sd)
    est, real = wref.case_signals("mfd")
    case("mfd", [("", mfd)], mfd, sd, est, real, wref.FULL_SIGNAL_SEEDS["mfd"])

    sd = wref.case_state_dict("discriminator_mpd")
    mpd, msd, mfd = (load(MultiPeriodDiscriminator(), sd, "mpd."), load(MelGANMultiScaleDiscriminator(), sd, "msd."),
                     load(MultiResolutionSTFTDiscriminator(), sd, "mfd."))
    est, real = wref.case_signals("discriminator_mpd")
    case("discriminator_mpd", [("mpd.", mpd), ("msd.", msd), ("mfd.", mfd)], lambda x: mpd(x) + msd(x) + mfd(x), sd,
         est, real, wref.FULL_SIGNAL_SEEDS["discriminator_mpd"])

    path = os.path.join(HERE, "mpd_mfd_param_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
