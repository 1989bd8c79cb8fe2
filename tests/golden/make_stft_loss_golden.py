"""Writes tests/golden/stft_loss.npz: seeded inputs and the reference's STFT loss values on them
(model/loss/stft_loss.py, model/loss/loss.py, model/generator/pqmf.py; torch on the CPU in float32).
Run once against a checkout of the reference, with the SciPy >= 1.13 shim make_golden.py uses:

    python tests/golden/make_stft_loss_golden.py /path/to/FastVocoder

Contents:
  x, y          [2, 12000] float32  estimate and target
  est_sub       [2, 4, 3000] float32 sub-band estimate (multiband Loss, target y)
  stft_terms    [3, 2] float32      STFTLoss(n_fft, hop, win)(x, y) -> (sc, mag) for the three default resolutions
  mr_terms      [2] float32         MultiResolutionSTFTLoss()(x, y)
  loss_single   float32             Loss()(x, y)[0]
  loss_multi    float32             Loss()(est_sub, y, pqmf=PQMF())[0]
The fixture is data only; no test reads the reference tree."""
import os
import sys
import types
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True

import numpy as np
import scipy.signal
import scipy.signal.windows
import torch

scipy.signal.kaiser = scipy.signal.windows.kaiser


def signals():
    rs = np.random.RandomState(2024)
    n = 12000
    t = np.arange(n) / 24000.0
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.0 * t)
    y = np.stack([0.3 * env * np.sin(2 * np.pi * 220 * t) + 0.05 * rs.randn(n),
                  0.2 * rs.randn(n) * np.exp(-t * 2.0)])
    x = y + 0.02 * rs.randn(2, n)
    est_sub = 0.1 * rs.randn(2, 4, n // 4)
    return x.astype(np.float32), y.astype(np.float32), est_sub.astype(np.float32)


def main(ref_root):
    for name in ("librosa", "librosa.filters", "tensorflow", "tensorboardX"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref_root)
    from model.loss.stft_loss import STFTLoss, MultiResolutionSTFTLoss
    from model.loss.loss import Loss
    from model.generator.pqmf import PQMF

    x, y, est_sub = signals()
    tx, ty, tsub = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(est_sub)
    with torch.no_grad():
        stft_terms = np.array([[float(v) for v in STFTLoss(nf, hop, wl)(tx, ty)]
                               for nf, hop, wl in ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))], np.float32)
        mr_terms = np.array([float(v) for v in MultiResolutionSTFTLoss()(tx, ty)], np.float32)
        loss_single = np.float32(Loss()(tx, ty.clone())[0])
        loss_multi = np.float32(Loss()(tsub, ty.clone(), pqmf=PQMF())[0])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stft_loss.npz")
    np.savez_compressed(out, x=x, y=y, est_sub=est_sub, stft_terms=stft_terms, mr_terms=mr_terms,
                        loss_single=loss_single, loss_multi=loss_multi)
    print(f"wrote {out}: {os.path.getsize(out)} bytes; stft_terms {stft_terms.tolist()} mr {mr_terms.tolist()} "
          f"single {loss_single} multi {loss_multi}")


if __name__ == "__main__":
    main(sys.argv[1])
