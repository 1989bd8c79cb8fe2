"""Writes tests/golden/stft_loss_grad.npz: seeded inputs and the reference's own autograd gradients of its STFT loss
on them (model/loss/stft_loss.py, model/loss/loss.py, model/generator/pqmf.py; torch on the CPU with the modules
and signals in float64; the Hann windows are rebuilt in float64, since .double() would keep the float32-rounded taps
of the modules' buffers).  Run once against a checkout of the reference, with the SciPy >= 1.13 shim
make_stft_loss_golden.py uses:

    python tests/golden/make_stft_loss_grad_golden.py /path/to/FastVocoder

Contents:
  x, y          [2, 4800] float32     estimate and target (cast to float64 for the gradients)
  est_sub       [2, 4, 1200] float32  sub-band estimate (multiband Loss, target y)
  g_sc, g_mag   [2, 4800] float64     d sc / dx and d mag / dx of MultiResolutionSTFTLoss()(x, y)
  g_single      [2, 4800] float64     d Loss()(x, y)[0] / dx
  g_multi       [2, 4, 1200] float64  d Loss()(est_sub, y, pqmf=PQMF())[0] / d est_sub
  analysis_filter, synthesis_filter  [4, 63] float64  the PQMF's banks as that call used them (float32 values)
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
    rs = np.random.RandomState(2025)
    n = 4800
    t = np.arange(n) / 24000.0
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 7.0 * t)
    y = np.stack([0.3 * env * np.sin(2 * np.pi * 220 * t) + 0.05 * rs.randn(n),
                  0.2 * rs.randn(n) * np.exp(-t * 5.0)])
    x = y + 0.02 * rs.randn(2, n)
    est_sub = 0.1 * rs.randn(2, 4, n // 4)
    return x.astype(np.float32), y.astype(np.float32), est_sub.astype(np.float32)


def main(ref_root):
    for name in ("librosa", "librosa.filters", "tensorflow", "tensorboardX"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref_root)
    from model.loss.stft_loss import MultiResolutionSTFTLoss
    from model.loss.loss import Loss
    from model.generator.pqmf import PQMF

    x, y, est_sub = signals()
    ty = torch.from_numpy(y).double()

    def grad(fn, leaf):
        leaf = torch.from_numpy(leaf).double().requires_grad_(True)
        fn(leaf).backward()
        return leaf.grad.numpy().copy()

    def double(mr):
        mr = mr.double()
        for f in mr.stft_losses:
            f.window = torch.hann_window(f.win_length, dtype=torch.float64)
        return mr

    def loss():
        m = Loss().double()
        double(m.stft_loss)
        return m

    mr = double(MultiResolutionSTFTLoss())
    pqmf = PQMF().double()
    g_sc = grad(lambda v: mr(v, ty)[0], x)
    g_mag = grad(lambda v: mr(v, ty)[1], x)
    g_single = grad(lambda v: loss()(v, ty.clone())[0], x)
    g_multi = grad(lambda v: loss()(v, ty.clone(), pqmf=pqmf)[0], est_sub)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stft_loss_grad.npz")
    np.savez_compressed(out, x=x, y=y, est_sub=est_sub, g_sc=g_sc, g_mag=g_mag, g_single=g_single, g_multi=g_multi,
                        analysis_filter=pqmf.analysis_filter[:, 0].numpy(), synthesis_filter=pqmf.synthesis_filter[0].numpy())
    print(f"wrote {out}: {os.path.getsize(out)} bytes; |g_sc| {np.linalg.norm(g_sc):.6e} |g_mag| "
          f"{np.linalg.norm(g_mag):.6e} |g_single| {np.linalg.norm(g_single):.6e} |g_multi| "
          f"{np.linalg.norm(g_multi):.6e}")


if __name__ == "__main__":
    main(sys.argv[1])
