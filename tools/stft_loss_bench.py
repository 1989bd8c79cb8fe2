"""Sustained ms per call of MultiResolutionSTFTLoss (one fv_stft_distance call: the fused launch over all three
resolutions plus the small fixed-order sum launch) against the same two terms computed on the device by the eager
torch chain of the reference (per resolution: torch.stft of x and of y, clamp, sqrt, Frobenius norms, log, mean),
at B = 1 and B = 64 pairs of n = 240 000 samples.  Prints one JSON line.  Timing: every shape warmed up first,
then device events around a run of back-to-back calls (at least ~0.5 s of device work per figure), best of three.

    python tools/stft_loss_bench.py [--n 240000] [--batches 1,64]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd.loss import MultiResolutionSTFTLoss  # noqa: E402
from tools.mel_bench import ms_per_call  # noqa: E402

RESOLUTIONS = ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))


def eager_chain(dev):
    windows = [torch.hann_window(wl, device=dev) for _, _, wl in RESOLUTIONS]

    def mag(x, nf, hop, wl, w):
        S = torch.stft(x, nf, hop, wl, w, return_complex=True)
        return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-7)).transpose(2, 1)

    def run(xy):
        x, y = xy
        sc = mg = 0.0
        for (nf, hop, wl), w in zip(RESOLUTIONS, windows):
            X, Y = mag(x, nf, hop, wl, w), mag(y, nf, hop, wl, w)
            sc = sc + torch.norm(Y - X, p="fro") / torch.norm(Y, p="fro")
            mg = mg + torch.nn.functional.l1_loss(torch.log(Y), torch.log(X))
        return sc / 3, mg / 3
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=240000)
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stft_loss_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    mr = MultiResolutionSTFTLoss().to(dev)
    eager = eager_chain(dev)
    frames = sum(1 + args.n // hop for _, hop, _ in RESOLUTIONS)
    out = {"tool": "stft_loss_bench", "n": args.n, "frames_per_utterance_all_resolutions": frames,
           "launches_per_call": 2, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            rs = np.random.RandomState(B)
            x = torch.from_numpy(rs.uniform(-1, 1, (B, args.n)).astype(np.float32)).to(dev)
            y = (x + 0.05 * torch.from_numpy(rs.randn(B, args.n).astype(np.float32)).to(dev)).contiguous()
            fused = ms_per_call(lambda xy: mr(*xy), (x, y))
            row = {"fused_ms": round(fused, 4), "fused_frames_per_s": round(B * frames / fused * 1e3)}
            try:
                f_sc, f_mag = (float(v) for v in mr(x, y))
                e_sc, e_mag = (float(v) for v in eager((x, y)))
                ms = ms_per_call(eager, (x, y))
                row.update(torch_ms=round(ms, 4), speedup=round(ms / fused, 2),
                           rel_diff_sc_vs_torch=abs(f_sc - e_sc) / e_sc, abs_diff_mag_vs_torch=abs(f_mag - e_mag))
            except RuntimeError as e:       # torch.stft not available on the device, or out of memory
                row.update(torch_ms=None, speedup=None, torch_error=str(e)[:200])
            out[f"B{B}"] = row
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
