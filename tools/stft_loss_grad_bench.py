"""Sustained ms of forward + backward of MultiResolutionSTFTLoss with ``differentiable`` set (fv_stft_distance, the
small torch composition of the terms, fv_stft_distance_grad) against forward + backward of the eager torch.stft chain
of tools/stft_loss_bench.py on the device, for sc + mag at B = 1 and B = 64 estimates of n = 240 000 samples, and the
peak device memory (torch.cuda.max_memory_allocated) of one forward + backward of each.  Prints one JSON line.
Timing: tools/mel_bench.ms_per_call (warm-up, device events around back-to-back calls, best of three).

    python tools/stft_loss_grad_bench.py [--samples 240000] [--batches 1,64] [--target-s 0.5]
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
from tools.stft_loss_bench import RESOLUTIONS, eager_chain  # noqa: E402


def step(terms):
    """forward + backward of sc + mag on a leaf estimate; returns the gradient"""
    def run(xy):
        x, y = xy
        x.grad = None
        sc, mag = terms((x, y))
        (sc + mag).backward()
        return x.grad
    return run


def peak_mb(fn, xy):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(xy)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=240000)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--target-s", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stft_loss_grad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    mr = MultiResolutionSTFTLoss().to(dev)
    mr.differentiable = True
    fused, eager = step(lambda xy: mr(*xy)), step(eager_chain(dev))
    n = args.samples
    out = {"tool": "stft_loss_grad_bench", "what": "forward + backward of sc + mag", "rows": [],
           "frames_per_utterance_all_resolutions": sum(1 + n // hop for _, hop, _ in RESOLUTIONS),
           "device": torch.cuda.get_device_name(dev)}
    for B in (int(b) for b in args.batches.split(",")):
        rs = np.random.RandomState(B)
        y = torch.from_numpy(rs.uniform(-1, 1, (B, n)).astype(np.float32)).to(dev)
        x = (y + 0.05 * torch.from_numpy(rs.randn(B, n).astype(np.float32)).to(dev)).contiguous().requires_grad_(True)
        row = {"B": B, "n": n, "fused_ms": round(ms_per_call(fused, (x, y), args.target_s), 4),
               "fused_peak_mb": round(peak_mb(fused, (x, y)), 2)}
        g_fused = fused((x, y)).clone()
        try:
            g_eager = eager((x, y)).clone()
            row.update(eager_ms=round(ms_per_call(eager, (x, y), args.target_s), 4),
                       eager_peak_mb=round(peak_mb(eager, (x, y)), 2),
                       grad_rel_l2_vs_eager=float((g_fused - g_eager).norm() / g_eager.norm()))
            row["speedup"] = round(row["eager_ms"] / row["fused_ms"], 2)
        except RuntimeError as e:           # torch.stft not available on the device, or out of memory
            row.update(eager_ms=None, eager_peak_mb=None, speedup=None, eager_error=str(e)[:200])
        out["rows"].append(row)
        del g_fused
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
