"""Sustained ms of forward + backward of adversarial + feature_map through MelGANMultiScaleDiscriminator() with
``differentiable`` set (the forward launches, loss.discriminator_terms(differentiable=True), the kernels of
csrc/disc_grad.hip) against forward + backward of the same chain in eager torch autograd on the device (folded
weights, F.conv1d / F.avg_pool1d / F.leaky_relu), at B = 1 and B = 16 rows of 24 000 samples, and the peak device
memory (torch.cuda.max_memory_allocated) of one forward + backward of each.  Prints one JSON line.
Timing: tools/mel_bench.ms_per_call (warm-up, device events around back-to-back calls, best of three).

    python tools/disc_grad_bench.py [--samples 24000] [--batches 1,16] [--target-s 0.5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd.discriminator import MelGANMultiScaleDiscriminator  # noqa: E402
from fastvocoder_amd.generator.engine import effective_weight  # noqa: E402
from fastvocoder_amd.loss import discriminator_terms  # noqa: E402
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402
from tools.mel_bench import ms_per_call  # noqa: E402
from tools.stft_loss_grad_bench import peak_mb  # noqa: E402


def eager_msd(msd):
    """The module's forward as eager torch on its folded weights (constants: only the input carries a gradient)."""
    with torch.no_grad():
        stacks = [[(spec, effective_weight(conv).detach(), None if conv.bias is None else conv.bias.detach())
                   for spec, conv in zip(d._spec, d._convs())] for d in msd.discriminators]

    def run(x):
        outs = []
        for i, layers in enumerate(stacks):
            maps, v = [], x
            for spec, w, b in layers:
                if spec[0] == "grouped":
                    _, k, pad, stride, slope = spec
                    v = F.conv1d(v, w, b, stride=stride, padding=pad, groups=v.shape[1] // 4)
                else:
                    _, k, pad, mode, slope = spec
                    v = F.conv1d(F.pad(v, (pad, pad), mode="reflect") if mode else v, w, b, padding=0 if mode else pad)
                if slope != 1.0:
                    v = F.leaky_relu(v, slope)
                maps.append(v)
            outs.append(maps)
            if i + 1 < len(stacks):
                x = F.avg_pool1d(x, *msd._pool, count_include_pad=False)
        return outs
    return run


def eager_terms(est_p, p):
    L = len(est_p)
    adv = sum(((e[-1] - 1) ** 2).mean() for e in est_p) / L
    fm = sum((e - r.detach()).abs().mean() for le, lr in zip(est_p, p) for e, r in zip(le[:-1], lr[:-1]))
    return adv + fm / (L * (len(est_p[0]) - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=24000)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--target-s", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "disc_grad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    msd = MelGANMultiScaleDiscriminator()
    msd.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("msd", 13).items()})
    msd = msd.to(dev).eval()
    msd.differentiable = True
    eager = eager_msd(msd)

    def fused_step(xy):
        x, p = xy
        x.grad = None
        t = discriminator_terms(msd(x), p, differentiable=True)
        (t["adversarial"] + t["feature_map"]).backward()
        return x.grad

    def eager_step(xy):
        x, p = xy
        x.grad = None
        eager_terms(eager(x), p).backward()
        return x.grad

    n = args.samples
    out = {"tool": "disc_grad_bench", "what": "forward + backward of adversarial + feature_map, MSD", "rows": [],
           "device": torch.cuda.get_device_name(dev)}
    for B in (int(b) for b in args.batches.split(",")):
        rs = np.random.RandomState(B)
        real = torch.from_numpy((0.5 * rs.randn(B, 1, n)).astype(np.float32)).to(dev)
        x = (real + 0.1 * torch.from_numpy(rs.randn(B, 1, n).astype(np.float32)).to(dev)).contiguous().requires_grad_(True)
        with torch.no_grad():
            p = msd(real)
        row = {"B": B, "n": n, "fused_ms": round(ms_per_call(fused_step, (x, p), args.target_s), 4),
               "fused_peak_mb": round(peak_mb(fused_step, (x, p)), 2)}
        g_fused = fused_step((x, p)).clone()
        try:
            g_eager = eager_step((x, p)).clone()
            row.update(eager_ms=round(ms_per_call(eager_step, (x, p), args.target_s), 4),
                       eager_peak_mb=round(peak_mb(eager_step, (x, p)), 2),
                       grad_rel_max_vs_eager=float((g_fused - g_eager).abs().max() / g_eager.abs().max()))
            row["speedup"] = round(row["eager_ms"] / row["fused_ms"], 2)
        except RuntimeError as e:           # out of memory
            row.update(eager_ms=None, eager_peak_mb=None, speedup=None, eager_error=str(e)[:200])
        out["rows"].append(row)
        del g_fused
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
