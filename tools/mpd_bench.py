#!/usr/bin/env python
"""Times MultiPeriodDiscriminator() forward at 240 000 samples, B = 1 and B = 8, with device events after a warm-up:
per period and in total, milliseconds, achieved TFLOP/s against the 157 TF fp32 matrix peak, and the same forward as
eager torch.nn.functional.conv2d on the same GPU (weights folded once, outside the timed region).

    python tools/mpd_bench.py [--samples 240000] [--batches 1 8] [--iters 10] [--warmup 3]

Prints one line per (batch, period) and a total per batch; the median of ``iters`` timed forwards."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd.discriminator import MultiPeriodDiscriminator  # noqa: E402
from fastvocoder_amd.discriminator.mpd import PERIODS, period_heights  # noqa: E402
from fastvocoder_amd.generator.engine import effective_weight  # noqa: E402
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402

PEAK_TFLOPS = 157.3
CHANNELS = ((32, 1, 5), (128, 32, 5), (512, 128, 5), (1024, 512, 5), (1024, 1024, 5), (1, 1024, 3))


def flops(T, period):
    """Multiply-adds x 2 of one row through DiscriminatorP(period)."""
    _, hs = period_heights(T, period)
    outs = hs[1:5] + [hs[4], hs[4]]
    return sum(2.0 * cout * cin * k * h * period for (cout, cin, k), h in zip(CHANNELS, outs))


def eager_forward(x, weights, period):
    B, _, T = x.shape
    n_pad = period - T % period if T % period else 0
    if n_pad:
        x = F.pad(x, (0, n_pad), "reflect")
    x = x.view(B, 1, -1, period)
    for j, (w, b) in enumerate(weights):
        if j < 5:
            x = F.leaky_relu(F.conv2d(x, w, b, stride=(3 if j < 4 else 1, 1), padding=(2, 0)), 0.1)
        else:
            x = F.conv2d(x, w, b, padding=(1, 0))
    return x


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=240000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    mpd = MultiPeriodDiscriminator()
    mpd.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("mpd", 21).items()})
    mpd = mpd.to(dev).eval()
    with torch.no_grad():
        folded = [[(effective_weight(c), c.bias.detach()) for c in list(d.convs) + [d.conv_post]]
                  for d in mpd.discriminators]
        for B in args.batches:
            x = (0.3 * torch.randn(B, 1, args.samples, device=dev)).contiguous()
            tot_ms = tot_eager = tot_fl = 0.0
            for d, w, p in zip(mpd.discriminators, folded, PERIODS):
                fl = B * flops(args.samples, p)
                ms = median_ms(lambda: d(x), args.iters, args.warmup)
                eager = median_ms(lambda: eager_forward(x, w, p), args.iters, args.warmup)
                tot_ms, tot_eager, tot_fl = tot_ms + ms, tot_eager + eager, tot_fl + fl
                tf = fl / ms / 1e9
                print(f"mpd-bench B={B} period={p} gflop={fl / 1e9:.1f} ms={ms:.3f} tflops={tf:.1f} "
                      f"peak_fraction={tf / PEAK_TFLOPS:.3f} eager_conv2d_ms={eager:.3f}")
            ms = median_ms(lambda: mpd(x), args.iters, args.warmup)
            tf = tot_fl / ms / 1e9
            print(f"mpd-bench B={B} total gflop={tot_fl / 1e9:.1f} ms={ms:.3f} tflops={tf:.1f} "
                  f"peak_fraction={tf / PEAK_TFLOPS:.3f} sum_of_periods_ms={tot_ms:.3f} eager_conv2d_ms={tot_eager:.3f}")


if __name__ == "__main__":
    main()
