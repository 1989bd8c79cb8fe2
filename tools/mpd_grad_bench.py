#!/usr/bin/env python
"""Times forward + backward of the generator's adversarial + feature-map terms through MultiPeriodDiscriminator()
(loss.generator_adversarial_terms(..., period_grad=True)) at 24 000 samples, B = 1 and B = 16, with device events after
a warm-up, beside the same objective as eager torch.nn.functional.conv2d autograd on the same GPU (weights folded
once, outside the timed region; D(real) is computed once, outside it, for both); and fv_period_conv_input_grad alone
per strided layer and period, with achieved TFLOP/s against the 157 TF fp32 matrix peak.

    python tools/mpd_grad_bench.py [--samples 24000] [--batches 1 16] [--iters 10] [--warmup 3]

Prints one line per measurement; the median of ``iters`` timed runs."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import _native  # noqa: E402
from fastvocoder_amd.discriminator import MultiPeriodDiscriminator  # noqa: E402
from fastvocoder_amd.discriminator.mpd import PERIODS, period_heights  # noqa: E402
from fastvocoder_amd.generator.engine import effective_weight  # noqa: E402
from fastvocoder_amd.loss import discriminator_terms  # noqa: E402
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402

PEAK_TFLOPS = 157.3
LAYERS = ((32, 128), (128, 512), (512, 1024))


def eager_lists(x, folded):
    B, _, T = x.shape
    outs = []
    for weights, period in zip(folded, PERIODS):
        n_pad = period - T % period if T % period else 0
        v = F.pad(x, (0, n_pad), "reflect") if n_pad else x
        v = v.view(B, 1, -1, period)
        fmap = []
        for j, (w, b) in enumerate(weights):
            if j < 5:
                v = F.leaky_relu(F.conv2d(v, w, b, stride=(3 if j < 4 else 1, 1), padding=(2, 0)), 0.1)
            else:
                v = F.conv2d(v, w, b, padding=(1, 0))
            fmap.append(v)
        outs.append(fmap + [v.flatten(1).unsqueeze(1)])
    return outs


def eager_objective(est_p, p):
    L = len(est_p)
    adv = sum(((lst[-1] - 1) ** 2).mean() for lst in est_p) / L
    fm = sum((a - b).abs().mean() for le, lr in zip(est_p, p) for a, b in zip(le[:-1], lr[:-1])) / (L * 6)
    return adv + fm


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
    ap.add_argument("--samples", type=int, default=24000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
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
        real = (0.3 * torch.randn(B, 1, args.samples, device=dev)).contiguous()
        est = (real + 0.1 * torch.randn_like(real)).contiguous()
        with torch.no_grad():
            p_native, p_eager = mpd(real), eager_lists(real, folded)

        def native():
            x = est.clone().requires_grad_(True)
            t = discriminator_terms(mpd._graph_forward(x), p_native, differentiable=True)
            (t["adversarial"] + t["feature_map"]).backward()
            return x.grad

        def eager():
            x = est.clone().requires_grad_(True)
            eager_objective(eager_lists(x, folded), p_eager).backward()
            return x.grad

        a, b = native(), eager()
        diff = float((a - b).abs().max() / b.abs().max())
        ms, ems = median_ms(native, args.iters, args.warmup), median_ms(eager, args.iters, args.warmup)
        print(f"mpd-grad-bench B={B} samples={args.samples} forward+backward ms={ms:.3f} eager_autograd_ms={ems:.3f} "
              f"max_diff_vs_eager={diff:.2e}")
        for i, period in enumerate(PERIODS):
            _, hs = period_heights(args.samples, period)
            for l, (cin, cout) in enumerate(LAYERS):
                H, hout = hs[l + 1], hs[l + 2]
                g = torch.randn(B, cout, hout, period, device=dev)
                y = torch.randn(B, cout, hout, period, device=dev)
                with torch.no_grad():
                    w = effective_weight(mpd.discriminators[i].convs[l + 1])
                    packed = _native.pack_period_conv_grad(w.reshape(cout, cin, 5))
                fl = 2.0 * B * cout * cin * 5 * hout * period
                kms = median_ms(lambda: _native.period_conv_input_grad(g, None, y, packed, cin, H, 0.1), args.iters,
                                args.warmup)
                tf = fl / kms / 1e9
                print(f"mpd-grad-bench B={B} period={period} layer={cin}->{cout} H={H} gflop={fl / 1e9:.2f} "
                      f"ms={kms:.3f} tflops={tf:.1f} peak_fraction={tf / PEAK_TFLOPS:.3f}")


if __name__ == "__main__":
    main()
