"""Sustained ms per call of the HIP Discriminator() forward and of a full score of one (estimate, real) pair (two
forwards + discriminator_terms), against the same work done by an eager torch chain on the same device with the same
folded weights (F.pad / F.conv1d / F.leaky_relu / F.avg_pool1d / torch.stft, then the train.py reductions), at
B = 1 and B = 16 rows of n = 240 000 samples.  Prints one JSON line.  Timing as tools/stft_loss_bench.py: every shape
warmed up first, then device events around back-to-back calls, best of three.  The per-kernel-family split comes
from one ``rocprofv3 --kernel-trace --stats -- python tools/discriminator_bench.py --hip-only`` run.

    python tools/discriminator_bench.py [--n 240000] [--batches 1,16] [--hip-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd.discriminator import Discriminator  # noqa: E402
from fastvocoder_amd.generator.engine import effective_weight  # noqa: E402
from fastvocoder_amd.loss import discriminator_terms  # noqa: E402
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402
from tools.mel_bench import ms_per_call  # noqa: E402

RESOLUTIONS = ((2048, 240, 1200), (1024, 120, 600), (512, 50, 240))


def forward_gflop(n):
    """Multiply-adds x 2 of one Discriminator() forward of one n-sample row (convs only)."""
    fl = 0.0

    def stack(cin, T, tap, scales, c0):
        nonlocal fl
        fl += 2.0 * c0 * cin * 15 * T
        c = c0
        for s in scales:
            T = (T - 1) // s + 1
            co = min(c * s, 1024)
            fl += 2.0 * co * 4 * tap(s) * T
            c = co
        fl += 2.0 * min(2 * c, 1024) * c * 5 * T + 2.0 * min(2 * c, 1024) * 3 * T

    T = n
    for _ in range(3):
        stack(1, T, lambda s: 10 * s + 1, (4, 4, 4, 4), 16)
        T = T // 2
    for nf, hop, _ in RESOLUTIONS:
        stack(nf // 2 + 1, 1 + n // hop, lambda s: 6 * s + 1, (4, 4), 64)
    return fl / 1e9


def eager_chain(d):
    """The reference's forward written with torch functionals, on the module's folded weights."""
    def convs(stack):
        out = []
        for spec, conv in zip(stack._spec, stack._convs()):
            out.append((spec, effective_weight(conv), conv.bias.detach().float(), conv.groups, conv.stride[0]))
        return out

    msd = [convs(m) for m in d.msd.discriminators]
    mfd = [(convs(m), m.window.float(), m.fft_size, m.shift_size, m.win_length) for m in d.mfd.stft_discriminator]

    def run_stack(x, layers):
        outs = []
        for spec, w, b, groups, stride in layers:
            kind, k, pad = spec[:3]
            slope = spec[-1]
            if kind == "dense" and spec[3] == 1:
                x = F.conv1d(F.pad(x, (pad, pad), mode="reflect"), w, b)
            else:
                x = F.conv1d(x, w, b, stride=stride, padding=pad, groups=groups)
            if slope != 1.0:
                x = F.leaky_relu(x, slope)
            outs.append(x)
        return outs

    def forward(x):
        outs = []
        y = x
        for layers in msd:
            outs.append(run_stack(y, layers))
            y = F.avg_pool1d(y, 4, 2, 1, count_include_pad=False)
        for layers, win, nf, hop, wl in mfd:
            S = torch.stft(x[:, 0], nf, hop, wl, win, return_complex=True)
            mag = torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-7))
            outs.append(run_stack(mag, layers))
        return outs

    def score(xy):
        est_p, p = forward(xy[0]), forward(xy[1])
        L = len(est_p)
        adv = sum(F.mse_loss(e[-1], torch.ones_like(e[-1])) for e in est_p) / L
        fm = sum(F.l1_loss(est_p[i][j], p[i][j]) for i in range(L) for j in range(len(est_p[i]) - 1))
        fm = fm / (L * (len(est_p[0]) - 1))
        real = sum(F.mse_loss(r[-1], torch.ones_like(r[-1])) for r in p) / L
        fake = sum(F.mse_loss(e[-1], torch.zeros_like(e[-1])) for e in est_p) / L
        return adv, fm, real + fake

    return forward, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=240000)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel-trace run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "discriminator_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    d = Discriminator()
    d.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict(seed=1).items()})
    d = d.to(dev).eval()
    gflop = forward_gflop(args.n)
    out = {"tool": "discriminator_bench", "n": args.n, "forward_gflop_per_row": round(gflop, 2),
           "device": torch.cuda.get_device_name(dev)}
    eager_fwd, eager_score = eager_chain(d)

    def hip_score(xy):
        return discriminator_terms(d(xy[0]), d(xy[1]))

    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            rs = np.random.RandomState(B)
            y = torch.from_numpy((0.3 * rs.randn(B, 1, args.n)).astype(np.float32)).to(dev)
            x = (y + 0.05 * torch.from_numpy(rs.randn(B, 1, args.n).astype(np.float32)).to(dev)).contiguous()
            fwd = ms_per_call(d, x)
            sc = ms_per_call(hip_score, (x, y))
            row = {"hip_forward_ms": round(fwd, 3), "hip_forward_tflops": round(B * gflop / fwd, 2),
                   "hip_score_ms": round(sc, 3)}
            if not args.hip_only:
                try:
                    efwd = ms_per_call(eager_fwd, x)
                    esc = ms_per_call(eager_score, (x, y))
                    h = hip_score((x, y))
                    e = eager_score((x, y))
                    row.update(eager_forward_ms=round(efwd, 3), eager_score_ms=round(esc, 3),
                               forward_speedup=round(efwd / fwd, 2), score_speedup=round(esc / sc, 2),
                               rel_diff_vs_eager={k: abs(float(h[k]) - float(v)) / abs(float(v)) for k, v in
                                                  zip(("adversarial", "feature_map", "discriminator"), e)})
                except RuntimeError as err:       # out of memory, or an op missing on the device
                    row.update(eager_forward_ms=None, eager_error=str(err)[:200])
            out[f"B{B}"] = row
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
