"""Sustained ms of the whole discriminator's own update step (bin/train.py:143-188 without the optimizer):
loss.discriminator_step_terms (two forwards on the parameters' graph) and the backward through the kernels of
csrc/mpd_wgrad.hip, csrc/disc_wgrad.hip and the data-gradient kernels, for MultiPeriodDiscriminator, Discriminator()
and Discriminator(use_mpd=True), against the same step in eager torch autograd on the device with the same weights
(weight norm folded inside the graph, F.conv2d / F.conv1d / F.avg_pool1d / F.leaky_relu; the STFT magnitude, a constant
of the parameters, from the library in both), at B rows of n samples (default 32 x 33 600, the training shape); and
each new weight-gradient call alone, per period and layer, with the rate its 2 B H' p Cout Cin k operations amount to.
``--grad-precision bf16`` prints the bf16 figures beside the fp32 figures of the same run: per layer and period
``bf16_ms`` / ``bf16_tflops`` (fv_period_conv_weight_grad_bf16; the first layer has none), and per step row with an MPD
``bf16_ms`` / ``bf16_peak_mb`` (``grad_precision = "bf16"`` on the module).
Prints one JSON line.  Timing: tools/mel_bench.ms_per_call (warm-up, device events around back-to-back calls, best of
three).

    python tools/mpd_wgrad_bench.py [--samples 33600] [--batch 32] [--target-s 0.5] [--skip-kernels] [--modules mpd,discriminator,discriminator_mpd]
        [--grad-precision bf16]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import _native  # noqa: E402
from _ablib import use_lib_from_env  # noqa: E402
use_lib_from_env(_native)       # FV_AB_LIB=<a library build>: A/B of two builds
from fastvocoder_amd.discriminator import (Discriminator, DiscriminatorP, MelGANMultiScaleDiscriminator,  # noqa: E402
                                           MultiPeriodDiscriminator, MultiResolutionSTFTDiscriminator,
                                           STFTDiscriminator)
from fastvocoder_amd.discriminator.mpd import LRELU_SLOPE, PERIODS, period_heights  # noqa: E402
from fastvocoder_amd.loss import discriminator_step_terms  # noqa: E402
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402
from tools.mel_bench import ms_per_call  # noqa: E402
from tools.stft_loss_grad_bench import peak_mb  # noqa: E402

# (Cin, Cout, k, stride) of the layers fv_period_conv_weight_grad serves, by layer index
LAYERS = {1: (32, 128, 5, 3), 2: (128, 512, 5, 3), 3: (512, 1024, 5, 3), 4: (1024, 1024, 5, 1), 5: (1024, 1, 3, 1)}
KEYWORDS = {"mpd": dict(period_grad=True), "discriminator": dict(stft_grad=True),
            "discriminator_mpd": dict(stft_grad=True, period_grad=True)}


def _fold(conv):
    if hasattr(conv, "weight_g"):
        v, g = conv.weight_v, conv.weight_g
        return v * (g / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))))
    return conv.weight


def _eager_stack(d, v):
    for spec, conv in zip(d._spec, d._convs()):
        w = _fold(conv)
        if spec[0] == "grouped":
            _, k, pad, stride, slope = spec
            v = F.conv1d(v, w, conv.bias, stride=stride, padding=pad, groups=v.shape[1] // 4)
        else:
            _, k, pad, mode, slope = spec
            v = F.conv1d(F.pad(v, (pad, pad), mode="reflect") if mode else v, w, conv.bias, padding=0 if mode else pad)
        if slope != 1.0:
            v = F.leaky_relu(v, slope)
    return v


def eager_scores(m, x):
    """The score maps of ``m`` on x (B, 1, n) as eager torch on the module's own parameters."""
    if isinstance(m, DiscriminatorP):
        p = m.period
        n_pad = _native.mpd_reflect_tail(x.shape[-1], p)
        v = (F.pad(x, (0, n_pad), "reflect") if n_pad else x).view(x.shape[0], 1, -1, p)
        for j, conv in enumerate(m._convs()):
            v = F.conv2d(v, _fold(conv), conv.bias, stride=conv.stride, padding=conv.padding)
            if j < 5:
                v = F.leaky_relu(v, LRELU_SLOPE)
        return [v]
    if isinstance(m, MultiPeriodDiscriminator):
        return [s for d in m.discriminators for s in eager_scores(d, x)]
    if isinstance(m, STFTDiscriminator):
        with torch.no_grad():
            mag = _native.stft_magnitude_bins(x[:, 0].contiguous(), m._table(), m.fft_size, m.shift_size, m.win_length)
        return [_eager_stack(m, mag)]
    if isinstance(m, MultiResolutionSTFTDiscriminator):
        return [s for d in m.stft_discriminator for s in eager_scores(d, x)]
    if isinstance(m, MelGANMultiScaleDiscriminator):
        outs = []
        for i, d in enumerate(m.discriminators):
            outs.append(_eager_stack(d, x))
            if i + 1 < len(m.discriminators):
                x = F.avg_pool1d(x, *m._pool, count_include_pad=False)
        return outs
    if isinstance(m, Discriminator):
        return (eager_scores(m.mpd, x) if m.use_mpd else []) + eager_scores(m.msd, x) + eager_scores(m.mfd, x)
    raise TypeError(type(m).__name__)


def eager_step_fn(m):
    def step(xy):
        est, real = xy
        m.zero_grad(set_to_none=True)
        p, est_p = eager_scores(m, real), eager_scores(m, est.detach())
        L = len(p)
        loss = sum(((r - 1) ** 2).mean() for r in p) / L + sum((e ** 2).mean() for e in est_p) / L
        loss.backward()
        return loss
    return step


def kernel_rows(B, n, target_s, dev, bf16=False):
    """Each new weight-gradient call alone (both launches, with the bias gradient), per period and layer; ``bf16``:
    the bf16 entry on the same tensors beside it."""
    rows = []
    rs = np.random.RandomState(3)
    for p in PERIODS:
        _, hs = period_heights(n, p)
        hs = hs + [hs[-1], hs[-1]]                         # the two stride-1 layers keep the height
        g = torch.from_numpy(rs.randn(B, 32, hs[1], p).astype(np.float32)).to(dev)
        x = torch.from_numpy(rs.randn(B, 1, n).astype(np.float32)).to(dev)
        ms = ms_per_call(lambda a: _native.mpd_first_weight_grad(a[0], a[1], True, True), (g, x), target_s)
        gflop = 2.0 * B * hs[1] * p * 32 * 5 / 1e9
        rows.append({"period": p, "layer": 0, "cin": 1, "cout": 32, "k": 5, "stride": 3, "H": hs[0], "Hout": hs[1],
                     "ms": round(ms, 4), "gflop": round(gflop, 3), "tflops": round(gflop / ms, 3)})
        for li, (cin, cout, k, stride) in LAYERS.items():
            H, hout = hs[li], hs[li + 1]
            g = torch.from_numpy(rs.randn(B, cout, hout, p).astype(np.float32)).to(dev)
            x = torch.from_numpy(rs.randn(B, cin, H, p).astype(np.float32)).to(dev)
            ws = torch.empty(_native.period_conv_weight_grad_workspace_floats(B, cin, cout, H, p, k, stride), device=dev)
            fn = lambda a: _native.period_conv_weight_grad(a[0], a[1], k, stride, True, True, ws)  # noqa: E731
            ms = ms_per_call(fn, (g, x), target_s)
            gflop = 2.0 * B * hout * p * cout * cin * k / 1e9
            rows.append({"period": p, "layer": li, "cin": cin, "cout": cout, "k": k, "stride": stride, "H": H,
                         "Hout": hout, "workspace_mb": round(ws.numel() * 4 / 2 ** 20, 2), "ms": round(ms, 4),
                         "gflop": round(gflop, 3), "tflops": round(gflop / ms, 2)})
            if bf16:
                del ws
                ws = torch.empty(_native.period_conv_weight_grad_workspace_floats(B, cin, cout, H, p, k, stride, "bf16"),
                                 device=dev)
                fn16 = lambda a: _native.period_conv_weight_grad(a[0], a[1], k, stride, True, True, ws,  # noqa: E731
                                                                 precision="bf16")
                ms16 = ms_per_call(fn16, (g, x), target_s)
                rows[-1].update(bf16_workspace_mb=round(ws.numel() * 4 / 2 ** 20, 2), bf16_ms=round(ms16, 4),
                                bf16_tflops=round(gflop / ms16, 2), bf16_speedup=round(ms / ms16, 2))
            del g, x, ws
        torch.cuda.empty_cache()
    return rows


def step_row(name, B, n, target_s, dev, bf16=False):
    kind = "mpd" if name == "mpd" else "discriminator"
    m = MultiPeriodDiscriminator() if name == "mpd" else Discriminator(use_mpd=name == "discriminator_mpd")
    sd = seeded_discriminator_state_dict(kind, 13, **({"use_mpd": True} if name == "discriminator_mpd" else {}))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).eval()
    rs = np.random.RandomState(B)
    real = torch.from_numpy((0.5 * rs.randn(B, 1, n)).astype(np.float32)).to(dev)
    est = (real + 0.1 * torch.from_numpy(rs.randn(B, 1, n).astype(np.float32)).to(dev)).contiguous()

    def fused_step(xy):
        m.zero_grad(set_to_none=True)
        loss = discriminator_step_terms(m, xy[0], xy[1], **KEYWORDS[name])["discriminator"]
        loss.backward()
        return loss

    def forward_only(xy):
        with torch.no_grad():
            return discriminator_step_terms(m, xy[0], xy[1], **KEYWORDS[name])["discriminator"]

    eager_step = eager_step_fn(m)
    row = {"module": name, "fused_ms": round(ms_per_call(fused_step, (est, real), target_s), 3),
           "fused_forward_only_ms": round(ms_per_call(forward_only, (est, real), target_s), 3),
           "fused_peak_mb": round(peak_mb(fused_step, (est, real)), 1)}
    if bf16 and name != "discriminator":                     # (without the MPD there is nothing in bf16)
        m.grad_precision = "bf16"
        row.update(bf16_ms=round(ms_per_call(fused_step, (est, real), target_s), 3),
                   bf16_peak_mb=round(peak_mb(fused_step, (est, real)), 1))
        m.grad_precision = "f32"
    loss_f = float(fused_step((est, real)).detach())
    g_fused = {k: q.grad.clone() for k, q in m.named_parameters()}
    try:
        loss_e = float(eager_step((est, real)).detach())
        worst = max(float((g_fused[k] - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30))
                    for k, q in m.named_parameters())
        row.update(eager_ms=round(ms_per_call(eager_step, (est, real), target_s), 3),
                   eager_peak_mb=round(peak_mb(eager_step, (est, real)), 1), loss_fused=loss_f, loss_eager=loss_e,
                   grad_rel_max_vs_eager=worst)
        row["speedup"] = round(row["eager_ms"] / row["fused_ms"], 2)
    except RuntimeError as e:               # out of memory
        row.update(eager_ms=None, eager_peak_mb=None, speedup=None, eager_error=str(e)[:200])
    del m, g_fused
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=33600)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--target-s", type=float, default=0.5)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--modules", default="mpd,discriminator,discriminator_mpd")
    ap.add_argument("--grad-precision", choices=("f32", "bf16"), default="f32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mpd_wgrad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    B, n, bf16 = args.batch, args.samples, args.grad_precision == "bf16"
    out = {"tool": "mpd_wgrad_bench", "what": "discriminator step (two forwards + backward)", "B": B, "n": n,
           "grad_precision": args.grad_precision, "device": torch.cuda.get_device_name(dev)}
    if not args.skip_kernels:
        out["kernels"] = kernel_rows(B, n, args.target_s, dev, bf16)
        out["kernels_ms_total"] = round(sum(r["ms"] for r in out["kernels"]), 3)
        out["kernels_gflop_total"] = round(sum(r["gflop"] for r in out["kernels"]), 1)
        if bf16:                                              # the first layer's fp32 call counts in both totals
            out["kernels_bf16_ms_total"] = round(sum(r.get("bf16_ms", r["ms"]) for r in out["kernels"]), 3)
    out["steps"] = [step_row(name, B, n, args.target_s, dev, bf16) for name in args.modules.split(",") if name]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
