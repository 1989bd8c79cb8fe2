"""Sustained ms of the multi-scale discriminator's own update step (bin/train.py:143-188 without the optimizer):
loss.discriminator_step_terms (two forwards of MelGANMultiScaleDiscriminator() on the parameters' graph) and the
backward through the kernels of csrc/disc_wgrad.hip and csrc/disc_grad.hip, against the same step in eager torch
autograd on the device with the same weights (weight norm folded inside the graph, F.conv1d / F.avg_pool1d /
F.leaky_relu), at B rows of n samples (default 32 x 33 600, the training shape); and each weight-gradient kernel alone,
per layer of every scale, with the rate its 2 B Tout Cout (Cin | 4) k operations amount to.  Prints one JSON line.
Timing: tools/mel_bench.ms_per_call (warm-up, device events around back-to-back calls, best of three).

    python tools/msd_wgrad_bench.py [--samples 33600] [--batch 32] [--target-s 0.5] [--accuracy-rows 2]

``--accuracy-rows R`` adds the error of both float32 gradients against float64 eager autograd on the CPU at R rows of
n samples, per parameter tensor and relative to that tensor's largest magnitude (the worst tensor is named).
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
from fastvocoder_amd.discriminator import MelGANMultiScaleDiscriminator  # noqa: E402
from fastvocoder_amd.loss import discriminator_step_terms  # noqa: E402
from fastvocoder_amd.synthetic import seeded_discriminator_state_dict  # noqa: E402
from tools.mel_bench import ms_per_call  # noqa: E402
from tools.stft_loss_grad_bench import peak_mb  # noqa: E402


def eager_step_fn(msd):
    """The update step as eager torch autograd on the module's own parameters."""
    def fold(conv):
        if hasattr(conv, "weight_g"):
            v, g = conv.weight_v, conv.weight_g
            return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
        return conv.weight

    def run(x):
        outs = []
        for i, d in enumerate(msd.discriminators):
            v = x
            for spec, conv in zip(d._spec, d._convs()):
                w = fold(conv)
                if spec[0] == "grouped":
                    _, k, pad, stride, slope = spec
                    v = F.conv1d(v, w, conv.bias, stride=stride, padding=pad, groups=v.shape[1] // 4)
                else:
                    _, k, pad, mode, slope = spec
                    v = F.conv1d(F.pad(v, (pad, pad), mode="reflect") if mode else v, w, conv.bias,
                                 padding=0 if mode else pad)
                if slope != 1.0:
                    v = F.leaky_relu(v, slope)
            outs.append(v)
            if i + 1 < len(msd.discriminators):
                x = F.avg_pool1d(x, *msd._pool, count_include_pad=False)
        return outs

    def step(xy):
        est, real = xy
        msd.zero_grad(set_to_none=True)
        p, est_p = run(real), run(est.detach())
        L = len(p)
        loss = sum(((r - 1) ** 2).mean() for r in p) / L + sum((e ** 2).mean() for e in est_p) / L
        loss.backward()
        return loss
    return step


def kernel_rows(msd, B, n, target_s, dev):
    """Each weight-gradient call alone (both launches, with the bias gradient), per layer of every scale."""
    rows = []
    rs = np.random.RandomState(3)
    for si, d in enumerate(msd.discriminators):
        tin = n
        for _ in range(si):
            tin = msd._pooled_length(tin)
        cin = 1
        for li, (spec, conv) in enumerate(zip(d._spec, d._convs())):
            cout = conv.out_channels
            if spec[0] == "grouped":
                _, k, pad, stride, _ = spec
                tout, per = (tin + 2 * pad - k) // stride + 1, 4
            else:
                _, k, pad, mode, _ = spec
                stride, tout, per = 1, tin + 2 * pad - k + 1, cin
            g = torch.from_numpy(rs.randn(B, cout, tout).astype(np.float32)).to(dev)
            x = torch.from_numpy(rs.randn(B, cin, tin).astype(np.float32)).to(dev)
            if spec[0] == "grouped":
                ws = torch.empty(_native.conv_weight_grad_workspace_floats(True, B, cin, cout, tin, k, stride, pad),
                                 device=dev)
                fn = lambda a: _native.grouped_conv1d_weight_grad(a[0], a[1], k, stride, pad, True, True, ws)  # noqa: E731
            else:
                ws = torch.empty(_native.conv_weight_grad_workspace_floats(False, B, cin, cout, tin, k, 1, pad, mode),
                                 device=dev)
                fn = lambda a: _native.conv1d_weight_grad(a[0], a[1], k, pad, mode, True, True, ws)  # noqa: E731
            ms = ms_per_call(fn, (g, x), target_s)
            gflop = 2.0 * B * tout * cout * per * k / 1e9
            rows.append({"scale": si, "layer": li, "kind": spec[0], "cin": cin, "cout": cout, "k": k, "stride": stride,
                         "tin": tin, "tout": tout, "workspace_mb": round(ws.numel() * 4 / 2 ** 20, 2),
                         "ms": round(ms, 4), "gflop": round(gflop, 3), "tflops": round(gflop / ms, 2)})
            del g, x, ws
            cin, tin = cout, tout
        torch.cuda.empty_cache()
    return rows


def accuracy(msd, eager_step, fused_step, R, n, dev):
    """Worst per-tensor error of the fused and of the eager float32 gradient against float64 on the CPU."""
    rs = np.random.RandomState(100 + R)
    real = (0.5 * rs.randn(R, 1, n)).astype(np.float32)
    est = (real + 0.1 * rs.randn(R, 1, n)).astype(np.float32)
    m64 = MelGANMultiScaleDiscriminator()
    m64.load_state_dict({k: v.detach().cpu() for k, v in msd.state_dict().items()})
    m64 = m64.double()
    eager_step_fn(m64)((torch.from_numpy(est).double(), torch.from_numpy(real).double()))
    want = {k: q.grad.clone() for k, q in m64.named_parameters()}
    out = {"rows": R, "n": n}
    for name, step in (("fused", fused_step), ("eager", eager_step)):
        step((torch.from_numpy(est).to(dev), torch.from_numpy(real).to(dev)))
        errs = {k: float((q.grad.detach().cpu().double() - want[k]).abs().max() / want[k].abs().max().clamp_min(1e-300))
                for k, q in msd.named_parameters()}
        worst = max(errs, key=errs.get)
        out[name] = {"worst": worst, "rel_max": errs[worst]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=33600)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--target-s", type=float, default=0.5)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--accuracy-rows", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "msd_wgrad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    msd = MelGANMultiScaleDiscriminator()
    msd.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_discriminator_state_dict("msd", 13).items()})
    msd = msd.to(dev).eval()
    B, n = args.batch, args.samples
    out = {"tool": "msd_wgrad_bench", "what": "discriminator step (two forwards + backward), MSD", "B": B, "n": n,
           "device": torch.cuda.get_device_name(dev)}
    if not args.skip_kernels:
        out["kernels"] = kernel_rows(msd, B, n, args.target_s, dev)
        out["kernels_ms_total"] = round(sum(r["ms"] for r in out["kernels"]), 3)

    rs = np.random.RandomState(B)
    real = torch.from_numpy((0.5 * rs.randn(B, 1, n)).astype(np.float32)).to(dev)
    est = (real + 0.1 * torch.from_numpy(rs.randn(B, 1, n).astype(np.float32)).to(dev)).contiguous()

    def fused_step(xy):
        msd.zero_grad(set_to_none=True)
        loss = discriminator_step_terms(msd, xy[0], xy[1])["discriminator"]
        loss.backward()
        return loss

    def forward_only(xy):
        with torch.no_grad():
            return discriminator_step_terms(msd, xy[0], xy[1])["discriminator"]

    eager_step = eager_step_fn(msd)
    row = {"fused_ms": round(ms_per_call(fused_step, (est, real), args.target_s), 4),
           "fused_forward_only_ms": round(ms_per_call(forward_only, (est, real), args.target_s), 4),
           "fused_peak_mb": round(peak_mb(fused_step, (est, real)), 2)}
    loss_f = float(fused_step((est, real)).detach())
    g_fused = {k: q.grad.clone() for k, q in msd.named_parameters()}
    try:
        loss_e = float(eager_step((est, real)).detach())
        worst = max(float((g_fused[k] - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30))
                    for k, q in msd.named_parameters())
        row.update(eager_ms=round(ms_per_call(eager_step, (est, real), args.target_s), 4),
                   eager_peak_mb=round(peak_mb(eager_step, (est, real)), 2),
                   loss_fused=loss_f, loss_eager=loss_e, grad_rel_max_vs_eager=worst)
        row["speedup"] = round(row["eager_ms"] / row["fused_ms"], 2)
    except RuntimeError as e:               # out of memory
        row.update(eager_ms=None, eager_peak_mb=None, speedup=None, eager_error=str(e)[:200])
    out["step"] = row
    if args.accuracy_rows > 0:
        out["accuracy_vs_float64"] = accuracy(msd, eager_step, fused_step, args.accuracy_rows, n, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
