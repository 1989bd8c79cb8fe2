"""The generator's half of the training step on HiFi-GAN light at the training shape (batch 32 x 140 frames):

  * forward + backward of ``parameter_grad`` (generator/grad.py, csrc/gen_grad.hip) beside eager torch autograd of the
    same chain on the same GPU (F.conv1d / F.conv_transpose1d / F.leaky_relu on the folded weights, written here),
    with the peak device memory of one step of each;
  * each new kernel alone per layer of the model: ms, TFLOP/s of the layer's algorithmic FLOPs and the fraction of the
    157 TF fp32 matrix peak;
  * with ``--grad-precision bf16``: the forward + backward with ``grad_precision = "bf16"``, and beside every fp32
    weight-gradient row the row of the bf16 entry (csrc/gen_grad_bf16.hip) with its fraction of the 2517 TF bf16
    matrix peak.  Eager autograd stays fp32: the two are then not the same arithmetic.

Timing: after a warm-up, ``--reps`` windows of back-to-back calls between device events; the median and the spread
(min .. max) of the windows are reported.  Prints one JSON line.

    python tools/generator_grad_bench.py [--batch 32] [--frames 140] [--reps 7] [--target-s 0.3] [--no-eager]
                                         [--grad-precision {f32,bf16}]
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
from fastvocoder_amd.generator import HiFiGANGenerator  # noqa: E402
from fastvocoder_amd.generator.engine import effective_weight  # noqa: E402
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict  # noqa: E402

PEAK_TF = 157.3          # fp32 matrix peak of the MI355X
PEAK_BF16_TF = 2516.8    # its bf16 matrix peak (16 x)
LIGHT = dict(resblock_kernel_sizes=[3, 7, 11], upsample_rates=[8, 5, 3, 2], upsample_initial_channel=256,
             resblock_type="1", upsample_kernel_sizes=[16, 10, 6, 4],
             resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], transposedconv=True, bias=True)


def windows_ms(fn, reps, target_s):
    """ms per call of ``fn``: (median, min, max) over ``reps`` windows of back-to-back calls between device events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    n = max(1, min(10000, int(target_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    out = []
    for _ in range(reps):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    return float(np.median(out)), float(min(out)), float(max(out))


def eager_generator(gen):
    """The module's forward as eager torch on leaf copies of its parameters (weight norm folded by torch._weight_norm)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in gen.named_parameters()}

    def w(p):
        if p + ".weight" in leaves:
            return leaves[p + ".weight"]
        return torch._weight_norm(leaves[p + ".weight_v"], leaves[p + ".weight_g"], 0)

    def b(p):
        return leaves.get(p + ".bias")

    nk = gen.num_kernels

    def run(mel):
        x = F.conv1d(mel, w("conv_pre"), b("conv_pre"), padding=3)
        for i, up in enumerate(gen.ups):
            x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w(f"ups.{i}"), b(f"ups.{i}"), stride=up.stride[0],
                                   padding=up.padding[0], output_padding=up.output_padding[0])
            xs = None
            for j in range(nk):
                blk, p, r = gen.resblocks[i * nk + j], f"resblocks.{i * nk + j}", x
                for m, c1 in enumerate(blk.convs1):
                    t = F.conv1d(F.leaky_relu(r, 0.1), w(f"{p}.convs1.{m}"), b(f"{p}.convs1.{m}"), padding=c1.padding[0],
                                 dilation=c1.dilation[0])
                    c2 = blk.convs2[m]
                    r = F.conv1d(F.leaky_relu(t, 0.1), w(f"{p}.convs2.{m}"), b(f"{p}.convs2.{m}"), padding=c2.padding[0]) + r
                xs = r if xs is None else xs + r
            x = xs / nk
        return torch.tanh(F.conv1d(F.leaky_relu(x), w("conv_post"), b("conv_post"), padding=3))[:, 0, :]
    return run, leaves


def peak_mb(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_rows(gen, B, frames, reps, target_s, dev, bf16=False):
    """Each new kernel alone on every distinct layer shape of the model; ``bf16``: the bf16 weight-gradient entries
    beside the fp32 ones."""
    rows, rs = [], torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=rs).to(dev)

    def row(kind, shape, flops, fn, peak=PEAK_TF):
        med, lo, hi = windows_ms(fn, reps, target_s)
        tf = flops / (med * 1e-3) / 1e12
        rows.append(dict(kernel=kind, shape=shape, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                         tflops=round(tf, 2), peak_fraction=round(tf / peak, 4)))

    t, seen = frames, set()
    convs = [(gen.conv_pre, t)]
    for i, up in enumerate(gen.ups):
        convs.append((up, t))
        t = (t - 1) * up.stride[0] - 2 * up.padding[0] + up.kernel_size[0] + up.output_padding[0]
        for j in range(gen.num_kernels):
            blk = gen.resblocks[i * gen.num_kernels + j]
            convs += [(c, t) for c in list(blk.convs1) + list(blk.convs2)]
    convs.append((gen.conv_post, t))
    for conv, tin in convs:
        k = conv.kernel_size[0]
        if isinstance(conv, torch.nn.ConvTranspose1d):
            cin, cout, s, p, op = conv.in_channels, conv.out_channels, conv.stride[0], conv.padding[0], conv.output_padding[0]
            key = ("convt", cin, cout, k, s)
            if key in seen:
                continue
            seen.add(key)
            tout = (tin - 1) * s - 2 * p + k + op
            g, xa, w = rnd(B, cout, tout), rnd(B, cin, tin), rnd(cin, cout, k)
            flops = 2.0 * B * tin * cin * cout * k
            ws = torch.empty(_native.conv_transpose1d_weight_grad_workspace_floats(B, cin, cout, tin, k, s, p, op),
                             device=dev)
            row("conv_transpose1d_weight_grad", [cin, cout, k, s, tin], flops,
                lambda: _native.conv_transpose1d_weight_grad(g, xa, k, s, p, op, True, True, workspace=ws))
            if bf16:
                wsb = torch.empty(_native.conv_transpose1d_weight_grad_workspace_floats(B, cin, cout, tin, k, s, p, op,
                                                                                        "bf16"), device=dev)
                row("conv_transpose1d_weight_grad_bf16", [cin, cout, k, s, tin], flops,
                    lambda: _native.conv_transpose1d_weight_grad(g, xa, k, s, p, op, True, True, workspace=wsb,
                                                                 precision="bf16"), PEAK_BF16_TF)
            row("conv_transpose1d_input_grad", [cin, cout, k, s, tin], flops,
                lambda: _native.conv_transpose1d_input_grad(g, w, tin, s, p, op))
        else:
            cin, cout, dil, pad = conv.in_channels, conv.out_channels, conv.dilation[0], conv.padding[0]
            key = ("conv", cin, cout, k, dil)
            if key in seen:
                continue
            seen.add(key)
            tout = tin + 2 * pad - dil * (k - 1)
            g, xa = rnd(B, cout, tout), rnd(B, cin, tin)
            ws = torch.empty(_native.conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, tin, k, dil, pad), device=dev)
            row("conv1d_weight_grad_dilated", [cin, cout, k, dil, tin], 2.0 * B * tout * cin * cout * k,
                lambda: _native.conv1d_weight_grad_dilated(g, xa, k, dil, pad, True, True, workspace=ws))
            if bf16:
                wsb = torch.empty(_native.conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, tin, k, dil, pad,
                                                                                      precision="bf16"), device=dev)
                row("conv1d_weight_grad_dilated_bf16", [cin, cout, k, dil, tin], 2.0 * B * tout * cin * cout * k,
                    lambda: _native.conv1d_weight_grad_dilated(g, xa, k, dil, pad, True, True, workspace=wsb,
                                                               precision="bf16"), PEAK_BF16_TF)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=140)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--target-s", type=float, default=0.3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--grad-precision", choices=["f32", "bf16"], default="f32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "generator_grad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = HiFiGANGenerator(**LIGHT)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", LIGHT, seed=0).items()})
    gen = gen.to(dev)
    gen.parameter_grad = True
    gen.grad_precision = args.grad_precision
    mel = torch.from_numpy(seeded_mel(args.frames, seed=0, batch=args.batch)).to(dev)
    n = gen(mel).shape[1]
    c = torch.randn(args.batch, n, device=dev)

    def native_step():
        gen.zero_grad(set_to_none=True)
        gen(mel).backward(c)

    result = dict(tool="generator_grad_bench", model="hifigan light", batch=args.batch, frames=args.frames, samples=n,
                  grad_precision=args.grad_precision, device=torch.cuda.get_device_name(dev))
    med, lo, hi = windows_ms(native_step, args.reps, args.target_s)
    result["native"] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), peak_mb=round(peak_mb(native_step), 1))
    if not args.no_eager:
        run, leaves = eager_generator(gen)

        def eager_step():
            for q in leaves.values():
                q.grad = None
            run(mel).backward(c)
        med, lo, hi = windows_ms(eager_step, args.reps, args.target_s)
        result["eager"] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), peak_mb=round(peak_mb(eager_step), 1))
        result["eager_over_native"] = round(result["eager"]["ms"] / result["native"]["ms"], 3)
        worst = max(float((dict(gen.named_parameters())[k].grad - q.grad).abs().max() / q.grad.abs().max())
                    for k, q in leaves.items())
        result["native_vs_eager_max_rel"] = float(f"{worst:.3e}")
    if not args.no_kernels:
        result["kernels"] = kernel_rows(gen, args.batch, args.frames, args.reps, min(args.target_s, 0.1), dev,
                                        bf16=args.grad_precision == "bf16")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
