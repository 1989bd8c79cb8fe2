"""MelGAN's parameter gradient on conf/melgan/original.yaml at the training shape (batch 32 x 140 frames):

  * forward + backward of ``stack_grad`` / ``parameter_grad`` (generator/stack_grad.py, csrc/gen_grad.hip) beside eager
    torch autograd of the same graph on the same GPU (oracle/torch_port.melgan_trunk on leaf copies of the
    parameters), with the peak device memory of one step of each;
  * each new kernel alone per distinct layer shape of the model -- the weight gradient through the reflection pad
    (fv_conv1d_weight_grad_dilated_mode) and the one-launch data gradient (fv_conv1d_input_grad_reflect), the latter
    beside the two-pass form it replaces (fv_conv1d_fused over the full correlation + fv_reflect_pad_fold): ms, TFLOP/s
    of the layer's algorithmic FLOPs and the fraction of the 157 TF fp32 matrix peak;
  * the pointwise and skip 1x1 weight gradients of a stack as two calls beside ONE call over the concatenated columns
    [lrelu(h) ; x] (what a fused entry would run, timed with the concatenation already made);
  * ms per whole ``Trainer.step`` in both phases (STFT only, and with the discriminator's terms and update);
  * with ``--grad-precision bf16``: the forward + backward and the steps with ``grad_precision = "bf16"``, and beside
    every fp32 weight-gradient row the row of the bf16 entry (csrc/gen_grad_bf16.hip) with its fraction of the bf16
    matrix peak.  Eager autograd stays fp32: the two are then not the same arithmetic.

Timing: after a warm-up, ``--reps`` windows of back-to-back calls between device events; the median and the spread
(min .. max) of the windows are reported.  Prints one JSON line.

    python tools/melgan_grad_bench.py [--batch 32] [--frames 140] [--reps 7] [--target-s 0.3] [--no-eager] [--no-kernels]
                                      [--no-steps] [--grad-precision {f32,bf16}]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastvocoder_amd import _native, optim  # noqa: E402
from _ablib import use_lib_from_env  # noqa: E402
use_lib_from_env(_native)       # FV_AB_LIB=<a library build>: A/B of two builds
from fastvocoder_amd.bin.synthesize import build_generator  # noqa: E402
from fastvocoder_amd.discriminator import Discriminator  # noqa: E402
from fastvocoder_amd.generator.modules import ResidualStack  # noqa: E402
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict  # noqa: E402
from fastvocoder_amd.train import Trainer  # noqa: E402
from oracle import torch_port  # noqa: E402
from tools.generator_grad_bench import PEAK_BF16_TF, PEAK_TF, peak_mb, windows_ms  # noqa: E402


def kernel_rows(gen, B, frames, reps, target_s, dev, bf16=False):
    rows, rs = [], torch.Generator(device="cpu").manual_seed(0)
    R = _native.PAD_REFLECT

    def rnd(*shape):
        return torch.randn(*shape, generator=rs).to(dev)

    def row(kind, shape, flops, fn, peak=PEAK_TF):
        med, lo, hi = windows_ms(fn, reps, target_s)
        tf = flops / (med * 1e-3) / 1e12
        rows.append(dict(kernel=kind, shape=shape, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                         tflops=round(tf, 2), peak_fraction=round(tf / peak, 4)))

    # (conv, pad, input length, has a data gradient) of every conv behind the pad, and the stacks' 1x1 pairs
    t, padded, pairs = frames, [], []
    for m in gen.melgan:
        if isinstance(m, torch.nn.ConvTranspose1d):
            t = (t - 1) * m.stride[0] - 2 * m.padding[0] + m.kernel_size[0] + m.output_padding[0]
        elif isinstance(m, ResidualStack):
            padded.append((m.stack[2], m._pad, t, True))
            pairs.append((m.channels, t))
        elif isinstance(m, torch.nn.Conv1d):
            padded.append((m, gen._first_pad[0], t, False))
    last = gen.melgan[-2 if isinstance(gen.melgan[-1], torch.nn.Tanh) else -1]
    padded.append((last.conv, last._pad, t, True))
    seen = set()
    for conv, pad, tin, data in padded:
        cin, cout, k, dil = conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.dilation[0]
        if (cin, cout, k, dil) in seen:
            continue
        seen.add((cin, cout, k, dil))
        g, xa, w = rnd(B, cout, tin), rnd(B, cin, tin), rnd(cout, cin, k)
        flops = 2.0 * B * tin * cin * cout * k
        ws = torch.empty(_native.conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, tin, k, dil, pad, R), device=dev)
        row("conv1d_weight_grad_dilated_mode", [cin, cout, k, dil, tin], flops,
            lambda: _native.conv1d_weight_grad_dilated(g, xa, k, dil, pad, True, True, workspace=ws, pad_mode=R))
        if bf16:
            wsb = torch.empty(_native.conv1d_weight_grad_dilated_workspace_floats(B, cin, cout, tin, k, dil, pad, R, "bf16"),
                              device=dev)
            row("conv1d_weight_grad_dilated_bf16", [cin, cout, k, dil, tin], flops,
                lambda: _native.conv1d_weight_grad_dilated(g, xa, k, dil, pad, True, True, workspace=wsb, pad_mode=R,
                                                           precision="bf16"), PEAK_BF16_TF)
        if not data:
            continue
        wt = w.transpose(0, 1).contiguous()
        row("conv1d_input_grad_reflect", [cin, cout, k, dil, tin], flops,
            lambda: _native.conv1d_input_grad_reflect(g, wt, tin, dil, pad))
        flipped = _native.pack_conv1d(w.flip(2).transpose(0, 1).contiguous())
        row("two-pass: conv1d_fused + reflect_pad_fold", [cin, cout, k, dil, tin], flops,
            lambda: _native.reflect_pad_fold(_native.conv1d_fused(g, flipped, None, cin, k, dil=dil, pad=dil * (k - 1)),
                                             pad))
    seen = set()
    for ch, tin in pairs:
        if (ch, tin) in seen:
            continue
        seen.add((ch, tin))
        g, ha, x = rnd(B, ch, tin), rnd(B, ch, tin), rnd(B, ch, tin)
        both = torch.cat([ha, x], dim=1).contiguous()
        flops = 2.0 * B * tin * ch * ch * 2
        floats = _native.conv1d_weight_grad_dilated_workspace_floats
        ws = torch.empty(max(floats(B, 2 * ch, ch, tin, 1, 1, 0), floats(B, ch, ch, tin, 1, 1, 0)), device=dev)

        def two():
            _native.conv1d_weight_grad_dilated(g, ha, 1, 1, 0, True, True, workspace=ws)
            _native.conv1d_weight_grad_dilated(g, x, 1, 1, 0, True, True, workspace=ws)
        row("pointwise + skip weight grad: two calls", [ch, tin], flops, two)
        row("pointwise + skip weight grad: one call on [lrelu(h) ; x]", [ch, tin], flops,
            lambda: _native.conv1d_weight_grad_dilated(g, both, 1, 1, 0, True, True, workspace=ws))
        if bf16:
            wsb = torch.empty(floats(B, ch, ch, tin, 1, 1, 0, precision="bf16"), device=dev)

            def two_bf16():
                _native.conv1d_weight_grad_dilated(g, ha, 1, 1, 0, True, True, workspace=wsb, precision="bf16")
                _native.conv1d_weight_grad_dilated(g, x, 1, 1, 0, True, True, workspace=wsb, precision="bf16")
            row("pointwise + skip weight grad: two bf16 calls", [ch, tin], flops, two_bf16, PEAK_BF16_TF)
    return rows


def eager_generator(gen, cfg):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in gen.named_parameters()}
    return (lambda mel: torch.tanh(torch_port.melgan_trunk(mel, leaves, cfg))[:, 0, :]), leaves


def step_rows(cfg, sd, mel, dev, reps, target_s, grad_precision="f32"):
    out = {}
    spf = int(np.prod(cfg["upsample_scales"]))
    wav = 0.3 * torch.randn(mel.shape[0], mel.shape[2] * spf, device=dev)
    for phase, start in (("stft_only", 10 ** 9), ("adversarial", 0)):
        gen = build_generator("melgan", cfg)
        gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        gen = gen.to(dev).train()
        torch.manual_seed(0)
        disc = Discriminator().to(dev)
        trainer = Trainer(gen, disc, optim.Adam(gen.parameters(), lr=1e-4, eps=1e-6),
                          optim.Adam(disc.parameters(), lr=5e-5, eps=1e-6), lambda_stft=cfg.get("lamda_stft", 1.0),
                          use_feature_map_loss=True, discriminator_train_start_steps=start, grad_clip_thresh=1.0,
                          stack_grad=True, grad_precision=grad_precision)
        step = [0]

        def one():
            step[0] += 1
            trainer.step(mel, wav, step[0])
        med, lo, hi = windows_ms(one, reps, target_s)
        out[phase] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), peak_mb=round(peak_mb(one), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=140)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--target-s", type=float, default=0.3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--grad-precision", choices=["f32", "bf16"], default="f32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "melgan_grad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(os.path.join(ROOT, "conf", "melgan", "original.yaml")) as f:
        cfg = yaml.safe_load(f)
    sd = seeded_state_dict("melgan", cfg, seed=0)
    gen = build_generator("melgan", cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    gen = gen.to(dev)
    gen.stack_grad = True
    gen.parameter_grad = True
    gen.grad_precision = args.grad_precision
    mel = torch.from_numpy(seeded_mel(args.frames, seed=0, batch=args.batch)).to(dev)
    n = gen(mel).shape[1]
    c = torch.randn(args.batch, n, device=dev)

    def native_step():
        gen.zero_grad(set_to_none=True)
        gen(mel).backward(c)

    result = dict(tool="melgan_grad_bench", model="melgan original", batch=args.batch, frames=args.frames, samples=n,
                  grad_precision=args.grad_precision, device=torch.cuda.get_device_name(dev))
    med, lo, hi = windows_ms(native_step, args.reps, args.target_s)
    result["native"] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), peak_mb=round(peak_mb(native_step), 1))
    if not args.no_eager:
        run, leaves = eager_generator(gen, cfg)

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
    if not args.no_steps:
        result["trainer_step"] = step_rows(cfg, sd, mel, dev, args.reps, args.target_s, args.grad_precision)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
