"""The whole training step (fastvocoder_amd/train.py) on HiFi-GAN light at the training shape, batch 32 x 140 frames:

  * ms per ``Trainer.step`` in both phases (STFT only; with the adversarial terms and the discriminator's update);
  * the split of the adversarial step: generator forward + backward of the STFT loss alone, the losses' share (the
    adversarial / feature-map terms through the discriminator, forward + backward down to the waveform), the
    discriminator's own update (forward of both signals + backward), and the two optimizer steps;
  * the fused clip + Adam (optim.Adam.step(max_norm), three launches) beside ``clip_grad_norm_`` + ``torch.optim.Adam``
    on the same generator and discriminator parameter sets, gradients in place.

``--grad-precision bf16`` runs all of it with ``Trainer(grad_precision="bf16")``: the generator's weight gradients on
the bf16 matrix cores (csrc/gen_grad_bf16.hip), everything else fp32.

Timing: after a warm-up, ``--reps`` windows of back-to-back calls between device events; the median and the spread
(min .. max) of the windows are reported.  Prints one JSON line.

    python tools/train_bench.py [--batch 32] [--frames 140] [--reps 5] [--target-s 0.5] [--use-mpd]
                                [--grad-precision {f32,bf16}]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import optim  # noqa: E402
from fastvocoder_amd.discriminator import Discriminator  # noqa: E402
from fastvocoder_amd.generator import HiFiGANGenerator  # noqa: E402
from fastvocoder_amd.loss import Loss, discriminator_step_terms, generator_adversarial_terms  # noqa: E402
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict  # noqa: E402
from fastvocoder_amd.train import Trainer  # noqa: E402

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
    return dict(ms=round(float(np.median(out)), 4), ms_min=round(float(min(out)), 4), ms_max=round(float(max(out)), 4))


def optimizer_rows(params, name, reps, target_s):
    """Fused clip + Adam against clip_grad_norm_ + torch.optim.Adam on one parameter set with fixed gradients."""
    params = [p.detach().clone().requires_grad_(True) for p in params]
    gen = torch.Generator(device="cpu").manual_seed(0)
    grads = [(1e-3 * torch.randn(p.shape, generator=gen)).to(p.device) for p in params]

    def fill():
        for p, g in zip(params, grads):
            p.grad = g.clone()

    ours, theirs = optim.Adam(params, lr=1e-4, eps=1e-6), torch.optim.Adam(params, lr=1e-4, eps=1e-6)
    # clip_grad_norm_ scales the gradients in place: both sides run on whatever the last step left, which costs the same
    fill()

    def fused():
        ours.step(max_norm=1.0)

    def eager():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        theirs.step()

    row = dict(parameters=name, tensors=len(params), elements=int(sum(p.numel() for p in params)),
               fused=windows_ms(fused, reps, target_s), torch=windows_ms(eager, reps, target_s))
    row["speedup"] = round(row["torch"]["ms"] / row["fused"]["ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=140)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.5)
    ap.add_argument("--use-mpd", action="store_true")
    ap.add_argument("--grad-precision", choices=["f32", "bf16"], default="f32")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = HiFiGANGenerator(**LIGHT)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", LIGHT, seed=0).items()})
    g = g.to(dev).train()
    d = Discriminator(use_mpd=args.use_mpd).to(dev)
    mel = torch.from_numpy(seeded_mel(args.frames, seed=1, batch=args.batch)).to(dev)
    wav = (0.1 * torch.randn(args.batch, args.frames * 240, generator=torch.Generator().manual_seed(2))).to(dev)
    kw = dict(lambda_stft=5.0, use_feature_map_loss=True, grad_clip_thresh=1.0)
    period = dict(period_grad=True) if args.use_mpd else {}

    def trainer(start):
        return Trainer(g, d, optim.Adam(g.parameters(), lr=1e-4, eps=1e-6), optim.Adam(d.parameters(), lr=5e-5, eps=1e-6),
                       discriminator_train_start_steps=start, grad_precision=args.grad_precision, **kw)

    out = dict(batch=args.batch, frames=args.frames, use_mpd=args.use_mpd, grad_precision=args.grad_precision,
               device=torch.cuda.get_device_name(0))
    t0, t1 = trainer(10 ** 9), trainer(0)
    out["step_stft_only"] = windows_ms(lambda: t0.step(mel, wav, 1), args.reps, args.target_s)
    out["step_adversarial"] = windows_ms(lambda: t1.step(mel, wav, 1), args.reps, args.target_s)

    # the split: each part alone, on the modules as the steps above left them
    loss = Loss().to(dev)
    loss.differentiable = True

    def generator_part():
        for p in g.parameters():
            p.grad = None
        est = g(mel)
        (5.0 * loss(est, wav)[0]).backward()

    def losses_part():
        est = wav.clone().requires_grad_(True)
        t = generator_adversarial_terms(d, est.unsqueeze(1), wav.unsqueeze(1), **period)
        (t["adversarial"] + t["feature_map"]).backward()

    def discriminator_part():
        for p in d.parameters():
            p.grad = None
        discriminator_step_terms(d, wav.unsqueeze(1), wav.flip(0).unsqueeze(1), stft_grad=True,
                                 **period)["discriminator"].backward()

    def inference_part():
        with torch.no_grad():
            g(mel)

    out["split"] = dict(generator_forward_backward=windows_ms(generator_part, args.reps, args.target_s),
                        adversarial_losses=windows_ms(losses_part, args.reps, args.target_s),
                        generator_inference_forward=windows_ms(inference_part, args.reps, args.target_s),
                        discriminator_update=windows_ms(discriminator_part, args.reps, args.target_s))
    out["optimizer"] = [optimizer_rows(list(g.parameters()), "generator", args.reps, args.target_s),
                        optimizer_rows(list(d.parameters()), "discriminator", args.reps, args.target_s)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
