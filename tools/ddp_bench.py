"""What data-parallel training adds to a step, on ONE GPU (HiFi-GAN light's 234 gradients, the discriminator's 108):

  * the pack launch (fv_grad_bucket_pack: every gradient into its span of the flat bucket, times 1 / world) over a
    table that is already on the device;
  * beside it ``torch.cat`` of the same gradients followed by a multiply -- what one would write without the kernel --
    and a device-to-device copy of the same bytes (the bandwidth a pure copy of that size reaches);
  * ``optim.Adam.step(max_norm, process_group=<one-rank RCCL group>)`` beside ``step(max_norm)``: table, pack,
    all-reduce, norm, Adam against table, norm, Adam;
  * ``Trainer.step`` with the one-rank group beside ``Trainer.step`` without one, batch 32 x 140 frames, both phases:
    the price of the path (pack, a one-rank all-reduce per optimizer step, one for the scalars).

Timing as tools/train_bench.py: after a warm-up, ``--reps`` windows of back-to-back calls between device events; median
and spread.  Prints one JSON line.  Scaling over several GPUs is not measured here: it needs a node with more than one.

    python tools/ddp_bench.py [--batch 32] [--frames 140] [--reps 5] [--target-s 0.5] [--pack-only]

``--pack-only`` stops after the pack rows and opens no process group: the run to put under a kernel trace for the
launch's own device time (``rocprofv3 --kernel-trace --stats -- python tools/ddp_bench.py --pack-only``).
"""
import argparse
import datetime
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastvocoder_amd import _native, optim  # noqa: E402
from fastvocoder_amd.discriminator import Discriminator  # noqa: E402
from fastvocoder_amd.generator import HiFiGANGenerator  # noqa: E402
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict  # noqa: E402
from fastvocoder_amd.train import Trainer  # noqa: E402
from tools.train_bench import LIGHT, windows_ms  # noqa: E402


def pack_rows(params, name, reps, target_s):
    dev = params[0].device
    gen = torch.Generator(device="cpu").manual_seed(0)
    grads = [(1e-3 * torch.randn(p.shape, generator=gen)).to(dev) for p in params]
    offsets, total = optim.bucket_layout(params)
    flat = torch.empty(total, dtype=torch.float32, device=dev)
    rows = [(0, flat.data_ptr() + 4 * off, 0, 0, p.numel(), 1.0, 1.0) for p, off in zip(params, offsets)]
    host, first = optim.adam_table(rows, [g.data_ptr() for g in grads])
    table = torch.from_numpy(host).to(dev)
    n_tensors, n_chunks = len(rows), int(first[-1])
    other = torch.empty_like(flat)

    def pack():
        _native.grad_bucket_pack(table, n_tensors, n_chunks, 0.125)

    def cat_mul():
        return torch.cat([g.reshape(-1) for g in grads]) * 0.125

    def copy():
        other.copy_(flat)

    row = dict(gradients=name, tensors=n_tensors, elements=int(sum(p.numel() for p in params)), bucket_floats=total,
               chunks=n_chunks, pack=windows_ms(pack, reps, target_s), cat_mul=windows_ms(cat_mul, reps, target_s),
               copy=windows_ms(copy, reps, target_s))
    moved = 2 * 4 * total                                      # read once, written once
    row["pack"]["gb_per_s"] = round(moved / (row["pack"]["ms"] * 1e-3) / 1e9, 1)
    row["copy"]["gb_per_s"] = round(moved / (row["copy"]["ms"] * 1e-3) / 1e9, 1)
    row["cat_mul_over_pack"] = round(row["cat_mul"]["ms"] / row["pack"]["ms"], 2)
    return row


def step_rows(params, name, group, reps, target_s):
    params = [p.detach().clone().requires_grad_(True) for p in params]
    gen = torch.Generator(device="cpu").manual_seed(0)
    grads = [(1e-3 * torch.randn(p.shape, generator=gen)).to(p.device) for p in params]
    plain, bucket = optim.Adam(params, lr=1e-4, eps=1e-6), optim.Adam(params, lr=1e-4, eps=1e-6)

    def fill():
        for p, g in zip(params, grads):
            p.grad = g

    def without():
        fill()
        plain.step(max_norm=1.0)

    def with_group():
        fill()
        bucket.step(max_norm=1.0, process_group=group)

    row = dict(parameters=name, without_group=windows_ms(without, reps, target_s),
               with_group=windows_ms(with_group, reps, target_s))
    row["added_ms"] = round(row["with_group"]["ms"] - row["without_group"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=140)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.5)
    ap.add_argument("--pack-only", action="store_true", help="the pack rows alone, no process group")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    g = HiFiGANGenerator(**LIGHT)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict("hifigan", LIGHT, seed=0).items()})
    g = g.to(dev).train()
    d = Discriminator().to(dev)
    out = dict(batch=args.batch, frames=args.frames, device=torch.cuda.get_device_name(0))
    out["pack"] = [pack_rows(list(g.parameters()), "generator", args.reps, args.target_s),
                   pack_rows(list(d.parameters()), "discriminator", args.reps, args.target_s)]
    if args.pack_only:
        print(json.dumps(out))
        return
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29570")
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=datetime.timedelta(seconds=120), device_id=dev)
    group = dist.group.WORLD
    out["optimizer_step"] = [step_rows(list(g.parameters()), "generator", group, args.reps, args.target_s),
                             step_rows(list(d.parameters()), "discriminator", group, args.reps, args.target_s)]

    mel = torch.from_numpy(seeded_mel(args.frames, seed=1, batch=args.batch)).to(dev)
    wav = (0.1 * torch.randn(args.batch, args.frames * 240, generator=torch.Generator().manual_seed(2))).to(dev)

    def trainer(start, grp):
        return Trainer(g, d, optim.Adam(g.parameters(), lr=1e-4, eps=1e-6), optim.Adam(d.parameters(), lr=5e-5, eps=1e-6),
                       lambda_stft=5.0, use_feature_map_loss=True, grad_clip_thresh=1.0,
                       discriminator_train_start_steps=start, process_group=grp)

    for phase, start in (("stft_only", 10 ** 9), ("adversarial", 0)):
        plain, grouped = trainer(start, None), trainer(start, group)
        a = windows_ms(lambda: plain.step(mel, wav, 1), args.reps, args.target_s)
        b = windows_ms(lambda: grouped.step(mel, wav, 1), args.reps, args.target_s)
        out["trainer_step_" + phase] = dict(without_group=a, one_rank_group=b, added_ms=round(b["ms"] - a["ms"], 4),
                                            samples_per_s_one_rank=round(args.batch / (b["ms"] * 1e-3), 1))
    out["scaling_over_ranks"] = "not measured (one GPU)"
    print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
