"""Basis-MelGAN's parameter gradient on conf/basis-melgan/light.yaml at the training shape (batch 32 x 140 frames):

  * forward + backward of ``basis_grad`` / ``parameter_grad`` (generator/basis_grad.py: ONE trunk pass over B + 1 rows,
    csrc/basis_grad.hip) beside eager torch autograd of the reference's TWO-PASS graph on the same GPU
    (oracle/torch_port.melgan_trunk on leaf copies of the trunk parameters, on the mel and on zeros_like(mel), the two
    differences), for the loss <c_est, est> + <c_w, weight>, with the peak device memory of one step of each;
  * the head adjoint alone, fv_basis_head_grad (one launch), beside the composed form it replaces --
    _native.conv_transpose1d_input_grad on the [C, 1, L] weight of a zero-padded g_est, then torch elementwise ops and
    a batch sum --, with the achieved bytes/s of its compulsory traffic (Y and g_w read, g_Y written) against the
    copy bandwidth measured on the same tensor size; fv_basis_head_forward and the two L1 entries likewise;
  * ms per whole ``Trainer.step`` in both phases (STFT + weight loss, and with the discriminator's terms and update).

Timing: after three warm-up calls, ``--reps`` windows of back-to-back calls (at least 20 per window) between device
events, the device synchronised after each; the median and the spread (min .. max) of the windows are reported.
Prints one JSON line.

    python tools/basis_grad_bench.py [--batch 32] [--frames 140] [--reps 7] [--target-s 0.3] [--no-eager] [--no-kernels]
                                     [--no-steps]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastvocoder_amd import _native, optim  # noqa: E402
from fastvocoder_amd.bin.synthesize import build_generator  # noqa: E402
from fastvocoder_amd.discriminator import Discriminator  # noqa: E402
from fastvocoder_amd.synthetic import seeded_mel, seeded_state_dict  # noqa: E402
from fastvocoder_amd.train import Trainer  # noqa: E402
from oracle import torch_port  # noqa: E402
from tools.generator_grad_bench import peak_mb  # noqa: E402

BASIS_KEY = "basis_signal.layer.weight"
MIN_CALLS = 20


def windows_ms(fn, reps, target_s):
    """ms per call of ``fn``: (median, min, max) over ``reps`` windows of at least MIN_CALLS back-to-back calls between
    device events, after three warm-up calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    n = max(MIN_CALLS, min(10000, int(target_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    out = []
    for _ in range(reps):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    return float(np.median(out)), float(min(out)), float(max(out))


def _ms(fn, reps, target_s):
    med, lo, hi = windows_ms(fn, reps, target_s)
    return dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))


def overlap_and_add(frames, hop):
    """[B, F, L] frames, L = 2 hop -> [B, (F - 1) hop + L]: the reference's overlap_and_add (an index_add_ over
    half-frames) with its index on the frames' device."""
    B, n, L = frames.shape
    halves = frames.reshape(B, 2 * n, hop)
    index = torch.arange(n + 1, device=frames.device).unfold(0, 2, 1).reshape(-1)
    return frames.new_zeros(B, n + 1, hop).index_add_(1, index, halves).reshape(B, -1)


def eager_generator(gen, cfg):
    """The reference's two-pass forward as eager torch on leaf copies of the trunk parameters; the basis a constant."""
    leaves = {k: v.detach().clone().requires_grad_(k != BASIS_KEY) for k, v in gen.named_parameters()}
    hop = cfg["L"] // 2

    def one(inp):
        w = torch.relu(torch_port.melgan_trunk(inp, leaves, cfg, with_last=False)).contiguous().transpose(1, 2)
        s = overlap_and_add(F.linear(w, leaves[BASIS_KEY]), hop)
        return s[:, : w.size(1) * hop], w

    def run(mel):
        zs, zw = one(torch.zeros_like(mel))
        s, w = one(mel)
        return s - zs, w - zw
    return run, {k: q for k, q in leaves.items() if k != BASIS_KEY}


def kernel_rows(B, C, Fr, L, reps, target_s, dev):
    rs = torch.Generator(device="cpu").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=rs).to(dev)

    hop = L // 2
    Y, basis, g_est, g_w = rnd(B + 1, C, Fr), rnd(L, C), rnd(B, Fr * hop), rnd(B, C, Fr)
    target = rnd(B, Fr, C)
    rows = {}
    src, dst = rnd(B + 1, C, Fr), torch.empty(B + 1, C, Fr, device=dev)
    copy = _ms(lambda: dst.copy_(src), reps, target_s)
    copy["gb_per_s"] = round(2 * src.numel() * 4 / (copy["ms"] * 1e-3) / 1e9, 1)
    rows["copy of [B+1, C, F]"] = copy

    def traffic(row, floats):
        row["gb_per_s"] = round(floats * 4 / (row["ms"] * 1e-3) / 1e9, 1)
        row["of_copy_bandwidth"] = round(row["gb_per_s"] / copy["gb_per_s"], 3)
        return row

    n, n1 = B * C * Fr, (B + 1) * C * Fr
    rows["basis_head_grad"] = traffic(_ms(lambda: _native.basis_head_grad(g_est, g_w, Y, basis), reps, target_s),
                                      2 * n1 + n + g_est.numel())
    rows["basis_head_grad, g_est alone"] = traffic(_ms(lambda: _native.basis_head_grad(g_est, None, Y, basis), reps,
                                                       target_s), 2 * n1 + g_est.numel())
    w = basis.t().contiguous().reshape(C, 1, L)
    padded = torch.zeros(B, 1, (Fr - 1) * hop + L, device=dev)

    def composed():
        padded[:, 0, : Fr * hop] = g_est
        post = _native.conv_transpose1d_input_grad(padded, w, Fr, hop, 0) + g_w
        out = torch.empty_like(Y)
        out[:B] = post * (Y[:B] > 0)
        out[B] = -post.sum(0) * (Y[B] > 0)
        return out
    worst = float((composed() - _native.basis_head_grad(g_est, g_w, Y, basis)).abs().max())
    rows["composed: conv_transpose1d_input_grad + torch"] = traffic(_ms(composed, reps, target_s), 2 * n1 + n + g_est.numel())
    rows["composed: conv_transpose1d_input_grad + torch"]["max_abs_against_fused"] = float(f"{worst:.3e}")
    rows["fused_over_composed"] = round(rows["basis_head_grad"]["ms"] /
                                        rows["composed: conv_transpose1d_input_grad + torch"]["ms"], 3)
    rows["basis_head_forward"] = traffic(_ms(lambda: _native.basis_head_forward(Y), reps, target_s), n1 + n)
    D = _native.basis_head_forward(Y)
    rows["basis_weight_l1"] = traffic(_ms(lambda: _native.basis_weight_l1(D, target), reps, target_s), 2 * n)
    rows["torch L1Loss on the view"] = _ms(lambda: F.l1_loss(D.transpose(1, 2), target), reps, target_s)
    rows["basis_weight_l1_grad"] = traffic(_ms(lambda: _native.basis_weight_l1_grad(D, target), reps, target_s), 3 * n)
    return rows


def step_rows(cfg, sd, mel, dev, reps, target_s):
    out = {}
    rate = int(np.prod(cfg["upsample_scales"]))
    wav = 0.3 * torch.randn(mel.shape[0], mel.shape[2] * rate * (cfg["L"] // 2), device=dev)
    weight = torch.rand(mel.shape[0], mel.shape[2] * rate, cfg["out_channels"], device=dev)
    for phase, start in (("stft_and_weight", 10 ** 9), ("adversarial", 0)):
        gen = build_generator("basis-melgan", cfg)
        gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        gen = gen.to(dev).train()
        torch.manual_seed(0)
        disc = Discriminator().to(dev)
        trainer = Trainer(gen, disc, optim.Adam(gen.melgan.parameters(), lr=1e-4, eps=1e-6),
                          optim.Adam(disc.parameters(), lr=5e-5, eps=1e-6), lambda_stft=cfg.get("lamda_stft", 1.0),
                          use_feature_map_loss=True, discriminator_train_start_steps=start, grad_clip_thresh=1.0,
                          basis_grad=True)
        step = [0]

        def one():
            step[0] += 1
            trainer.step(mel, wav, step[0], weight)
        out[phase] = dict(_ms(one, reps, target_s), peak_mb=round(peak_mb(one), 1))
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
    args = ap.parse_args()
    assert torch.cuda.is_available(), "basis_grad_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(os.path.join(ROOT, "conf", "basis-melgan", "light.yaml")) as f:
        cfg = yaml.safe_load(f)
    sd = seeded_state_dict("basis-melgan", cfg, seed=0)
    gen = build_generator("basis-melgan", cfg)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    gen = gen.to(dev)
    gen.basis_grad = True
    gen.parameter_grad = True
    mel = torch.from_numpy(seeded_mel(args.frames, seed=0, batch=args.batch)).to(dev)
    est, weight = gen(mel)
    c_est, c_w = torch.randn(est.shape, device=dev), torch.randn(weight.shape, device=dev).transpose(1, 2).contiguous()
    c_w = c_w.transpose(1, 2)                      # [B, F, C] in [B, C, F] storage, as loss.BasisWeightL1 hands it over
    del est, weight

    def loss(pair):
        return (pair[0] * c_est).sum() + (pair[1] * c_w).sum()

    def native_step():
        gen.zero_grad(set_to_none=True)
        loss(gen(mel)).backward()

    result = dict(tool="basis_grad_bench", model="basis-melgan light", batch=args.batch, frames=args.frames,
                  weight_frames=int(c_w.shape[1]), samples=int(c_est.shape[1]), device=torch.cuda.get_device_name(dev))
    result["native"] = dict(_ms(native_step, args.reps, args.target_s), peak_mb=round(peak_mb(native_step), 1))
    if not args.no_eager:
        run, leaves = eager_generator(gen, cfg)

        def eager_step():
            for q in leaves.values():
                q.grad = None
            loss(run(mel)).backward()
        result["eager_two_pass"] = dict(_ms(eager_step, args.reps, args.target_s), peak_mb=round(peak_mb(eager_step), 1))
        result["eager_over_native"] = round(result["eager_two_pass"]["ms"] / result["native"]["ms"], 3)
        worst = max(float((dict(gen.named_parameters())[k].grad - q.grad).abs().max() / q.grad.abs().max())
                    for k, q in leaves.items())
        result["native_vs_eager_max_rel"] = float(f"{worst:.3e}")
    if not args.no_kernels:
        result["kernels"] = kernel_rows(args.batch, cfg["out_channels"], int(c_w.shape[1]), cfg["L"], args.reps,
                                        min(args.target_s, 0.1), dev)
    if not args.no_steps:
        result["trainer_step"] = step_rows(cfg, sd, mel, dev, args.reps, args.target_s)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
