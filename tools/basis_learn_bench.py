"""Learning Basis-MelGAN's basis (fastvocoder_amd/basis.py, csrc/basis_learn.hip) at the training shape of
conf/basis-melgan/light.yaml, batch 32 x 140 frames x 240 samples, L 30, C 256:

  * ms per whole step (forward, STFT loss, backward, clip + Adam) and its split -- the encode launch, the overlap-add,
    the STFT loss forward + backward on a fixed estimate, the gradient launch with its combine, the Adam step --
    beside eager torch autograd of the same graph (conv1d / relu / einsum / fold, the same STFT loss module, the same
    Adam) on the same GPU;
  * the encode kernel's written bytes per second beside the copy bandwidth measured on a tensor of W's size.

Timing: tools/basis_grad_bench.windows_ms (three warm-up calls, ``--reps`` windows of back-to-back calls between device
events; median and spread).  Prints one JSON line.

    python tools/basis_learn_bench.py [--batch 32] [--frames 140] [--reps 7] [--target-s 0.3] [--no-eager]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastvocoder_amd import _native, optim  # noqa: E402
from fastvocoder_amd.basis import BasisAutoencoder  # noqa: E402
from fastvocoder_amd.loss import MultiResolutionSTFTLoss  # noqa: E402
from tools.basis_grad_bench import _ms  # noqa: E402


def eager_forward(wav, enc, basis):
    """The same graph in eager torch on the device: conv1d on the right-padded waveform, relu, einsum, fold, cut."""
    C, L = enc.shape
    hop, n = L // 2, wav.shape[1]
    Fr = (n + hop - 1) // hop
    x = F.pad(wav, (0, (Fr - 1) * hop + L - n))
    W = torch.relu(F.conv1d(x[:, None, :], enc[:, None, :], stride=hop))
    frames = torch.einsum("jc,bcf->bjf", basis, W)
    out = F.fold(frames, output_size=(1, (Fr - 1) * hop + L), kernel_size=(1, L), stride=(1, hop))
    return out[:, 0, 0, : Fr * hop]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=140)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--target-s", type=float, default=0.3)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "basis_learn_bench measures on the ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(os.path.join(ROOT, "conf", "basis-melgan", "light.yaml")) as f:
        cfg = yaml.safe_load(f)
    L, C = cfg["L"], cfg["out_channels"]
    hop, n = L // 2, args.frames * 240
    torch.manual_seed(0)
    model = BasisAutoencoder(L=L, channels=C).to(dev)
    t = torch.arange(n, device=dev) / 24000.0
    wav = torch.stack([0.3 * torch.sin(2 * torch.pi * (150.0 + 7 * i) * t) for i in range(args.batch)])
    wav = (wav + 0.02 * torch.randn(args.batch, n, device=dev)).contiguous()
    stft = MultiResolutionSTFTLoss().to(dev)
    stft.differentiable = True
    opt = optim.Adam(model.parameters(), lr=1e-4, eps=1e-6)
    reps, target = args.reps, args.target_s

    def step():
        est, _ = model(wav)
        sc, mag = stft(est, wav)
        opt.zero_grad(set_to_none=True)
        (sc + mag).backward()
        opt.step(max_norm=1.0)

    Fr = _native.basis_frames(n, L)
    result = dict(tool="basis_learn_bench", batch=args.batch, samples=n, L=L, C=C, weight_frames=Fr,
                  device=torch.cuda.get_device_name(dev),
                  gemm_gflop_per_step=round(5 * 2.0 * args.batch * Fr * C * L / 1e9, 2),
                  W_mb=round(args.batch * C * Fr * 4 / 1e6, 1),
                  workspace_mb=round(_native.lib().fv_basis_learn_grad_workspace_bytes(args.batch, n, C, L) / 1e6, 1))
    result["step"] = _ms(step, reps, target)

    # the split, each part alone on fixed inputs
    enc = model.encoder.weight.detach().reshape(C, L).contiguous()
    basis = model.basis_signal.layer.weight.detach().contiguous()
    packed = _native.pack_basis(basis)
    W = _native.basis_encode(wav, enc)
    est = _native.basis_ola(W, packed, L)[:, 0, : Fr * hop].contiguous()
    g_est = torch.randn_like(est)
    split = {}
    split["encode"] = _ms(lambda: _native.basis_encode(wav, enc), reps, target)
    split["pack_basis + overlap_add"] = _ms(lambda: _native.basis_ola(W, _native.pack_basis(basis), L), reps, target)
    leaf = est.clone().requires_grad_(True)

    def loss_both():
        leaf.grad = None
        sc, mag = stft(leaf, wav)
        (sc + mag).backward()
    split["stft_loss forward + backward"] = _ms(loss_both, reps, target)
    split["learn_grad + combine"] = _ms(lambda: _native.basis_learn_grad(wav, g_est, W, basis), reps, target)
    for p in model.parameters():
        p.grad = torch.randn_like(p)
    split["clip + adam"] = _ms(lambda: opt.step(max_norm=1.0), reps, target)
    split["sum_of_parts_ms"] = round(sum(v["ms"] for v in split.values()), 4)
    result["split"] = split

    # the encode kernel against the copy bandwidth on W's size
    src, dst = torch.randn_like(W), torch.empty_like(W)
    copy = _ms(lambda: dst.copy_(src), reps, target)
    copy["gb_per_s"] = round(2 * W.numel() * 4 / (copy["ms"] * 1e-3) / 1e9, 1)
    written = round(W.numel() * 4 / (split["encode"]["ms"] * 1e-3) / 1e9, 1)
    result["encode_write"] = dict(written_gb_per_s=written, copy=copy,
                                  of_copy_bandwidth=round(written / copy["gb_per_s"], 3))

    if not args.no_eager:
        e = enc.clone().requires_grad_(True)
        b = basis.clone().requires_grad_(True)
        eager_opt = optim.Adam([e, b], lr=1e-4, eps=1e-6)

        def eager_step():
            sc, mag = stft(eager_forward(wav, e, b), wav)
            eager_opt.zero_grad(set_to_none=True)
            (sc + mag).backward()
            eager_opt.step(max_norm=1.0)
        result["eager_step"] = _ms(eager_step, reps, target)
        result["eager_over_native"] = round(result["eager_step"]["ms"] / result["step"]["ms"], 3)

        def eager_graph():
            e.grad = b.grad = None
            (eager_forward(wav, e, b) * g_est).sum().backward()
        result["eager_forward_backward_alone"] = _ms(eager_graph, reps, target)
        result["native_forward_backward_alone_ms"] = round(split["encode"]["ms"] + split["pack_basis + overlap_add"]["ms"]
                                                           + split["learn_grad + combine"]["ms"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
