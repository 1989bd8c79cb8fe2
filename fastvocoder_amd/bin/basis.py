"""``MODE=basis``: learn Basis-MelGAN's basis and write the dataset ``MODE=train --model_name basis-melgan`` reads.

The reference takes ``Basis-MelGAN-dataset/`` from a separate project (its README: "Refer to ConvTasNet4BasisMelGAN to
get dataset for Basis-MelGAN").  That project's code, loss and hyper-parameters are not known here and are not guessed
at: this flow trains ``basis.BasisAutoencoder`` (Conv-TasNet's encoder / decoder pair with no separator) on the
multi-resolution STFT loss this repository already has, with the optimizer settings of ``MODE=train``, and writes the
file formats ``MODE=train`` reads.  ``--lambda_wave`` adds a time-domain mean-squared-error term; its default is 0 and
no default was tuned.

``--stage learn``: crops from ``data.load_data_to_buffer`` + ``data.BatchIterator`` (the mel only fixes the crop
geometry), the loss ``sc + mag`` of ``MultiResolutionSTFTLoss`` (``differentiable = True``), the step
``optim.Adam(eps=1e-6).step(max_norm=hparams.grad_clip_thresh)``.  Every ``log_step`` one line
``basis <step> stft=%.8e grad_norm=%.8e``; every ``save_step`` ``checkpoint/<time>/basis_<step>.pth.tar`` with ``model``
and ``optimizer``, which ``--checkpoint_path`` / ``--restore_step`` continue.

``--stage encode``: with the model just learnt (``--stage all``, the default) or the one in ``--checkpoint_path``, writes
``<basis_dataset_path>/basis_signal_weight.npy`` float32 [L, C], ``encoder_weight.npy`` [C, L] and, for every utterance
of both index pairs, ``weight/<basename of the audio path>`` float32 [C, ceil(n / (L/2))] -- one utterance at a time,
one device-to-host copy each -- then prints ``valid stft=... snr=... dB`` over the validation utterances.

A missing index file, an odd ``L`` or a ``hop_size`` that ``L // 2`` does not divide exits with one sentence.
``--gpus`` above 1 and ``--mixprecision 1`` are refused: this flow is one GPU, fp32.
"""
import argparse
import os
import sys
from datetime import datetime

import numpy as np
import torch
import yaml

from .. import hparams as hp
from ..basis import BasisAutoencoder, export_dataset
from ..data import BatchIterator, load_data_to_buffer, parse_path_file
from ..loss import MultiResolutionSTFTLoss
from ..optim import Adam
from .synthesize import default_device, load_checkpoint

STAGES = ("learn", "encode", "all")
MIN_SAMPLES = 1025          # the 2048-point STFT's reflect pad takes more than 1024 samples


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, help="the Basis-MelGAN yaml file: L and out_channels are read from it")
    parser.add_argument("--audio_index_path", type=str, default=os.path.join("dataset", "audio", "train"))
    parser.add_argument("--mel_index_path", type=str, default=os.path.join("dataset", "mel", "train"))
    parser.add_argument("--audio_index_valid_path", type=str, default=os.path.join("dataset", "audio", "valid"))
    parser.add_argument("--mel_index_valid_path", type=str, default=os.path.join("dataset", "mel", "valid"))
    parser.add_argument("--basis_dataset_path", type=str, default="Basis-MelGAN-dataset")
    parser.add_argument("--learning_rate", type=float, default=hp.learning_rate)
    parser.add_argument("--batch_size", type=int, default=hp.batch_size)
    parser.add_argument("--fixed_length", type=int, default=hp.fixed_length, help="frames per training crop")
    parser.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (0: run the epochs)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the crops, the shuffling and the initial weights")
    parser.add_argument("--log_step", type=int, default=hp.log_step)
    parser.add_argument("--save_step", type=int, default=hp.save_step)
    parser.add_argument("--checkpoint_path", type=str, default="")
    parser.add_argument("--restore_step", type=int, default=0)
    parser.add_argument("--stage", type=str, default="all", choices=STAGES)
    parser.add_argument("--lambda_wave", type=float, default=0.0,
                        help="weight of a time-domain mean-squared-error term (0: the STFT loss alone; not tuned)")
    parser.add_argument("--gpus", type=int, default=argparse.SUPPRESS, help="refused above 1: this flow is one GPU")
    parser.add_argument("--mixprecision", type=int, default=0, help="refused: the kernels train in fp32")
    return parser


def check_args(args):
    """Exit, with one sentence that names the problem, for what this flow does not do."""
    if getattr(args, "gpus", 1) != 1:
        sys.exit("MODE=basis: --gpus is not supported: learning the basis runs on one GPU")
    if args.mixprecision:
        sys.exit("MODE=basis: --mixprecision 1 is not supported: the kernels train in fp32")
    if not args.config:
        sys.exit("MODE=basis: --config (the Basis-MelGAN yaml file, for L and out_channels) is required")
    for name in ("batch_size", "fixed_length", "log_step", "save_step"):
        if getattr(args, name) < 1:
            sys.exit(f"MODE=basis: --{name} must be at least 1")
    if args.lambda_wave < 0.0:
        sys.exit("MODE=basis: --lambda_wave must not be negative")
    for flag in ("audio_index_path", "mel_index_path", "audio_index_valid_path", "mel_index_valid_path"):
        if not os.path.isfile(getattr(args, flag)):
            sys.exit(f"MODE=basis: the index file {getattr(args, flag)} (--{flag}) does not exist")
    if args.stage == "encode" and not args.checkpoint_path:
        sys.exit("MODE=basis: --stage encode needs --checkpoint_path, the basis_<step>.pth.tar to encode with")
    return args


def read_geometry(config_path):
    """(L, C, samples per mel frame) of the yaml file; exits for what the framing cannot take.  The samples per frame
    come from the generator's ``upsample_scales`` times L / 2, as MODE=train takes them from the generator, and are
    ``hparams.hop_size`` for a config without that key."""
    if not os.path.isfile(config_path):
        sys.exit(f"MODE=basis: the config file {config_path} does not exist")
    with open(config_path) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    try:
        L, C = int(config["L"]), int(config["out_channels"])
    except (KeyError, TypeError, ValueError):
        sys.exit(f"MODE=basis: {config_path} has no integer L and out_channels: not a Basis-MelGAN config")
    if L < 2 or L % 2:
        sys.exit(f"MODE=basis: L = {L} in {config_path} must be even and at least 2 (the hop is L / 2)")
    if hp.hop_size % (L // 2):
        sys.exit(f"MODE=basis: hop_size {hp.hop_size} is not divisible by L // 2 = {L // 2}: a mel frame must hold a "
                 "whole number of weight frames")
    if C < 1:
        sys.exit(f"MODE=basis: out_channels = {C} in {config_path} must be at least 1")
    spf = hp.hop_size
    if isinstance(config.get("upsample_scales"), (list, tuple)):
        spf = int(np.prod([int(r) for r in config["upsample_scales"]])) * (L // 2)
    return L, C, spf


def _timestamp():
    return str(datetime.now()).replace(" ", "-").replace(":", "-").replace(".", "-")


def _restore(args, model, optimizer, device):
    try:
        checkpoint = load_checkpoint(args.checkpoint_path, device)
        missing = [k for k in ("model", "optimizer") if k not in checkpoint]
    except Exception as e:                     # noqa: BLE001 -- whatever the loader raises ends the run
        sys.exit(f"MODE=basis: cannot load --checkpoint_path {args.checkpoint_path}: {type(e).__name__}: {e}")
    if missing:
        sys.exit(f"MODE=basis: --checkpoint_path {args.checkpoint_path} has no {missing} entry: not a basis checkpoint")
    try:
        model.load_state_dict(checkpoint["model"])
    except RuntimeError as e:
        sys.exit(f"MODE=basis: --checkpoint_path {args.checkpoint_path} does not fit L = {model.L}, "
                 f"out_channels = {model.channels}: {str(e).splitlines()[0]}")
    if optimizer is not None:
        optimizer.load_state_dict(checkpoint["optimizer"])


def learn(args, model, device, spf):
    """The ``learn`` stage -> the directory of its checkpoints."""
    optimizer = Adam(model.parameters(), lr=args.learning_rate, eps=1.0e-6, weight_decay=0.0)
    if args.checkpoint_path:
        _restore(args, model, optimizer, device)
        print("\n---Model Restored at Step %d---\n" % args.restore_step)
    else:
        print("\n---Start New Training---\n")
    stft_loss = MultiResolutionSTFTLoss().to(device)
    stft_loss.differentiable = True
    print("Load data to buffer")
    buffer = load_data_to_buffer(args.audio_index_path, args.mel_index_path)
    batches = BatchIterator(buffer, args.batch_size, args.fixed_length, spf, seed=args.seed, name="train")
    if len(batches) < 1:
        sys.exit(f"MODE=basis: {len(batches.items)} usable training utterances do not fill one batch of {args.batch_size}")
    if args.fixed_length * spf < MIN_SAMPLES:
        sys.exit(f"MODE=basis: --fixed_length {args.fixed_length} gives crops of {args.fixed_length * spf} "
                 f"samples, the STFT loss needs {MIN_SAMPLES}")
    out_dir = os.path.join(hp.checkpoint_path, _timestamp())
    os.makedirs(out_dir, exist_ok=True)
    model.train()
    done = 0
    for epoch in range(hp.epochs):
        for i, (_mel, wav) in enumerate(batches.epoch()):
            step = i + args.restore_step + epoch * len(batches) + 1
            wav = wav.to(device)
            est, _ = model(wav)
            sc, mag = stft_loss(est, wav)
            stft = sc + mag
            total = stft if args.lambda_wave == 0.0 else stft + args.lambda_wave * torch.mean((est - wav) ** 2)
            optimizer.zero_grad(set_to_none=True)
            total.backward()
            norm = optimizer.step(max_norm=hp.grad_clip_thresh)
            if step % args.log_step == 0:
                print("basis %d stft=%.8e grad_norm=%.8e" % (step, float(stft), float(norm)), flush=True)
            if step % args.save_step == 0:
                torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()},
                           os.path.join(out_dir, "basis_%d.pth.tar" % step))
                print("save basis at step %d ..." % step, flush=True)
            done += 1
            if args.max_steps and done >= args.max_steps:
                return out_dir
    return out_dir


def _utterance(path, device):
    wav = torch.from_numpy(np.ascontiguousarray(np.load(path), dtype=np.float32)).reshape(1, -1)
    return wav.to(device)


def encode(args, model, device):
    """The ``encode`` stage: the three kinds of files, then the validation line -> (files written, stft, snr)."""
    model.eval()
    train_paths = parse_path_file(args.audio_index_path)
    valid_paths = parse_path_file(args.audio_index_valid_path)

    def weights():
        for path in train_paths + valid_paths:
            storage = model.encode(_utterance(path, device)).transpose(1, 2)[0]      # the [C, F] storage itself
            yield path.split("/")[-1], storage.cpu().numpy()
    basis = model.basis_signal.layer.weight.detach().cpu().numpy()
    encoder = model.encoder.weight.detach().reshape(model.channels, model.L).cpu().numpy()
    count = export_dataset(args.basis_dataset_path, basis, encoder, weights())
    print(f"wrote {count} weight files, basis_signal_weight.npy and encoder_weight.npy to {args.basis_dataset_path}")
    stft_loss = MultiResolutionSTFTLoss().to(device)
    losses, signal, noise = [], 0.0, 0.0
    with torch.no_grad():
        for path in valid_paths:
            wav = _utterance(path, device)
            if wav.shape[1] < MIN_SAMPLES:
                continue
            est = model(wav)[0][:, : wav.shape[1]].contiguous()
            sc, mag = stft_loss(est, wav)
            losses.append(float(sc + mag))
            signal += float(wav.double().pow(2).sum())
            noise += float((wav.double() - est.double()).pow(2).sum())
    stft = float(np.mean(losses)) if losses else float("nan")
    snr = 10.0 * float(np.log10(signal / noise)) if losses and noise > 0.0 else float("nan")
    print("valid stft=%.8e snr=%.2f dB" % (stft, snr), flush=True)
    return count, stft, snr


def run(args):
    L, C, spf = read_geometry(args.config)
    device = default_device()
    torch.manual_seed(args.seed)
    model = BasisAutoencoder(L=L, channels=C).to(device)
    if args.stage in ("learn", "all"):
        learn(args, model, device, spf)
    else:
        _restore(args, model, None, device)
    if args.stage in ("encode", "all"):
        encode(args, model, device)
    return model


def run_basis(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    return run(check_args(build_parser().parse_args(argv)))


if __name__ == "__main__":
    run_basis()
