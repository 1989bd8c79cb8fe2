"""``MODE=train``: the reference's bin/train.py for the generators that have a parameter gradient, HiFi-GAN,
Multiband-HiFi-GAN and (opted in with ``--stack_grad 1`` / ``--basis_grad 1``) MelGAN and Basis-MelGAN, on the MI355X
kernels: ``train.Trainer`` runs the
step, ``optim.Adam`` clips and updates in three launches, ``data.BatchIterator`` cuts the crops.

``run_train()`` takes the reference's arguments (train.py:478-499) and, for a test or a short run, ``--max_steps``,
``--seed``, ``--batch_size``, ``--fixed_length``, ``--discriminator_train_start_steps``, ``--log_step``,
``--save_step``, ``--valid_step``, ``--valid_num`` (defaults: hparams), ``--use_mpd``, ``--stack_grad``, ``--basis_grad``,
``--basis_dataset_path``, ``--grad_precision`` and ``--discriminator_grad_precision``.
``lamda_stft`` (sic) and ``use_feature_map_loss`` come from the yaml, as there.  Both optimizers are
``Adam(lr, eps=1e-6)``; ``--use_scheduler 1`` adds ``CosineAnnealingLR(T_max=2500, eta_min=lr / 10)`` to both.

Every ``log_step`` steps the reference's log lines are printed and appended to ``<logger_path>/<timestamp>/logger.txt``
(format_log_lines, format_time_line); ``total_loss.txt`` and ``stft_loss.txt`` get one value per step.  Scalars also
go to tensorboardX when it can be imported (it is optional).  Every ``save_step`` steps
``<checkpoint_path>/<timestamp>/checkpoint_<step>.pth.tar`` is written with the reference's four keys (``model``,
``optimizer``, ``discriminator``, ``discriminator_optimizer``), which MODE=synthesize, MODE=evaluation --discriminator
and the reference itself load.  Every ``valid_step`` steps the mean STFT loss of up to ``valid_num`` whole validation
utterances is printed as ``valid <step> stft=<%.8e>``.

Deviations from the reference, on purpose: ``--checkpoint_path ""`` starts new, but a path that cannot be loaded exits
(the reference's bare ``except`` starts a new training silently); whether the checkpoint's discriminator holds the
multi-period discriminator is read from its ``mpd.`` keys, as MODE=evaluation does; the validation mean divides by the
number of utterances scored (the reference scores ``valid_num + 1`` and divides by ``valid_num``) and takes them in
index order; the samples per frame come from the generator's upsample rates, not from ``hparams.hop_size``.
``--model_name melgan`` trains with ``--stack_grad 1`` (``MelGANGenerator.stack_grad``: the backward of ResidualStack
and of the reflection-padded edge convs) and exits without it; the flag is absent from the parsed arguments unless it
is given.  ``--model_name basis-melgan`` trains with ``--basis_grad 1`` (``BasisMelGANGenerator.basis_grad``) and exits
without it, ``--stack_grad 1`` or not.  Its flow is the reference's (train.py:297-331, 390-466): the basis comes from
``<basis_dataset_path>/basis_signal_weight.npy`` [L, C] (``--basis_dataset_path``, ``Basis-MelGAN-dataset`` when absent;
a resumed checkpoint's ``basis_signal.layer.weight`` wins), the target weights from ``<basis_dataset_path>/weight/``
(data.load_data_to_buffer), the optimizer covers ``model.melgan.parameters()`` only -- the basis is frozen and gets no
gradient --, the validation scores ``model(mel)[0]``, the log line's "Weight Loss" is filled and the ``weight_loss`` and
``weight_average_value`` scalars are written.  A missing basis or weight file ends the run with one sentence that
names the path.  Both flags are absent from the parsed arguments unless given.  ``--mixprecision 1`` exits: there is no
mixed-precision (apex amp) path.  ``--grad_precision bf16`` (absent from the parsed arguments unless given; every
trainable ``--model_name``, with or without ``--gpus``) is this hardware's reduced-precision mode,
``Trainer(grad_precision="bf16")``: the convs' weight gradients on the bf16 matrix cores with fp32 accumulation,
everything else fp32 -- no loss scale, the same checkpoint and log lines, and a checkpoint resumes under either value.
``--discriminator_grad_precision bf16`` (absent unless given; needs ``--use_mpd 1``) is
``Trainer(discriminator_grad_precision="bf16")``: the multi-period discriminator's weight gradients in the same
arithmetic, the MSD and MFD untouched.  It is not stored in the checkpoint either.

Several GPUs of one node: ``--gpus N`` (absent from the parsed arguments unless given) with no ``WORLD_SIZE`` in the
environment starts ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...`` as a child -- the parent
never touches a GPU -- and returns its exit status; started under ``torch.distributed.run`` directly (``WORLD_SIZE`` in
the environment) every process is one rank.  The backend is ``nccl`` (RCCL), one GPU per rank by ``LOCAL_RANK``; a world
larger than the visible devices is refused.  ``FV_TRAIN_BACKEND=gloo`` together with ``FV_TRAIN_ONE_GPU=1`` puts every
rank on device 0 and moves the collectives through the host: for tests on a one-GPU box.  ``--batch_size`` is PER RANK,
so a step sees ``batch_size * N`` crops (``BatchIterator(rank=, world_size=)``: the ranks cut one global batch) and an
epoch has ``utterances // (batch_size * N)`` steps.  The learning rates are NOT rescaled by N.  A fresh start broadcasts
rank 0's seeded weights (model and discriminator) to every rank; a resume loads the checkpoint on every rank.  The
gradients are averaged inside the optimizer step (``Trainer(process_group=)``) and the logged scalars are the ranks'
means.  Only rank 0 prints the log lines, writes the logger files, the tensorboard scalars and the checkpoints, and
validates.  At every ``save_step``, before saving, all ranks compare one float64 checksum of their parameters (a MIN and
a MAX all-reduce) and all exit with one sentence when the two differ.  The process group has a finite timeout
(``COLLECTIVE_TIMEOUT`` seconds): when a rank dies the launcher ends the others, and a rank that merely stops arriving
at a collective ends the run after that time instead of hanging it.
"""
import argparse
import os
import subprocess
import sys
import time
from datetime import datetime, timedelta

import numpy as np
import torch
import yaml

from .. import hparams as hp
from .. import parallel
from ..data import BatchIterator, MissingWeightFile, load_data_to_buffer
from ..discriminator import Discriminator
from ..generator import PQMF
from ..optim import Adam
from ..train import Trainer, fit_estimate, samples_per_frame
from .evaluation import discriminator_uses_mpd
from .synthesize import build_generator, default_device, load_checkpoint

SUPPORTED = ("hifigan", "multiband-hifigan")
COLLECTIVE_TIMEOUT = 600        # seconds a rank waits in a collective before the run ends
CHECKPOINT_KEYS = ("model", "optimizer", "discriminator", "discriminator_optimizer")


def format_log_lines(epoch, epochs, current_step, total_step, s_l, w_l, t_l, a_l, d_l, f_l, lr, lr_discriminator):
    """The four log lines of a step in the reference's format (train.py:201-207); ``epoch`` counts from 0."""
    return [f"Epoch [{epoch + 1}/{epochs}], Step [{current_step}/{total_step}]:",
            "STFT Loss: {:.6f}, Weight Loss: {:.6f}, Total Loss: {:.6f};".format(s_l, w_l, t_l),
            "Adversarial Loss: {:.6f}, Discriminator Loss: {:.6f}, Feature Map Loss: {:.6f};".format(a_l, d_l, f_l),
            "Current Learning Rate is {:.6f}, discriminator Learning Rate is {:.6f};".format(lr, lr_discriminator)]


def format_time_line(used, remaining):
    """The line that follows them (train.py:208)."""
    return "Time Used: {:.3f}s, Estimated Time Remaining: {:.3f}s.".format(used, remaining)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--audio_index_path", type=str, default=os.path.join("dataset", "audio", "train"))
    parser.add_argument("--mel_index_path", type=str, default=os.path.join("dataset", "mel", "train"))
    parser.add_argument("--audio_index_valid_path", type=str, default=os.path.join("dataset", "audio", "valid"))
    parser.add_argument("--mel_index_valid_path", type=str, default=os.path.join("dataset", "mel", "valid"))
    parser.add_argument("--checkpoint_path", type=str, default="")
    parser.add_argument("--restore_step", type=int, default=0)
    parser.add_argument("--learning_rate", type=float, default=hp.learning_rate)
    parser.add_argument("--learning_rate_discriminator", type=float, default=hp.learning_rate_discriminator)
    parser.add_argument("--model_name", type=str, help="hifigan and multiband-hifigan.")
    parser.add_argument("--config", type=str, help="path to model configuration file")
    parser.add_argument("--use_scheduler", type=int, default=0)
    parser.add_argument("--mixprecision", type=int, default=0)
    # what a test or a short run needs
    parser.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (0: run the epochs)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the crops, the shuffling and the initial weights")
    parser.add_argument("--batch_size", type=int, default=hp.batch_size)
    parser.add_argument("--fixed_length", type=int, default=hp.fixed_length, help="frames per training crop")
    parser.add_argument("--discriminator_train_start_steps", type=int, default=hp.discriminator_train_start_steps)
    parser.add_argument("--log_step", type=int, default=hp.log_step)
    parser.add_argument("--save_step", type=int, default=hp.save_step)
    parser.add_argument("--valid_step", type=int, default=hp.valid_step)
    parser.add_argument("--valid_num", type=int, default=hp.valid_num)
    parser.add_argument("--use_mpd", type=int, default=0,
                        help="1: train Discriminator(use_mpd=True), HiFi-GAN's multi-period discriminator included")
    parser.add_argument("--stack_grad", type=int, default=argparse.SUPPRESS,
                        help="1: opt in to MelGAN's parameter gradient (--model_name melgan trains only with it)")
    parser.add_argument("--basis_grad", type=int, default=argparse.SUPPRESS,
                        help="1: opt in to Basis-MelGAN's parameter gradient (--model_name basis-melgan trains only with it)")
    parser.add_argument("--basis_dataset_path", type=str, default=argparse.SUPPRESS,
                        help="directory of basis_signal_weight.npy and weight/ (default: Basis-MelGAN-dataset)")
    parser.add_argument("--grad_precision", type=str, default=argparse.SUPPRESS,
                        help="f32 (default) or bf16: the generator's weight gradients on the bf16 matrix cores, fp32 "
                             "accumulation; everything else stays fp32")
    parser.add_argument("--discriminator_grad_precision", type=str, default=argparse.SUPPRESS,
                        help="f32 (default) or bf16: the multi-period discriminator's weight gradients on the bf16 "
                             "matrix cores (needs --use_mpd 1); the MSD and MFD stay fp32")
    parser.add_argument("--gpus", type=int, default=argparse.SUPPRESS,
                        help="data-parallel training over this many GPUs of the node, one rank each (--batch_size is "
                             "per rank)")
    return parser


def check_args(args):
    """Exit, with one sentence that names what is missing, for what this loop does not train."""
    if args.model_name == "melgan" and getattr(args, "stack_grad", 0):
        pass                                   # opted in: MelGANGenerator.stack_grad
    elif args.model_name == "melgan":
        sys.exit("MODE=train: --model_name melgan has no parameter gradient unless --stack_grad 1 opts in to the "
                 "backward of ResidualStack; supported without it: " + ", ".join(SUPPORTED))
    elif args.model_name == "basis-melgan" and getattr(args, "basis_grad", 0):
        pass                                   # opted in: BasisMelGANGenerator.basis_grad
    elif args.model_name == "basis-melgan":
        sys.exit(f"MODE=train: --model_name {args.model_name} cannot be trained here: the ResidualStack generators "
                 "(MelGAN, Basis-MelGAN) have no parameter gradient yet; supported: " + ", ".join(SUPPORTED))
    elif args.model_name not in SUPPORTED:
        sys.exit(f"MODE=train: --model_name must be one of {', '.join(SUPPORTED)}, got {args.model_name!r}")
    if args.mixprecision:
        sys.exit("MODE=train: --mixprecision 1 is not supported: there is no mixed-precision (apex amp) path; "
                 "--grad_precision bf16 is the reduced-precision mode (bf16 weight gradients, no loss scaling)")
    if getattr(args, "grad_precision", "f32") not in ("f32", "bf16"):
        sys.exit(f"MODE=train: --grad_precision must be f32 or bf16, got {args.grad_precision!r}")
    if getattr(args, "discriminator_grad_precision", "f32") not in ("f32", "bf16"):
        sys.exit("MODE=train: --discriminator_grad_precision must be f32 or bf16, got "
                 f"{args.discriminator_grad_precision!r}")
    if getattr(args, "discriminator_grad_precision", "f32") == "bf16" and not args.use_mpd:
        sys.exit("MODE=train: --discriminator_grad_precision bf16 needs --use_mpd 1: only the multi-period "
                 "discriminator's weight gradients have bf16 kernels")
    if not args.config:
        sys.exit("MODE=train: --config (the model's yaml file) is required")
    for name in ("batch_size", "fixed_length", "log_step", "save_step", "valid_step"):
        if getattr(args, name) < 1:
            sys.exit(f"MODE=train: --{name} must be at least 1")
    if getattr(args, "gpus", 1) < 1:
        sys.exit("MODE=train: --gpus must be at least 1")
    return args


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch_argv(gpus, argv, port):
    """``--gpus N`` started as ONE process: the command of the child that runs the N ranks, one per GPU of this node,
    rendezvous on 127.0.0.1 (``MODE=train`` and the package's directory travel in the child's environment)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "fastvocoder_amd.bin.launcher", *argv]


def visible_devices_error(world, visible):
    """The one sentence that refuses a world larger than the node's visible devices, or None."""
    if world > visible:
        return (f"MODE=train: --gpus {world} needs {world} visible devices, this node shows {visible} "
                "(HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES?): refusing to run ranks on shared devices")
    return None


def launch(gpus, argv):
    """Run the ``gpus`` ranks as a child process -> its exit status.  Nothing here initialises a GPU."""
    if os.environ.get("FV_TRAIN_ONE_GPU", "0") != "1":
        err = visible_devices_error(gpus, torch.cuda.device_count())
        if err:
            sys.exit(err)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    path = os.environ.get("PYTHONPATH")
    env = dict(os.environ, MODE="train", PYTHONPATH=root + (os.pathsep + path if path else ""))
    sys.stdout.flush()
    sys.stderr.flush()
    port = int(os.environ.get("MASTER_PORT") or free_port())        # the rendezvous port: the caller's, or a free one
    return subprocess.call(self_launch_argv(gpus, list(argv), port), env=env)


def init_distributed(args):
    """(process group or None, rank, world, device) from the launcher's environment; exits with one sentence for a
    launch that cannot run as asked."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return None, 0, 1, default_device()
    import torch.distributed as dist
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if getattr(args, "gpus", world) != world:
        sys.exit(f"MODE=train: --gpus {args.gpus} but WORLD_SIZE = {world}: launch exactly one rank per GPU asked for")
    backend = os.environ.get("FV_TRAIN_BACKEND", "nccl")
    one_gpu = os.environ.get("FV_TRAIN_ONE_GPU", "0") == "1"
    if not torch.cuda.is_available():
        sys.exit("MODE=train: fastvocoder_amd needs a ROCm GPU (MI355X); no CPU training path exists")
    if one_gpu and backend != "gloo":
        sys.exit("MODE=train: FV_TRAIN_ONE_GPU=1 (every rank on device 0) needs FV_TRAIN_BACKEND=gloo: RCCL wants one "
                 "GPU per rank")
    if one_gpu:
        local_rank = 0
    else:
        err = visible_devices_error(world, torch.cuda.device_count())
        if err:
            sys.exit(err)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    kw = dict(device_id=device) if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=COLLECTIVE_TIMEOUT), **kw)
    return dist.group.WORLD, rank, world, device


def parameter_checksum(*modules):
    """One float64 device scalar over every parameter of the modules (the sum of the tensors' float64 sums)."""
    with torch.no_grad():
        return torch.stack([p.detach().double().sum() for m in modules for p in m.parameters()]).sum()


def check_replicas(group, step, *modules):
    """All ranks compare their parameter checksum (MIN and MAX over the group); all exit when the two differ."""
    import torch.distributed as dist
    value = parameter_checksum(*modules).reshape(1)
    if dist.get_backend(group) == "gloo":
        value = value.cpu()
    lo, hi = value.clone(), value.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    lo, hi = float(lo), float(hi)
    if not lo == hi:
        sys.exit(f"MODE=train: at step {step} the ranks' parameter checksums differ ({lo!r} to {hi!r}): the replicas "
                 "have diverged, nothing is saved")


def _timestamp():
    return str(datetime.now()).replace(" ", "-").replace(":", "-").replace(".", "-")


def _summary_writer(path):
    """A tensorboardX SummaryWriter, or None when tensorboardX is not installed."""
    try:
        from tensorboardX import SummaryWriter
    except ImportError:
        return None
    return SummaryWriter(path)


def load_basis(model, path):
    """``basis_signal_weight.npy`` [L, C] into the model's basis layer; exits with the path when it is missing or has
    another shape."""
    if not os.path.isfile(path):
        sys.exit(f"MODE=train: the basis {path} does not exist (--basis_dataset_path names the directory that holds "
                 "basis_signal_weight.npy and weight/)")
    value = torch.from_numpy(np.ascontiguousarray(np.load(path), dtype=np.float32))
    weight = model.basis_signal.layer.weight
    if value.shape != weight.shape:
        sys.exit(f"MODE=train: the basis {path} is {tuple(value.shape)}, the model's is {tuple(weight.shape)} (L, C)")
    with torch.no_grad():
        weight.copy_(value)


def validate(model, vocoder_loss, pqmf, buffer, valid_num, device, spf):
    """(mean STFT loss, utterances scored) over the first ``valid_num`` whole utterances, under no_grad."""
    losses = []
    with torch.no_grad():
        for item in buffer[:max(0, valid_num)]:
            frames = min(item["mel"].shape[0], item["wav"].shape[0] // spf)
            if frames < 1:
                continue
            mel = item["mel"][:frames].to(device).t().unsqueeze(0).contiguous()
            wav = item["wav"][:frames * spf].to(device).unsqueeze(0).contiguous()
            est = model(mel)
            est = est[0] if isinstance(est, tuple) else est          # Basis-MelGAN: (est, weight)
            losses.append(vocoder_loss(fit_estimate(est, wav.shape[1], pqmf), wav, pqmf=pqmf)[0].reshape(()))
        if not losses:
            return float("nan"), 0
        return float(torch.stack(losses).mean()), len(losses)


def run(args):
    group, rank, world, device = init_distributed(args)
    try:
        return _run(args, group, rank, world, device)
    finally:
        if group is not None:
            torch.distributed.destroy_process_group()


def _run(args, group, rank, world, device):
    main = rank == 0                               # the rank that prints, logs, saves and validates

    def say(*a, **kw):                             # the other ranks run the same lines silently
        if main:
            print(*a, **kw)
    torch.manual_seed(args.seed)
    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    lambda_stft = config["lamda_stft"]
    use_feature_map_loss = config["use_feature_map_loss"]
    say(f"Loading Model of {args.model_name}...")
    model = build_generator(args.model_name, config).to(device)
    basis = args.model_name == "basis-melgan"
    basis_dir = getattr(args, "basis_dataset_path", "Basis-MelGAN-dataset")
    if basis:
        load_basis(model, os.path.join(basis_dir, "basis_signal_weight.npy"))
    pqmf = PQMF().to(device) if config["multiband"] else None

    # the checkpoint first: it decides which discriminator is built
    checkpoint = None
    if args.checkpoint_path:
        try:
            checkpoint = load_checkpoint(args.checkpoint_path, device)
            missing = [k for k in ("model", "optimizer") if k not in checkpoint]
        except Exception as e:                     # noqa: BLE001 -- whatever the loader raises ends the run
            sys.exit(f"MODE=train: cannot load --checkpoint_path {args.checkpoint_path}: {type(e).__name__}: {e}")
        if missing:
            sys.exit(f"MODE=train: --checkpoint_path {args.checkpoint_path} has no {missing} entry: not a training "
                     "checkpoint")
    use_mpd = bool(args.use_mpd)
    if checkpoint is not None and "discriminator" in checkpoint:
        use_mpd = discriminator_uses_mpd(checkpoint["discriminator"])
        if not use_mpd and getattr(args, "discriminator_grad_precision", "f32") == "bf16":
            sys.exit(f"MODE=train: --discriminator_grad_precision bf16 needs the multi-period discriminator, and "
                     f"--checkpoint_path {args.checkpoint_path} was trained without it")
    discriminator = Discriminator(use_mpd=use_mpd).to(device)
    say(f"Number of Parameters: {sum(p.numel() for p in model.parameters())}")

    # Basis-MelGAN: the trunk alone; the basis is frozen (reference train.py:329-331)
    optimizer = Adam((model.melgan if basis else model).parameters(), lr=args.learning_rate, eps=1.0e-6,
                     weight_decay=0.0)
    discriminator_optimizer = Adam(discriminator.parameters(), lr=args.learning_rate_discriminator, eps=1.0e-6,
                                   weight_decay=0.0)
    if checkpoint is not None:
        model.load_state_dict(checkpoint["model"])
        optimizer.load_state_dict(checkpoint["optimizer"])
        if "discriminator" in checkpoint:
            discriminator.load_state_dict(checkpoint["discriminator"])
            discriminator_optimizer.load_state_dict(checkpoint["discriminator_optimizer"])
        counts = [int(s["step"]) for s in optimizer.state.values()]
        say("\n---Model Restored at Step %d---\n" % args.restore_step)
        say("optimizer state at step count %d" % (max(counts) if counts else 0))
    else:
        if group is not None:                      # every rank starts from rank 0's seeded weights
            parallel.broadcast_weights(model, src=0, group=group)
            parallel.broadcast_weights(discriminator, src=0, group=group)
        say("\n---Start New Training---\n")
    scheduler = discriminator_scheduler = None
    if args.use_scheduler:
        from torch.optim.lr_scheduler import CosineAnnealingLR
        scheduler = CosineAnnealingLR(optimizer, T_max=2500, eta_min=args.learning_rate / 10.)
        discriminator_scheduler = CosineAnnealingLR(discriminator_optimizer, T_max=2500,
                                                    eta_min=args.learning_rate_discriminator / 10.)

    stamp = _timestamp()
    current_checkpoint_path = os.path.join(hp.checkpoint_path, stamp)
    current_logger_path = os.path.join(hp.logger_path, stamp)
    writer = None
    if main:
        os.makedirs(current_checkpoint_path, exist_ok=True)
        os.makedirs(current_logger_path, exist_ok=True)
        writer = _summary_writer(os.path.join(hp.tensorboard_path, stamp))

    model.train()
    trainer = Trainer(model, discriminator, optimizer, discriminator_optimizer, scheduler, discriminator_scheduler,
                      pqmf, lambda_stft=lambda_stft, use_feature_map_loss=use_feature_map_loss,
                      discriminator_train_start_steps=args.discriminator_train_start_steps,
                      grad_clip_thresh=hp.grad_clip_thresh, lambda_adv=hp.lambda_adv, lambda_fm=hp.lambda_fm,
                      stack_grad=bool(getattr(args, "stack_grad", 0)), basis_grad=bool(getattr(args, "basis_grad", 0)),
                      process_group=group,
                      discriminator_grad_precision=getattr(args, "discriminator_grad_precision", "f32"),
                      grad_precision=getattr(args, "grad_precision", "f32"))
    spf = samples_per_frame(model, pqmf)

    say("Load data to buffer")
    try:
        train_buffer = load_data_to_buffer(args.audio_index_path, args.mel_index_path,
                                           weight_dir=os.path.join(basis_dir, "weight") if basis else None)
    except MissingWeightFile as e:                 # Basis-MelGAN's weight/ alone; other missing files raise as before
        sys.exit(f"MODE=train: {e}")
    batches = BatchIterator(train_buffer, args.batch_size, args.fixed_length, spf, seed=args.seed, name="train",
                            basis_L=model.L if basis else None, rank=rank, world_size=world)
    say("Load valid data to buffer")
    valid_buffer = load_data_to_buffer(args.audio_index_valid_path, args.mel_index_valid_path)
    if len(batches) < 1:
        sys.exit(f"MODE=train: {len(batches.items)} usable training utterances do not fill one batch of "
                 f"{args.batch_size}" + (f" on each of {world} ranks" if world > 1 else ""))
    say(f"Length of training loader is {len(batches)}")
    total_step = hp.epochs * len(batches)

    start = time.perf_counter()
    step_times = []
    done = 0
    for epoch in range(hp.epochs):
        for i, (mel, wav, *weight) in enumerate(batches.epoch()):
            current_step = i + args.restore_step + epoch * len(batches) + 1
            step_start = time.perf_counter()
            mel = mel.to(device).transpose(1, 2).contiguous()
            wav = wav.to(device)
            out = trainer.step(mel, wav, current_step, *(w.to(device) for w in weight))
            s_l, t_l = out["stft"], out["total"]
            if main:
                with open(os.path.join(current_logger_path, "total_loss.txt"), "a") as f:
                    f.write(str(t_l) + "\n")
                with open(os.path.join(current_logger_path, "stft_loss.txt"), "a") as f:
                    f.write(str(s_l) + "\n")

            if main and current_step % args.log_step == 0:
                if scheduler is None:
                    lrs = args.learning_rate, args.learning_rate_discriminator
                else:
                    lrs = scheduler.get_last_lr()[-1], discriminator_scheduler.get_last_lr()[-1]
                now = time.perf_counter()
                mean_time = float(np.mean(step_times)) if step_times else now - step_start
                lines = format_log_lines(epoch, hp.epochs, current_step, total_step, s_l, out.get("weight", 0.), t_l,
                                         out["adversarial"],
                                         out["discriminator"], out["feature_map"], *lrs)
                lines.append(format_time_line(now - start, (total_step - current_step) * mean_time))
                say("\n" + "\n".join(lines), flush=True)
                with open(os.path.join(current_logger_path, "logger.txt"), "a") as f:
                    f.write("\n".join(lines) + "\n\n")
                if writer is not None:
                    for tag, value in (("total_loss", t_l), ("stft_loss", s_l), ("adversarial_loss", out["adversarial"]),
                                       ("discriminator_loss", out["discriminator"]),
                                       ("feature_map_loss", out["feature_map"]), ("grad_norm", out["grad_norm"])):
                        writer.add_scalar(tag, value, global_step=current_step)
                    if basis:
                        writer.add_scalar("weight_loss", out["weight"], global_step=current_step)
                        writer.add_scalar("weight_average_value", round(out["weight_average"], 6),
                                          global_step=current_step)
                    if scheduler is not None:
                        writer.add_scalar("learning_rate", lrs[0], global_step=current_step)

            if group is not None and current_step % args.save_step == 0:
                check_replicas(group, current_step, model, discriminator)
            if main and current_step % args.save_step == 0:
                torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict(),
                            "discriminator": discriminator.state_dict(),
                            "discriminator_optimizer": discriminator_optimizer.state_dict()},
                           os.path.join(current_checkpoint_path, "checkpoint_%d.pth.tar" % current_step))
                say("save model at step %d ..." % current_step, flush=True)

            step_times.append(time.perf_counter() - step_start)
            if len(step_times) == hp.clear_time:
                step_times = [float(np.mean(step_times))]

            if main and current_step % args.valid_step == 0:
                value, scored = validate(model, trainer.vocoder_loss, pqmf, valid_buffer, args.valid_num, device, spf)
                say("valid %d stft=%.8e" % (current_step, value), flush=True)
                if writer is not None and scored:
                    writer.add_scalar("valid_stft_loss", value, global_step=current_step)

            done += 1
            if args.max_steps and done >= args.max_steps:
                break
        else:
            continue
        break
    if writer is not None:
        writer.close()
    return current_checkpoint_path


def run_train(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = check_args(build_parser().parse_args(argv))
    if getattr(args, "gpus", 1) > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch(args.gpus, argv))          # the ranks run in a child; this process never opens a GPU
    return run(args)


if __name__ == "__main__":
    run_train()
