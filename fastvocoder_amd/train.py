"""One training step of the reference's loop (bin/train.py:48-188, ``trainer``) as a library call.

``Trainer.step(mel, wav, current_step)`` runs, in the reference's order: zero both optimizers' gradients; the
generator's training forward (``parameter_grad = True``); the composed STFT loss (``Loss``, through the PQMF synthesis
for a multiband generator); past ``discriminator_train_start_steps`` the adversarial and feature-map terms of the
discriminator on the estimate (``generator_adversarial_terms``, the multiband waveform being ``pqmf.synthesis`` of the
sub-bands ON the graph); one backward; clip + Adam in three launches (``optim.Adam.step(max_norm=...)``) and the
scheduler; then the discriminator's own update on a fresh ``no_grad`` forward of the UPDATED generator
(train.py:148-155), ``discriminator_step_terms``, backward, clip + Adam, scheduler.

The scalars of a step stay on the device until its end and are read with one copy to the host (the reference reads
five times, ``.item()`` each).  (The backward of the discriminator terms still reads its incoming coefficient on the
host, as it does outside this loop: loss/discriminator_loss.py.)

MelGAN trains with ``Trainer(..., stack_grad=True)``, which sets the generator's ``stack_grad`` opt-in before
``parameter_grad``; without the keyword it is refused as before.  Basis-MelGAN trains with
``Trainer(..., basis_grad=True)`` in the same way (``BasisMelGANGenerator.basis_grad``).  Its step takes the target
weights, ``step(mel, wav, current_step, weight)``; ``model(mel)`` is the pair (est, est_weight); the L1 weight term
(loss.BasisWeightL1) is part of the total only up to ``discriminator_train_start_steps`` (reference train.py:87-89);
the adversarial terms and the discriminator's update see ``est``; the step's dict gains ``"weight"`` and
``"weight_average"`` (the reference's ``weight_average_value``).  The optimizer should cover ``model.melgan``'s
parameters only: the basis is a constant of the training graph and gets no gradient (the reference gives it one that
it never applies, train.py:64, 329-331 -- which its ``clip_grad_norm_`` over ``model.parameters()`` does count; the
norm here is the trunk's alone).  The ``transposedconv: False`` upsampler has no parameter gradient and is refused
where the ``parameter_grad`` attribute refuses it.

Reduced-precision gradients: ``Trainer(..., grad_precision="bf16")`` sets the generator's ``grad_precision``
(generator/engine.py ``GradPrecision``): the convs' weight gradients round their two operands to bf16 and accumulate
in fp32 on the bf16 matrix cores; the forward, the data and bias gradients, the parameters and the optimizer state stay
fp32, so there is no loss scale and no skipped step, and a checkpoint resumes under either value.  The reference's
mixed-precision flag (apex amp O1: fp16 activations with dynamic loss scaling) is not part of this loop.
``Trainer(..., discriminator_grad_precision="bf16")`` does the same to ``Discriminator(use_mpd=True)``: the weight
gradients of the multi-period discriminator's layers 1-5 (discriminator/mpd.py), nothing of the MSD and MFD, whose
weight gradients have fp32 kernels only (a discriminator without the MPD refuses it).  The two keywords are
independent: ``grad_precision`` alone leaves the discriminator in fp32.

Data-parallel training: ``Trainer(..., process_group=<a torch.distributed group>)`` hands the group to both optimizer
steps (``optim.Adam.step(process_group=...)``: the gradients of the ranks' shards are averaged with one collective over
one flat bucket per optimizer step) and, at the end of the step, all-reduces the stacked scalar vector once and divides
it by the world size before the step's one host read: the dict then holds the means over the ranks.  There is no other
collective; the generators and discriminators have no cross-batch op, so a step over ``world`` shards of ``B`` rows is
the step over the ``world * B`` rows up to the rounding of the sums.  Learning rates are not rescaled.
"""
import torch

from . import parallel
from .loss import Loss, discriminator_step_terms, generator_adversarial_terms, pqmf_synthesis
from .optim import Adam

KEYS = ("stft", "total", "adversarial", "feature_map", "discriminator", "grad_norm", "discriminator_grad_norm")


def samples_per_frame(model, pqmf=None):
    """Waveform samples the generator makes of one mel frame: the product of its upsample rates (the strides of
    ``model.ups``, or of the trunk's ConvTranspose1d layers for a generator without ``ups``), times the sub-band count
    when its output goes through a PQMF synthesis, times the basis hop L/2 for Basis-MelGAN (whose trunk makes weight
    frames, not samples)."""
    ups = getattr(model, "ups", None)
    if ups is None:
        ups = [m for m in model.modules() if isinstance(m, torch.nn.ConvTranspose1d)]
    n = 1
    for up in ups:
        n *= int(up.stride[0])
    if hasattr(model, "basis_signal"):
        n *= int(model.L) // 2
    return n * (int(pqmf.subbands) if pqmf is not None else 1)


def fit_estimate(est, n, pqmf=None):
    """The generator's output cropped to a target of ``n`` samples: a ConvTranspose1d whose kernel is not twice its
    stride makes a few samples more than frames x rate (the reference's configurations never do).  est (B, T), or the
    sub-bands (B, S, T / S) with ``pqmf``; a shorter estimate is returned as it is (the loss refuses it)."""
    if pqmf is not None:
        n //= int(pqmf.subbands)
    return est[..., :n].contiguous() if est.shape[-1] > n else est


class Trainer:
    def __init__(self, model, discriminator, optimizer, discriminator_optimizer, scheduler=None,
                 discriminator_scheduler=None, pqmf=None, *, lambda_stft, use_feature_map_loss,
                 discriminator_train_start_steps, grad_clip_thresh, lambda_adv=1.0, lambda_fm=1.0, stack_grad=False,
                 basis_grad=False, process_group=None, discriminator_grad_precision="f32", grad_precision="f32"):
        for opt, name in ((optimizer, "optimizer"), (discriminator_optimizer, "discriminator_optimizer")):
            if not isinstance(opt, Adam):
                raise TypeError(f"{name} must be a fastvocoder_amd.optim.Adam (its step clips and updates in three "
                                f"launches), got {type(opt).__name__}")
        if stack_grad and hasattr(type(model), "stack_grad"):
            model.stack_grad = True           # MelGAN's opt-in; raises for the graphs whose backward is missing
        if basis_grad and hasattr(type(model), "basis_grad"):
            model.basis_grad = True           # Basis-MelGAN's
        model.parameter_grad = True           # raises for the generators that have no parameter gradient
        if hasattr(type(model), "grad_precision"):
            model.grad_precision = grad_precision     # raises ValueError for anything but "f32" / "bf16"
        elif grad_precision != "f32":
            raise NotImplementedError(f"{type(model).__name__} has no grad_precision: its weight gradients are not "
                                      "the generators' kernels")
        if hasattr(type(discriminator), "grad_precision"):
            # ValueError for anything but "f32" / "bf16"; NotImplementedError for "bf16" without the MPD
            discriminator.grad_precision = discriminator_grad_precision
        elif discriminator_grad_precision != "f32":
            raise NotImplementedError(f"{type(discriminator).__name__} has no grad_precision: its weight gradients "
                                      "have fp32 kernels only")
        self.model, self.discriminator = model, discriminator
        self.optimizer, self.discriminator_optimizer = optimizer, discriminator_optimizer
        self.scheduler, self.discriminator_scheduler = scheduler, discriminator_scheduler
        self.pqmf = pqmf
        self.lambda_stft, self.lambda_adv, self.lambda_fm = float(lambda_stft), float(lambda_adv), float(lambda_fm)
        self.use_feature_map_loss = bool(use_feature_map_loss)
        self.discriminator_train_start_steps = int(discriminator_train_start_steps)
        self.grad_clip_thresh = float(grad_clip_thresh)
        self.period_grad = bool(getattr(discriminator, "use_mpd", False))
        self.vocoder_loss = Loss().to(next(model.parameters()).device)
        self.vocoder_loss.differentiable = True
        self.samples_per_frame = samples_per_frame(model, pqmf)
        self.basis = hasattr(model, "basis_signal")
        self.process_group = process_group
        # the keyword is passed only when there is a group: any Adam subclass written against step(max_norm=) still works
        self._step_kw = {} if process_group is None else {"process_group": process_group}

    def _waveform(self, est):
        """The generator's output as (B, T) full band: the PQMF synthesis of sub-bands, on their graph."""
        if self.pqmf is None:
            return est
        return pqmf_synthesis(est, self.pqmf)[:, 0, :]

    def step(self, mel, wav, current_step, weight=None):
        """mel (B, 80, T) and wav (B, T * samples_per_frame), fp32 device tensors -> {key: float for key in KEYS}
        (with a process group: this rank's shard of the batch, and the means over the ranks):
        the STFT loss (before lambda_stft), the generator's total, its adversarial and feature-map terms, the
        discriminator's loss (0.0 up to discriminator_train_start_steps) and the two gradient norms before clipping.
        Basis-MelGAN: ``weight`` (B, T * prod(upsample_scales), C), the target weights; the dict also holds "weight"
        (the L1 weight loss while it is part of the total, else 0.0, as the reference logs it) and "weight_average"."""
        if weight is not None and not self.basis:
            raise ValueError("weight is the target of Basis-MelGAN's weight loss; this generator has none")
        if wav.dim() != 2 or mel.dim() != 3 or wav.shape[1] != mel.shape[2] * self.samples_per_frame:
            raise ValueError(f"mel (B, 80, T) and wav (B, T * {self.samples_per_frame}) expected, got "
                             f"{tuple(mel.shape)} and {tuple(wav.shape)}")
        adversarial_phase = current_step > self.discriminator_train_start_steps
        zero = torch.zeros((), dtype=torch.float32, device=wav.device)
        self.optimizer.zero_grad()
        self.discriminator_optimizer.zero_grad()

        est_weight = None
        if self.basis:
            est, est_weight = self.model(mel)
            est = fit_estimate(est, wav.shape[1])
        else:
            est = fit_estimate(self.model(mel), wav.shape[1], self.pqmf)
        stft_loss, _ = self.vocoder_loss(est, wav, pqmf=self.pqmf)
        weight_loss = average = None
        if est_weight is not None and weight is not None:
            weight_loss, average = self.vocoder_loss.weight_term(est_weight, weight)
        total = self.lambda_stft * stft_loss
        if weight_loss is not None and not adversarial_phase:
            total = total + weight_loss
        adv = fm = zero
        if adversarial_phase:
            real = wav.unsqueeze(1) if self.use_feature_map_loss else None
            terms = generator_adversarial_terms(self.discriminator, self._waveform(est).unsqueeze(1), real,
                                                period_grad=self.period_grad)
            adv = terms["adversarial"]
            total = total + self.lambda_adv * adv
            if self.use_feature_map_loss:
                fm = terms["feature_map"]
                total = total + self.lambda_fm * fm
        total.backward()
        grad_norm = self.optimizer.step(max_norm=self.grad_clip_thresh, **self._step_kw)
        if self.scheduler is not None:
            self.scheduler.step()

        d_loss = d_norm = zero
        if adversarial_phase:
            self.discriminator_optimizer.zero_grad()
            with torch.no_grad():             # the plain forward, with the weights the step above left
                est_for_d = self.model(mel)
                est_for_d = self._waveform(fit_estimate(est_for_d[0] if self.basis else est_for_d, wav.shape[1],
                                                        self.pqmf))
            kw = dict(period_grad=True) if self.period_grad else {}
            d_loss = discriminator_step_terms(self.discriminator, est_for_d.unsqueeze(1), wav.unsqueeze(1),
                                              stft_grad=True, **kw)["discriminator"]
            d_loss.backward()
            d_norm = self.discriminator_optimizer.step(max_norm=self.grad_clip_thresh, **self._step_kw)
            if self.discriminator_scheduler is not None:
                self.discriminator_scheduler.step()

        values = [stft_loss, total, adv, fm, d_loss, zero if grad_norm is None else grad_norm,
                  zero if d_norm is None else d_norm]
        keys = KEYS
        if self.basis:
            keys = KEYS + ("weight", "weight_average")
            average = est_weight.mean() if average is None else average     # no target: the weight term did not run
            # the reference's w_l: the weight loss while it is part of the total, 0 afterwards (train.py:86-89)
            values += [zero if weight_loss is None or adversarial_phase else weight_loss, average]
        scalars = torch.stack([t.detach().float().reshape(()) for t in values])
        if self.process_group is not None:                        # the ranks' means
            scalars = parallel.all_reduce_sum(scalars, self.process_group) / torch.distributed.get_world_size(
                self.process_group)
        return dict(zip(keys, scalars.cpu().tolist()))            # the step's one read on the host
