"""The reference's STFT losses (model/loss/) as GPU evaluators: ``stft``, ``STFTLoss``,
``MultiResolutionSTFTLoss`` (stft_loss.py) and ``Loss`` (loss.py).  The magnitudes and the partial sums
come from one HIP launch per call (csrc/stft_loss.hip); there is no CPU path.  They are forward-only by default;
setting a module's ``differentiable`` attribute gives the gradient with respect to the estimate, from fused HIP
kernels as well (csrc/stft_loss_grad.hip).  The target and the discriminator scores have no gradient.
``discriminator_terms`` forms the reference's adversarial / feature-map / discriminator scores from the outputs of
fastvocoder_amd.discriminator in one fused reduction (csrc/disc.hip); ``generator_adversarial_terms`` runs a
discriminator on an estimate that requires grad and returns the generator's adversarial and feature-map terms on its
graph (csrc/disc_grad.hip, csrc/stft_mag_grad.hip); ``discriminator_step_terms`` runs a discriminator on a real
signal and a detached estimate and returns the terms of its own update on the graph of its parameters
(csrc/disc_wgrad.hip, csrc/mpd_wgrad.hip): the multi-scale discriminator as it is, the STFT discriminators with
``stft_grad=True``, the period discriminators with ``period_grad=True``, Discriminator() with ``stft_grad=True`` and
Discriminator(use_mpd=True) with both.  ``pqmf_synthesis`` is PQMF.synthesis on the graph of the sub-bands (the
multiband waveform the discriminator sees in training)."""
from .discriminator_loss import discriminator_step_terms, discriminator_terms, generator_adversarial_terms
from .loss import Loss, PqmfSynthesis, pqmf_synthesis
from .stft_loss import MultiResolutionSTFTLoss, STFTLoss, stft, stft_tables

__all__ = ["Loss", "PqmfSynthesis", "pqmf_synthesis", "discriminator_step_terms", "discriminator_terms", "generator_adversarial_terms", "MultiResolutionSTFTLoss", "STFTLoss", "stft", "stft_tables"]
