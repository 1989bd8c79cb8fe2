"""The reference's STFT losses (model/loss/) as forward-only GPU evaluators: ``stft``, ``STFTLoss``,
``MultiResolutionSTFTLoss`` (stft_loss.py) and ``Loss`` (loss.py).  The magnitudes and the partial sums
come from one HIP launch per call (csrc/stft_loss.hip); there is no CPU path and no autograd.
``discriminator_terms`` forms the reference's adversarial / feature-map / discriminator scores from the outputs of
fastvocoder_amd.discriminator in one fused reduction (csrc/disc.hip)."""
from .discriminator_loss import discriminator_terms
from .loss import Loss
from .stft_loss import MultiResolutionSTFTLoss, STFTLoss, stft, stft_tables

__all__ = ["Loss", "discriminator_terms", "MultiResolutionSTFTLoss", "STFTLoss", "stft", "stft_tables"]
