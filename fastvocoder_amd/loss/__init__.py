"""The reference's STFT losses (model/loss/) as forward-only GPU evaluators: ``stft``, ``STFTLoss``,
``MultiResolutionSTFTLoss`` (stft_loss.py) and ``Loss`` (loss.py).  The magnitudes and the partial sums
come from one HIP launch per call (csrc/stft_loss.hip); there is no CPU path and no autograd."""
from .loss import Loss
from .stft_loss import MultiResolutionSTFTLoss, STFTLoss, stft, stft_tables

__all__ = ["Loss", "MultiResolutionSTFTLoss", "STFTLoss", "stft", "stft_tables"]
